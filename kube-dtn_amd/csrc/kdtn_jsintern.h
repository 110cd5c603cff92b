// kdtn_jsintern.h — the ingests' lock-free intern table (device side): string windows, hashes
// and the probe. Shared by the JSON ingest (kdtn_ingest.hip) and the LinksBatchQuery decoder
// (kdtn_unwire.hip); a string is named by its byte range in the uploaded bytes (or the decode heap).
#pragma once
#include "kdtn_kernels.h"

namespace kdtn {

KD_INLINE uint64_t fnv_step(uint64_t h, uint32_t c) { return (h ^ c) * 1099511628211ull; }

// The 32 document bytes starting at byte a, as 8 words aligned to a: nine aligned dword
// loads issued together (the document has >= 128 bytes of padding), so a short string costs
// one memory round trip instead of one per byte.
constexpr uint32_t WIN = 32;
KD_INLINE void load_window(const uint8_t* doc, uint32_t a, uint32_t u[8]) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(doc + (a & ~3u));
    uint32_t w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = p[k];
    const uint32_t sh = a & 3u;
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
}
KD_INLINE uint32_t win_byte(const uint32_t u[8], int k) { return (u[k >> 2] >> (8 * (k & 3))) & 0xFFu; }
// Hash of a string of len (<= WIN) bytes held in a window: one 64-bit FNV-style step per
// 4-byte word (bytes past len masked off, len folded into the seed). Every string of at most
// WIN bytes is hashed this way, from the document or the decode heap alike, and longer
// strings by the byte loop, so equal strings always hash equally. Words past the longest
// string of the wave are skipped (wave-uniform test), the rest predicated without branches.
KD_INLINE uint64_t word_hash(const uint32_t u[8], uint32_t len) {
    uint64_t h = 1469598103934665603ull ^ len;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t lo = 4u * k;
        if (__ballot(lo < len)) {
            const uint32_t m = len >= lo + 4 ? 0xFFFFFFFFu : len <= lo ? 0u : (1u << (8 * (len - lo))) - 1u;
            const uint64_t hn = fnv_step(h, u[k] & m);
            h = lo < len ? hn : h;
        }
    }
    return h;
}
// first len (<= WIN) bytes of two windows equal
KD_INLINE bool window_eq(const uint32_t a[8], const uint32_t b[8], uint32_t len) {
    bool eq = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t lo = 4u * k;
        const uint32_t m = len >= lo + 4 ? 0xFFFFFFFFu : len <= lo ? 0u : (1u << (8 * (len - lo))) - 1u;
        eq &= ((a[k] ^ b[k]) & m) == 0;
    }
    return eq;
}

// intern table key word: [63:57] hash tag | [56] heap | [55:32] length | [31:0] offset
KD_INLINE const uint8_t* key_bytes(const JsIntern& in, uint64_t kw) {
    return ((kw >> 56) & 1 ? in.heap : in.doc) + (uint32_t)kw;
}

// a zero byte among the first len (<= JS_INL) bytes of w: inline bytes not (yet) available
KD_INLINE bool inline_has_zero(const uint32_t w[6], uint32_t len) {
    bool z = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t lo = 4u * k;
        const uint32_t m = len >= lo + 4 ? 0xFFFFFFFFu : len <= lo ? 0u : (1u << (8 * (len - lo))) - 1u;
        z |= (((w[k] - 0x01010101u) & ~w[k] & 0x80808080u) & (m & 0x80808080u)) != 0;
    }
    return z;
}

// returns the table slot of the string [p, p+len) (len ≥ 1), or JS_NONE on overflow
KD_INLINE uint32_t intern(const JsIntern& in, const JsDict& dt, const uint8_t* p, uint32_t len, uint64_t kw_self,
                          uint64_t h, uint32_t occ, const uint32_t (&pw)[8], bool have_pw) {
    const uint64_t tag = h >> 57;
    const uint64_t kw = (tag << 57) | kw_self;
    bool inl = have_pw && len <= JS_INL;
    if constexpr (KDTN_PROFILING != 0) {
        const uint32_t off = in.variant & (JSV_NO_INLINE | (dt.slots == in.kd.slots ? JSV_NO_INLINE_K : JSV_NO_INLINE_P));
        if (off) inl = false;
    }
    uint32_t s = (uint32_t)h & dt.mask;
    const uint32_t probes = dt.mask < JS_MAX_PROBE ? dt.mask + 1 : JS_MAX_PROBE;   // a run this long: grow the table
    for (uint32_t probe = 0; probe < probes; ++probe) {
        // slots are written once (CAS from 0): a plain load is either that final key or a stale 0,
        // and a stale 0 only sends us to the CAS, which returns the real key. The key word and
        // the inline bytes come from one 32-byte slot (two 16-B loads of one line).
        const uint4 q0 = *reinterpret_cast<const uint4*>(dt.slots + s);
        const uint4 q1 = *reinterpret_cast<const uint4*>(&dt.slots[s].b[2]);
        unsigned long long cur = (KDTN_PROFILING && (in.variant & JSV_COHERENT))
                                     ? __hip_atomic_load(&dt.slots[s].kw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                     : ((unsigned long long)q0.y << 32) | q0.x;
        if (cur == 0) {
            if ((kw >> 56) & 1) __threadfence();       // heap bytes visible before the key
            cur = atomicCAS(&dt.slots[s].kw, 0ull, (unsigned long long)kw);
            if (cur == 0) {
                atomicMin(dt.rep + s, occ);
                dt.keys[s] = kw;
                if (inl && !inline_has_zero(pw, len)) {   // bytes past len stored as they are (ignored)
                    *reinterpret_cast<uint2*>(&dt.slots[s].b[0]) = make_uint2(pw[0], pw[1]);
                    *reinterpret_cast<uint4*>(&dt.slots[s].b[2]) = make_uint4(pw[2], pw[3], pw[4], pw[5]);
                }
                return s;
            }
        }
        if ((cur >> 57) == tag && ((cur >> 32) & 0xFFFFFFu) == len) {
            uint32_t k = 0;
            const uint32_t ib[8] = {q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, 0u, 0u};
            if (inl && !((cur >> 56) & 1) && !inline_has_zero(ib, len)) {
                // the inserter's bytes, final (a string with a zero byte is never stored inline,
                // a word not yet stored reads as zero): they decide equality
                k = window_eq(pw, ib, len) ? len : 0u;
            } else if ((cur >> 56) & 1) {             // heap bytes of another thread: coherent loads
                const uint32_t off = (uint32_t)cur;
                while (k < len) {
                    const uint32_t wd = __hip_atomic_load(reinterpret_cast<const uint32_t*>(in.heap) + ((off + k) >> 2),
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (((wd >> (8 * ((off + k) & 3))) & 0xFFu) != p[k]) break;
                    ++k;
                }
            } else if (have_pw && len <= WIN) {       // both in the document: compare windows
                uint32_t qw[8];
                load_window(in.doc, (uint32_t)cur, qw);
                k = window_eq(pw, qw, len) ? len : 0u;
            } else {
                const uint8_t* q = in.doc + (uint32_t)cur;
                while (k < len && q[k] == p[k]) ++k;
            }
            if (k == len) {                           // hot strings: skip the atomic when it cannot lower
                // an occurrence later in the document than the one that inserted the key cannot
                // lower the first occurrence (the inserter's own atomicMin is <= its index, and
                // document offsets grow with token indices): no rep read, no atomic
                const bool later = !((kw_self >> 56) & 1) && !((cur >> 56) & 1) && (uint32_t)kw_self > (uint32_t)cur;
                if (!later && !(KDTN_PROFILING && (in.variant & JSV_NO_REP)) && occ < dt.rep[s])
                    atomicMin(dt.rep + s, occ);
                return s;
            }
        }
        s = (s + 1) & dt.mask;
    }
    atomicOr(in.status, JS_ST_OVERFLOW);
    return JS_NONE;
}

}  // namespace kdtn
