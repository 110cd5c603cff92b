// kdtn_wirewalk.h — walking protobuf wire format out of a wave's LDS window: the window view,
// its fill, the varint and field readers, the string check and the Link walker shared by the
// LinksBatchQuery decoder (kdtn_unwire.hip), the RemotePod planner (kdtn_remote.hip) and the
// UpdateLinks planner (kdtn_update.hip).
#pragma once
#include "kdtn_encode.h"

namespace kdtn {

// The wave's view of the stream: the bytes [base, base + lim) staged in LDS (base and lim
// multiples of 16), anything else from memory (the stream is padded past its end).
typedef const __attribute__((address_space(3))) uint32_t* UwLds;   // (an LDS pointer, never a flat one)
struct UwWin {
    UwLds lds;
    uint32_t base, lim;
    const uint8_t* doc;
    KD_INLINE uint32_t word(uint32_t p) const {            // the aligned dword at p
        const uint32_t q = p - base;
        return q < lim ? lds[q >> 2] : *reinterpret_cast<const uint32_t*>(doc + p);
    }
    KD_INLINE uint32_t byte(uint32_t p) const { return (word(p & ~3u) >> (8 * (p & 3u))) & 0xFFu; }
};

// all lanes of the (one-wave) workgroup: stage the window at base (16-aligned, <= the stream's end)
KD_INLINE void uw_fill(uint4* win, const UwIn& in, UwWin& w, uint32_t base) {
    const uint32_t lim = min(UW_WIN, in.lim - base);
    __syncthreads();                                        // the previous window's readers
    const uint4* src = reinterpret_cast<const uint4*>(in.doc + base);
    for (uint32_t i = threadIdx.x; i < lim / 16; i += UW_BLOCK) win[i] = src[i];
    __syncthreads();
    w.base = base;
    w.lim = lim;
}

// all lanes of the (one-wave) workgroup: stage only [base, base + lim) (both multiples of 16)
KD_INLINE void uw_fill_span(uint4* win, const uint8_t* doc, UwWin& w, uint32_t base, uint32_t lim) {
    __syncthreads();                                        // the previous window's readers
    const uint4* src = reinterpret_cast<const uint4*>(doc + base);
    for (uint32_t i = threadIdx.x; i < lim / 16; i += UW_BLOCK) win[i] = src[i];
    __syncthreads();
    w.base = base;
    w.lim = lim;
}

// lanes [cur, cur + run) of the wave hold ascending byte ranges ending at e: the longest run
// from lane cur whose ranges all end inside a window placed at base (0: not even the first)
KD_INLINE uint32_t uw_run(bool on, uint32_t lane, uint32_t cur, uint32_t e, uint32_t base) {
    const uint64_t fit = __ballot(on && lane >= cur && e - base <= UW_WIN);
    const uint64_t x = ~(fit >> cur);
    return x ? (uint32_t)__builtin_ctzll(x) : 64u;
}

// protowire.ConsumeVarint within [pos, e): at most 10 bytes, the 10th 0 or 1
KD_INLINE uint32_t uw_varint(const UwWin& w, uint32_t& pos, uint32_t e, uint64_t& v) {
    v = 0;
    for (uint32_t i = 0; i < 10; ++i) {
        if (pos + i >= e) return KDTN_WIRE_TRUNCATED;
        const uint32_t b = w.byte(pos + i);
        if (i == 9 && b > 1) return KDTN_WIRE_VARINT;
        v |= (uint64_t)(b & 0x7Fu) << (7 * i);
        if (b < 0x80u) {
            pos += i + 1;
            return KDTN_WIRE_OK;
        }
    }
    return KDTN_WIRE_VARINT;
}

struct UwField {
    uint32_t fn, wt;      // field number, wire type (0, 1, 2 or 5)
    uint32_t off, len;    // payload of a length-delimited or fixed field
    uint64_t v;           // value of a varint field
};
// One field at pos (< e) of a message ending at e; pos moves past it. Field numbers 0 and above
// 2^29 - 1 and wire types 6, 7 are KDTN_WIRE_TAG, groups KDTN_WIRE_GROUP, a payload or a varint
// running past e KDTN_WIRE_TRUNCATED.
KD_INLINE uint32_t uw_field(const UwWin& w, uint32_t& pos, uint32_t e, UwField& f) {
    uint64_t tag;
    uint32_t r = uw_varint(w, pos, e, tag);
    if (r) return r;
    f.wt = (uint32_t)tag & 7u;
    if ((tag >> 3) == 0 || (tag >> 3) > 0x1FFFFFFFull || f.wt >= 6u) return KDTN_WIRE_TAG;
    if (f.wt == 3u || f.wt == 4u) return KDTN_WIRE_GROUP;
    f.fn = (uint32_t)(tag >> 3);
    f.off = pos;
    f.len = 0;
    f.v = 0;
    if (f.wt == 0u) return uw_varint(w, pos, e, f.v);
    uint64_t len = f.wt == 1u ? 8u : 4u;
    if (f.wt == 2u) {
        r = uw_varint(w, pos, e, len);
        if (r) return r;
        f.off = pos;
    }
    if (len > (uint64_t)(e - pos)) return KDTN_WIRE_TRUNCATED;
    f.len = (uint32_t)len;
    pos += f.len;
    return KDTN_WIRE_OK;
}

// a string field's bytes: ASCII by a masked dword scan of the window, else the validator
KD_INLINE bool uw_str_ok(const UwWin& w, uint32_t off, uint32_t len) {
    if (!len) return true;
    const uint32_t end = off + len;
    uint32_t acc = 0;
    for (uint32_t p = off & ~3u; p < end; p += 4) {
        uint32_t m = 0xFFFFFFFFu;
        if (p < off) m <<= 8 * (off - p);
        if (p + 4 > end) m &= 0xFFFFFFFFu >> (8 * (p + 4 - end));
        acc |= w.word(p) & m;
    }
    return !(acc & 0x80808080u) || utf8_ok(w.doc + off, len);
}

// a message's first error: the lowest (offset, code) of those the passes meet
KD_INLINE void uw_fail(unsigned long long* merr, uint32_t at, uint32_t code) {
    atomicMin(merr, ((unsigned long long)at << 8) | code);
}

// ---------------------------------------------------------------- Link and LinkProperties
// The decoded Link in registers: (offset, length) of the 7 key columns (KDTN_K_*) and the 12
// property columns (KDTN_P_*), uid, gap, whether a properties field was met. Columns are selected
// without indexing (no scratch).
constexpr int UW_NSTR = KDTN_NKEY + KDTN_NPROP;
struct UwLink {
    uint32_t so[UW_NSTR], sl[UW_NSTR];
    uint64_t uid;
    uint32_t gap, has_props;
};
KD_INLINE void uw_set(UwLink& L, uint32_t col, uint32_t off, uint32_t len) {
#pragma unroll
    for (int k = 0; k < UW_NSTR; ++k) {
        L.so[k] = col == (uint32_t)k ? off : L.so[k];
        L.sl[k] = col == (uint32_t)k ? len : L.sl[k];
    }
}

// LinkProperties (kube_dtn.proto:36-53) at [a, e) merged into L: strings 1-6, 8-13, gap 7
template <bool CHECK>
KD_INLINE uint32_t uw_props(const UwWin& w, uint32_t a, uint32_t e, UwLink& L, uint32_t& nf, uint32_t& at) {
    uint32_t pos = a;
    while (pos < e) {
        at = pos;
        UwField f;
        const uint32_t r = uw_field(w, pos, e, f);
        if (r) return r;
        ++nf;
        if (f.wt == 2u && f.fn >= 1u && f.fn <= 13u && f.fn != 7u) {
            if (CHECK && !uw_str_ok(w, f.off, f.len)) return KDTN_WIRE_UTF8;
            uw_set(L, KDTN_NKEY + (f.fn < 7u ? f.fn - 1u : f.fn - 2u), f.off, f.len);
        } else if (f.wt == 0u && f.fn == 7u) {
            L.gap = (uint32_t)f.v;                          // uint32: the varint's low 32 bits
        }
    }
    return KDTN_WIRE_OK;
}

// Link (kube_dtn.proto:19-34) at [a, e): peer_pod 1, local_intf 2, peer_intf 3, local_ip 4,
// peer_ip 5, uid 6, properties 7 (every occurrence merged), local_mac 8, peer_mac 9
template <bool CHECK>
KD_INLINE uint32_t uw_link(const UwWin& w, uint32_t a, uint32_t e, UwLink& L, uint32_t& nf, uint32_t& at) {
#pragma unroll
    for (int k = 0; k < UW_NSTR; ++k) L.so[k] = L.sl[k] = 0;
    L.uid = 0;
    L.gap = L.has_props = 0;
    // KDTN_K_* column of field number fn, a nibble each
    constexpr uint64_t COLS = (uint64_t)KDTN_K_PEER_POD << 4 | (uint64_t)KDTN_K_LOCAL_INTF << 8 |
                              (uint64_t)KDTN_K_PEER_INTF << 12 | (uint64_t)KDTN_K_LOCAL_IP << 16 |
                              (uint64_t)KDTN_K_PEER_IP << 20 | (uint64_t)KDTN_K_LOCAL_MAC << 32 |
                              (uint64_t)KDTN_K_PEER_MAC << 36;
    uint32_t pos = a;
    while (pos < e) {
        at = pos;
        UwField f;
        uint32_t r = uw_field(w, pos, e, f);
        if (r) return r;
        ++nf;
        if (f.wt == 2u && f.fn == 7u) {
            L.has_props = 1;
            r = uw_props<CHECK>(w, f.off, f.off + f.len, L, nf, at);
            if (r) return r;
        } else if (f.wt == 2u && f.fn >= 1u && f.fn <= 9u && f.fn != 6u) {
            if (CHECK && !uw_str_ok(w, f.off, f.len)) return KDTN_WIRE_UTF8;
            uw_set(L, (uint32_t)(COLS >> (4 * f.fn)) & 15u, f.off, f.len);
        } else if (f.wt == 0u && f.fn == 6u) {
            L.uid = f.v;                                    // int64: two's complement
        }
    }
    return KDTN_WIRE_OK;
}

}  // namespace kdtn
