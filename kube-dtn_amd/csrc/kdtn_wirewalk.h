// kdtn_wirewalk.h — walking protobuf wire format out of a wave's LDS window: the window view,
// its fill, the varint and field readers and the string check shared by the LinksBatchQuery
// decoder (kdtn_unwire.hip) and the RemotePod planner (kdtn_remote.hip).
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

}  // namespace kdtn
