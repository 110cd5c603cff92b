// kdtn_status.hip — the status write-back bodies on the GPU: for every Topology whose Reconcile
// writes its status (topology.Status.Links = topology.Spec.Links; r.Status().Update,
// controllers/topology_controller.go:125-138) the bytes of json.Marshal(topology.Status.Links)
// as Go 1.19's encoding/json writes them (HTML escaping on), so the driver splices the value
// into the object it sends instead of marshalling every Link (api/v1/topology_types.go:59-176).
//
// Layout: one byte arena in store order; the body of Topology t = bytes[off[t], off[t+1]): the
// JSON array of its spec.links when it is written (action != SKIP and committed), else empty;
// `null` for a nil spec.links, `[]` for an empty one.
//
// Kernels (launch order, kdtn_epoch_status_encode):
//   k_status_esc      per dictionary string (only those appended since the last build): its
//                     escaped length and whether it must be rewritten; dwords classified by SWAR,
//                     the byte automaton (encodeState.string) only for strings that need it
//   k_status_select   per Topology: written or not, and the bytes of a written Topology that
//                     has no records
//   k_status_sizes    per desired record: the size of its object (+ its `[` or `,`, + `]` for
//                     the last record), 0 when its Topology is not written
//   k_scan_*          u64 exclusive scans of both; k_status_offsets: the [T+1] body offsets
//   k_status_write    one wave per 64 consecutive records: the lanes compose their objects into
//                     the wave's LDS window (WSink), whose origin is the wave's arena range start
//                     rounded down to 16 B, and the wave flushes it with 16-B stores
// The sizes and the writer run the same composer (write_record) over a counting or a storing
// sink, so a record's size is the number of bytes its lane writes.
#include "kdtn_encode.h"

namespace kdtn {

// ---- encodeState.string: which bytes are escaped, and how ------------------------------------
// utf8.DecodeRune at s[i] (a byte >= 0x80): the sequence's size, 0 when s[i] starts no valid
// sequence (RuneError of width 1); ls: the rune is U+2028 or U+2029
KD_INLINE uint32_t rune_size(const uint8_t* s, uint32_t i, uint32_t n, bool* ls) {
    const uint32_t c = s[i];
    *ls = false;
    uint32_t need, lo = 0x80u, hi = 0xBFu;
    if (c >= 0xC2u && c <= 0xDFu) need = 1;
    else if (c == 0xE0u) { need = 2; lo = 0xA0u; }
    else if (c >= 0xE1u && c <= 0xEFu) { need = 2; if (c == 0xEDu) hi = 0x9Fu; }
    else if (c == 0xF0u) { need = 3; lo = 0x90u; }
    else if (c >= 0xF1u && c <= 0xF3u) need = 3;
    else if (c == 0xF4u) { need = 3; hi = 0x8Fu; }
    else return 0u;
    if (i + need >= n) return 0u;                          // truncated at the end of the string
    const uint32_t c1 = s[i + 1];
    if (c1 < lo || c1 > hi) return 0u;
    for (uint32_t k = 2; k <= need; ++k)
        if (s[i + k] < 0x80u || s[i + k] > 0xBFu) return 0u;
    *ls = c == 0xE2u && c1 == 0x80u && (s[i + 2] & 0xFEu) == 0xA8u;
    return need + 1u;
}
KD_INLINE uint32_t hex_digit(uint32_t x) { return x < 10u ? 0x30u + x : 0x57u + x; }

// sinks of the composer: put(v, n) appends the low n (1..4) bytes of v; plain(arena, b, len)
// appends arena bytes verbatim
struct CountSink {                       // sizes: counts, reads no string
    static constexpr bool COUNT = true;
    uint64_t n = 0;
    bool over = false;                   // a string of 2 GiB or more
    KD_INLINE void put(uint32_t, uint32_t k) { n += k; }
    KD_INLINE void plain(const uint8_t*, uint32_t, uint32_t len) { n += len; }
};
struct LaneSink {                        // one lane's object into the wave's LDS window
    static constexpr bool COUNT = false;
    WSink o;
    KD_INLINE void put(uint32_t v, uint32_t k) { o.put(v, k); }
    KD_INLINE void plain(const uint8_t* arena, uint32_t b, uint32_t len) {
        if (len <= 32u) o.str(arena, b, len);
        else o.copy(arena, b, len);                        // 32 bytes a round (the arena has 64 B of slack)
    }
};
// an object larger than the window, written by its wave straight to global memory: every lane
// runs the composer on the same record; lane 0 stores the stream, and a long plain string is
// copied by all 64 lanes (the stream stops before it and resumes after it)
struct CoopSink {
    static constexpr bool COUNT = false;
    static constexpr uint32_t COOP_MIN = 256;
    WSink o;
    uint8_t* arena;
    uint64_t cur;
    bool lead;
    KD_INLINE void begin(uint8_t* a, uint64_t at) {
        arena = a;
        cur = at;
        lead = (threadIdx.x & 63) == 0;
        if (lead) o.init(arena + cur);
    }
    KD_INLINE void put(uint32_t v, uint32_t k) {
        if (lead) o.put(v, k);
        cur += k;
    }
    KD_INLINE void plain(const uint8_t* src, uint32_t b, uint32_t len) {
        if (len < COOP_MIN) {
            if (lead) o.str(src, b, len);
            cur += len;
            return;
        }
        if (lead) o.finish();
        for (uint32_t k = threadIdx.x & 63; k < len; k += 64) arena[cur + k] = src[b + k];
        cur += len;
        if (lead) o.init(arena + cur);
    }
    KD_INLINE void end() {
        if (lead) o.finish();
    }
};

// the bytes of s[0, n) between the quotes (Go 1.19 encodeState.string, escapeHTML)
template <class S>
KD_INLINE void emit_escaped(S& o, const uint8_t* s, uint32_t n) {
    uint32_t i = 0;
    while (i < n) {
        const uint32_t c = s[i];
        if (c < 0x80u) {
            if (c == '"' || c == '\\') o.put('\\' | c << 8, 2u);
            else if (c == '\n') o.put('\\' | 'n' << 8, 2u);
            else if (c == '\r') o.put('\\' | 'r' << 8, 2u);
            else if (c == '\t') o.put('\\' | 't' << 8, 2u);
            else if (c < 0x20u || c == '<' || c == '>' || c == '&') {
                o.put('\\' | 'u' << 8 | '0' << 16 | '0' << 24, 4u);
                o.put(hex_digit(c >> 4) | hex_digit(c & 15u) << 8, 2u);
            } else o.put(c, 1u);
            ++i;
            continue;
        }
        bool ls;
        const uint32_t sz = rune_size(s, i, n, &ls);
        if (sz == 0u) {                                    // RuneError (U+FFFD): resume one byte later
            o.put('\\' | 'u' << 8 | 'f' << 16 | 'f' << 24, 4u);
            o.put('f' | 'd' << 8, 2u);
            ++i;
        } else if (ls) {                                   // U+2028 / U+2029
            o.put('\\' | 'u' << 8 | '2' << 16 | '0' << 24, 4u);
            o.put('2' | (uint32_t)('8' + (s[i + 2] & 1u)) << 8, 2u);
            i += 3u;
        } else {
            uint32_t v = c;
            for (uint32_t k = 1; k < sz; ++k) v |= (uint32_t)s[i + k] << (8u * k);
            o.put(v, sz);
            i += sz;
        }
    }
}

// the storing sinks' copy of the automaton, out of line: a rewritten string is the rare case, and
// inlined at all nineteen strings of the composer it would be most of the writer's code
template <class S>
__device__ __attribute__((noinline)) S escaped_out(S o, const uint8_t* s, uint32_t n) {
    emit_escaped(o, s, n);
    return o;
}

// ---- escape tables ------------------------------------------------------------------------------
// bytes of a dword that need a decision: below 0x20, 0x80 and above, " \ < > &
KD_INLINE uint32_t swar_eq(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
KD_INLINE uint32_t swar_special(uint32_t w) {
    const uint32_t lt20 = ~((w & 0x7F7F7F7Fu) + 0x60606060u) & 0x80808080u;
    return (w & 0x80808080u) | lt20 | swar_eq(w, '"') | swar_eq(w, '\\') | swar_eq(w, '<') | swar_eq(w, '>') |
           swar_eq(w, '&');
}

// One thread per dictionary string: its escape-table word. The string's first 32 bytes come from
// one 16-B load pair (+ a dword) as in k_str_inline, the rest a dword at a time; bytes past the
// string count as spaces.
__global__ void __launch_bounds__(BLOCK) k_status_esc(const uint8_t* bytes, const uint32_t* offs, uint32_t n,
                                                      uint32_t* esc) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = offs[i], len = offs[i + 1] - b;
    uint32_t flag = 0;
    if (len) {
        typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
        const uint32_t* a32 = reinterpret_cast<const uint32_t*>(bytes) + (b >> 2);
        const uint32_t sh = b & 3u, nw = (sh + len + 3u) >> 2;
        const u32x4a A = *reinterpret_cast<const u32x4a*>(a32);
        u32x4a B = {0u, 0u, 0u, 0u};
        if (nw > 4u) B = *reinterpret_cast<const u32x4a*>(a32 + 4);
        const uint32_t c8 = nw > 8u ? a32[8] : 0u;
        const uint32_t w[9] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, c8};
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            if (4u * q < len) {
                const uint32_t r = len - 4u * q;
                const uint32_t m = r >= 4u ? 0xFFFFFFFFu : ((1u << (8u * r)) - 1u);
                flag |= swar_special((__builtin_amdgcn_alignbyte(w[q + 1], w[q], sh) & m) | (0x20202020u & ~m));
            }
        }
        for (uint32_t k = 32; k < len; k += 4u) {          // (the arena has 64 B of slack)
            const uint32_t* p = a32 + (k >> 2);
            const uint32_t r = len - k;
            const uint32_t m = r >= 4u ? 0xFFFFFFFFu : ((1u << (8u * r)) - 1u);
            flag |= swar_special((__builtin_amdgcn_alignbyte(p[1], p[0], sh) & m) | (0x20202020u & ~m));
        }
    }
    uint64_t el = len;
    if (flag) {
        CountSink cs;
        emit_escaped(cs, bytes + b, len);
        el = cs.n;
    }
    esc[i] = el >= SE_OVERFLOW ? (SE_OVERFLOW | SE_REWRITE) : ((uint32_t)el | (el != len ? SE_REWRITE : 0u));
}

// ---- the composer -------------------------------------------------------------------------------
struct StatusRec {
    uint32_t key[KDTN_NKEY], prop[KDTN_NPROP], gap;
    int64_t uid;
};
KD_INLINE StatusRec status_rec_load(const DevLinks& L, uint32_t j) {
    StatusRec r;
    const uint32_t* p = L.rec(j);
#pragma unroll
    for (int k = 0; k < KDTN_NKEY; ++k) r.key[k] = L.col<false>(p, COL_KEY0 + k);
#pragma unroll
    for (int k = 0; k < KDTN_NPROP; ++k) r.prop[k] = L.col<false>(p, COL_PROP0 + k);
    r.gap = L.col<false>(p, COL_GAP);
    r.uid = L.uid_at<false>(p, j);
    return r;
}

// key text: a literal, four bytes per put (the constant image is folded into the instructions)
template <class S, int N>
KD_INLINE void jlit(S& o, const char (&t)[N]) {
#pragma unroll
    for (int k = 0; k < N - 1; k += 4) {
        uint32_t w = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (k + c < N - 1) w |= (uint32_t)(uint8_t)t[k + c] << (8 * c);
        o.put(w, (uint32_t)(N - 1 - k < 4 ? N - 1 - k : 4));
    }
}
// strconv.AppendUint(v, 10): base-10000 limbs, the top one without leading zeros
template <class S>
KD_INLINE void emit_u64(S& o, uint64_t v) {
    uint32_t l0, l1, l2, l3 = 0u, l4 = 0u;
    if (v >> 32) {
        l0 = (uint32_t)(v % 10000u);
        v /= 10000u;
        l1 = (uint32_t)(v % 10000u);
        v /= 10000u;
        l2 = (uint32_t)(v % 10000u);
        v /= 10000u;
        l3 = (uint32_t)(v % 10000u);
        l4 = (uint32_t)(v / 10000u);
    } else {
        uint32_t x = (uint32_t)v;
        l0 = x % 10000u;
        x /= 10000u;
        l1 = x % 10000u;
        l2 = x / 10000u;
    }
    const int k = l4 ? 4 : l3 ? 3 : l2 ? 2 : l1 ? 1 : 0;
    const uint32_t top = k == 4 ? l4 : k == 3 ? l3 : k == 2 ? l2 : k == 1 ? l1 : l0;
    const uint32_t nd = ndigits32(top);
    o.put(dig4(top) >> (8u * (4u - nd)), nd);
    if (k >= 4) o.put(dig4(l3), 4u);
    if (k >= 3) o.put(dig4(l2), 4u);
    if (k >= 2) o.put(dig4(l1), 4u);
    if (k >= 1) o.put(dig4(l0), 4u);
}

// string `id` between its quotes: ew = its escape-table word, e = its inline entry (unused by
// the counting sink and for a rewritten string)
template <int W, class S>
KD_INLINE void emit_string(S& o, const StrTab& tab, const uint32_t* offs, uint32_t id, uint32_t ew, const SIE<W>& e) {
    if (!id) return;
    if constexpr (S::COUNT) {
        if ((ew & SE_LEN) == SE_OVERFLOW) o.over = true;
        o.n += ew & SE_LEN;
        return;
    } else {
        if (ew & SE_REWRITE) {
            const uint32_t b = offs[id];
            o = escaped_out(o, tab.bytes + b, offs[id + 1] - b);
            return;
        }
        const uint32_t b0 = e.w[0] & 0xFFu;
        if (b0 >= SI_LONG) {
            o.plain(tab.bytes, e.w[1], e.w[2]);
            return;
        }
#pragma unroll
        for (int q = 0; q < W; ++q)
            if (4u * q < b0)
                o.put(__builtin_amdgcn_alignbyte(q + 1 < W ? e.w[q + 1] : 0u, e.w[q], 1u), b0 - 4u * q < 4u ? b0 - 4u * q : 4u);
    }
}
template <int W, class S>
KD_INLINE SIE<W> entry_for(const StrTab& tab, uint32_t id, uint32_t ew) {
    if constexpr (S::COUNT) return SIE<W>{};
    else return si_load<W>(tab, (ew & SE_REWRITE) ? 0u : id);
}

// One Link object with the array punctuation it carries: `[` (first record of its Topology) or
// `,` before it, `]` after the last. Fields in struct order (api/v1/topology_types.go:59-95,
// 119-176); a property is omitted when "" (gap: when 0), `properties` itself never is.
template <class S>
KD_INLINE void write_record(S& o, const StatusIn& s, const StatusRec& r, bool first, bool last) {
    uint32_t ke[KDTN_NKEY], pe[KDTN_NPROP];
    SIE<SI_KW> k[KDTN_NKEY];
#pragma unroll
    for (int q = 0; q < KDTN_NKEY; ++q) ke[q] = r.key[q] ? s.kesc[r.key[q]] : 0u;
#pragma unroll
    for (int q = 0; q < KDTN_NPROP; ++q) pe[q] = r.prop[q] ? s.pesc[r.prop[q]] : 0u;
#pragma unroll
    for (int q = 0; q < KDTN_NKEY; ++q) k[q] = entry_for<SI_KW, S>(s.kd, r.key[q], ke[q]);
    o.put(first ? '[' : ',', 1u);
    jlit(o, "{\"local_intf\":\"");
    emit_string<SI_KW>(o, s.kd, s.kd_offs, r.key[KDTN_K_LOCAL_INTF], ke[KDTN_K_LOCAL_INTF], k[KDTN_K_LOCAL_INTF]);
    jlit(o, "\",\"local_ip\":\"");
    emit_string<SI_KW>(o, s.kd, s.kd_offs, r.key[KDTN_K_LOCAL_IP], ke[KDTN_K_LOCAL_IP], k[KDTN_K_LOCAL_IP]);
    jlit(o, "\",\"local_mac\":\"");
    emit_string<SI_KW>(o, s.kd, s.kd_offs, r.key[KDTN_K_LOCAL_MAC], ke[KDTN_K_LOCAL_MAC], k[KDTN_K_LOCAL_MAC]);
    jlit(o, "\",\"peer_intf\":\"");
    emit_string<SI_KW>(o, s.kd, s.kd_offs, r.key[KDTN_K_PEER_INTF], ke[KDTN_K_PEER_INTF], k[KDTN_K_PEER_INTF]);
    jlit(o, "\",\"peer_ip\":\"");
    emit_string<SI_KW>(o, s.kd, s.kd_offs, r.key[KDTN_K_PEER_IP], ke[KDTN_K_PEER_IP], k[KDTN_K_PEER_IP]);
    jlit(o, "\",\"peer_mac\":\"");
    emit_string<SI_KW>(o, s.kd, s.kd_offs, r.key[KDTN_K_PEER_MAC], ke[KDTN_K_PEER_MAC], k[KDTN_K_PEER_MAC]);
    jlit(o, "\",\"peer_pod\":\"");
    emit_string<SI_KW>(o, s.kd, s.kd_offs, r.key[KDTN_K_PEER_POD], ke[KDTN_K_PEER_POD], k[KDTN_K_PEER_POD]);
    jlit(o, "\",\"uid\":");
    if (r.uid < 0) o.put('-', 1u);
    emit_u64(o, r.uid < 0 ? 0ull - (uint64_t)r.uid : (uint64_t)r.uid);
    jlit(o, ",\"properties\":{");
    bool sep = false;                                      // a field was written: the next takes a comma
#define KDTN_STATUS_PROP(P, NAME)                                                             \
    if (r.prop[P]) {                                                                          \
        if (sep) o.put(',', 1u);                                                              \
        sep = true;                                                                           \
        jlit(o, "\"" NAME "\":\"");                                                           \
        emit_string<SI_PW>(o, s.pd, s.pd_offs, r.prop[P], pe[P], entry_for<SI_PW, S>(s.pd, r.prop[P], pe[P])); \
        o.put('"', 1u);                                                                       \
    }
    KDTN_STATUS_PROP(KDTN_P_LATENCY, "latency")
    KDTN_STATUS_PROP(KDTN_P_LATENCY_CORR, "latency_corr")
    KDTN_STATUS_PROP(KDTN_P_JITTER, "jitter")
    KDTN_STATUS_PROP(KDTN_P_LOSS, "loss")
    KDTN_STATUS_PROP(KDTN_P_LOSS_CORR, "loss_corr")
    KDTN_STATUS_PROP(KDTN_P_RATE, "rate")
    if (r.gap) {
        if (sep) o.put(',', 1u);
        sep = true;
        jlit(o, "\"gap\":");
        emit_u64(o, r.gap);
    }
    KDTN_STATUS_PROP(KDTN_P_DUPLICATE, "duplicate")
    KDTN_STATUS_PROP(KDTN_P_DUPLICATE_CORR, "duplicate_corr")
    KDTN_STATUS_PROP(KDTN_P_REORDER_PROB, "reorder_prob")
    KDTN_STATUS_PROP(KDTN_P_REORDER_CORR, "reorder_corr")
    KDTN_STATUS_PROP(KDTN_P_CORRUPT_PROB, "corrupt_prob")
    KDTN_STATUS_PROP(KDTN_P_CORRUPT_CORR, "corrupt_corr")
#undef KDTN_STATUS_PROP
    if (last) o.put('}' | '}' << 8 | ']' << 16, 3u);
    else o.put('}' | '}' << 8, 2u);
}

// ---- selection and sizes ------------------------------------------------------------------------
// Per Topology: its body is written when Reconcile reaches the status update — not SKIP (the
// gate returns at :78) and committed: the caller's mask, else CREATED or a DIFF none of whose
// entries fails (cut: k_reach_cuts' first failing entry per list), as k_commit_plan decides. A
// written Topology without records carries `null` (spec.links nil) or `[]` itself.
__global__ void __launch_bounds__(BLOCK) k_status_select(DevTopos T, const uint8_t* action, const uint32_t* cut,
                                                         const uint8_t* mask, uint8_t* sel, uint32_t* tsz,
                                                         uint32_t* tot) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    bool w = false;
    if (t < T.n) {
        const uint8_t a = action[t];
        bool commit = false;
        if (mask) commit = mask[t] != 0;
        else if (a == KDTN_ACT_CREATED) commit = true;
        else if (a == KDTN_ACT_DIFF)
            commit = cut[3 * t] == 0xFFFFFFFFu && cut[3 * t + 1] == 0xFFFFFFFFu && cut[3 * t + 2] == 0xFFFFFFFFu;
        w = commit && a != KDTN_ACT_SKIP;
        sel[t] = w ? 1 : 0;
        const bool none = T.des_off[t + 1] == T.des_off[t];
        tsz[t] = (w && none) ? ((T.flags[t] & KDTN_TOPO_SPEC_NIL) ? 4u : 2u) : 0u;
    }
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint64_t m = __ballot(w);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < BLOCK / 64; ++k) n += wsum[k];
        if (n) atomicAdd(tot + (blockIdx.x & 31u), n);
    }
}

// One lane per desired record: its Topology (wave-cooperative search) and the bytes it writes.
__global__ void __launch_bounds__(BLOCK) k_status_sizes(StatusIn s, uint32_t* rsz, uint32_t* rtopo, uint32_t* tot) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    const bool on = j < s.N.n;
    const uint32_t t = entry_topo_wave(s.T.des_off, s.T.n, j, on);
    if (!on) return;
    uint32_t size = 0;
    if (s.sel[t]) {
        CountSink cs;
        write_record(cs, s, status_rec_load(s.N, j), j == s.T.des_off[t], j + 1u == s.T.des_off[t + 1]);
        if (cs.over || cs.n > 0xFFFFFFFFull) atomicOr(tot + ST_TOT_ERR, 1u);
        else size = (uint32_t)cs.n;
        if (size > (uint32_t)STATUS_WIN - 16u && !tot[ST_TOT_BIG]) atomicOr(tot + ST_TOT_BIG, 1u);
    }
    rsz[j] = size;
    rtopo[j] = t;
}

// body offsets: Topology t starts at its first record's position plus the bytes of the
// record-less Topologies before it; off[T] = the arena size, also left in the totals block
__global__ void __launch_bounds__(BLOCK) k_status_offsets(StatusIn s, uint64_t* off, uint32_t* tot) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t > s.T.n) return;
    const uint64_t at = s.rpos[s.T.des_off[t]] + s.tpos[t];
    off[t] = at;
    if (t == s.T.n) *reinterpret_cast<uint64_t*>(tot + ST_TOT_BYTES) = at;
}

// ---- writer -------------------------------------------------------------------------------------
// Blocks [0, nwb): one wave per 64 consecutive desired records. The written records of a wave
// lie back to back in the arena except where a record-less written Topology stands between two
// of them, so the wave proceeds in rounds: the longest prefix of its pending lanes whose bytes
// are contiguous and fit the window. The window's origin is the round's first byte rounded down
// to 16, so LDS and arena addresses agree mod 16 and the flush is 16-B stores (byte stores on
// the ragged head and tail, which share their 16 bytes with other writers). A single object
// larger than the window is left to k_status_write_big.
// Blocks [nwb, ...): one thread per Topology, the `null` / `[]` of the record-less ones.
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(STATUS_WAVES)))
k_status_write(StatusIn s, const uint64_t* off, uint32_t nwb, uint8_t* arena) {
    __shared__ uint4 win[BLOCK / 64][STATUS_WIN / 16];
    if (blockIdx.x >= nwb) {
        const uint32_t t = (blockIdx.x - nwb) * BLOCK + threadIdx.x;
        const uint32_t z = t < s.T.n ? s.tsz[t] : 0u;
        if (z) {
            uint8_t* p = arena + off[t];
            const uint32_t v = z == 4u ? ('n' | 'u' << 8 | 'l' << 16 | 'l' << 24) : ('[' | ']' << 8);
            for (uint32_t k = 0; k < z; ++k) p[k] = (uint8_t)(v >> (8u * k));
        }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = (blockIdx.x * (BLOCK / 64) + wave) * 64u + lane;
    const uint32_t size = j < s.N.n ? s.rsz[j] : 0u;
    const bool act = size != 0u;
    uint64_t pos = 0;
    bool first = false, last = false;
    StatusRec rec{};
    if (act) {
        const uint32_t t = s.rtopo[j];
        pos = s.rpos[j] + s.tpos[t];
        first = j == s.T.des_off[t];
        last = j + 1u == s.T.des_off[t + 1];
        rec = status_rec_load(s.N, j);
    }
    const uint64_t end = pos + size;
    // brk: this lane's bytes do not follow the previous written lane's (positions ascend)
    uint64_t pe = act ? end : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(pe, d, 64);
        if (lane >= d && o > pe) pe = o;
    }
    uint64_t prev = __shfl_up(pe, 1, 64);
    if (lane == 0) prev = 0ull;
    const bool brk = act && prev != pos;
    uint8_t* wb = reinterpret_cast<uint8_t*>(win[wave]);
    uint64_t pending = __ballot(act);
    while (pending) {                                      // wave-uniform
        const int a = __builtin_ctzll(pending);
        const uint64_t r0 = __shfl(pos, a, 64), base = r0 & ~15ull;
        if (__shfl(end, a, 64) - base > (uint64_t)STATUS_WIN) {   // k_status_write_big's
            pending &= ~(1ull << a);
            continue;
        }
        const bool mine0 = (pending >> lane) & 1ull;
        const uint64_t stop = __ballot(mine0 && lane > a && (brk || end - base > (uint64_t)STATUS_WIN));
        const uint64_t round = stop ? pending & ((1ull << __builtin_ctzll(stop)) - 1ull) : pending;
        if ((round >> lane) & 1ull) {
            LaneSink o;
            o.o.init(wb + (uint32_t)(pos - base));
            write_record(o, s, rec, first, last);
            o.o.finish();
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t r1 = __shfl(end, 63 - __builtin_clzll(round), 64);
        const uint32_t nch = (uint32_t)((r1 - base + 15ull) >> 4);
        for (uint32_t q = lane; q < nch; q += 64u) {
            const uint64_t ga = base + 16ull * q;
            if (ga >= r0 && ga + 16ull <= r1) {
                *reinterpret_cast<uint4*>(arena + ga) = win[wave][q];
            } else {                                       // the round's first or last 16 bytes
#pragma unroll 1
                for (uint32_t k = 0; k < 16; ++k)
                    if (ga + k >= r0 && ga + k < r1) arena[ga + k] = wb[16u * q + k];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        pending &= ~round;
    }
}

// The objects larger than the window (launched when k_status_sizes saw one that may be): the
// same wave as in k_status_write owns the record; every lane runs the composer on it (the
// record broadcast from its lane), straight to global memory (CoopSink).
__global__ void __launch_bounds__(BLOCK) k_status_write_big(StatusIn s, uint8_t* arena) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t size = j < s.N.n ? s.rsz[j] : 0u;
    uint64_t pos = 0;
    uint32_t t = 0;
    if (size) {
        t = s.rtopo[j];
        pos = s.rpos[j] + s.tpos[t];
    }
    const bool big = (pos & 15ull) + size > (uint64_t)STATUS_WIN;
    uint64_t pending = __ballot(big);
    if (!pending) return;                                  // wave-uniform
    StatusRec rec{};
    bool first = false, last = false;
    if (big) {
        rec = status_rec_load(s.N, j);
        first = j == s.T.des_off[t];
        last = j + 1u == s.T.des_off[t + 1];
    }
    for (; pending; pending &= pending - 1ull) {
        const int a = __builtin_ctzll(pending);
        StatusRec rb;
#pragma unroll
        for (int q = 0; q < KDTN_NKEY; ++q) rb.key[q] = __shfl(rec.key[q], a, 64);
#pragma unroll
        for (int q = 0; q < KDTN_NPROP; ++q) rb.prop[q] = __shfl(rec.prop[q], a, 64);
        rb.gap = __shfl(rec.gap, a, 64);
        rb.uid = __shfl(rec.uid, a, 64);
        CoopSink o;
        o.begin(arena, __shfl(pos, a, 64));
        write_record(o, s, rb, __shfl((int)first, a, 64) != 0, __shfl((int)last, a, 64) != 0);
        o.end();
    }
}

}  // namespace kdtn
