// kdtn_remote.hip — RemotePod request bodies → Remote.Update plans on the GPU (include/kdtn.h
// kdtn_remote_ingest): the receiving side of kdtn_epoch_remote_encode. A batch of bare RemotePod
// messages (proto/v1/kube_dtn.proto:65-79) in HBM becomes one fixed-size plan per message: the
// pure prefix of KubeDTN.Update (daemon/kubedtn/handler.go:149-198), which is proto.Unmarshal, the
// VNI conflict check against the daemon's VxlanManager map (:177-185), net.ParseCIDR(IntfIp)
// (daemon/vxlan/vxlan.go:80-83) and MakeQdiscs(Properties) (vxlan.go:40, common/qdisc.go:20-126).
//
// A RemotePod is flat and small and its plan is numeric, so nothing of the LinksBatchQuery
// decoder's structure is needed (no frame lists, no second pass, no dictionaries):
//   k_rp_vni_build   the snapshot's VNIs into an open-addressing table (slot = entry index,
//                    atomicMin: the lowest entry of a key wins)
//   k_rp_plan        one wave per 64 consecutive messages, one lane per message. The wave copies
//                    a run of its bodies into its LDS window (16-B loads, only the run's span),
//                    each lane walks its own body once out of LDS — six string (offset, length)
//                    pairs, vni, the merged properties' twelve pairs and gap, all in registers —
//                    then parses the strings it needs in place (cidr_ok, and the kdtn_parse.h
//                    parsers from a loop with three call sites), composes the qdisc record as
//                    qdisc_from does (kdtn_qplan.h), probes the VNI table and compares the netns bytes. Plans
//                    and qdisc records of the wave are staged in LDS and stored coalesced.
// A body that does not fit the window, and every body of a wave whose starts are not ascending
// or leave a gap of more than a window, is walked from memory instead (UwWin falls back to
// memory for any byte outside the staged range, so the result never depends on the window).
#include "kdtn_qplan.h"

namespace kdtn {

// The decoded message in registers. Columns are selected by unrolled compares, never indexed.
struct RpMsg {
    uint32_t so[KDTN_RP_NSTR], sl[KDTN_RP_NSTR];     // RemotePod strings (fields 1-5, 8)
    uint32_t po[KDTN_NPROP], pl[KDTN_NPROP];         // LinkProperties strings (KDTN_P_*)
    uint32_t vni, gap, has_props;
};

// LinkProperties (kube_dtn.proto:36-53) at [a, e) merged into M: strings 1-6, 8-13, gap 7
KD_INLINE uint32_t rp_props(const UwWin& w, uint32_t a, uint32_t e, RpMsg& M) {
    uint32_t pos = a;
    while (pos < e) {
        UwField f;
        const uint32_t r = uw_field(w, pos, e, f);
        if (r) return r;
        if (f.wt == 2u && f.fn >= 1u && f.fn <= 13u && f.fn != 7u) {
            if (!uw_str_ok(w, f.off, f.len)) return KDTN_WIRE_UTF8;
            const uint32_t col = f.fn < 7u ? f.fn - 1u : f.fn - 2u;
#pragma unroll
            for (int k = 0; k < KDTN_NPROP; ++k) {
                M.po[k] = col == (uint32_t)k ? f.off : M.po[k];
                M.pl[k] = col == (uint32_t)k ? f.len : M.pl[k];
            }
        } else if (f.wt == 0u && f.fn == 7u) {
            M.gap = (uint32_t)f.v;                          // uint32: the varint's low 32 bits
        }
    }
    return KDTN_WIRE_OK;
}

// RemotePod at [a, e): net_ns 1, intf_name 2, intf_ip 3, peer_vtep 4, kube_ns 5, vni 6,
// properties 7 (every occurrence merged where it is met), name 8. One sequential walk, so the
// error returned is the first fault in stream order.
KD_INLINE uint32_t rp_walk(const UwWin& w, uint32_t a, uint32_t e, RpMsg& M) {
#pragma unroll
    for (int k = 0; k < KDTN_RP_NSTR; ++k) M.so[k] = M.sl[k] = 0;
#pragma unroll
    for (int k = 0; k < KDTN_NPROP; ++k) M.po[k] = M.pl[k] = 0;
    M.vni = M.gap = M.has_props = 0;
    uint32_t pos = a;
    while (pos < e) {
        UwField f;
        uint32_t r = uw_field(w, pos, e, f);
        if (r) return r;
        if (f.wt == 2u && f.fn == 7u) {
            M.has_props = 1;
            r = rp_props(w, f.off, f.off + f.len, M);
            if (r) return r;
        } else if (f.wt == 2u && ((f.fn >= 1u && f.fn <= 5u) || f.fn == 8u)) {
            if (!uw_str_ok(w, f.off, f.len)) return KDTN_WIRE_UTF8;
            const uint32_t col = f.fn == 8u ? (uint32_t)KDTN_RP_NAME : f.fn - 1u;
#pragma unroll
            for (int k = 0; k < KDTN_RP_NSTR; ++k) {
                M.so[k] = col == (uint32_t)k ? f.off : M.so[k];
                M.sl[k] = col == (uint32_t)k ? f.len : M.sl[k];
            }
        } else if (f.wt == 0u && f.fn == 6u) {
            M.vni = (uint32_t)f.v;                          // int32: the varint's low 32 bits
        }
    }
    return KDTN_WIRE_OK;
}

KD_INLINE uint32_t rp_home(uint32_t vni, uint32_t shift) { return (vni * 0x9E3779B1u) >> shift; }

// Open addressing over the snapshot, keyed by vni: a slot holds an entry index, RP_EMPTY when
// free. Entries with one key follow one probe sequence and meet in one slot, where atomicMin
// leaves the lowest of them.
__global__ void __launch_bounds__(BLOCK) k_rp_vni_build(const int32_t* vni, uint32_t n, uint32_t* slots, uint32_t mask,
                                                        uint32_t shift) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = (uint32_t)vni[i];
    for (uint32_t h = rp_home(key, shift), step = 0; step <= mask; ++step, h = (h + 1u) & mask) {
        const uint32_t was = atomicCAS(slots + h, RP_EMPTY, i);
        if (was == RP_EMPTY) return;
        if ((uint32_t)vni[was] == key) {
            atomicMin(slots + h, i);
            return;
        }
    }
}

// the entry holding vni, RP_EMPTY when the snapshot has none
KD_INLINE uint32_t rp_lookup(const RpIn& in, uint32_t vni) {
    if (!in.n_vni) return RP_EMPTY;
    for (uint32_t h = rp_home(vni, in.vshift), step = 0; step <= in.vmask; ++step, h = (h + 1u) & in.vmask) {
        const uint32_t ent = in.slots[h];
        if (ent == RP_EMPTY || (uint32_t)in.vni[ent] == vni) return ent;
    }
    return RP_EMPTY;
}

// One message: the walk, then the plan (16 dwords at P) and the qdisc record (18 dwords at Q),
// both in the wave's LDS images. wbytes: the window as bytes, for the parsers.
KD_INLINE void rp_one(const RpIn& in, const UwWin& w, const uint8_t* wbytes, uint32_t a, uint32_t e, uint32_t* P,
                      uint32_t* Q, bool& rejected, bool& conflict) {
    RpMsg M;
    const uint32_t werr = rp_walk(w, a, e, M);
    rejected = werr != 0;
    conflict = false;
    if (werr) {                                             // wire_err alone: every other field 0
#pragma unroll
        for (int k = 0; k < 16; ++k) P[k] = k == 14 ? werr : 0u;
#pragma unroll
        for (int k = 0; k < 18; ++k) Q[k] = 0u;
        return;
    }
    // a staged body lies whole inside the window; anything else is read from memory
    auto at = [&](uint32_t off) -> const uint8_t* {
        const uint32_t q = off - w.base;
        return q < w.lim ? wbytes + q : w.doc + off;
    };
    uint32_t err = 0;
    if (M.sl[KDTN_RP_INTF_IP] && !cidr_ok(at(M.so[KDTN_RP_INTF_IP]), M.sl[KDTN_RP_INTF_IP])) err = KDTN_E_REMOTE_CIDR;

    const uint32_t qerr = qdisc_plan(at, M.po, M.pl, M.gap, in.tick, Q);
    if (!err) err = qerr;

    // handler.go:177-185: Get(vni) found and the stored netns is not this message's
    const uint32_t ent = rp_lookup(in, M.vni);
    if (ent != RP_EMPTY) {
        const uint32_t b = in.ns_offs[ent], n = in.ns_offs[ent + 1] - b;
        bool same = n == M.sl[KDTN_RP_NET_NS];
        for (uint32_t i = 0; same && i < n; ++i) same = in.ns_bytes[b + i] == w.byte(M.so[KDTN_RP_NET_NS] + i);
        conflict = !same;
    }
#pragma unroll
    for (int k = 0; k < KDTN_RP_NSTR; ++k) {
        P[2 * k] = M.sl[k] ? M.so[k] : 0u;
        P[2 * k + 1] = M.sl[k];
    }
    P[12] = M.vni;
    P[13] = ent;
    P[14] = (err << 8) | ((conflict ? 1u : 0u) << 16) | (M.has_props << 24);
    P[15] = 0;
}

__global__ void __launch_bounds__(UW_BLOCK) k_rp_plan(RpIn in, uint4* plan, uint2* qdisc, uint32_t* ctl) {
    // (two more words: parse_pct loads the 20 bytes from a short string's first dword at once)
    __shared__ uint4 win[UW_WIN / 16 + 2];
    __shared__ uint4 pimg[64 * 4];                          // the wave's plans, 64 B each
    __shared__ uint2 qimg[64 * 9];                          // and qdisc records, 72 B each
    const uint32_t lane = threadIdx.x, m0 = blockIdx.x * 64u, m = m0 + lane;
    const uint32_t cnt = min(64u, in.n_msgs - m0);
    const bool on = lane < cnt;
    const uint32_t a = on ? (uint32_t)in.start[m] : 0u, sz = on ? in.size[m] : 0u, e = a + sz;
    // the wave stages only when its starts ascend and no gap between two bodies exceeds a window
    const uint32_t a_prev = __shfl_up(a, 1, 64), e_prev = __shfl_up(e, 1, 64);
    const bool apart = on && lane > 0 && (a < a_prev || (a > e_prev && a - e_prev > UW_WIN));
    const bool staging = __ballot(apart) == 0;
    const bool direct = on && (!staging || (a & 15u) + sz > UW_WIN);
    UwWin w{(UwLds)reinterpret_cast<const uint32_t*>(win), 0u, 0u, in.doc};
    const uint8_t* wbytes = reinterpret_cast<const uint8_t*>(win);
    uint32_t* P = reinterpret_cast<uint32_t*>(pimg) + lane * 16u;
    uint32_t* Q = reinterpret_cast<uint32_t*>(qimg) + lane * 18u;
    bool rejected = false, conflict = false;
    for (uint32_t cur = 0; cur < cnt;) {
        uint32_t run = cnt;                                 // an unstaged wave: every lane at once
        if (staging) {
            const uint32_t base = __shfl(a, cur, 64) & ~15u;
            run = uw_run(on, lane, cur, e, base);           // (ascending: no start lies below base)
            if (run) {
                uint32_t hi = on && lane >= cur && lane < cur + run ? e : base;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) hi = max(hi, (uint32_t)__shfl_xor(hi, o, 64));
                uw_fill_span(win, in.doc, w, base, (hi - base + 15u) & ~15u);
            } else {
                run = 1;                                    // larger than the window: from memory
            }
        }
        if (on && lane >= cur && lane < cur + run) {
            UwWin mine = w;
            if (direct) mine.lim = 0;
            rp_one(in, mine, wbytes, a, e, P, Q, rejected, conflict);
        }
        cur += run;
    }
    __syncthreads();
    // the wave's records are contiguous: coalesced 16-B and 8-B stores out of the images
    for (uint32_t i = lane; i < cnt * 4u; i += UW_BLOCK) plan[(size_t)m0 * 4 + i] = pimg[i];
    if (qdisc)
        for (uint32_t i = lane; i < cnt * 9u; i += UW_BLOCK) qdisc[(size_t)m0 * 9 + i] = qimg[i];
    const uint32_t nd = __popcll(__ballot(direct)), nr = __popcll(__ballot(rejected)), nc = __popcll(__ballot(conflict));
    if (lane == 0) {
        if (nd) atomicAdd(ctl + RP_CTL_DIRECT, nd);
        if (nr) atomicAdd(ctl + RP_CTL_REJECTED, nr);
        if (nc) atomicAdd(ctl + RP_CTL_CONFLICT, nc);
    }
}

}  // namespace kdtn
