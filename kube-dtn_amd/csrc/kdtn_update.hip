// kdtn_update.hip — Local.UpdateLinks request bodies → per-link plans on the GPU (include/kdtn.h
// kdtn_update_ingest). A stream of LinksBatchQuery messages (proto/v1/kube_dtn.proto:8-53) in
// HBM becomes, per link, the pure part of the handler's loop body (daemon/kubedtn/handler.go:
// 644-657): MakeVeth(localPod.NetNs, LocalIntf, LocalIp, LocalMac) (common/veth.go:13-41), which
// is net.ParseCIDR and net.ParseMAC, then MakeQdiscs(Properties) (common/qdisc.go:20-126); and
// per message the handler's first-error abort as a cut index.
//
// UpdateLinks reads none of the epoch's tables (no pods, no VXLAN map), so nothing is interned:
// the decoder's frame pass (k_uw_frame<0/1>, kdtn_unwire.hip) finds the links elements and the
// local_pod occurrences, and then
//   k_ul_plan   one lane per Link frame, one wave per 64 consecutive frames. The wave copies a
//               run of its frames into its LDS window (16-B loads, only the run's span); each
//               lane walks its Link once out of LDS (uw_link<true>: 19 (offset, length) pairs,
//               uid, gap in registers), checks LocalIp and LocalMac where they lie (cidr_ok,
//               mac_ok), parses the property strings in place and composes the qdisc record
//               (kdtn_qplan.h, the copy k_rp_plan uses). Plans and qdisc records go through two
//               LDS images and are stored coalesced at the frame's index. The cut: the lanes of
//               one message are adjacent and their indexes ascend, so the segment's lowest
//               failing link is its lowest failing lane: two ballots, one shuffle for that
//               lane's err, one atomicMin per (wave, message) into the message's cut word.
//   k_ul_msgs   one lane per message: its local_pod occurrences merged and validated, the cut
//               word resolved, the record written; a rejected message counts no links
//   k_ul_pack   after the scan of those counts: link_base into the records, and every plan of
//               a surviving message from its frame's index to its place
// A Link frame that does not fit the window is walked from memory by its lane (UwWin falls
// back to memory for any byte outside the staged range).
#include "kdtn_qplan.h"

namespace kdtn {

// One Link at [a, e): the plan (8 dwords at P) and the qdisc record (18 dwords at Q), both in
// the wave's LDS images. wbytes: the window as bytes, for the parsers. Returns the link's err.
KD_INLINE uint32_t ul_one(const UwWin& w, const uint8_t* wbytes, unsigned long long* merr, uint32_t a, uint32_t e,
                          uint32_t m, uint32_t idx, double tick, uint32_t* P, uint32_t* Q) {
    UwLink L;
    uint32_t nf = 0, fault = a;
    const uint32_t r = uw_link<true>(w, a, e, L, nf, fault);
    if (r) {                                                // the message is rejected: k_ul_pack drops the plan
        uw_fail(merr, fault, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) P[k] = 0u;
#pragma unroll
        for (int k = 0; k < 18; ++k) Q[k] = 0u;
        return 0u;
    }
    // a staged frame lies whole inside the window; anything else is read from memory
    auto at = [&](uint32_t off) -> const uint8_t* {
        const uint32_t q = off - w.base;
        return q < w.lim ? wbytes + q : w.doc + off;
    };
    // handler.go:649-657: MakeVeth (the CIDR, then the MAC), then MakeQdiscs
    uint32_t err = 0;
    if (L.sl[KDTN_K_LOCAL_IP] && !cidr_ok(at(L.so[KDTN_K_LOCAL_IP]), L.sl[KDTN_K_LOCAL_IP])) err = KDTN_E_VETH_CIDR;
    else if (L.sl[KDTN_K_LOCAL_MAC] && !mac_ok(at(L.so[KDTN_K_LOCAL_MAC]), L.sl[KDTN_K_LOCAL_MAC])) err = KDTN_E_VETH_MAC;
    const uint32_t qerr = qdisc_plan(at, L.so + KDTN_NKEY, L.sl + KDTN_NKEY, L.gap, tick, Q);
    if (!err) err = qerr;
    P[0] = L.sl[KDTN_K_LOCAL_INTF] ? L.so[KDTN_K_LOCAL_INTF] : 0u;
    P[1] = L.sl[KDTN_K_LOCAL_INTF];
    P[2] = (uint32_t)L.uid;
    P[3] = (uint32_t)(L.uid >> 32);
    P[4] = m;
    P[5] = idx;
    P[6] = err | (L.has_props << 8);
    P[7] = 0u;
    return err;
}

__global__ void __launch_bounds__(UW_BLOCK) k_ul_plan(UwIn in, UwFrames f, uint32_t nfr, double tick, UlOut o) {
    // (two more words: parse_pct loads the 20 bytes from a short string's first dword at once)
    __shared__ uint4 win[UW_WIN / 16 + 2];
    __shared__ uint4 pimg[64 * 2];                          // the wave's plans, 32 B each
    __shared__ uint2 qimg[64 * 9];                          // and qdisc records, 72 B each
    const uint32_t lane = threadIdx.x, i0 = blockIdx.x * 64u, i = i0 + lane;
    const uint32_t cnt = min(64u, nfr - i0);
    const bool on = lane < cnt;
    const uint2 fr = on ? f.lfr[i] : make_uint2(0u, 0u);
    const uint32_t a = fr.x, e = fr.x + fr.y;
    const uint32_t m = on ? f.lmsg[i] : 0xFFFFFFFFu;        // (no message: a segment of its own)
    const uint32_t idx = on ? i - (uint32_t)f.loff[m] : 0u;
    const bool direct = on && (a & 15u) + fr.y > UW_WIN;
    UwWin w{(UwLds)reinterpret_cast<const uint32_t*>(win), 0u, 0u, in.doc};
    const uint8_t* wbytes = reinterpret_cast<const uint8_t*>(win);
    uint32_t* P = reinterpret_cast<uint32_t*>(pimg) + lane * 8u;
    uint32_t* Q = reinterpret_cast<uint32_t*>(qimg) + lane * 18u;
    uint32_t err = 0;
    // frames ascend in the stream (messages do, and a message's links): runs that fit a window
    for (uint32_t cur = 0; cur < cnt;) {
        const uint32_t base = __shfl(a, cur, 64) & ~15u;
        const uint32_t fit = uw_run(on, lane, cur, e, base);
        const uint32_t run = max(1u, fit);                  // larger than the window: alone, from memory
        const bool mine = on && lane >= cur && lane < cur + run;
        if (fit) {
            uint32_t hi = mine ? e : base;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) hi = max(hi, (uint32_t)__shfl_xor(hi, s, 64));
            uw_fill_span(win, in.doc, w, base, (hi - base + 15u) & ~15u);
        }
        if (mine) {
            UwWin v = w;
            if (direct) v.lim = 0;
            err = ul_one(v, wbytes, f.merr + m, a, e, m, idx, tick, P, Q);
        }
        cur += run;
    }
    // the cut: per run of equal m, the lowest lane with err != 0 holds the lowest failing index
    const uint32_t m_prev = __shfl_up(m, 1, 64);
    const uint64_t heads = __ballot(on && (lane == 0 || m != m_prev)), bad = __ballot(err != 0);
    const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
    const uint32_t end = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : 64u;
    const uint64_t seg = ((bad >> lane) << lane) & (end == 64u ? ~0ull : (1ull << end) - 1ull);
    const uint32_t src = seg ? (uint32_t)__builtin_ctzll(seg) : lane;
    const uint32_t err_src = __shfl(err, src, 64);
    if ((heads >> lane & 1ull) && seg)
        atomicMin(o.mcut + m, ((unsigned long long)(idx + (src - lane)) << 8) | err_src);
    __syncthreads();
    // the wave's records are contiguous: coalesced 16-B and 8-B stores out of the images
    for (uint32_t k = lane; k < cnt * 2u; k += UW_BLOCK) o.link[(size_t)i0 * 2 + k] = pimg[k];
    for (uint32_t k = lane; k < cnt * 9u; k += UW_BLOCK) o.qdisc[(size_t)i0 * 9 + k] = qimg[k];
    const uint32_t nd = __popcll(__ballot(direct));
    if (lane == 0 && nd) atomicAdd(o.ctl + UL_CTL_DIRECT, nd);
}

// One lane per message, after k_ul_plan: the local_pod occurrences (Pod, kube_dtn.proto:8-17)
// merged in order as k_uw_pods<false> walks them (name 1, net_ns 3; src_ip 2 and kube_ns 4 only
// validated; a nested links element decoded for its errors only), the cut word resolved, the
// record written without its link_base, and cnt[m] = the links it reports (0 when rejected).
__global__ void __launch_bounds__(BLOCK) k_ul_msgs(UwIn in, UwFrames f, UlOut o, uint4* msg, uint32_t* cnt) {
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    const bool on = m < in.n_msgs;
    const UwWin w{(UwLds)0, 0u, 0u, in.doc};
    bool rejected = false, is_cut = false;
    if (on) {
        unsigned long long werr = f.merr[m];
        uint32_t no = 0, nl = 0, so = 0, sl = 0;            // name, net_ns
        if (werr == ~0ull) {
            uint32_t r = 0, fault = 0, nf = 0;
            for (uint64_t p = f.poff[m]; p < f.poff[m + 1] && !r; ++p) {
                const uint2 fr = f.pfr[p];
                uint32_t pos = fr.x;
                const uint32_t e = fr.x + fr.y;
                while (pos < e && !r) {
                    fault = pos;
                    UwField fld;
                    r = uw_field(w, pos, e, fld);
                    if (r) break;
                    if (fld.wt != 2u) continue;
                    if (fld.fn >= 1u && fld.fn <= 4u) {
                        if (!uw_str_ok(w, fld.off, fld.len)) r = KDTN_WIRE_UTF8;
                        no = fld.fn == 1u ? fld.off : no;
                        nl = fld.fn == 1u ? fld.len : nl;
                        so = fld.fn == 3u ? fld.off : so;
                        sl = fld.fn == 3u ? fld.len : sl;
                    } else if (fld.fn == 5u) {
                        UwLink L;
                        r = uw_link<true>(w, fld.off, fld.off + fld.len, L, nf, fault);
                    }
                }
            }
            if (r) werr = ((unsigned long long)fault << 8) | r;
        }
        const uint32_t code = werr == ~0ull ? 0u : (uint32_t)(werr & 0xFFu);
        rejected = code != 0;
        const uint32_t n = rejected ? 0u : f.nl[m];
        const unsigned long long cw = o.mcut[m];
        is_cut = !rejected && cw != ~0ull;
        const uint32_t cut = is_cut ? (uint32_t)(cw >> 8) : n;
        const uint32_t err = is_cut ? (uint32_t)(cw & 0xFFu) : 0u;
        cnt[m] = n;
        // net_ns, name | link_base (k_ul_pack), n_links, cut, wire_err + err << 8
        msg[2 * (size_t)m] = rejected ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(sl ? so : 0u, sl, nl ? no : 0u, nl);
        msg[2 * (size_t)m + 1] = make_uint4(0u, n, cut, code | (err << 8));
    }
    const uint32_t nr = __popcll(__ballot(rejected)), nc = __popcll(__ballot(is_cut));
    if ((threadIdx.x & 63u) == 0) {
        if (nr) atomicAdd(o.ctl + UL_CTL_REJECTED, nr);
        if (nc) atomicAdd(o.ctl + UL_CTL_CUT, nc);
    }
}

// After the scan of cnt: one thread per 8-byte word of a staged record (4 of the plan, 9 of the
// qdisc record) moves it to its place, link_base[m] + the link's index; the plans of a rejected
// message drop out. The first n_msgs threads also write link_base into the message records.
__global__ void __launch_bounds__(BLOCK) k_ul_pack(UwFrames f, uint32_t n_msgs, uint32_t nfr, const uint64_t* base64,
                                                   UlOut o, uint4* msg, uint2* link, uint2* qdisc) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t < n_msgs) reinterpret_cast<uint32_t*>(msg + 2 * t + 1)[0] = (uint32_t)base64[t];
    const uint64_t i = t / 13u;
    const uint32_t k = (uint32_t)(t % 13u);
    if (i >= nfr) return;
    const uint32_t m = f.lmsg[i];
    if (base64[m + 1] == base64[m]) return;                 // rejected (a surviving message here has links)
    const uint64_t dst = base64[m] + (i - f.loff[m]);
    if (k < 4u) link[dst * 4 + k] = reinterpret_cast<const uint2*>(o.link)[i * 4 + k];
    else qdisc[dst * 9 + (k - 4u)] = o.qdisc[i * 9 + (k - 4u)];
}

}  // namespace kdtn
