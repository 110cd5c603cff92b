// kdtn_unwire.hip — LinksBatchQuery streams → epoch tables on the GPU (include/kdtn.h
// kdtn_wire_ingest): the inverse of kdtn_wire.hip. A stream of protobuf messages
// (proto/v1/kube_dtn.proto:8-53) in HBM becomes one Topology per message: the LocalPod strings
// in the topology row, the links in the desired (ADD / UPD) or realised (DEL) store, every
// string interned through the ingest's lock-free table (kdtn_jsintern.h). Decoding follows
// protobuf-go's proto.Unmarshal for proto3 (fields in any order, unknown fields skipped by wire
// type, last scalar wins, sub-messages merge, links append); a malformed message is rejected
// alone (kdtn_wire_err per message).
//
// Protobuf has no structural index to build in parallel: a field is found only by walking the
// tags before it, a serial chain of (tag, length, jump) per nesting level. The passes therefore
// split the work by nesting level, and every chain runs out of LDS:
//   k_uw_frame<0/1>  top level, count then write (with the scans between): the (offset, length)
//                    of every `links` element and every `local_pod` occurrence. One lane per
//                    message, 64 messages per wave; the wave first copies a run of its messages
//                    into its LDS window (UW_WIN bytes, 16-B loads), so the dependent steps cost
//                    LDS latency. A message larger than the window takes the whole wave: the
//                    window slides over it, 64 lanes refill, lane 0 walks.
//   k_uw_links<0>    one lane per Link frame, the wave's frames staged through LDS the same way
//                    (the links of a message are adjacent): nine fields and the merged
//                    properties into registers, the strings validated (utf8_ok, the wire
//                    writer's validator); the first error of a message lands in merr
//   k_uw_pods<0>     one lane per message: its local_pod occurrences merged and validated
//   k_uw_counts      rejected messages drop out: record counts per message and side
//   k_uw_links<1> / k_uw_pods<1>   the surviving values interned (occurrence = stream offset / 2,
//                    unique per value: two non-empty strings lie at least 3 bytes apart) and the
//                    provisional slots written to the row staging / topology columns
// The ingest's k_js_rep_mark … k_js_finalize_* then turn slots into first-occurrence ids.
#include "kdtn_jsintern.h"
#include "kdtn_wirewalk.h"

namespace kdtn {

// every lane of the wave: add the lanes' field counts to the stage's total
KD_INLINE void uw_count(unsigned long long* ctl, uint32_t nf) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nf += __shfl_xor(nf, o, 64);
    if ((threadIdx.x & 63u) == 0 && nf) atomicAdd(ctl + UW_CTL_FIELDS, (unsigned long long)nf);
}

// 1 + intern slot of the string at [off, off + len) (0 = ""); JS_NONE when the table is full
KD_INLINE uint32_t uw_slot(const UwWin& w, const JsIntern& it, const JsDict& dt, uint32_t off, uint32_t len) {
    if (!len) return 0;
    if (len > 0xFFFFFFu) {
        atomicOr(it.status, JS_ST_LONG);
        return JS_NONE;
    }
    uint32_t x[9], pw[8];
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = w.word((off & ~3u) + 4u * k);
#pragma unroll
    for (int k = 0; k < 8; ++k) pw[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], off & 3u);
    const bool win = len <= WIN;
    uint64_t h;
    if (win) {
        h = word_hash(pw, len);
    } else {
        h = 1469598103934665603ull;
        for (uint32_t k = 0; k < len; ++k) h = fnv_step(h, w.byte(off + k));
    }
    h ^= h >> 29;
    const uint32_t s = intern(it, dt, w.doc + off, len, ((uint64_t)len << 32) | off, h, off >> 1, pw, win);
    return s == JS_NONE ? JS_NONE : s + 1;
}

// ---------------------------------------------------------------- frame pass
// One top-level field of message m at pos: a links element or a local_pod occurrence is counted
// (and, in the write pass, its frame stored at the message's next slot), anything else skipped.
template <bool WRITE>
KD_INLINE uint32_t uw_top(const UwWin& w, const UwFrames& f, uint32_t m, uint32_t& pos, uint32_t e, uint64_t lo,
                          uint64_t po, uint32_t& nl, uint32_t& np) {
    UwField fld;
    const uint32_t r = uw_field(w, pos, e, fld);
    if (r) return r;
    if (fld.wt == 2u && fld.fn == 2u) {
        if (WRITE) {
            f.lfr[lo + nl] = make_uint2(fld.off, fld.len);
            f.lmsg[lo + nl] = m;
        }
        ++nl;
    } else if (fld.wt == 2u && fld.fn == 1u) {
        if (WRITE) f.pfr[po + np] = make_uint2(fld.off, fld.len);
        ++np;
    }
    return KDTN_WIRE_OK;
}

template <bool WRITE>
__global__ void __launch_bounds__(UW_BLOCK) k_uw_frame(UwIn in, UwFrames f) {
    __shared__ uint4 win[UW_WIN / 16];
    const uint32_t lane = threadIdx.x, m0 = blockIdx.x * 64u, m = m0 + lane;
    const uint32_t cnt = min(64u, in.n_msgs - m0);
    const bool on = lane < cnt;
    const uint32_t a = on ? (uint32_t)in.off[m] : 0u, e = on ? (uint32_t)in.off[m + 1] : 0u;
    // the write pass walks only the messages whose top level the count pass accepted
    const bool live = on && (!WRITE || f.merr[m] == ~0ull);
    const uint64_t lo = WRITE && on ? f.loff[m] : 0ull, po = WRITE && on ? f.poff[m] : 0ull;
    uint32_t nl = 0, np = 0, nf = 0, err = 0;
    UwWin w{(UwLds)reinterpret_cast<const uint32_t*>(win), 0u, 0u, in.doc};
    for (uint32_t cur = 0; cur < cnt;) {
        const uint32_t a_cur = __shfl(a, cur, 64), e_cur = __shfl(e, cur, 64);
        const uint32_t run = uw_run(on, lane, cur, e, a_cur & ~15u);
        if (run) {                                          // short messages: one lane each
            uw_fill(win, in, w, a_cur & ~15u);
            if (live && lane >= cur && lane < cur + run) {
                uint32_t pos = a;
                while (pos < e) {
                    const uint32_t at = pos;
                    err = uw_top<WRITE>(w, f, m, pos, e, lo, po, nl, np);
                    if (err) {
                        uw_fail(f.merr + m, at, err);
                        break;
                    }
                    ++nf;
                }
            }
            cur += run;
            continue;
        }
        // a long message: the wave slides its window over it, lane 0 walks. A refill leaves at
        // least a whole field header (two varints) inside the window, so every round advances.
        const uint32_t mc = m0 + cur;
        const bool walk = __shfl((int)live, cur, 64) != 0;
        const uint64_t clo = WRITE ? f.loff[mc] : 0ull, cpo = WRITE ? f.poff[mc] : 0ull;
        uint32_t pos = a_cur, cl = 0, cp = 0, cf = 0, fin = walk ? 0u : 1u;
        if (!WRITE && lane == 0) {
            atomicMin(f.ctl + UW_CTL_FIRST_LONG, (unsigned long long)mc);
            atomicAdd(f.ctl + UW_CTL_N_LONG, 1ull);
        }
        while (!fin) {
            uw_fill(win, in, w, pos & ~15u);
            if (lane == 0) {
                while (pos < e_cur && (pos + 20u <= w.base + w.lim || e_cur <= w.base + w.lim)) {
                    const uint32_t at = pos;
                    const uint32_t r = uw_top<WRITE>(w, f, mc, pos, e_cur, clo, cpo, cl, cp);
                    if (r) {
                        uw_fail(f.merr + mc, at, r);
                        fin = 2;
                        break;
                    }
                    ++cf;
                }
                if (!fin && pos >= e_cur) fin = 1;
            }
            fin = __shfl(fin, 0, 64);
            pos = __shfl(pos, 0, 64);
        }
        const uint32_t tl = __shfl(cl, 0, 64), tp = __shfl(cp, 0, 64);
        if (lane == cur) {                                  // the message's own lane keeps its result
            nl = tl;
            np = tp;
            err = fin == 2 ? 1u : 0u;
        }
        if (lane == 0) nf += cf;
        cur += 1;
    }
    if (!WRITE) {
        if (on) {
            f.nl[m] = err ? 0u : nl;
            f.np[m] = err ? 0u : np;
        }
        uw_count(f.ctl, nf);
    }
}
template __global__ void k_uw_frame<false>(UwIn, UwFrames);
template __global__ void k_uw_frame<true>(UwIn, UwFrames);

// ---------------------------------------------------------------- link pass
// INTERN = false: decode and validate, the message's first error into merr. INTERN = true (the
// messages that survived): decode again, intern the surviving values, write the record's row.
template <bool INTERN>
__global__ void __launch_bounds__(UW_BLOCK) k_uw_links(UwIn in, UwFrames f, uint32_t nfr, const uint32_t* rbase,
                                                       JsStore des, JsStore real, JsIntern it) {
    __shared__ uint4 win[UW_WIN / 16];
    const uint32_t lane = threadIdx.x, i0 = blockIdx.x * 64u, i = i0 + lane;
    const uint32_t cnt = min(64u, nfr - i0);
    const bool on = lane < cnt;
    const uint2 fr = on ? f.lfr[i] : make_uint2(0u, 0u);
    const uint32_t a = fr.x, e = fr.x + fr.y;
    const uint32_t m = on ? f.lmsg[i] : 0u;
    const bool live = on && (!INTERN || f.merr[m] == ~0ull);
    uint32_t nf = 0;
    UwWin w{(UwLds)reinterpret_cast<const uint32_t*>(win), 0u, 0u, in.doc};
    for (uint32_t cur = 0; cur < cnt;) {
        const uint32_t base = __shfl(a, cur, 64) & ~15u;
        // (a Link larger than the window goes alone: its lane reads past the staged part from memory)
        const uint32_t run = max(1u, uw_run(on, lane, cur, e, base));
        const bool mine = live && lane >= cur && lane < cur + run;
        if (__ballot(mine)) {
            uw_fill(win, in, w, base);
            if (mine) {
                UwLink L;
                uint32_t at = a;
                const uint32_t r = uw_link<!INTERN>(w, a, e, L, nf, at);
                if (!INTERN) {
                    if (r) uw_fail(f.merr + m, at, r);
                } else {
                    const uint32_t rec = rbase[m] + (i - (uint32_t)f.loff[m]);
                    uint32_t* row = (in.kind[m] == KDTN_BATCH_DEL ? real : des).base + (size_t)rec * JS_ROW;
#pragma unroll
                    for (int k = 0; k < KDTN_NKEY; ++k) row[COL_KEY0 + k] = uw_slot(w, it, it.kd, L.so[k], L.sl[k]);
#pragma unroll
                    for (int k = 0; k < KDTN_NPROP; ++k)
                        row[COL_PROP0 + k] = uw_slot(w, it, it.pd, L.so[KDTN_NKEY + k], L.sl[KDTN_NKEY + k]);
                    row[COL_GAP] = L.gap;
                    *reinterpret_cast<uint64_t*>(row + LINK_COLS32) = L.uid;   // 8-B aligned (88-B rows)
                }
            }
        }
        cur += run;
    }
    if (!INTERN) uw_count(f.ctl, nf);
}
template __global__ void k_uw_links<false>(UwIn, UwFrames, uint32_t, const uint32_t*, JsStore, JsStore, JsIntern);
template __global__ void k_uw_links<true>(UwIn, UwFrames, uint32_t, const uint32_t*, JsStore, JsStore, JsIntern);

// ---------------------------------------------------------------- local pod pass
// One lane per message: its local_pod occurrences (Pod, kube_dtn.proto:8-17) merged in order:
// name 1, src_ip 2, net_ns 3, kube_ns 4; a nested links element (5) is decoded for its errors
// only, as Unmarshal would meet them. The few strings per message are read from memory.
template <bool INTERN>
__global__ void __launch_bounds__(BLOCK) k_uw_pods(UwIn in, UwFrames f, JsTopoOut to, JsIntern it) {
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    const UwWin w{(UwLds)0, 0u, 0u, in.doc};
    uint32_t nf = 0;
    if (m < in.n_msgs && f.merr[m] == ~0ull) {
        uint32_t so[4] = {0, 0, 0, 0}, sl[4] = {0, 0, 0, 0}, r = 0, at = 0;
        for (uint64_t p = f.poff[m]; p < f.poff[m + 1] && !r; ++p) {
            const uint2 fr = f.pfr[p];
            uint32_t pos = fr.x;
            const uint32_t e = fr.x + fr.y;
            while (pos < e && !r) {
                at = pos;
                UwField fld;
                r = uw_field(w, pos, e, fld);
                if (r) break;
                ++nf;
                if (fld.wt != 2u) continue;
                if (fld.fn >= 1u && fld.fn <= 4u) {
                    if (!INTERN && !uw_str_ok(w, fld.off, fld.len)) r = KDTN_WIRE_UTF8;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        so[k] = fld.fn == (uint32_t)k + 1u ? fld.off : so[k];
                        sl[k] = fld.fn == (uint32_t)k + 1u ? fld.len : sl[k];
                    }
                } else if (!INTERN && fld.fn == 5u) {
                    UwLink L;
                    r = uw_link<true>(w, fld.off, fld.off + fld.len, L, nf, at);
                }
            }
        }
        if (!INTERN) {
            if (r) uw_fail(f.merr + m, at, r);
        } else {
            to.name[m] = uw_slot(w, it, it.kd, so[0], sl[0]);
            to.src_ip[m] = uw_slot(w, it, it.kd, so[1], sl[1]);
            to.net_ns[m] = uw_slot(w, it, it.kd, so[2], sl[2]);
            to.ns[m] = uw_slot(w, it, it.kd, so[3], sl[3]);
        }
    }
    if (!INTERN) uw_count(f.ctl, nf);
}
template __global__ void k_uw_pods<false>(UwIn, UwFrames, JsTopoOut, JsIntern);
template __global__ void k_uw_pods<true>(UwIn, UwFrames, JsTopoOut, JsIntern);

// ---------------------------------------------------------------- sizes and offsets
// per message: its error byte, and its record count on the side its kind selects (a rejected
// message keeps its Topology with both lists empty)
__global__ void __launch_bounds__(BLOCK) k_uw_counts(UwIn in, UwFrames f, uint32_t* cdes, uint32_t* creal, uint8_t* err8) {
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= in.n_msgs) return;
    const unsigned long long e = f.merr[m];
    const uint32_t code = e == ~0ull ? 0u : (uint32_t)(e & 0xFFu);
    const uint32_t n = code ? 0u : f.nl[m];
    const bool del = in.kind[m] == KDTN_BATCH_DEL;
    err8[m] = (uint8_t)code;
    cdes[m] = del ? 0u : n;
    creal[m] = del ? n : 0u;
}

// the scanned counts as the topology table's u32 offsets, and each message's first record
__global__ void __launch_bounds__(BLOCK) k_uw_offsets(UwIn in, const uint64_t* des64, const uint64_t* real64,
                                                      JsTopoOut to, uint32_t* rbase) {
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    if (m > in.n_msgs) return;
    to.des_off[m] = (uint32_t)des64[m];
    to.real_off[m] = (uint32_t)real64[m];
    if (m < in.n_msgs) rbase[m] = (uint32_t)(in.kind[m] == KDTN_BATCH_DEL ? real64[m] : des64[m]);
}

}  // namespace kdtn
