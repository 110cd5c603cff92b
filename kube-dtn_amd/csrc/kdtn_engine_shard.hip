// kdtn_engine_shard.hip — the multi-GPU entry points of the C-ABI: RCCL setup, pod-table exchange, late pods,
// and the VXLAN map's ops and apply
// (host side of libkdtn.so; the context and the shared helpers are in kdtn_engine.h)
#include "kdtn_engine.h"

extern "C" {

int kdtn_comm_unique_id(uint8_t out[128]) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return KDTN_EIO;
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(out, &id, 128);
    return KDTN_OK;
}

int kdtn_comm_init(kdtn_ctx* c, const uint8_t uid[128], int nranks, int rank) {
    if (!c || !uid || nranks < 1 || rank < 0 || rank >= nranks) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (c->comm) {
        (void)ncclCommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->nranks = nranks;
    c->rank = rank;
    c->uploaded = false;
    c->sh_active = false;
    c->pods_rank_major = true;
    if (!c->comm_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_fill, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_ag, hipEventDisableTiming));
    }
    ncclUniqueId id;
    std::memcpy(&id, uid, 128);
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        std::snprintf(g_last_error, sizeof(g_last_error), "ncclCommInitRank: %s", ncclGetErrorString(r));
        c->comm = nullptr;
        c->nranks = 1;
        c->rank = 0;
        return KDTN_EIO;
    }
    return KDTN_OK;
}

int kdtn_comm_set_ranks(kdtn_ctx* c, int nranks, int rank) {
    if (!c || nranks < 1 || rank < 0 || rank >= nranks) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (c->comm) {
        (void)ncclCommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->nranks = nranks;
    c->rank = rank;
    c->uploaded = false;
    c->pods_imported = false;
    c->sh_active = false;                 // a new rank setup replaces a sharded ingest's
    c->pods_rank_major = true;
    return KDTN_OK;
}

int kdtn_pods_export(kdtn_ctx* c, kdtn_pod_row* rows) {
    if (!c || !c->uploaded || (c->slice && !rows)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t rank_base = c->slice * (uint32_t)c->rank;
    uint4* pods = dp<uint4>(c->pods);
    if (c->slice) {
        k_pods_fill<<<nblocks(c->slice), BLOCK, 0, c->stream>>>(topo_view(c), c->slice, rank_base, pods);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rows, pods + rank_base, (size_t)c->slice * 16, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KDTN_OK;
}

int kdtn_pods_import(kdtn_ctx* c, const kdtn_pod_row* rows, uint64_t n) {
    if (!c || !c->uploaded || n != c->pod_total || (n && !rows)) {
        if (c) std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_pods_import: %llu rows, expected pod_slice*nranks = %u",
                             (unsigned long long)n, c->pod_total);
        return KDTN_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (n) HIP_TRY(hipMemcpyAsync(c->pods.p, rows, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pods_imported = true;
    return KDTN_OK;
}

// getPod's API-server fallback (include/kdtn.h): rows of Topologies the informer store missed,
// after the gathered pod table, in every following run's peer lookup
int kdtn_epoch_late_pods(kdtn_ctx* c, const kdtn_pod_row* rows, uint32_t n) {
    if (!c || !c->uploaded || (n && !rows)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    g_last_error[0] = 0;
    const uint32_t D = c->D;
    for (uint32_t i = 0; i < n; ++i) {
        const kdtn_pod_row& r = rows[i];
        if (r.ns >= D || r.name >= D || r.src_ip >= D || (r.net_ns_nil & 0x7FFFFFFFu) >= D) {
            std::snprintf(g_last_error, sizeof(g_last_error),
                          "kdtn_epoch_late_pods: row %u names a string past the dictionary (%u strings)", i, D);
            return KDTN_EINVAL;
        }
    }
    const uint64_t all = (uint64_t)c->pod_total + n;
    if (all > POD_INDEX) {
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_epoch_late_pods: pod table of %llu entries exceeds 2^30",
                      (unsigned long long)all);
        return KDTN_EINVAL;
    }
    hipStream_t s = c->stream;
    // the gathered rows stay (a host-transport import, a sharded ingest's fill)
    TRY(ensure_keep(c->pods, (size_t)all * 16, (size_t)c->pod_total * 16, s));
    c->ovf_mask = next_pow2(all * 2) - 1;
    if (c->pod_ovf.cap < (size_t)(c->ovf_mask + 1) * 8) {       // stamped slots start zeroed
        TRY(ensure(c->pod_ovf, (size_t)(c->ovf_mask + 1) * 8));
        HIP_TRY(hipMemsetAsync(c->pod_ovf.p, 0, c->pod_ovf.cap, s));
    }
    if (n) HIP_TRY(hipMemcpyAsync(dp<uint4>(c->pods) + c->pod_total, rows, (size_t)n * 16, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));             // the caller's rows may be released on return
    c->n_late = n;
    c->pods_ready = false;                        // the next run builds the lookup over every row
    c->pods_delta = false;
    return KDTN_OK;
}

int kdtn_debug_wg_trace(kdtn_ctx* c, uint64_t* out, uint32_t cap) {
    if (!c || !c->traced) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t n = std::min<uint64_t>(cap, (uint64_t)c->nwg * TRACE_WORDS);
    HIP_TRY(hipMemcpy(out, c->trace.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return (int)n;
}

}  // extern "C"

namespace {

// this rank's VxlanManager ops of the last run into vx_ops: [n_del del slots][2 n_add add slots]
int vni_ops_compute(kdtn_ctx* c, uint32_t* nd_out, uint32_t* na_out) {
    const uint32_t need = KDTN_STAGE_RESOLVE | KDTN_STAGE_QDISC;
    if (!c->ran || (c->last_stages & need) != need) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "VXLAN ops: need an epoch run with the resolve and qdisc stages");
        return KDTN_EINVAL;
    }
    hipStream_t s = c->stream;
    HIP_TRY(hipStreamSynchronize(s));                 // counts of the run (h_misc)
    TRY(counts_fresh(c));
    const uint32_t nd = c->h_misc[1], na = c->h_misc[3];
    if (2ull * na + nd + c->V >= 0x7FFFFFFFull) return KDTN_EINVAL;
    TRY(ensure(c->vx_ops, ((size_t)nd + 2ull * na) * 16));
    VniOpsIn f{ReachIn{dp<uint32_t>(c->del_off), dp<uint4>(c->del_res), dp<uint32_t>(c->add_off), dp<uint4>(c->add_res),
                       dp<uint2>(c->add_qdisc), dp<uint32_t>(c->upd_off), dp<uint4>(c->upd_res), c->T, 0u},
               dp<uint32_t>(c->t_src), dp<uint32_t>(c->t_netns), dp<uint4>(c->pods), nd, na};
    TRY(ensure(c->vx_cut, (size_t)c->T * 8 + 8));
    uint32_t* cut = dp<uint32_t>(c->vx_cut);
    if (c->T) {
        HIP_TRY(hipMemsetAsync(cut, 0xFF, (size_t)c->T * 8, s));
        if (nd + na) {
            k_vni_cuts<<<nblocks((uint64_t)nd + na), BLOCK, 0, s>>>(f, cut);
            k_vni_ops<<<nblocks((uint64_t)nd + na), BLOCK, 0, s>>>(f, cut, dp<uint4>(c->vx_ops));
        }
    }
    HIP_TRY(hipGetLastError());
    *nd_out = nd;
    *na_out = na;
    return KDTN_OK;
}

// Every rank's ops in rank order, [all del slots][all add slots], into vx_gops over RCCL:
// the per-rank counts first, then one all-gather of lists padded to the largest rank's.
int vni_ops_gather_rccl(kdtn_ctx* c, uint32_t nd, uint32_t na, uint64_t* gd, uint64_t* ga) {
    hipStream_t s = c->stream;
    const int G = c->nranks;
    TRY(ensure(c->vx_cnt, (size_t)G * 8 + 16));
    uint32_t* cnt = dp<uint32_t>(c->vx_cnt);
    const uint32_t mine[2] = {nd, na};
    HIP_TRY(hipMemcpyAsync(cnt + 2 * c->rank, mine, 8, hipMemcpyHostToDevice, s));
    ncclResult_t r = ncclAllGather(cnt + 2 * c->rank, cnt, 2, ncclUint32, c->comm, s);
    if (r != ncclSuccess) {
        std::snprintf(g_last_error, sizeof(g_last_error), "ncclAllGather (VXLAN op counts): %s", ncclGetErrorString(r));
        return KDTN_EIO;
    }
    std::vector<uint32_t> h(2 * (size_t)G);
    HIP_TRY(hipMemcpyAsync(h.data(), cnt, 8 * (size_t)G, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t md = 0, ma = 0;
    for (int g = 0; g < G; ++g) {
        md = std::max(md, h[2 * g]);
        ma = std::max(ma, h[2 * g + 1]);
    }
    const size_t row = (size_t)md + 2ull * ma;                 // ops per rank, padded
    TRY(ensure(c->vx_send, row * 16 + 16));
    TRY(ensure(c->vx_recv, row * G * 16 + 16));
    TRY(ensure(c->vx_gops, row * G * 16 + 16));
    uint8_t* send = dp<uint8_t>(c->vx_send);
    HIP_TRY(hipMemsetAsync(send, 0, row * 16, s));             // VOP_NONE padding
    if (nd) HIP_TRY(hipMemcpyAsync(send, c->vx_ops.p, (size_t)nd * 16, hipMemcpyDeviceToDevice, s));
    if (na)
        HIP_TRY(hipMemcpyAsync(send + (size_t)md * 16, dp<uint8_t>(c->vx_ops) + (size_t)nd * 16, 2ull * na * 16,
                               hipMemcpyDeviceToDevice, s));
    if (row) {
        r = ncclAllGather(send, c->vx_recv.p, row * 4, ncclUint32, c->comm, s);
        if (r != ncclSuccess) {
            std::snprintf(g_last_error, sizeof(g_last_error), "ncclAllGather (VXLAN ops): %s", ncclGetErrorString(r));
            return KDTN_EIO;
        }
        uint8_t* g = dp<uint8_t>(c->vx_gops);
        const uint8_t* rv = dp<uint8_t>(c->vx_recv);
        if (md) HIP_TRY(hipMemcpy2DAsync(g, (size_t)md * 16, rv, row * 16, (size_t)md * 16, G, hipMemcpyDeviceToDevice, s));
        if (ma)
            HIP_TRY(hipMemcpy2DAsync(g + (size_t)md * G * 16, 2ull * ma * 16, rv + (size_t)md * 16, row * 16,
                                     2ull * ma * 16, G, hipMemcpyDeviceToDevice, s));
    }
    *gd = (uint64_t)md * G;
    *ga = 2ull * ma * G;
    return KDTN_OK;
}

}  // namespace

extern "C" {

int kdtn_vni_ops_export(kdtn_ctx* c, kdtn_vni_op* dels, uint32_t del_cap, kdtn_vni_op* adds, uint32_t add_cap,
                        uint32_t* n_del, uint32_t* n_add) {
    if (!c || !n_del || !n_add) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t nd = 0, na = 0;
    TRY(vni_ops_compute(c, &nd, &na));
    *n_del = nd;
    *n_add = 2 * na;
    if ((dels && nd > del_cap) || (adds && 2 * na > add_cap)) return KDTN_ENOSPC;
    hipStream_t s = c->stream;
    if (dels && nd) HIP_TRY(hipMemcpyAsync(dels, c->vx_ops.p, (size_t)nd * 16, hipMemcpyDeviceToHost, s));
    if (adds && na)
        HIP_TRY(hipMemcpyAsync(adds, dp<uint8_t>(c->vx_ops) + (size_t)nd * 16, 2ull * na * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}

int kdtn_vni_ops_import(kdtn_ctx* c, const kdtn_vni_op* dels, uint32_t n_del, const kdtn_vni_op* adds, uint32_t n_add) {
    if (!c || !c->ran || (n_del && !dels) || (n_add && !adds) || (uint64_t)n_del + n_add + c->V >= 0x7FFFFFFFull)
        return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    TRY(ensure(c->vx_gops, ((size_t)n_del + n_add) * 16 + 16));
    if (n_del) HIP_TRY(hipMemcpyAsync(c->vx_gops.p, dels, (size_t)n_del * 16, hipMemcpyHostToDevice, s));
    if (n_add)
        HIP_TRY(hipMemcpyAsync(dp<uint8_t>(c->vx_gops) + (size_t)n_del * 16, adds, (size_t)n_add * 16,
                               hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->vx_gd = n_del;
    c->vx_ga = n_add;
    c->vx_imported = true;
    return KDTN_OK;
}

int kdtn_epoch_vni_apply(kdtn_ctx* c, kdtn_vni_state* out) {
    if (!c || !c->ran) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const bool host_xchg = c->nranks > 1 && !c->comm;
    if (host_xchg && !c->vx_imported) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "host transport: kdtn_vni_ops_import every rank's VXLAN ops before kdtn_epoch_vni_apply");
        return KDTN_EINVAL;
    }
    if (c->nranks > 1 && !c->pods_rank_major && !host_xchg) {
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_epoch_vni_apply: sharded ingest contexts use the host transport");
        return KDTN_EINVAL;
    }
    stage_begin(c);
    const uint32_t V = c->V;
    uint64_t nd_all = 0, n_ops = 0;
    const uint4* ops = nullptr;
    if (!host_xchg) {
        uint32_t nd = 0, na = 0;
        TRY(vni_ops_compute(c, &nd, &na));
        if (c->nranks > 1) {
            TRY(vni_ops_gather_rccl(c, nd, na, &nd_all, &n_ops));
            ops = dp<uint4>(c->vx_gops);
        } else {
            nd_all = nd;
            n_ops = 2ull * na;
            ops = dp<uint4>(c->vx_ops);
        }
    } else {
        nd_all = c->vx_gd;
        n_ops = c->vx_ga;
        ops = dp<uint4>(c->vx_gops);
    }
    const uint64_t n_ext = n_ops + V;
    if (n_ext + nd_all >= 0x7FFFFFFFull) return KDTN_EINVAL;
    TRY(ensure(c->vx_dead, (size_t)V + 16));
    const uint4* ents = dp<uint4>(c->v_ents);
    uint8_t* dead = dp<uint8_t>(c->vx_dead);
    if (V) {                                          // the run built the snapshot table
        k_vni_shadow<<<nblocks(V), BLOCK, 0, s>>>(ents, V, dp<uint32_t>(c->v_slots), c->vni_mask, dead);
        if (nd_all) k_vni_del<<<nblocks(nd_all), BLOCK, 0, s>>>(ops, (uint32_t)nd_all, ents, dp<uint32_t>(c->v_slots),
                                                                c->vni_mask, dead);
    }
    timer_mark(c, "vni_ops");
    const uint32_t mask = next_pow2(n_ext * 2) - 1;
    TRY(ensure(c->vx_slots, ((size_t)mask + 1) * 4));
    HIP_TRY(hipMemsetAsync(c->vx_slots.p, 0xFF, ((size_t)mask + 1) * 4, s));
    uint32_t* slots = dp<uint32_t>(c->vx_slots);
    const uint4* aops = ops + nd_all;
    const uint32_t nb = nblocks(n_ext, SCAN_CHUNK);
    TRY(ensure(c->vx_part, (size_t)nb * 8 + 8));
    TRY(ensure(c->vx_node, (size_t)n_ext * 4));
    TRY(ensure(c->vx_vni, (size_t)n_ext * 4));
    TRY(ensure(c->vx_netns, (size_t)n_ext * 4));
    TRY(ensure(c->vx_vis, (size_t)n_ext + 16));
    uint32_t* n_out = dp<uint32_t>(c->misc) + MISC_VNI_N;
    HIP_TRY(hipMemsetAsync(n_out, 0, 4, s));
    if (n_ext) {
        k_vni_insert<<<nblocks(n_ext), BLOCK, 0, s>>>(aops, (uint32_t)n_ops, ents, dead, V, slots, mask);
        uint8_t* vis = dp<uint8_t>(c->vx_vis);
        k_vni_vis_count<<<nb, BLOCK, 0, s>>>(aops, (uint32_t)n_ops, ents, dead, V, slots, mask, vis,
                                            dp<uint64_t>(c->vx_part));
        k_scan_top<<<1, SCAN_TOP_BLOCK, 0, s>>>(dp<uint64_t>(c->vx_part), nb);
        k_vni_vis_write<<<nb, BLOCK, 0, s>>>(aops, (uint32_t)n_ops, ents, dead, V, vis, dp<uint64_t>(c->vx_part),
                                            dp<uint32_t>(c->vx_node), dp<int32_t>(c->vx_vni), dp<uint32_t>(c->vx_netns),
                                            n_out);
    }
    HIP_TRY(hipGetLastError());
    timer_mark(c, "vni_map");
    // keys whose result depends on the reference's goroutine order (kdtn_vni_contested)
    const uint32_t dmask = nd_all ? next_pow2(nd_all * 2) - 1 : 0u;
    const uint32_t nbf = nblocks(n_ops + 1, SCAN_CHUNK);
    TRY(ensure(c->vx_flag, (size_t)n_ops * 4 + 16));
    TRY(ensure(c->vx_dkeys, ((size_t)dmask + 1) * 16));
    TRY(ensure(c->vx_dused, ((size_t)dmask + 1) * 4));
    TRY(ensure(c->vx_cpos, ((size_t)n_ops + 1) * 8));
    TRY(ensure(c->vx_cpart, (size_t)nbf * 8 + 8));
    TRY(ensure(c->vx_cnode, (size_t)n_ops * 4 + 16));
    TRY(ensure(c->vx_cvni, (size_t)n_ops * 4 + 16));
    HIP_TRY(hipMemsetAsync(c->vx_flag.p, 0, (size_t)n_ops * 4 + 16, s));
    HIP_TRY(hipMemsetAsync(c->vx_dused.p, 0, ((size_t)dmask + 1) * 4, s));
    if (nd_all) k_vni_dtab_insert<<<nblocks(nd_all), BLOCK, 0, s>>>(ops, (uint32_t)nd_all, dp<uint4>(c->vx_dkeys),
                                                                     dp<uint32_t>(c->vx_dused), dmask);
    if (n_ops) k_vni_contest<<<nblocks(n_ops), BLOCK, 0, s>>>(aops, (uint32_t)n_ops, ents, dead, slots, mask,
                                                             dp<uint4>(c->vx_dkeys), dp<uint32_t>(c->vx_dused),
                                                             nd_all ? dmask : 0u, dp<uint32_t>(c->vx_flag));
    k_scan_partial<<<nbf, BLOCK, 0, s>>>(dp<uint32_t>(c->vx_flag), (uint32_t)n_ops, dp<uint64_t>(c->vx_cpart));
    k_scan_top<<<1, SCAN_TOP_BLOCK, 0, s>>>(dp<uint64_t>(c->vx_cpart), nbf);
    k_scan_final<<<nbf, BLOCK, 0, s>>>(dp<uint32_t>(c->vx_flag), (uint32_t)n_ops, dp<uint64_t>(c->vx_cpart),
                                       dp<uint64_t>(c->vx_cpos));
    if (n_ops) k_vni_contest_write<<<nblocks(n_ops), BLOCK, 0, s>>>(aops, dp<uint32_t>(c->vx_flag),
                                                                   dp<uint64_t>(c->vx_cpos), (uint32_t)n_ops,
                                                                   dp<uint32_t>(c->vx_cnode), dp<int32_t>(c->vx_cvni));
    HIP_TRY(hipGetLastError());
    timer_mark(c, "vni_contested");
    HIP_TRY(hipMemcpyAsync(c->h_misc + 5, n_out, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c->h_misc + 6, dp<uint64_t>(c->vx_cpos) + n_ops, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t n = c->h_misc[5];
    c->vx_ncont = c->h_misc[6];
    c->vx_contest_ok = true;
    // the new map becomes the resident one (the next upload's KDTN_VNI_RESIDENT); this upload's
    // snapshot (v_*, v_ents, V) stays as it is, so a re-run or a second apply of this upload
    // sees the same epoch-start map
    std::swap(c->r_node, c->vx_node);
    std::swap(c->r_vni, c->vx_vni);
    std::swap(c->r_netns, c->vx_netns);
    c->vres_ok = true;
    c->vres_in_r = true;
    c->vres_n = n;
    c->vres_D = c->D;
    return out ? kdtn_vni_download(c, out) : KDTN_OK;
}

int kdtn_vni_contested(kdtn_ctx* c, uint32_t* node, int32_t* vni, uint32_t cap, uint32_t* n) {
    if (!c || !n || !c->vx_contest_ok) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    *n = c->vx_ncont;
    if (!node && !vni) return KDTN_OK;
    if (c->vx_ncont > cap) return KDTN_ENOSPC;
    hipStream_t s = c->stream;
    if (c->vx_ncont && node)
        HIP_TRY(hipMemcpyAsync(node, c->vx_cnode.p, (size_t)c->vx_ncont * 4, hipMemcpyDeviceToHost, s));
    if (c->vx_ncont && vni) HIP_TRY(hipMemcpyAsync(vni, c->vx_cvni.p, (size_t)c->vx_ncont * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}

int kdtn_vni_download(kdtn_ctx* c, kdtn_vni_state* out) {
    if (!c || !out) return KDTN_EINVAL;
    if (!c->vres_ok) {
        out->n = 0;
        return KDTN_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = c->vres_n;
    out->n = n;
    if (!out->node && !out->vni && !out->net_ns) return KDTN_OK;
    if (n > out->cap) return KDTN_ENOSPC;
    hipStream_t s = c->stream;
    DevBuf& bn = c->vres_in_r ? c->r_node : c->v_node;
    DevBuf& bv = c->vres_in_r ? c->r_vni : c->v_vni;
    DevBuf& bs = c->vres_in_r ? c->r_netns : c->v_netns;
    if (n && out->node) HIP_TRY(hipMemcpyAsync(out->node, bn.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (n && out->vni) HIP_TRY(hipMemcpyAsync(out->vni, bv.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (n && out->net_ns) HIP_TRY(hipMemcpyAsync(out->net_ns, bs.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}
}  // extern "C"
