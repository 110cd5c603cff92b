// kdtn_engine_out.hip — the output stages of the C-ABI: wire encoding, RemotePod fan-out and messages,
// tc argv, status write-back bodies, and their downloads
// (host side of libkdtn.so; the context and the shared helpers are in kdtn_engine.h)
#include "kdtn_engine.h"

extern "C" {

int kdtn_epoch_encode(kdtn_ctx* c, uint64_t* n_bytes) {
    if (!c || !c->ran) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRY(counts_fresh(c));
    hipStream_t s = c->stream;
    const uint32_t nd = c->h_misc[1], nu = c->h_misc[2], na = c->h_misc[3];
    const uint32_t T = c->T;
    const uint64_t ne = (uint64_t)nd + na + nu;
    if (ne > 0xFFFFFFFFull || 3ull * T + 1 > 0xFFFFFFFFull) return KDTN_EINVAL;
    TRY(ensure(c->w_rel, (size_t)ne * 4 + 16));                 // entry sizes
    TRY(ensure(c->w_topo, (size_t)ne * 4 + 16));
    TRY(ensure(c->w_size, ((size_t)ne + 1) * 8));                // entry offsets (u64)
    const size_t err_bytes = align_up(((size_t)T + 1) * 4, 16);  // err[T]: a batch over 4 GiB
    TRY(ensure(c->w_err, err_bytes));
    TRY(ensure(c->w_off, ((size_t)3 * T + 1) * 8));
    const uint32_t nb = nblocks(ne + 1, SCAN_CHUNK);
    TRY(ensure(c->w_part, (size_t)nb * 8 + 16));
    stage_begin(c);
    TRY(str_tables(c));
    timer_mark(c, "wire_strtab");
    HIP_TRY(hipMemsetAsync(c->w_err.p, 0, err_bytes, s));
    WireIn w{};
    w.kd = str_tab_kd(c);
    w.pd = str_tab_pd(c);
    TRY(list_coarse(c));
    for (int l = 0; l < 3; ++l) w.coarse[l] = dp<uint32_t>(c->lc[l]);
    w.t_name = dp<uint32_t>(c->t_name);
    w.t_src = dp<uint32_t>(c->t_src);
    w.t_netns = dp<uint32_t>(c->t_netns);
    w.t_ns = dp<uint32_t>(c->t_ns);
    w.list_off[0] = dp<uint32_t>(c->del_off);
    w.list_off[1] = dp<uint32_t>(c->add_off);
    w.list_off[2] = dp<uint32_t>(c->upd_off);
    w.list_idx[0] = dp<uint32_t>(c->del_idx);
    w.list_idx[1] = dp<uint32_t>(c->add_idx);
    w.list_idx[2] = dp<uint32_t>(c->upd_idx);
    w.list_base[0] = 0;
    w.list_base[1] = nd;
    w.list_base[2] = nd + na;
    w.n_entries = (uint32_t)ne;
    w.T = T;
    TRY(ensure(c->w_pinfo, (size_t)na * 8 + 16));
    WireWork wk{dp<uint32_t>(c->w_rel), dp<uint32_t>(c->w_topo), dp<uint64_t>(c->w_size), dp<uint32_t>(c->w_err),
                dp<uint64_t>(c->w_off), dp<uint64_t>(c->w_pinfo)};
    uint64_t total = 0;
    uint32_t big = 0;
    {   // sizes, one scan, then the writer (a single pass with a look-back scan measured slower:
        // 2.85 ms vs 0.79 + 0.14 + 1.78 ms on config 2, profiles/r03g_stages.json)
        if (ne) k_wire_entry_sizes<<<nblocks(ne), BLOCK, 0, s>>>(w, c->real.view, c->des.view, wk);
        timer_mark(c, "wire_sizes");
        k_wire_scan_partial<<<nb, BLOCK, 0, s>>>(w, wk, dp<uint64_t>(c->w_part));
        k_scan_top<<<1, SCAN_TOP_BLOCK, 0, s>>>(dp<uint64_t>(c->w_part), nb);
        k_wire_scan_final<<<nb, BLOCK, 0, s>>>(w, wk, dp<uint64_t>(c->w_part));
        k_wire_batch_off<<<nblocks((uint64_t)3 * T + 1), BLOCK, 0, s>>>(w, wk);
        timer_mark(c, "wire_scan");
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&total, dp<uint64_t>(c->w_size) + ne, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&big, dp<uint32_t>(c->w_err) + T, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!big) TRY(ensure(c->w_arena, (size_t)total + 64));   // (WSink::copy reads past a range)
        timer_mark(c, "wire_host_sync");                // the arena size crosses to the host
        if (ne && !big) k_wire_write<<<nblocks(ne), BLOCK, 0, s>>>(w, c->real.view, c->des.view, wk, dp<uint8_t>(c->w_arena));
        timer_mark(c, "wire_write");
    }
    if (big) {
        std::snprintf(g_last_error, sizeof(g_last_error), "a LinksBatchQuery of more than 4 GiB");
        return KDTN_EINVAL;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    c->w_bytes = total;
    c->encoded = true;
    if (n_bytes) *n_bytes = total;
    return KDTN_OK;
}

int kdtn_epoch_download_wire(kdtn_ctx* c, kdtn_wire* o) {
    if (!c || !o || !c->encoded) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    o->n_bytes = c->w_bytes;
    if (o->bytes && c->w_bytes > o->cap) return KDTN_ENOSPC;
    hipStream_t s = c->stream;
    if (o->bytes && c->w_bytes)
        HIP_TRY(hipMemcpyAsync(o->bytes, c->w_arena.p, c->w_bytes, hipMemcpyDeviceToHost, s));
    if (o->off) HIP_TRY(hipMemcpyAsync(o->off, c->w_off.p, ((size_t)3 * c->T + 1) * 8, hipMemcpyDeviceToHost, s));
    if (o->err && c->T) HIP_TRY(hipMemcpyAsync(o->err, c->w_err.p, (size_t)c->T * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}

}  // extern "C"

namespace {

// The RemotePod fan-out of the last run (k_reach, node compaction, stable grouping) into
// f_nodes / f_idx / f_base; cached until the next run.
int fanout_compute(kdtn_ctx* c) {
    if (c->fan_valid) return KDTN_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRY(counts_fresh(c));
    hipStream_t s = c->stream;
    const uint32_t na = c->h_misc[3], D = c->D;
    const uint32_t nw = (D + 3) / 4;                          // destination-daemon flag bytes (words of 4)
    TRY(ensure(c->f_mark, (size_t)nw * 4 + 16));
    HIP_TRY(hipMemsetAsync(c->f_mark.p, 0, (size_t)nw * 4, s));
    const uint32_t nchunks = nblocks(na, FAN_CHUNK);
    const uint32_t nbd = nblocks(nw, SCAN_CHUNK);
    TRY(ensure(c->f_node_idx, (size_t)D * 4));
    TRY(ensure(c->f_nodes, (size_t)FAN_NODE_CAP * 4 + 16));
    TRY(ensure(c->f_part, (size_t)nbd * 8 + 16));
    TRY(ensure(c->f_idx, (size_t)na * 4 + 16));
    TRY(ensure(c->f_inv, (size_t)na * 4 + 16));
    uint32_t* misc = dp<uint32_t>(c->misc);
    uint32_t* n_nodes = misc + MISC_FAN_NODES;
    TRY(run_reach(c, dp<uint32_t>(c->f_mark), 0));
    const FanIn f{dp<uint32_t>(c->add_off), dp<uint4>(c->add_res), dp<uint2>(c->add_qdisc), c->T, na, 0u,
                  dp<uint32_t>(c->f_node)};            // (after run_reach: it sizes f_node)
    k_fan_nodes_count<<<nbd, BLOCK, 0, s>>>(dp<uint32_t>(c->f_mark), nw, dp<uint64_t>(c->f_part));
    k_scan_top<<<1, SCAN_TOP_BLOCK, 0, s>>>(dp<uint64_t>(c->f_part), nbd);
    k_fan_nodes_write<<<nbd, BLOCK, 0, s>>>(dp<uint32_t>(c->f_mark), nw, dp<uint64_t>(c->f_part),
                                           dp<uint32_t>(c->f_node_idx), dp<uint32_t>(c->f_nodes), n_nodes);
    timer_mark(c, "fanout_nodes");
    uint32_t nn = 0;
    HIP_TRY(hipMemcpyAsync(&nn, n_nodes, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nn > (uint32_t)FAN_NODE_CAP) {
        std::snprintf(g_last_error, sizeof(g_last_error), "fan-out over %u daemons (cap %d)", nn, FAN_NODE_CAP);
        return KDTN_EINVAL;
    }
    timer_mark(c, "fanout_host_sync");
    const uint32_t ncells = nn * nchunks;
    TRY(ensure(c->f_counts, (size_t)ncells * 4 + 16));
    TRY(ensure(c->f_base, ((size_t)ncells + 1) * 8 + 16));
    uint32_t nsend = 0;
    if (na && nn) {
        const size_t lds = (size_t)nn * 4;
        k_fan_count<<<nchunks, 64, lds, s>>>(f, dp<uint8_t>(c->f_send), dp<uint32_t>(c->f_node_idx), n_nodes,
                                           dp<uint32_t>(c->f_counts), nchunks);
        TRY(scan_u32(c, dp<uint32_t>(c->f_counts), ncells, dp<uint64_t>(c->f_base)));
        k_fan_scatter<<<nchunks, 64, lds, s>>>(f, dp<uint8_t>(c->f_send), dp<uint32_t>(c->f_node_idx), n_nodes,
                                             dp<uint64_t>(c->f_base), nchunks, dp<uint32_t>(c->f_idx),
                                             dp<uint32_t>(c->f_inv));
        HIP_TRY(hipGetLastError());
        uint64_t tot = 0;
        HIP_TRY(hipMemcpyAsync(&tot, dp<uint64_t>(c->f_base) + ncells, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        nsend = (uint32_t)tot;
    }
    timer_mark(c, "fanout_group");
    c->fan_nn = nn;
    c->fan_nsend = nsend;
    c->fan_valid = true;
    return KDTN_OK;
}

}  // namespace

namespace kdtn {
namespace host {

bool fanout_stages_ok(const kdtn_ctx* c) {
    return (c->last_stages & (KDTN_STAGE_RESOLVE | KDTN_STAGE_QDISC)) == (KDTN_STAGE_RESOLVE | KDTN_STAGE_QDISC);
}

}  // namespace host
}  // namespace kdtn

extern "C" {

int kdtn_epoch_fanout(kdtn_ctx* c, kdtn_fanout* o) {
    if (!c || !o || !c->ran) return KDTN_EINVAL;
    if (!fanout_stages_ok(c)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    TRY(counts_fresh(c));
    hipStream_t s = c->stream;
    stage_begin(c);
    c->fan_valid = false;                                    // recomputed per call (timed stage)
    TRY(fanout_compute(c));
    const uint32_t nn = c->fan_nn, nsend = c->fan_nsend, na = c->h_misc[3];
    const uint32_t nchunks = nblocks(na, FAN_CHUNK);
    o->n_nodes = nn;
    o->n_send = nsend;
    if (nn > o->node_cap || nsend > o->idx_cap) return KDTN_ENOSPC;
    if (o->node && nn) HIP_TRY(hipMemcpyAsync(o->node, c->f_nodes.p, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
    if (o->idx && nsend) HIP_TRY(hipMemcpyAsync(o->idx, c->f_idx.p, (size_t)nsend * 4, hipMemcpyDeviceToHost, s));
    if (o->off) {
        // off[k] = base of (node k, chunk 0): strided 8-B reads of the scanned (node, chunk) matrix
        std::vector<uint64_t> b(nn ? nn : 1);
        if (nn && na)
            HIP_TRY(hipMemcpy2DAsync(b.data(), 8, dp<uint64_t>(c->f_base), (size_t)nchunks * 8, 8, nn,
                                     hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t k = 0; k < nn; ++k) o->off[k] = na ? (uint32_t)b[k] : 0u;
        o->off[nn] = nsend;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}

int kdtn_epoch_remote_encode(kdtn_ctx* c, kdtn_remote_info* info) {
    if (!c || !c->ran || !fanout_stages_ok(c)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    TRY(counts_fresh(c));
    hipStream_t s = c->stream;
    stage_begin(c);
    TRY(fanout_compute(c));                                  // f_idx (fan-out order) and f_send (reach)
    const uint32_t na = c->h_misc[3], nr = c->fan_nsend;
    // physical peers' local Updates: reached PHYSICAL adds whose MakeVeth passed, add-list order
    TRY(ensure(c->rp_flag, (size_t)na * 4 + 16));
    TRY(ensure(c->rp_pos, ((size_t)na + 1) * 8));
    TRY(ensure(c->rp_phys, (size_t)na * 4 + 16));
    if (na) k_remote_phys_flags<<<nblocks(na), BLOCK, 0, s>>>(dp<uint8_t>(c->f_send), dp<uint4>(c->add_res), na,
                                                              dp<uint32_t>(c->rp_flag));
    TRY(scan_u32(c, dp<uint32_t>(c->rp_flag), na, dp<uint64_t>(c->rp_pos)));
    if (na) k_remote_phys_scatter<<<nblocks(na), BLOCK, 0, s>>>(dp<uint32_t>(c->rp_flag), dp<uint64_t>(c->rp_pos), na,
                                                                dp<uint32_t>(c->rp_phys));
    uint64_t nphys = 0;
    HIP_TRY(hipMemcpyAsync(&nphys, dp<uint64_t>(c->rp_pos) + na, 8, hipMemcpyDeviceToHost, s));
    // UTF-8 validity of every dictionary string (proto.Marshal fails on invalid strings)
    TRY(str_tables(c));

    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "remote_select");
    const uint64_t n = (uint64_t)nr + nphys;
    if (n >= 0xFFFFFFFFull) return KDTN_EINVAL;
    RemoteIn r{};
    r.kd = str_tab_kd(c);
    r.pd = str_tab_pd(c);
    r.kd_offs = dp<uint32_t>(c->kd_offs);
    if (c->encoded) {                        // the run's wire encoding: its properties fields
        r.w_pinfo = dp<uint64_t>(c->w_pinfo);
        r.w_pos = dp<uint64_t>(c->w_size);
        r.w_arena = dp<uint8_t>(c->w_arena);
        r.w_err = dp<uint32_t>(c->w_err);
        r.w_nd = c->h_misc[1];
    }
    TRY(list_coarse(c));
    r.add_coarse = dp<uint32_t>(c->lc[1]);
    r.t_ns = dp<uint32_t>(c->t_ns);
    r.t_src = dp<uint32_t>(c->t_src);
    r.t_netns = dp<uint32_t>(c->t_netns);
    r.add_off = dp<uint32_t>(c->add_off);
    r.add_idx = dp<uint32_t>(c->add_idx);
    r.add_res = dp<uint4>(c->add_res);
    r.add_qdisc = dp<uint2>(c->add_qdisc);
    r.pods = dp<uint4>(c->pods);
    r.rem_idx = dp<uint32_t>(c->f_idx);
    r.phys_idx = dp<uint32_t>(c->rp_phys);
    r.send = dp<uint8_t>(c->f_send);
    r.phys_flag = dp<uint32_t>(c->rp_flag);
    r.phys_pos = dp<uint64_t>(c->rp_pos);
    r.rem_inv = dp<uint32_t>(c->f_inv);
    r.N = c->des.view;
    r.n_msgs = (uint32_t)n;
    r.n_remote = nr;
    r.T = c->T;
    r.n_add = na;
    TRY(ensure(c->rp_msz, (size_t)n * 4 + 16));
    TRY(ensure(c->rp_tsz, (size_t)n * 4 + 16));
    TRY(ensure(c->rp_moff, (n + 1) * 8));
    TRY(ensure(c->rp_toff, (n + 1) * 8));
    // sizes per add entry (coalesced columns), stored at the message indices
    if (n) k_remote_sizes<<<nblocks(na), BLOCK, 0, s>>>(r, dp<uint32_t>(c->rp_msz), dp<uint32_t>(c->rp_tsz));
    TRY(scan_u32(c, dp<uint32_t>(c->rp_msz), (uint32_t)n, dp<uint64_t>(c->rp_moff)));   // message offsets
    TRY(scan_u32(c, dp<uint32_t>(c->rp_tsz), (uint32_t)n, dp<uint64_t>(c->rp_toff)));   // tc argv offsets
    timer_mark(c, "remote_sizes");
    HIP_TRY(hipGetLastError());
    uint64_t tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(tot, dp<uint64_t>(c->rp_moff) + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(tot + 1, dp<uint64_t>(c->rp_toff) + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    TRY(ensure(c->rp_arena, (size_t)tot[0] + 16));
    TRY(ensure(c->rp_tc, (size_t)tot[1] + 16));
    timer_mark(c, "remote_host_sync");
    if (n) {
        k_remote_write<<<nblocks(na), BLOCK, 0, s>>>(r, dp<uint64_t>(c->rp_moff), dp<uint8_t>(c->rp_arena));
        timer_mark(c, "remote_write");
        if (nr) k_tc_remote_write<<<nblocks(na), BLOCK, 0, s>>>(r, dp<uint64_t>(c->rp_toff), dp<uint8_t>(c->rp_tc));
        timer_mark(c, "remote_tc_write");
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    c->rp_n = (uint32_t)n;
    c->rp_nr = nr;
    c->rp_bytes = tot[0];
    c->rp_tc_bytes = tot[1];
    c->rp_done = true;
    if (info) {
        info->n_msgs = c->rp_n;
        info->n_remote = nr;
        info->n_bytes = tot[0];
        info->n_tc_bytes = tot[1];
    }
    return KDTN_OK;
}

int kdtn_epoch_download_remote(kdtn_ctx* c, kdtn_remote_pods* o) {
    if (!c || !o || !c->rp_done) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if ((o->bytes && c->rp_bytes > o->cap) || (o->tc_bytes && c->rp_tc_bytes > o->tc_cap) ||
        ((o->off || o->entry || o->tc_off) && c->rp_n > o->msg_cap))
        return KDTN_ENOSPC;
    hipStream_t s = c->stream;
    const size_t n = c->rp_n, nr = c->rp_nr;
    if (o->bytes && c->rp_bytes) HIP_TRY(hipMemcpyAsync(o->bytes, c->rp_arena.p, c->rp_bytes, hipMemcpyDeviceToHost, s));
    if (o->tc_bytes && c->rp_tc_bytes)
        HIP_TRY(hipMemcpyAsync(o->tc_bytes, c->rp_tc.p, c->rp_tc_bytes, hipMemcpyDeviceToHost, s));
    if (o->off) HIP_TRY(hipMemcpyAsync(o->off, c->rp_moff.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (o->tc_off) HIP_TRY(hipMemcpyAsync(o->tc_off, c->rp_toff.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (o->entry) {
        if (nr) HIP_TRY(hipMemcpyAsync(o->entry, c->f_idx.p, nr * 4, hipMemcpyDeviceToHost, s));
        if (n > nr) HIP_TRY(hipMemcpyAsync(o->entry + nr, c->rp_phys.p, (n - nr) * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}

int kdtn_epoch_tc(kdtn_ctx* c, uint64_t* n_bytes) {
    if (!c || !c->ran) return KDTN_EINVAL;
    if (!fanout_stages_ok(c)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRY(counts_fresh(c));
    hipStream_t s = c->stream;
    const uint32_t nu = c->h_misc[2], na = c->h_misc[3];
    const uint64_t n = 2ull * na + nu;                   // command slots: 2 per add entry, 1 per update
    if (n >= 0xFFFFFFFFull) return KDTN_EINVAL;
    TRY(ensure(c->tc_size, (size_t)n * 4 + 16));
    TRY(ensure(c->tc_off, ((size_t)n + 1) * 8));
    stage_begin(c);
    TRY(run_reach(c, nullptr, 0));
    TRY(str_tables(c));                                   // the interface names' entries
    timer_mark(c, "tc_reach");
    TcIn w{c->des.view, dp<uint8_t>(c->f_send), dp<uint8_t>(c->f_reach_upd), dp<uint32_t>(c->add_idx),
           dp<uint32_t>(c->upd_idx), dp<uint4>(c->add_res),
           dp<uint4>(c->upd_res), dp<uint2>(c->add_qdisc), dp<uint2>(c->upd_qdisc), str_tab_kd(c), na, nu};
    if (n) k_tc_sizes<<<nblocks(n), BLOCK, 0, s>>>(w, dp<uint32_t>(c->tc_size));
    uint64_t total = 0;
    TRY(scan_arena(c, dp<uint32_t>(c->tc_size), (uint32_t)n, dp<uint64_t>(c->tc_off), "tc_sizes", c->tc_arena, 16,
                   &total));
    timer_mark(c, "tc_host_sync");
    if (n) k_tc_write<<<nblocks(n), BLOCK, 0, s>>>(w, dp<uint64_t>(c->tc_off), dp<uint8_t>(c->tc_arena));
    timer_mark(c, "tc_write");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    c->tc_bytes = total;
    c->tc_n = (uint32_t)n;
    c->tc_done = true;
    if (n_bytes) *n_bytes = total;
    return KDTN_OK;
}

int kdtn_epoch_download_tc(kdtn_ctx* c, kdtn_tc_argv* o) {
    if (!c || !o || !c->tc_done) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    o->n_bytes = c->tc_bytes;
    if (o->bytes && c->tc_bytes > o->cap) return KDTN_ENOSPC;
    if (o->bytes && c->tc_bytes)
        HIP_TRY(hipMemcpyAsync(o->bytes, c->tc_arena.p, c->tc_bytes, hipMemcpyDeviceToHost, c->stream));
    if (o->off) HIP_TRY(hipMemcpyAsync(o->off, c->tc_off.p, ((size_t)c->tc_n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KDTN_OK;
}

int kdtn_epoch_status_encode(kdtn_ctx* c, const uint8_t* mask, kdtn_status_info* info) {
    if (!c || !c->ran) return KDTN_EINVAL;
    if (!mask && !fanout_stages_ok(c)) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "kdtn_epoch_status_encode without a mask needs a run with the resolve and qdisc stages");
        return KDTN_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRY(counts_fresh(c));
    hipStream_t s = c->stream;
    const uint32_t T = c->T, N = c->des.n;
    TRY(ensure(c->sj_sel, (size_t)T + 16));
    TRY(ensure(c->sj_tsz, (size_t)T * 4 + 16));
    TRY(ensure(c->sj_tpos, ((size_t)T + 1) * 8));
    TRY(ensure(c->sj_rsz, (size_t)N * 4 + 16));
    TRY(ensure(c->sj_rtopo, (size_t)N * 4 + 16));
    TRY(ensure(c->sj_rpos, ((size_t)N + 1) * 8));
    TRY(ensure(c->sj_off, ((size_t)T + 1) * 8));
    TRY(ensure(c->sj_tot, ST_TOT_WORDS * 4));
    stage_begin(c);
    TRY(str_tables(c));
    TRY(esc_tables(c));
    timer_mark(c, "status_tables");
    const uint8_t* dmask = nullptr;
    const uint32_t* cut = nullptr;
    if (mask) {
        TRY(upload(c, c->sj_mask, mask, T));
        dmask = dp<uint8_t>(c->sj_mask);
    } else {
        TRY(run_reach(c, nullptr, 0));                      // per-topology first failing entries
        cut = dp<uint32_t>(c->f_cut);
    }
    uint32_t* tot = dp<uint32_t>(c->sj_tot);
    HIP_TRY(hipMemsetAsync(tot, 0, ST_TOT_WORDS * 4, s));
    StatusIn in{c->des.view, topo_view(c), str_tab_kd(c), str_tab_pd(c), dp<uint32_t>(c->kd_offs),
                dp<uint32_t>(c->pd_offs), dp<uint32_t>(c->kd_esc), dp<uint32_t>(c->pd_esc), dp<uint8_t>(c->sj_sel),
                dp<uint32_t>(c->sj_rsz), dp<uint32_t>(c->sj_rtopo), dp<uint64_t>(c->sj_rpos),
                dp<uint32_t>(c->sj_tsz), dp<uint64_t>(c->sj_tpos)};
    if (T)
        k_status_select<<<nblocks(T), BLOCK, 0, s>>>(in.T, dp<uint8_t>(c->action), cut, dmask, dp<uint8_t>(c->sj_sel),
                                                     dp<uint32_t>(c->sj_tsz), tot);
    if (N) k_status_sizes<<<nblocks(N), BLOCK, 0, s>>>(in, dp<uint32_t>(c->sj_rsz), dp<uint32_t>(c->sj_rtopo), tot);
    timer_mark(c, "status_sizes");
    TRY(scan_u32(c, dp<uint32_t>(c->sj_rsz), N, dp<uint64_t>(c->sj_rpos)));
    TRY(scan_u32(c, dp<uint32_t>(c->sj_tsz), T, dp<uint64_t>(c->sj_tpos)));
    k_status_offsets<<<nblocks((uint64_t)T + 1), BLOCK, 0, s>>>(in, dp<uint64_t>(c->sj_off), tot);
    timer_mark(c, "status_scan");
    HIP_TRY(hipGetLastError());
    uint32_t h[ST_TOT_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(h, tot, sizeof h, hipMemcpyDeviceToHost, s));   // the one read: n_written, n_bytes
    HIP_TRY(hipStreamSynchronize(s));
    if (h[ST_TOT_ERR]) {
        std::snprintf(g_last_error, sizeof(g_last_error), "a Link object of 2 GiB or more");
        return KDTN_EINVAL;
    }
    uint64_t total;
    std::memcpy(&total, h + ST_TOT_BYTES, 8);
    uint32_t nw = 0;
    for (int k = 0; k < 32; ++k) nw += h[k];
    TRY(ensure(c->sj_arena, (size_t)total + 64));
    timer_mark(c, "status_host_sync");
    const uint32_t nwb = nblocks(N), ntb = nblocks(T);
    if (nwb + ntb)
        k_status_write<<<nwb + ntb, BLOCK, 0, s>>>(in, dp<uint64_t>(c->sj_off), nwb, dp<uint8_t>(c->sj_arena));
    if (h[ST_TOT_BIG]) k_status_write_big<<<nwb, BLOCK, 0, s>>>(in, dp<uint8_t>(c->sj_arena));
    timer_mark(c, "status_write");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    c->sj_bytes = total;
    c->sj_T = T;
    c->sj_done = true;
    if (info) {
        info->n_written = nw;
        info->reserved = 0;
        info->n_bytes = total;
    }
    return KDTN_OK;
}

int kdtn_epoch_download_status(kdtn_ctx* c, kdtn_status_json* o) {
    if (!c || !o || !c->ran || !c->sj_done) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    o->n_bytes = c->sj_bytes;
    if (o->bytes && c->sj_bytes > o->cap) return KDTN_ENOSPC;
    hipStream_t s = c->stream;
    if (o->bytes && c->sj_bytes) HIP_TRY(hipMemcpyAsync(o->bytes, c->sj_arena.p, c->sj_bytes, hipMemcpyDeviceToHost, s));
    if (o->off) HIP_TRY(hipMemcpyAsync(o->off, c->sj_off.p, ((size_t)c->sj_T + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}

}  // extern "C"
