// kdtn_engine_state.hip — resident epoch state (kdtn_state.hip): commit, delta upload, tables info, the
// resident string indexes and the incremental CR ingest
// (host side of libkdtn.so; the context and the shared helpers are in kdtn_engine.h)
#include "kdtn_engine.h"

namespace {

// Device layout of a delta's arrays (and the host layout that lets them travel in one copy,
// kdtn.engine.pin_delta): topo, src_ip, net_ns, des_off, [prev, ns, name], spec_nil, then the
// references 4-B aligned.
struct DeltaPack {
    size_t topo, src, netns, off, prev, ns, name, nil, ref, total;
    DeltaPack(uint32_t n, uint32_t nref, uint32_t remap_T) {
        topo = 0;
        src = topo + (size_t)n * 4;
        netns = src + (size_t)n * 4;
        off = netns + (size_t)n * 4;
        prev = off + (n ? ((size_t)n + 1) * 4 : 0);
        ns = prev + (size_t)remap_T * 4;
        name = ns + (remap_T ? (size_t)n * 4 : 0);
        nil = name + (remap_T ? (size_t)n * 4 : 0);
        ref = align_up(nil + n, 4);
        total = ref + (size_t)nref * 4;
    }
};

// offsets of a store from per-topology lengths: u64 (off64[T] = total) and u32, no readback
int scan_lengths(kdtn_ctx* c, DevBuf& len, uint32_t T, DevBuf& off64, DevBuf& part, DevBuf& off32) {
    hipStream_t s = c->stream;
    const uint32_t nb = nblocks((uint64_t)T + 1, SCAN_CHUNK);
    TRY(ensure(off64, ((size_t)T + 1) * 8));
    TRY(ensure(part, (size_t)nb * 8 + 16));
    TRY(ensure(off32, ((size_t)T + 1) * 4));
    k_scan_partial<<<nb, BLOCK, 0, s>>>(dp<uint32_t>(len), T, dp<uint64_t>(part));
    k_scan_top<<<1, SCAN_TOP_BLOCK, 0, s>>>(dp<uint64_t>(part), nb);
    k_scan_final<<<nb, BLOCK, 0, s>>>(dp<uint32_t>(len), T, dp<uint64_t>(part), dp<uint64_t>(off64));
    k_off_narrow<<<nblocks((uint64_t)T + 1), BLOCK, 0, s>>>(dp<uint64_t>(off64), T, dp<uint32_t>(off32));
    HIP_TRY(hipGetLastError());
    return KDTN_OK;
}

// new u32 offsets of a store from per-topology lengths (st_len) into st_off32; returns the total
int plan_offsets(kdtn_ctx* c, uint32_t T, uint64_t* total) {
    hipStream_t s = c->stream;
    TRY(scan_lengths(c, c->st_len, T, c->st_off64, c->st_part, c->st_off32));
    HIP_TRY(hipMemcpyAsync(total, dp<uint64_t>(c->st_off64) + T, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*total >= 0x7FFFFFFFull) {
        std::snprintf(g_last_error, sizeof(g_last_error), "link store of %llu records", (unsigned long long)*total);
        return KDTN_EINVAL;
    }
    return KDTN_OK;
}

// The resident pod tables after a delta: the changed Topologies' rows (dl_rows, n of them on
// this rank) patched into the pod table and their lookup slots, instead of the next runs
// refilling, exchanging and rebuilding all of them. Across RCCL ranks the changed rows are
// all-gathered (the per-rank counts first, then the rows padded to the largest count); when
// some rank changed more than a quarter of a slice, or the tables are not resident (host
// transport, no full build yet), the next run does the full build instead.
int patch_pods(kdtn_ctx* c, uint32_t n) {
    c->pods_delta = false;
    if (!c->pods_ready) return KDTN_OK;
    const bool rccl = c->comm != nullptr;
    if (c->nranks > 1 && (!rccl || !c->pods_rank_major)) {
        c->pods_ready = false;
        return KDTN_OK;
    }
    hipStream_t s = c->stream;
    const int G = rccl ? c->nranks : 1;
    uint32_t m = n;
    if (G > 1) {
        TRY(ensure(c->pd_cnt, (size_t)G * 4 + 16));
        uint32_t* cnt = dp<uint32_t>(c->pd_cnt);
        HIP_TRY(hipMemcpyAsync(cnt + c->rank, &n, 4, hipMemcpyHostToDevice, s));
        ncclResult_t r = ncclAllGather(cnt + c->rank, cnt, 1, ncclUint32, c->comm, s);
        if (r != ncclSuccess) {
            std::snprintf(g_last_error, sizeof(g_last_error), "ncclAllGather (changed pod rows): %s", ncclGetErrorString(r));
            return KDTN_EIO;
        }
        std::vector<uint32_t> h((size_t)G);
        HIP_TRY(hipMemcpyAsync(h.data(), cnt, (size_t)G * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        m = *std::max_element(h.begin(), h.end());
    }
    if ((uint64_t)m * 4 > (uint64_t)c->slice + 4096) {      // a full exchange is cheaper
        c->pods_ready = false;
        return KDTN_OK;
    }
    if (m) {
        TRY(ensure(c->pd_send, (size_t)m * 32));
        TRY(ensure(c->pd_recv, (size_t)m * G * 32));
        k_pods_pack<<<nblocks(m), BLOCK, 0, s>>>(topo_view(c), dp<uint32_t>(c->dl_rows), n, m,
                                                 c->slice * (uint32_t)c->rank, dp<uint4>(c->pd_send));
        const uint4* ent = dp<uint4>(c->pd_send);
        if (G > 1) {
            ncclResult_t r = ncclAllGather(c->pd_send.p, c->pd_recv.p, (size_t)m * 8, ncclUint32, c->comm, s);
            if (r != ncclSuccess) {
                std::snprintf(g_last_error, sizeof(g_last_error), "ncclAllGather (pod rows): %s", ncclGetErrorString(r));
                return KDTN_EIO;
            }
            ent = dp<uint4>(c->pd_recv);
        }
        k_pods_patch<<<nblocks((uint64_t)m * G), BLOCK, 0, s>>>(ent, m * (uint32_t)G, dp<uint4>(c->pods),
                                                               dp<uint4>(c->pod_direct), c->pod_stamp, c->D);
        HIP_TRY(hipGetLastError());
    }
    c->pods_delta = true;
    return KDTN_OK;
}

// per-topology plan arrays for T topologies
int plan_alloc(kdtn_ctx* c, uint32_t T) {
    TRY(ensure(c->st_cnt, 32 * 4));
    TRY(ensure(c->st_len, (size_t)T * 4 + 16));
    TRY(ensure(c->st_base, (size_t)T * 4 + 16));
    TRY(ensure(c->st_mode, (size_t)T + 16));
    TRY(ensure(c->st_flags, (size_t)T + 16));
    return KDTN_OK;
}

// A delta's assembled tables become the context's: the desired store and its columns (N from
// the delta's misc words hm), and with a topology-set change (remap) the realised store, the
// names and T = Tn as well. The replaced tables stay behind as the next delta's scratch.
void install_delta_tables(kdtn_ctx* c, const uint32_t* hm, bool remap, uint32_t Tn) {
    const uint64_t N = (uint64_t)hm[MISC_DELTA_N] | ((uint64_t)hm[MISC_DELTA_N + 1] << 32);
    std::swap(c->des, c->sh_des);
    c->des.n = c->des.view.n = (uint32_t)N;
    std::swap(c->t_noff, c->st_off32);
    std::swap(c->t_src, c->sh_src);
    std::swap(c->t_netns, c->sh_netns);
    std::swap(c->t_flags, c->sh_flags);
    if (remap) {
        const uint64_t M = (uint64_t)hm[MISC_DELTA_M] | ((uint64_t)hm[MISC_DELTA_M + 1] << 32);
        std::swap(c->real, c->sh_real);
        c->real.n = c->real.view.n = (uint32_t)M;
        std::swap(c->t_roff, c->st_roff32);
        std::swap(c->t_ns, c->sh_ns);
        std::swap(c->t_name, c->sh_name);
        c->T = Tn;
    }
}

void state_changed(kdtn_ctx* c) {
    c->ran = false;
    c->encoded = false;
    c->tc_done = false;
    c->fan_valid = false;
    c->lc_valid = false;
    c->si_run = false;
    c->se_run = false;
    c->sj_done = false;
    c->rp_done = false;
    c->j_done = false;
    c->tables_cur = false;
}

}  // namespace

extern "C" {

int kdtn_epoch_commit(kdtn_ctx* c, const uint8_t* mask, uint32_t* n_committed) {
    if (!c || !c->uploaded) return KDTN_EINVAL;
    if (!mask && (!c->ran || !fanout_stages_ok(c))) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "kdtn_epoch_commit without a mask needs a run with the resolve and qdisc stages");
        return KDTN_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t T = c->T;
    if (mask && T && std::memchr(mask, 0, T) == nullptr) {
        // every Topology committed: the realised store IS the desired store (the same records at
        // the same offsets), so no reassembly — real takes the desired store's buffer, des keeps
        // reading that memory (every writer of des resets its view to its own buffer first),
        // real_off := des_off and the status-nil flags follow the spec's
        k_commit_all_flags<<<nblocks(T), BLOCK, 0, s>>>(dp<uint8_t>(c->t_flags), T);
        HIP_TRY(hipMemcpyAsync(c->t_roff.p, c->t_noff.p, ((size_t)T + 1) * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipGetLastError());
        std::swap(c->real, c->des);
        c->des.view = c->real.view;
        c->des.n = c->real.n;
        TRY(prepare_work(c, c->slice, c->real.n, c->des.n));
        HIP_TRY(hipStreamSynchronize(s));
        state_changed(c);
        c->pods_imported = false;
        if (n_committed) *n_committed = T;
        return KDTN_OK;
    }
    TRY(plan_alloc(c, T));
    const uint8_t* dmask = nullptr;
    const uint32_t* cut = nullptr;
    if (mask) {
        TRY(upload(c, c->st_mask, mask, T));
        dmask = dp<uint8_t>(c->st_mask);
    } else {
        TRY(counts_fresh(c));
        TRY(run_reach(c, nullptr, 0));                      // per-topology first failing entries
        cut = dp<uint32_t>(c->f_cut);
    }
    uint32_t* ncnt = dp<uint32_t>(c->st_cnt);
    HIP_TRY(hipMemsetAsync(ncnt, 0, 32 * 4, s));
    if (T)
        k_commit_plan<<<nblocks(T), BLOCK, 0, s>>>(topo_view(c), dp<uint8_t>(c->action), cut, dmask,
                                                   dp<uint32_t>(c->st_len), dp<uint32_t>(c->st_base),
                                                   dp<uint8_t>(c->st_mode), dp<uint8_t>(c->st_flags), ncnt);
    uint64_t M = 0;
    TRY(plan_offsets(c, T, &M));
    TRY(link_store_alloc(c, c->sh_real, (uint32_t)M));
    if (M)
        k_store_assemble<<<nblocks(M), BLOCK, 0, s>>>(dp<uint32_t>(c->st_off32), T, dp<uint32_t>(c->st_base),
                                                      dp<uint8_t>(c->st_mode), nullptr, c->real.view, c->des.view,
                                                      (uint32_t)M, AsmGuard{}, dp<uint32_t>(c->sh_real.buf));
    HIP_TRY(hipGetLastError());
    uint32_t cnt[32] = {};
    HIP_TRY(hipMemcpyAsync(cnt, ncnt, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t nc = 0;
    for (uint32_t v : cnt) nc += v;
    std::swap(c->real, c->sh_real);
    std::swap(c->t_roff, c->st_off32);
    std::swap(c->t_flags, c->st_flags);
    TRY(prepare_work(c, c->slice, c->real.n, c->des.n));
    HIP_TRY(hipStreamSynchronize(s));
    state_changed(c);
    c->pods_imported = false;
    if (n_committed) *n_committed = nc;
    return KDTN_OK;
}

int kdtn_epoch_upload_delta(kdtn_ctx* c, const kdtn_epoch_delta* d) {
    if (!c || !d || !c->uploaded) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    g_last_error[0] = 0;
    end_shard_ingest(c);
    TRY(check_strtab(d->kdict, "kdict", d->kdict_keep));
    TRY(check_strtab(d->pdict, "pdict", d->pdict_keep));
    const bool remap = d->prev != nullptr;                 // the Topology set changes
    const uint32_t T0 = c->T, Tn = remap ? d->n_topos : T0, n = d->n_changed;
    const uint32_t N0 = c->des.n, M0 = c->real.n, D = d->kdict.n, P = d->pdict.n;
    const uint32_t kk = d->kdict_keep, pk = d->pdict_keep;
    auto bad = [&](const char* what, uint32_t i) {
        std::snprintf(g_last_error, sizeof(g_last_error), "delta: %s (at %u)", what, i);
        return KDTN_EINVAL;
    };
    // O(1) host checks; everything per element is checked on the GPU (k_delta_check, k_delta_plan,
    // the inline records' column maxima) and read back with the call's one synchronisation
    if (kk != c->D || pk != c->P) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "delta: kdict_keep %u / pdict_keep %u must equal the resident dictionaries' sizes %u / %u "
                      "(a delta extends them; a shrunk or rewritten dictionary needs kdtn_epoch_upload)",
                      kk, pk, c->D, c->P);
        return KDTN_EINVAL;
    }
    if (kk > c->kd_valid || pk > c->pd_valid) return bad("the resident dictionaries were not parsed (run first)", kk);
    // the kept prefixes end where the resident arenas end (before any copy is enqueued: the
    // suffixes are written at the host's offsets, which must not overlap resident bytes)
    if (d->kdict.offs[kk] != c->kd_arena || d->pdict.offs[pk] != c->pd_arena) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "delta: the kept dictionary prefixes end at byte %u / %u, the resident arenas at %llu / %llu",
                      d->kdict.offs[kk], d->pdict.offs[pk], (unsigned long long)c->kd_arena,
                      (unsigned long long)c->pd_arena);
        return KDTN_EINVAL;
    }
    if (n > Tn) return bad("more changed topologies than topologies", n);
    if (n && (!d->topo || !d->src_ip || !d->net_ns || !d->spec_nil || !d->des_off)) return bad("missing column", 0);
    if (remap && n && (!d->ns || !d->name)) return bad("missing ns / name of the changed topologies", 0);
    const uint32_t nref = n ? d->des_off[n] : 0;
    if (n && d->des_off[0] != 0) return bad("des_off[0] != 0", 0);
    if (nref && !d->ref) return bad("missing ref", 0);
    const uint32_t slice = remap ? (d->pod_slice ? d->pod_slice : Tn) : c->slice;
    if (slice < Tn) return bad("pod_slice below n_topos", slice);
    const uint64_t nbound = (uint64_t)N0 + nref;            // kept segments + the changed lists
    if (nbound >= 0x7FFFFFFFull) return bad("desired store over 2^31 records", (uint32_t)(nbound >> 32));
    TRY(check_vnis(c, d->vnis, D, kk));
    const kdtn_link_table& L = d->records;
    const uint32_t nr = L.n;
    if (nr) {
        for (int k = 0; k < KDTN_NKEY; ++k)
            if (!L.key[k]) return bad("records: missing key column", k);
        for (int k = 0; k < KDTN_NPROP; ++k)
            if (!L.prop[k]) return bad("records: missing prop column", k);
        if (!L.uid || !L.gap) return bad("records: missing uid / gap", 0);
    }
    // Two streams: the host-to-device copies on the copy stream, in the order the kernels need
    // them (the delta's arrays, its references, the dictionary suffixes, the inline records),
    // and the kernels on the context stream, each waiting only for its inputs — so the plan and
    // the assembly of the kept and referenced records run while the inline records cross the
    // host link. Buffers are sized first (an allocation may synchronise the device).
    hipStream_t s = c->stream;
    hipStream_t cs = c->copy_stream ? c->copy_stream : s;
    TRY(ensure(c->misc, 256));
    uint32_t* misc = dp<uint32_t>(c->misc);
    // the delta's arrays in one device block (DeltaPack): a caller whose host arrays sit in the
    // same layout (kdtn.engine.pin_delta) has them copied by one or two copies
    const DeltaPack pk_{n, nref, remap ? Tn : 0u};
    TRY(ensure(c->dl_pack, pk_.total + 64));
    uint8_t* pack = dp<uint8_t>(c->dl_pack);
    uint32_t* p_topo = reinterpret_cast<uint32_t*>(pack + pk_.topo);
    uint32_t* p_src = reinterpret_cast<uint32_t*>(pack + pk_.src);
    uint32_t* p_netns = reinterpret_cast<uint32_t*>(pack + pk_.netns);
    uint32_t* p_off = reinterpret_cast<uint32_t*>(pack + pk_.off);
    uint32_t* p_prev = reinterpret_cast<uint32_t*>(pack + pk_.prev);
    uint32_t* p_ns = reinterpret_cast<uint32_t*>(pack + pk_.ns);
    uint32_t* p_name = reinterpret_cast<uint32_t*>(pack + pk_.name);
    uint8_t* p_nil = pack + pk_.nil;
    uint32_t* p_ref = reinterpret_cast<uint32_t*>(pack + pk_.ref);
    TRY(link_store_alloc(c, c->dl_rec, nr));
    const size_t col = (size_t)nr * 4, uid_at = align_up(col * LINK_COLS32, 8);
    TRY(ensure(c->stage, uid_at + (size_t)nr * 8 + 128));
    TRY(ensure(c->dl_dest, (size_t)nr * 4));
    TRY(plan_alloc(c, Tn));
    TRY(ensure(c->st_chg, (size_t)Tn * 4 + 16));
    TRY(ensure(c->dl_rows, (size_t)n * 4 + 16));
    TRY(ensure(c->sh_src, (size_t)Tn * 4));
    TRY(ensure(c->sh_netns, (size_t)Tn * 4));
    TRY(ensure(c->sh_flags, (size_t)Tn));
    if (remap) {
        TRY(ensure(c->sh_ns, (size_t)Tn * 4));
        TRY(ensure(c->sh_name, (size_t)Tn * 4));
        TRY(ensure(c->st_rlen, (size_t)Tn * 4 + 16));
        TRY(ensure(c->st_rbase, (size_t)Tn * 4 + 16));
        TRY(ensure(c->st_mask, (size_t)Tn + 16));
        TRY(ensure(c->st_seen, ((size_t)T0 + 31) / 32 * 4 + 16));
    }
    TRY(link_store_alloc(c, c->sh_des, (uint32_t)nbound));
    if (remap) TRY(link_store_alloc(c, c->sh_real, M0));
    // --- copies (copy stream), after everything already queued on the context stream. From here
    // on an error return first waits for both streams: the copies read the caller's arrays,
    // which it may release once the call has returned
    StreamsDrain drain{s, cs};
    HIP_TRY(hipEventRecord(c->ev_cp[0], s));
    if (cs != s) HIP_TRY(hipStreamWaitEvent(cs, c->ev_cp[0], 0));
    {   // segments in pack order; host-adjacent neighbours merge into one copy. The per-Topology
        // arrays go first and alone (the plan and the kept segments' assembly need only them),
        // then the references
        const void* src[9] = {d->topo, d->src_ip, d->net_ns, d->des_off, d->prev, d->ns, d->name, d->spec_nil, d->ref};
        const size_t at[9] = {pk_.topo, pk_.src, pk_.netns, pk_.off, pk_.prev, pk_.ns, pk_.name, pk_.nil, pk_.ref};
        const size_t len[9] = {(size_t)n * 4, (size_t)n * 4, (size_t)n * 4, pk_.prev - pk_.off, pk_.ns - pk_.prev,
                               pk_.name - pk_.ns, pk_.nil - pk_.name, (size_t)n, (size_t)nref * 4};
        int i = 0;
        while (i < 9) {
            if (!len[i]) { ++i; continue; }
            const uint8_t* h0 = static_cast<const uint8_t*>(src[i]);
            size_t bytes = len[i];
            int j = i + 1;
            // the device block is contiguous (padding included): the host array must sit at the
            // same distance from the run's start
            while (j < (i < 8 ? 8 : 9) && (!len[j] || static_cast<const uint8_t*>(src[j]) == h0 + (at[j] - at[i]))) {
                if (len[j]) bytes = at[j] + len[j] - at[i];
                ++j;
            }
            HIP_TRY(hipMemcpyAsync(pack + at[i], h0, bytes, hipMemcpyHostToDevice, cs));
            if (i <= 7 && j >= 8) HIP_TRY(hipEventRecord(c->ev_cp[1], cs));   // the small arrays are in
            i = j;
        }
        if (!n) HIP_TRY(hipEventRecord(c->ev_cp[1], cs));
    }
    HIP_TRY(hipEventRecord(c->ev_cp[2], cs));                                   // and the references
    c->uploaded = false;                            // (restored below when the delta is rejected)
    const uint32_t saved[6] = {c->D, c->P, c->kd_valid, c->pd_valid, c->kd_from, c->pd_from};
    const uint64_t saved_arena[2] = {c->kd_arena, c->pd_arena};
    // appends past the resident strings (the kept prefix's end offset is not rewritten: the
    // check below compares it with the host's)
    TRY(upload_dicts(c, d->kdict, d->pdict, kk, pk, cs));
    uint8_t* st = static_cast<uint8_t*>(c->stage.p);
    uint32_t segs[LINK_COLS32][2];
    int nseg = 0;
    if (nr) {
        TRY(stage_columns(c, st, L, col, cs, segs, &nseg));
        HIP_TRY(hipMemcpyAsync(st + uid_at, L.uid, (size_t)nr * 8, hipMemcpyHostToDevice, cs));
        HIP_TRY(hipEventRecord(c->ev_col[nseg], cs));
    }
    HIP_TRY(hipEventRecord(c->ev_cp[3], cs));
    // --- kernels (context stream)
    uint32_t* colmax = misc + MISC_COLMAX;
    HIP_TRY(hipMemsetAsync(misc + MISC_DELTA_ERR, 0, 4, s));
    HIP_TRY(hipMemsetAsync(misc + MISC_ROWCHG_N, 0, 4, s));
    HIP_TRY(hipMemsetAsync(colmax, 0, COL_GAP * 4, s));
    HIP_TRY(hipMemsetAsync(misc + MISC_DELTA_MULTI, 0, 4, s));
    if (nr) HIP_TRY(hipMemsetAsync(c->dl_dest.p, 0xFF, (size_t)nr * 4, s));
    HIP_TRY(hipMemsetAsync(c->st_chg.p, 0xFF, (size_t)Tn * 4, s));
    if (remap) {
        HIP_TRY(hipMemsetAsync(c->st_seen.p, 0, ((size_t)T0 + 31) / 32 * 4 + 16, s));
        HIP_TRY(hipMemsetAsync(c->st_mask.p, ASM_SEG_A, (size_t)Tn + 16, s));
    }
    if (cs != s) HIP_TRY(hipStreamWaitEvent(s, c->ev_cp[1], 0));
    if (n) k_delta_map<<<nblocks(n), BLOCK, 0, s>>>(p_topo, n, Tn, dp<uint32_t>(c->st_chg));
    const DeltaCheckIn ci{p_topo, p_off, p_nil,
                          p_src, p_netns, p_ref,
                          dp<uint32_t>(c->kd_offs), dp<uint32_t>(c->pd_offs), n, nref, Tn, D, nr, N0,
                          kk, pk, d->kdict.offs[kk], d->pdict.offs[pk]};
    {   // the per-Topology arrays and the kept dictionaries now; the references once they are in
        DeltaCheckIn c1 = ci;
        c1.nref = 0;
        k_delta_check<<<std::max<uint32_t>(1u, nblocks(n)), BLOCK, 0, s>>>(c1, misc + MISC_DELTA_ERR);
    }
    // plan over the new topology table: new rows into scratch columns, the state is untouched
    DeltaPlanIn pi{topo_view(c), dp<uint32_t>(c->st_chg), remap ? p_prev : nullptr,
                   p_off, p_src, p_netns, p_nil,
                   p_ns, p_name, Tn, D};
    DeltaPlanOut po{dp<uint32_t>(c->sh_ns), dp<uint32_t>(c->sh_name), dp<uint32_t>(c->sh_src),
                    dp<uint32_t>(c->sh_netns), dp<uint8_t>(c->sh_flags), dp<uint32_t>(c->st_len),
                    dp<uint32_t>(c->st_base), dp<uint8_t>(c->st_mode), dp<uint32_t>(c->st_rlen),
                    dp<uint32_t>(c->st_rbase), dp<uint32_t>(c->dl_rows), misc + MISC_ROWCHG_N,
                    dp<uint32_t>(c->st_seen), misc + MISC_DELTA_ERR};
    if (Tn) k_delta_plan<<<nblocks(Tn), BLOCK, 0, s>>>(pi, po);
    // the new desired store: kept segments and previous-record references now (grid over the
    // bound, the exact count stays on the device), the inline records once they have arrived
    TRY(scan_lengths(c, c->st_len, Tn, c->st_off64, c->st_part, c->st_off32));
    const AsmGuard g{misc + MISC_DELTA_ERR, dp<uint64_t>(c->st_off64) + Tn, 1u, 1u};
    if (nbound)
        k_store_assemble<<<nblocks(nbound), BLOCK, 0, s>>>(dp<uint32_t>(c->st_off32), Tn, dp<uint32_t>(c->st_base),
                                                           dp<uint8_t>(c->st_mode), p_ref, c->des.view,
                                                           c->dl_rec.view, (uint32_t)nbound, g,
                                                           dp<uint32_t>(c->sh_des.buf));
    if (remap) {                                    // kept Topologies' status segments move with them
        TRY(scan_lengths(c, c->st_rlen, Tn, c->st_roff64, c->st_rpart, c->st_roff32));
        const AsmGuard gr{misc + MISC_DELTA_ERR, dp<uint64_t>(c->st_roff64) + Tn, 0u, 0u};
        if (M0)
            k_store_assemble<<<nblocks(M0), BLOCK, 0, s>>>(dp<uint32_t>(c->st_roff32), Tn, dp<uint32_t>(c->st_rbase),
                                                           dp<uint8_t>(c->st_mask), nullptr, c->real.view, c->real.view,
                                                           M0, gr, dp<uint32_t>(c->sh_real.buf));
    }
    // the references once they have arrived: checked, previous records copied to their places,
    // the inline records' destinations noted (before the records themselves have arrived)
    if (cs != s) HIP_TRY(hipStreamWaitEvent(s, c->ev_cp[2], 0));
    if (nref) {
        DeltaCheckIn c2 = ci;
        c2.n = 0;
        c2.kd_keep = c2.pd_keep = 0;                   // (checked above)
        k_delta_check<<<std::min<uint32_t>(nblocks(nref), 4 * c->n_cus), BLOCK, 0, s>>>(c2, misc + MISC_DELTA_ERR);
        k_delta_refs<<<nblocks(nref), BLOCK, 0, s>>>(p_off, p_topo, n, p_ref, nref, dp<uint32_t>(c->st_off32),
                                                     c->des.view, misc + MISC_DELTA_ERR, dp<uint32_t>(c->dl_dest),
                                                     misc + MISC_DELTA_MULTI, dp<uint32_t>(c->sh_des.buf));
    }
    // staging columns straight to their places as each copy arrives, with the id-range maxima
    const uint32_t place_grid = std::min<uint32_t>(nblocks(nr), 4 * c->n_cus);
    for (int k = 0; nr && k <= nseg; ++k) {
        if (cs != s) HIP_TRY(hipStreamWaitEvent(s, c->ev_col[k], 0));
        const bool uid_seg = k == nseg;
        k_delta_place<<<place_grid, BLOCK, 0, s>>>(
            reinterpret_cast<const uint32_t*>(st), reinterpret_cast<const int64_t*>(st + uid_at), nr,
            dp<uint32_t>(c->dl_dest), misc + MISC_DELTA_ERR, dp<uint32_t>(c->sh_des.buf), colmax,
            uid_seg ? (uint32_t)LINK_COLS32 : segs[k][0], uid_seg ? (uint32_t)LINK_COLS32 : segs[k][1], uid_seg ? 1u : 0u);
    }
    if (cs != s) HIP_TRY(hipStreamWaitEvent(s, c->ev_cp[3], 0));
    k_delta_totals<<<1, 64, 0, s>>>(dp<uint64_t>(c->st_off64), Tn, remap ? dp<uint64_t>(c->st_roff64) : nullptr, misc);
    HIP_TRY(hipGetLastError());
    uint32_t* hm = c->h_misc + 64;
    HIP_TRY(hipMemcpyAsync(hm, misc, 64 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));              // the call's one synchronisation
    uint32_t err = hm[MISC_DELTA_ERR];
    if (d->records.n)
        for (int k = 0; k < COL_GAP; ++k)
            if (hm[MISC_COLMAX + k] >= (k < KDTN_NKEY ? D : P)) err |= DERR_COLS;
    if (err) {
        static const char* what[] = {"topo not strictly ascending below n_topos", "des_off not monotone",
                                     "spec nil but records", "status / name id out of range", "ref out of range",
                                     "prev: index out of range or named twice", "a created topology has no spec",
                                     "kept dictionary prefix differs from the resident one",
                                     "inline record id out of range"};
        int b = 0;
        while (!(err & (1u << b))) ++b;
        bad(what[b], err);
        state_changed(c);
        // nothing resident was replaced: the dictionaries only wrote past the resident strings
        // (unless their kept prefix itself disagreed), so their sizes go back and a corrected
        // delta can follow; the next run re-parses the previous upload's suffix
        c->D = saved[0], c->P = saved[1], c->kd_valid = saved[2], c->pd_valid = saved[3];
        c->kd_from = saved[4], c->pd_from = saved[5];
        c->kd_arena = saved_arena[0], c->pd_arena = saved_arena[1];
        c->uploaded = !(err & DERR_KEEP);
        if (err & DERR_KEEP) {                     // the resident strings themselves are suspect
            c->kd_valid = c->pd_valid = c->si_k = c->si_p = c->se_k = c->se_p = 0;
            c->ix_k.n = c->ix_k.mask = 0;
            c->ix_p.n = c->ix_p.mask = 0;
        }
        return KDTN_EINVAL;
    }
    if (hm[MISC_DELTA_MULTI]) {
        // an inline record referenced more than once: the staged delta's tiles, then every
        // reference placed from them (rare; one more synchronisation)
        k_soa_to_tiles<<<std::min<uint32_t>(nblocks(nr), 4 * c->n_cus), BLOCK, 0, s>>>(
            reinterpret_cast<const uint32_t*>(st), reinterpret_cast<const int64_t*>(st + uid_at), nr,
            dp<uint32_t>(c->dl_rec.buf), colmax);
        k_delta_inline<<<nblocks(nref), BLOCK, 0, s>>>(p_off, p_topo, n,
                                                       p_ref, nref, dp<uint32_t>(c->st_off32),
                                                       c->dl_rec.view, misc + MISC_DELTA_ERR,
                                                       dp<uint32_t>(c->sh_des.buf));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    install_delta_tables(c, hm, remap, Tn);
    TRY(prepare_vnis(c, d->vnis));
    TRY(prepare_work(c, slice, c->real.n, c->des.n));
    if (remap) {                                    // rows moved: the next run builds the pod tables
        c->pods_ready = false;
        c->pods_delta = false;
    } else {
        TRY(patch_pods(c, hm[MISC_ROWCHG_N]));
    }
    if (d->vnis.n && d->vnis.n != KDTN_VNI_RESIDENT)
        HIP_TRY(hipStreamSynchronize(s));          // the snapshot's host arrays may be released after return
    state_changed(c);
    c->pods_imported = false;
    c->uploaded = true;
    drain.armed = false;
    return KDTN_OK;
}

int kdtn_epoch_tables_info(kdtn_ctx* c, kdtn_ingest_info* info) {
    if (!c || !c->uploaded) return KDTN_EINVAL;
    kdtn_ingest_info& I = c->j_info;             // host-known sizes: no device access
    I = kdtn_ingest_info{};
    I.n_topos = c->T;
    I.n_desired = c->des.n;
    I.n_realised = c->real.n;
    I.n_kdict = c->D;
    I.n_pdict = c->P;
    I.kdict_bytes = c->kd_arena;
    I.pdict_bytes = c->pd_arena;
    c->tables_cur = true;
    if (info) *info = I;
    return KDTN_OK;
}

}  // extern "C"

// ======================================================================================
// Incremental CR ingest on the resident state (kdtn_informer.hip kernels)
// ======================================================================================
namespace {

// The resident string index of one dictionary (bytes / offs, D strings) brought up to date:
// extended with the strings appended since it was built, rebuilt (twice the capacity) when it
// would pass half full with `extra` more strings, or when the dictionary was rewritten.
int strix_update(kdtn_ctx* c, kdtn_ctx::StrIndex& ix, DevBuf& bytes, DevBuf& offs, uint32_t D, uint32_t extra) {
    hipStream_t s = c->stream;
    const uint64_t want = next_pow2(2ull * ((uint64_t)D + extra) + 64);
    uint32_t from = ix.n;
    if (ix.n > D || !ix.slots.p || !ix.mask || (uint64_t)ix.mask + 1 < want) {
        const uint64_t cap = std::max<uint64_t>(want, (uint64_t)ix.mask + 1);
        if (cap > (1ull << 31)) {
            std::snprintf(g_last_error, sizeof(g_last_error), "string index of %llu slots", (unsigned long long)cap);
            return KDTN_ENOMEM;
        }
        TRY(ensure(ix.slots, (size_t)cap * 8));
        HIP_TRY(hipMemsetAsync(ix.slots.p, 0, (size_t)cap * 8, s));
        ix.mask = (uint32_t)cap - 1;
        from = 0;
    }
    if (D > from)
        k_strix_insert<<<nblocks(D - from), BLOCK, 0, s>>>(dp<uint8_t>(bytes), dp<uint32_t>(offs), from, D,
                                                             dp<unsigned long long>(ix.slots), ix.mask);
    ix.n = D;
    return KDTN_OK;
}

// Local (document) strings → resident ids; misses ranked (new ids) and sized (arena offsets)
int strix_lookup(kdtn_ctx* c, kdtn_ctx::StrIndex& ix, DevBuf& lb, DevBuf& lo, uint32_t nl, DevBuf& rb,
                 DevBuf& ro, DevBuf& map, DevBuf& rank, DevBuf& boff) {
    hipStream_t s = c->stream;
    TRY(ensure(map, (size_t)nl * 4));
    TRY(ensure(c->ji_miss, (size_t)nl * 4));
    TRY(ensure(c->ji_mlen, (size_t)nl * 4));
    TRY(ensure(rank, ((size_t)nl + 1) * 8));
    TRY(ensure(boff, ((size_t)nl + 1) * 8));
    if (nl)
        k_strix_lookup<<<nblocks(nl), BLOCK, 0, s>>>(dp<uint8_t>(lb), dp<uint32_t>(lo), nl, dp<uint8_t>(rb),
                                                     dp<uint32_t>(ro), dp<unsigned long long>(ix.slots), ix.mask,
                                                     dp<uint32_t>(map), dp<uint32_t>(c->ji_miss),
                                                     dp<uint32_t>(c->ji_mlen));
    TRY(scan_u32(c, dp<uint32_t>(c->ji_miss), nl, dp<uint64_t>(rank)));
    TRY(scan_u32(c, dp<uint32_t>(c->ji_mlen), nl, dp<uint64_t>(boff)));
    return KDTN_OK;
}

}  // namespace

extern "C" {

// Incremental CR ingest (include/kdtn.h): the informer's added / updated Topology CRs as a
// TopologyList document decoded into scratch tables, interned into the resident dictionaries,
// matched to the resident rows by (namespace, name), and applied as a delta.
int kdtn_json_ingest_delta(kdtn_ctx* c, const uint32_t* deleted, uint32_t n_deleted, const kdtn_vni_table* vnis,
                           kdtn_ingest_info* info) {
    if (!c || !c->j_loaded || !c->uploaded || (n_deleted && !deleted)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    end_shard_ingest(c);
    g_last_error[0] = 0;
    if (c->nranks > 1) {
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_json_ingest_delta: single-shard contexts");
        return KDTN_EINVAL;
    }
    if (c->kd_valid < c->D || c->pd_valid < c->P) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "kdtn_json_ingest_delta: the resident dictionaries were not parsed (run the epoch first)");
        return KDTN_EINVAL;
    }
    const kdtn_vni_table resident{KDTN_VNI_RESIDENT, nullptr, nullptr, nullptr};
    const kdtn_vni_table& vn = vnis ? *vnis : resident;
    hipStream_t s = c->stream;
    const uint32_t T0 = c->T, N0 = c->des.n, M0 = c->real.n, D0 = c->D, P0 = c->P;
    // 1. decode into scratch (the resident tables are untouched; a rejected document leaves them)
    const JsTargets tg{&c->ji_ns, &c->ji_name, &c->ji_src, &c->ji_netns, &c->ji_flags, &c->ji_roff, &c->ji_noff,
                       &c->ji_des, &c->ji_real, &c->ji_kb, &c->ji_ko, &c->ji_pb, &c->ji_po};
    JsCounts k{};
    {
        const int rc = json_decode(c, tg, &k, info);
        c->uploaded = true;                          // (json_reject clears it: the state stands)
        if (rc != KDTN_OK) return rc;
    }
    const uint32_t Tl = k.T, Nl = k.N;
    const uint64_t n_tokens = c->j_info.n_tokens;
    // 2. intern the document's strings into the resident dictionaries
    TRY(strix_update(c, c->ix_k, c->kd_bytes, c->kd_offs, D0, k.D));
    TRY(strix_update(c, c->ix_p, c->pd_bytes, c->pd_offs, P0, k.P));
    TRY(strix_lookup(c, c->ix_k, c->ji_kb, c->ji_ko, k.D, c->kd_bytes, c->kd_offs, c->ji_kmap, c->ji_rank, c->ji_boff));
    uint64_t cnt[4] = {0, 0, 0, 0};                  // new key strings, their bytes, new prop strings, bytes
    TRY(d2h(c, cnt, dp<uint64_t>(c->ji_rank) + k.D));
    TRY(d2h(c, cnt + 1, dp<uint64_t>(c->ji_boff) + k.D));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t D1w = (uint64_t)D0 + cnt[0];
    const uint64_t kar1 = c->kd_arena + cnt[1];
    // offsets are u32 (arena0 + boff): bounded before anything is appended
    if (kar1 > 0xFFFFFF00ull || D1w >= 0x7FFFFFFFull) {
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_json_ingest_delta: key dictionary over 4 GiB / 2^31");
        return KDTN_EINVAL;
    }
    const uint32_t D1 = (uint32_t)D1w;
    TRY(ensure_keep(c->kd_bytes, kar1 + 64, c->kd_arena, s));
    TRY(ensure_keep(c->kd_offs, ((size_t)D1 + 1) * 4, ((size_t)D0 + 1) * 4, s));
    if (k.D)
        k_strix_append<<<nblocks(k.D), BLOCK, 0, s>>>(dp<uint8_t>(c->ji_kb), dp<uint32_t>(c->ji_ko), k.D,
                                                      dp<uint64_t>(c->ji_rank), dp<uint64_t>(c->ji_boff), D0,
                                                      (uint32_t)c->kd_arena, dp<uint32_t>(c->ji_kmap),
                                                      dp<uint8_t>(c->kd_bytes), dp<uint32_t>(c->kd_offs));
    // (the rank / offset scratch is reused for the property dictionary after the key append)
    TRY(strix_lookup(c, c->ix_p, c->ji_pb, c->ji_po, k.P, c->pd_bytes, c->pd_offs, c->ji_pmap, c->ji_kpos, c->ji_cpos));
    TRY(d2h(c, cnt + 2, dp<uint64_t>(c->ji_kpos) + k.P));
    TRY(d2h(c, cnt + 3, dp<uint64_t>(c->ji_cpos) + k.P));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t P1w = (uint64_t)P0 + cnt[2];
    const uint64_t par1 = c->pd_arena + cnt[3];
    const uint32_t P1 = (uint32_t)P1w;
    if (par1 > 0xFFFFFF00ull || P1w >= 0x7FFFFFFFull) {
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_json_ingest_delta: dictionaries over 4 GiB / 2^31");
        return KDTN_EINVAL;
    }
    TRY(ensure_keep(c->pd_bytes, par1 + 64, c->pd_arena, s));
    TRY(ensure_keep(c->pd_offs, ((size_t)P1 + 1) * 4, ((size_t)P0 + 1) * 4, s));
    if (k.P)
        k_strix_append<<<nblocks(k.P), BLOCK, 0, s>>>(dp<uint8_t>(c->ji_pb), dp<uint32_t>(c->ji_po), k.P,
                                                      dp<uint64_t>(c->ji_kpos), dp<uint64_t>(c->ji_cpos), P0,
                                                      (uint32_t)c->pd_arena, dp<uint32_t>(c->ji_pmap),
                                                      dp<uint8_t>(c->pd_bytes), dp<uint32_t>(c->pd_offs));
    // the appended strings join the indexes
    if (D1 > D0)
        k_strix_insert<<<nblocks(D1 - D0), BLOCK, 0, s>>>(dp<uint8_t>(c->kd_bytes), dp<uint32_t>(c->kd_offs), D0, D1,
                                                          dp<unsigned long long>(c->ix_k.slots), c->ix_k.mask);
    if (P1 > P0)
        k_strix_insert<<<nblocks(P1 - P0), BLOCK, 0, s>>>(dp<uint8_t>(c->pd_bytes), dp<uint32_t>(c->pd_offs), P0, P1,
                                                          dp<unsigned long long>(c->ix_p.slots), c->ix_p.mask);
    c->ix_k.n = D1;
    c->ix_p.n = P1;
    // 3. the document's tables in resident ids
    TRY(ensure(c->ji_nil, (size_t)Tl + 16));
    if (Tl)
        k_ix_map_topos<<<nblocks(Tl), BLOCK, 0, s>>>(dp<uint32_t>(c->ji_ns), dp<uint32_t>(c->ji_name),
                                                     dp<uint32_t>(c->ji_src), dp<uint32_t>(c->ji_netns),
                                                     dp<uint8_t>(c->ji_flags), Tl, dp<uint32_t>(c->ji_kmap),
                                                     dp<uint8_t>(c->ji_nil));
    constexpr uint32_t IDW = (KDTN_NKEY + KDTN_NPROP) * TILE_RECS;
    if (Nl)
        k_ix_map_links<<<nblocks((uint64_t)(Nl + TILE_RECS - 1) / TILE_RECS * IDW), BLOCK, 0, s>>>(
            dp<uint32_t>(c->ji_des.buf), Nl, dp<uint32_t>(c->ji_kmap), dp<uint32_t>(c->ji_pmap));
    // 4. the document's Topologies against the resident rows; the deletions; the new table
    const uint64_t kcap = next_pow2(2ull * T0 + 64);
    TRY(ensure(c->ji_keys, (size_t)kcap * 8));
    TRY(ensure(c->ji_vals, (size_t)kcap * 4));
    const uint64_t dcap = next_pow2(2ull * Tl + 64);
    TRY(ensure(c->ji_dkeys, (size_t)dcap * 8));
    TRY(ensure(c->ji_keep, (size_t)T0 * 4 + 16));
    TRY(ensure(c->ji_kpos, ((size_t)T0 + 1) * 8));
    TRY(ensure(c->ji_claim, (size_t)T0 * 4 + 16));
    TRY(ensure(c->ji_res, (size_t)Tl * 4 + 16));
    TRY(ensure(c->ji_created, (size_t)Tl * 4 + 16));
    TRY(ensure(c->ji_cpos, ((size_t)Tl + 1) * 8));
    TRY(ensure(c->misc, 256));
    uint32_t* misc = dp<uint32_t>(c->misc);
    HIP_TRY(hipMemsetAsync(misc + MISC_DELTA_ERR, 0, 4, s));
    HIP_TRY(hipMemsetAsync(c->ji_keys.p, 0, (size_t)kcap * 8, s));
    HIP_TRY(hipMemsetAsync(c->ji_vals.p, 0xFF, (size_t)kcap * 4, s));
    HIP_TRY(hipMemsetAsync(c->ji_dkeys.p, 0, (size_t)dcap * 8, s));
    HIP_TRY(hipMemsetAsync(c->ji_claim.p, 0xFF, (size_t)T0 * 4 + 16, s));
    if (T0) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->ji_keep.p), 1, T0, s));
    if (T0)
        k_topokey_insert<<<nblocks(T0), BLOCK, 0, s>>>(dp<uint32_t>(c->t_ns), dp<uint32_t>(c->t_name), T0,
                                                       dp<unsigned long long>(c->ji_keys), dp<uint32_t>(c->ji_vals),
                                                       (uint32_t)kcap - 1);
    if (n_deleted) {
        TRY(upload(c, c->ji_del, deleted, (size_t)n_deleted * 4));
        k_topo_delete<<<nblocks(n_deleted), BLOCK, 0, s>>>(dp<uint32_t>(c->ji_del), n_deleted, T0,
                                                           dp<uint32_t>(c->ji_keep), misc + MISC_DELTA_ERR);
    }
    if (Tl)
        k_topokey_match<<<nblocks(Tl), BLOCK, 0, s>>>(dp<uint32_t>(c->ji_ns), dp<uint32_t>(c->ji_name), Tl,
                                                      dp<unsigned long long>(c->ji_keys), dp<uint32_t>(c->ji_vals),
                                                      (uint32_t)kcap - 1, dp<unsigned long long>(c->ji_dkeys),
                                                      (uint32_t)dcap - 1, dp<uint32_t>(c->ji_keep),
                                                      dp<uint32_t>(c->ji_claim), dp<uint32_t>(c->ji_res),
                                                      dp<uint32_t>(c->ji_created), misc + MISC_DELTA_ERR);
    TRY(scan_u32(c, dp<uint32_t>(c->ji_keep), T0, dp<uint64_t>(c->ji_kpos)));
    TRY(scan_u32(c, dp<uint32_t>(c->ji_created), Tl, dp<uint64_t>(c->ji_cpos)));
    uint64_t tot[2] = {0, 0};
    uint32_t err = 0;
    TRY(d2h(c, tot, dp<uint64_t>(c->ji_kpos) + T0));
    TRY(d2h(c, tot + 1, dp<uint64_t>(c->ji_cpos) + Tl));
    TRY(d2h(c, &err, misc + MISC_DELTA_ERR));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    auto refuse = [&](const char* what) {
        // the dictionaries only grew past the resident strings: their sizes stay, the arena
        // tails are overwritten later, and the indexes (which hold the appended strings) are
        // rebuilt by the next incremental ingest (mask 0)
        c->ix_k.n = c->ix_k.mask = c->ix_p.n = c->ix_p.mask = 0;
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_json_ingest_delta: %s", what);
        state_changed(c);
        return KDTN_EINVAL;
    };
    if (err & 4u) return refuse("a deleted index is out of range");
    if (err & 1u) return refuse("a Topology is both deleted and listed in the document");
    if (err & 2u) return refuse("a Topology is listed twice in the document");
    const uint32_t n_kept = (uint32_t)tot[0], n_created = (uint32_t)tot[1], Tn = n_kept + n_created;
    const bool remap = n_kept != T0 || n_created;
    // 5. the delta: the document's Topologies are the changed list (row l: spec from its
    // records, all inline), laid out over the new table
    TRY(plan_alloc(c, Tn));
    TRY(ensure(c->st_chg, (size_t)Tn * 4 + 16));
    HIP_TRY(hipMemsetAsync(c->st_chg.p, 0xFF, (size_t)Tn * 4 + 16, s));
    if (remap) TRY(ensure(c->dl_prev, (size_t)Tn * 4 + 16));
    const uint32_t nl = std::max(T0, Tl);
    if (nl)
        k_ix_layout<<<nblocks(nl), BLOCK, 0, s>>>(dp<uint32_t>(c->ji_keep), dp<uint64_t>(c->ji_kpos), T0,
                                                  dp<uint32_t>(c->ji_claim), dp<uint32_t>(c->ji_created),
                                                  dp<uint64_t>(c->ji_cpos), Tl, n_kept,
                                                  remap ? dp<uint32_t>(c->dl_prev) : nullptr, dp<uint32_t>(c->st_chg));
    TRY(ensure(c->ji_ref, (size_t)Nl * 4 + 16));
    if (Nl) k_ix_refs<<<nblocks(Nl), BLOCK, 0, s>>>(dp<uint32_t>(c->ji_ref), Nl);
    TRY(ensure(c->dl_rows, (size_t)Tl * 4 + 16));
    TRY(ensure(c->sh_src, (size_t)Tn * 4));
    TRY(ensure(c->sh_netns, (size_t)Tn * 4));
    TRY(ensure(c->sh_flags, (size_t)Tn));
    if (remap) {
        TRY(ensure(c->sh_ns, (size_t)Tn * 4));
        TRY(ensure(c->sh_name, (size_t)Tn * 4));
        TRY(ensure(c->st_rlen, (size_t)Tn * 4 + 16));
        TRY(ensure(c->st_rbase, (size_t)Tn * 4 + 16));
        TRY(ensure(c->st_mask, (size_t)Tn + 16));
        TRY(ensure(c->st_seen, ((size_t)T0 + 31) / 32 * 4 + 16));
        HIP_TRY(hipMemsetAsync(c->st_seen.p, 0, ((size_t)T0 + 31) / 32 * 4 + 16, s));
        HIP_TRY(hipMemsetAsync(c->st_mask.p, ASM_SEG_A, (size_t)Tn + 16, s));
    }
    HIP_TRY(hipMemsetAsync(misc + MISC_ROWCHG_N, 0, 4, s));
    const uint64_t nbound = (uint64_t)N0 + Nl;
    if (nbound >= 0x7FFFFFFFull) return refuse("desired store over 2^31 records");
    TRY(link_store_alloc(c, c->sh_des, (uint32_t)nbound));
    if (remap) TRY(link_store_alloc(c, c->sh_real, M0));
    DeltaPlanIn pi{topo_view(c), dp<uint32_t>(c->st_chg), remap ? dp<uint32_t>(c->dl_prev) : nullptr,
                   dp<uint32_t>(c->ji_noff), dp<uint32_t>(c->ji_src), dp<uint32_t>(c->ji_netns), dp<uint8_t>(c->ji_nil),
                   dp<uint32_t>(c->ji_ns), dp<uint32_t>(c->ji_name), Tn, D1};
    DeltaPlanOut po{dp<uint32_t>(c->sh_ns), dp<uint32_t>(c->sh_name), dp<uint32_t>(c->sh_src),
                    dp<uint32_t>(c->sh_netns), dp<uint8_t>(c->sh_flags), dp<uint32_t>(c->st_len),
                    dp<uint32_t>(c->st_base), dp<uint8_t>(c->st_mode), dp<uint32_t>(c->st_rlen),
                    dp<uint32_t>(c->st_rbase), dp<uint32_t>(c->dl_rows), misc + MISC_ROWCHG_N,
                    dp<uint32_t>(c->st_seen), misc + MISC_DELTA_ERR};
    if (Tn) k_delta_plan<<<nblocks(Tn), BLOCK, 0, s>>>(pi, po);
    TRY(scan_lengths(c, c->st_len, Tn, c->st_off64, c->st_part, c->st_off32));
    const AsmGuard g{misc + MISC_DELTA_ERR, dp<uint64_t>(c->st_off64) + Tn, 0u};
    if (nbound)
        k_store_assemble<<<nblocks(nbound), BLOCK, 0, s>>>(dp<uint32_t>(c->st_off32), Tn, dp<uint32_t>(c->st_base),
                                                           dp<uint8_t>(c->st_mode), dp<uint32_t>(c->ji_ref), c->des.view,
                                                           c->ji_des.view, (uint32_t)nbound, g,
                                                           dp<uint32_t>(c->sh_des.buf));
    if (remap) {
        TRY(scan_lengths(c, c->st_rlen, Tn, c->st_roff64, c->st_rpart, c->st_roff32));
        const AsmGuard gr{misc + MISC_DELTA_ERR, dp<uint64_t>(c->st_roff64) + Tn, 0u};
        if (M0)
            k_store_assemble<<<nblocks(M0), BLOCK, 0, s>>>(dp<uint32_t>(c->st_roff32), Tn, dp<uint32_t>(c->st_rbase),
                                                           dp<uint8_t>(c->st_mask), nullptr, c->real.view, c->real.view,
                                                           M0, gr, dp<uint32_t>(c->sh_real.buf));
    }
    k_delta_totals<<<1, 64, 0, s>>>(dp<uint64_t>(c->st_off64), Tn, remap ? dp<uint64_t>(c->st_roff64) : nullptr, misc);
    HIP_TRY(hipGetLastError());
    uint32_t* hm = c->h_misc + 64;
    HIP_TRY(hipMemcpyAsync(hm, misc, 64 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hm[MISC_DELTA_ERR]) return refuse("the document's tables failed the delta checks");
    // 6. the new state
    install_delta_tables(c, hm, remap, Tn);
    // dictionaries: the appended strings are parsed by the next run (kd_from / pd_from)
    c->D = D1;
    c->P = P1;
    c->kd_arena = kar1;
    c->pd_arena = par1;
    c->kd_valid = c->kd_from = D0;
    c->pd_valid = c->pd_from = P0;
    c->si_k = std::min(c->si_k, D0);
    c->si_p = std::min(c->si_p, P0);
    c->se_k = std::min(c->se_k, D0);
    c->se_p = std::min(c->se_p, P0);
    TRY(prepare_dicts(c));
    TRY(check_vnis(c, vn, D1, D0));
    TRY(prepare_vnis(c, vn));
    TRY(prepare_work(c, remap ? Tn : c->slice, c->real.n, c->des.n));
    c->pods_ready = false;                         // rows changed: the next run rebuilds the pod tables
    c->pods_delta = false;
    HIP_TRY(hipStreamSynchronize(s));
    state_changed(c);
    c->pods_imported = false;
    c->uploaded = true;
    c->j_info = kdtn_ingest_info{};
    c->j_info.n_topos = c->T;
    c->j_info.n_desired = c->des.n;
    c->j_info.n_realised = c->real.n;
    c->j_info.n_kdict = D1;
    c->j_info.n_pdict = P1;
    c->j_info.n_tokens = n_tokens;
    c->j_info.kdict_bytes = kar1;
    c->j_info.pdict_bytes = par1;
    if (info) *info = c->j_info;
    return KDTN_OK;
}

}  // extern "C"
