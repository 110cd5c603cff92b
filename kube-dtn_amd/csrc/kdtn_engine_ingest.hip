// kdtn_engine_ingest.hip — the ingest entry points of the C-ABI: TopologyList JSON, LinksBatchQuery streams,
// RemotePod bodies, UpdateLinks bodies, the sharded ingest, and the ingested tables' download
// (host side of libkdtn.so; the context and the shared helpers are in kdtn_engine.h)
#include "kdtn_engine.h"

// ======================================================================================
// CR ingest: TopologyList JSON → device-resident epoch tables (kdtn_ingest.hip)
// ======================================================================================
namespace {

// small control block: [0] syntax error, [1] decode error (pos << 8 | code, ~0 = none),
// [2] heap bytes used, [3] status | seen_root << 32, [4] kd fill | pd fill << 32
constexpr size_t J_SMALL = 64;

int json_reject(kdtn_ctx* c, kdtn_ingest_info* info, unsigned long long word) {
    c->j_info.json_err = (int32_t)(word & 0xFF);
    c->j_info.err_offset = word >> 8;
    if (info) *info = c->j_info;
    c->j_done = false;
    c->uploaded = false;
    std::snprintf(g_last_error, sizeof(g_last_error), "TopologyList rejected: json error %d at byte %llu",
                  c->j_info.json_err, (unsigned long long)c->j_info.err_offset);
    return KDTN_EBADMSG;
}

// ids of one dictionary in first-occurrence order, its arena and offsets
int json_dict(kdtn_ctx* c, const JsDict& dt, const JsIntern& in, uint32_t ntok, DevBuf& slot_id, DevBuf& bytes,
              DevBuf& offs, uint32_t* n_out, uint64_t* bytes_out) {
    hipStream_t s = c->stream;
    const uint32_t nw = (ntok + 31) / 32, cap = dt.mask + 1;
    TRY(ensure(c->j_bits, (size_t)nw * 4));
    TRY(ensure(c->j_bcnt, (size_t)nw * 4));
    TRY(ensure(c->j_wrank, ((size_t)nw + 1) * 8));
    HIP_TRY(hipMemsetAsync(c->j_bits.p, 0, (size_t)nw * 4, s));
    k_js_rep_mark<<<nblocks(cap), BLOCK, 0, s>>>(dt, dp<uint32_t>(c->j_bits));
    k_js_popc<<<nblocks(nw), BLOCK, 0, s>>>(dp<uint32_t>(c->j_bits), nw, dp<uint32_t>(c->j_bcnt));
    TRY(scan_u32(c, dp<uint32_t>(c->j_bcnt), nw, dp<uint64_t>(c->j_wrank)));
    timer_mark(c, "js_intern");
    uint64_t uniq = 0;
    TRY(d2h(c, &uniq, dp<uint64_t>(c->j_wrank) + nw));
    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "js_sync");
    const uint32_t n = (uint32_t)uniq + 1;                    // + id 0 = ""
    TRY(ensure(slot_id, (size_t)cap * 4));
    TRY(ensure(c->j_len, (size_t)n * 4));
    TRY(ensure(c->j_off64, ((size_t)n + 1) * 8));
    TRY(ensure(c->j_sofid, (size_t)n * 4));
    HIP_TRY(hipMemsetAsync(c->j_len.p, 0, (size_t)n * 4, s));
    k_js_ids<<<nblocks(cap), BLOCK, 0, s>>>(dt, dp<uint32_t>(c->j_bits), dp<uint64_t>(c->j_wrank),
                                            dp<uint32_t>(slot_id), dp<uint32_t>(c->j_len), dp<uint32_t>(c->j_sofid));
    TRY(scan_u32(c, dp<uint32_t>(c->j_len), n, dp<uint64_t>(c->j_off64)));
    timer_mark(c, "js_intern");
    uint64_t total = 0;
    TRY(d2h(c, &total, dp<uint64_t>(c->j_off64) + n));
    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "js_sync");
    if (total > 0xFFFFFF00ull) {
        std::snprintf(g_last_error, sizeof(g_last_error), "dictionary arena of %llu bytes exceeds 4 GiB",
                      (unsigned long long)total);
        return KDTN_EINVAL;
    }
    TRY(ensure(bytes, (size_t)total + 64));
    TRY(ensure(offs, ((size_t)n + 1) * 4));
    HIP_TRY(hipMemsetAsync(offs.p, 0, 4, s));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dp<uint32_t>(offs) + n), (int)(uint32_t)total, 1, s));
    if (n > 1)
        k_js_dict_copy<<<nblocks(n - 1), BLOCK, 0, s>>>(dt, in, dp<uint32_t>(c->j_sofid), n, dp<uint64_t>(c->j_off64),
                                                        dp<uint32_t>(offs), dp<uint8_t>(bytes));
    *n_out = n;
    *bytes_out = total;
    return KDTN_OK;
}

}  // namespace

namespace kdtn {
namespace host {

int link_store_alloc(kdtn_ctx* c, DevLinkStore& st, uint32_t n) {
    const size_t tiles = ((size_t)std::max<uint32_t>(n, 1) + TILE_RECS - 1) / TILE_RECS;
    TRY(ensure(st.buf, tiles * TILE_WORDS * 4));
    st.view.base = dp<uint32_t>(st.buf);
    st.view.n = n;
    st.n = n;
    return KDTN_OK;
}

}  // namespace host
}  // namespace kdtn

extern "C" {

int kdtn_json_upload(kdtn_ctx* c, const uint8_t* doc, uint64_t n) {
    if (!c || (n && !doc)) return KDTN_EINVAL;
    if (n >= 0xFFFFFF00ull) {
        std::snprintf(g_last_error, sizeof(g_last_error), "document of %llu bytes: the GPU ingest takes < 4 GiB",
                      (unsigned long long)n);
        return KDTN_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t nb = (uint32_t)((n + 63) / 64);
    const size_t padded = (size_t)nb * 64 + 128;             // whitespace tail: blocks and look-ahead
    TRY(ensure(c->j_doc, padded));
    if (n) HIP_TRY(hipMemcpyAsync(c->j_doc.p, doc, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dp<uint8_t>(c->j_doc) + n, ' ', padded - n, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->j_n = n;
    c->j_nb = nb;
    c->j_loaded = true;
    c->j_done = false;
    return KDTN_OK;
}

}  // extern "C"

namespace kdtn {
namespace host {

// The decode of the uploaded document into `tg` (the context's own tables for a full ingest,
// scratch tables for an incremental one): topology columns, both link stores, first-occurrence
// dictionaries. Counts into `o`. A rejected document returns KDTN_EBADMSG (json_reject).
int json_decode(kdtn_ctx* c, const JsTargets& tg, JsCounts* o, kdtn_ingest_info* info) {
    hipStream_t s = c->stream;
    c->j_info = kdtn_ingest_info{};
    stage_begin(c);
    const uint32_t nb = c->j_nb;
    if (nb == 0) return json_reject(c, info, (0ull << 8) | KDTN_JSON_SYNTAX);   // empty document

    TRY(ensure(c->j_small, J_SMALL));
    unsigned long long* small = dp<unsigned long long>(c->j_small);
    HIP_TRY(hipMemsetAsync(small, 0xFF, 16, s));
    HIP_TRY(hipMemsetAsync(small + 2, 0, J_SMALL - 16, s));
    // one word past the end: any_in reads the word after a string's first (its bits are masked)
    for (DevBuf* b : {&c->j_q, &c->j_bs, &c->j_hb, &c->j_esc, &c->j_tok, &c->j_open, &c->j_close}) TRY(ensure(*b, ((size_t)nb + 1) * 8));
    // per-workgroup counts (quotes; tokens, depth, opens, colons, scalars) and their offsets
    const uint32_t nwg = nblocks(nb);
    TRY(ensure(c->j_qcnt, (size_t)nwg * 4));
    TRY(ensure(c->j_qoff, ((size_t)nwg + 1) * 8));
    TRY(ensure(c->j_gcnt, (size_t)5 * nwg * 4));
    TRY(ensure(c->j_goff, (size_t)5 * (nwg + 1) * 8));
    JsDoc j{dp<uint8_t>(c->j_doc), (uint32_t)c->j_n, nb, dp<uint64_t>(c->j_q), dp<uint64_t>(c->j_bs),
            dp<uint64_t>(c->j_hb), dp<uint64_t>(c->j_esc), 0u};
#if KDTN_PROFILING
    j.variant = (uint32_t)std::strtoul(std::getenv("KDTN_JS_VARIANT") ? std::getenv("KDTN_JS_VARIANT") : "0", nullptr, 0);
#endif
    JsMasks m{dp<uint64_t>(c->j_tok), dp<uint64_t>(c->j_open), dp<uint64_t>(c->j_close), dp<uint32_t>(c->j_gcnt)};
    const uint64_t* goff = dp<uint64_t>(c->j_goff);
    auto gtotal = [&](int f) { return goff + (size_t)f * (nwg + 1) + nwg; };   // f: 0 tokens, 2 opens, 3 colons, 4 scalars

    // 1. block masks, string state, token counts, depth
    k_js_quotes<<<nblocks(nb), BLOCK, 0, s>>>(j, dp<uint64_t>(c->j_q), dp<uint64_t>(c->j_bs), dp<uint64_t>(c->j_hb),
                                              dp<uint64_t>(c->j_esc),
                                             dp<uint32_t>(c->j_qcnt));
    TRY(scan_u32(c, dp<uint32_t>(c->j_qcnt), nwg, dp<uint64_t>(c->j_qoff)));
    k_js_classify<<<nwg, BLOCK, 0, s>>>(j, dp<uint64_t>(c->j_qoff), m, nwg, small);
    for (int f = 0; f < 5; ++f)
        TRY(scan_u32(c, dp<uint32_t>(c->j_gcnt) + (size_t)f * nwg, nwg, dp<uint64_t>(c->j_goff) + (size_t)f * (nwg + 1)));
    timer_mark(c, "js_blocks");
    uint64_t quotes = 0, ntok64 = 0, nopen64 = 0;
    TRY(d2h(c, &nopen64, gtotal(2)));
    uint64_t nval64 = 0;
    TRY(d2h(c, &nval64, gtotal(3)));
    uint64_t nscal64 = 0;
    TRY(d2h(c, &nscal64, gtotal(4)));
    unsigned long long serr = 0;
    TRY(d2h(c, &quotes, dp<uint64_t>(c->j_qoff) + nwg));
    TRY(d2h(c, &ntok64, gtotal(0)));
    TRY(d2h(c, &serr, small));
    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "js_sync");                       // host round trips are timed apart
    HIP_TRY(hipGetLastError());
    if (quotes & 1) serr = std::min<unsigned long long>(serr, (c->j_n << 8) | KDTN_JSON_SYNTAX);   // unterminated
    if (ntok64 == 0) serr = std::min<unsigned long long>(serr, KDTN_JSON_SYNTAX);
    if (serr != ~0ull) return json_reject(c, info, serr);
    const uint32_t ntok = (uint32_t)ntok64;
    c->j_info.n_tokens = ntok64;

    // 2. token stream, parents, checkValid
    TRY(ensure(c->j_toks, (size_t)ntok * 8));
    TRY(ensure(c->j_par, (size_t)ntok * 4));
    TRY(ensure(c->j_role, (size_t)ntok));
    TRY(ensure(c->j_ecls, ((size_t)ntok + JS_TILE - 1) / JS_TILE * JS_TILE));   // whole tiles (uint4 reads)
    TRY(ensure(c->j_ord, (size_t)ntok * 4));
    const uint32_t nopen = (uint32_t)nopen64;
    TRY(ensure(c->j_olist, (size_t)nopen * 4));
    TRY(ensure(c->j_odep, (size_t)nopen));
    const uint32_t nval = (uint32_t)nval64;
    TRY(ensure(c->j_vlist, (size_t)nval * 4));
    const uint32_t nscal = (uint32_t)nscal64;
    TRY(ensure(c->j_slist, (size_t)nscal * 4 + 4));
    const JsToks tk{dp<uint32_t>(c->j_toks), dp<uint32_t>(c->j_toks) + ntok};   // offsets, then meta words
    uint32_t* par = dp<uint32_t>(c->j_par);
    k_js_tokens<<<nwg, BLOCK, 0, s>>>(j, m, goff, nwg, tk, dp<uint32_t>(c->j_olist), dp<uint8_t>(c->j_odep),
                                             dp<uint32_t>(c->j_vlist), dp<uint32_t>(c->j_slist), small);
    timer_mark(c, "js_tokens");
    const uint32_t ntiles = (ntok + JS_TILE - 1) / JS_TILE, ng = (ntiles + BLOCK - 1) / BLOCK;
    TRY(ensure(c->j_tagg, (size_t)ntiles * JS_PD * 4));
    TRY(ensure(c->j_gagg, (size_t)ng * JS_PD * 4));
    k_js_par_agg<<<ntiles, BLOCK, 0, s>>>(tk.meta, ntok, dp<uint32_t>(c->j_tagg));
    k_js_par_group<<<ng, BLOCK, 0, s>>>(dp<uint32_t>(c->j_tagg), ntiles, dp<uint32_t>(c->j_gagg));
    k_js_par_top<<<1, BLOCK, 0, s>>>(dp<uint32_t>(c->j_gagg), ng);
    k_js_par_tiles<<<ng, BLOCK, 0, s>>>(dp<uint32_t>(c->j_tagg), ntiles, dp<uint32_t>(c->j_gagg));
    uint32_t* deep = reinterpret_cast<uint32_t*>(small + 4);   // zeroed with the small words above
    k_js_par_apply<<<ntiles, BLOCK, 0, s>>>(tk.meta, ntok, dp<uint32_t>(c->j_tagg), par, deep);
    k_js_deep<<<std::min<uint32_t>(nblocks(ntok), 2048), BLOCK, 0, s>>>(tk.meta, ntok, par, deep);
    timer_mark(c, "js_parents");
    k_js_validate<<<nblocks(ntok), BLOCK, 0, s>>>(j, tk, ntok, par, dp<uint8_t>(c->j_ecls), small);
    k_js_tail<<<1, 64, 0, s>>>(j, tk, ntok, par, small);
    if (nscal) k_js_scalars<<<nblocks(nscal), BLOCK, 0, s>>>(j, tk.pos, dp<uint32_t>(c->j_slist), nscal, small);
    timer_mark(c, "js_validate");
    TRY(d2h(c, &serr, small));
    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "js_sync");
    HIP_TRY(hipGetLastError());
    if (serr != ~0ull) return json_reject(c, info, serr);

    // 3. schema roles, items / links ordinals
    uint8_t* role = dp<uint8_t>(c->j_role);
    uint32_t* ord = dp<uint32_t>(c->j_ord);
    HIP_TRY(hipMemsetAsync(role, 0, ntok, s));                  // R_NONE below the schema levels
    for (uint32_t level : {0u, 1u, 3u, 4u})            // levels 2 and 5: k_js_elems_count
        if (nopen) k_js_roles<<<nblocks(nopen), BLOCK, 0, s>>>(j, tk, dp<uint32_t>(c->j_olist), nopen, par, role,
                                                    dp<uint8_t>(c->j_odep), level);
    TRY(ensure(c->j_cnt3, (size_t)3 * ntiles * 4));
    TRY(ensure(c->j_coff3, (size_t)3 * (ntiles + 1) * 8));
    k_js_elems_count<<<ntiles, BLOCK, 0, s>>>(j, tk, ntok, par, role, dp<uint32_t>(c->j_cnt3),
                                              dp<uint8_t>(c->j_ecls), small + 1);
    if (nopen)                                          // properties objects, under the links elements
        k_js_roles<<<nblocks(nopen), BLOCK, 0, s>>>(j, tk, dp<uint32_t>(c->j_olist), nopen, par, role,
                                                    dp<uint8_t>(c->j_odep), 6u);
    for (int q = 0; q < 3; ++q)
        TRY(scan_u32(c, dp<uint32_t>(c->j_cnt3) + (size_t)q * ntiles, ntiles,
                     dp<uint64_t>(c->j_coff3) + (size_t)q * (ntiles + 1)));
    timer_mark(c, "js_elements");
    uint64_t tot[3];
    for (int q = 0; q < 3; ++q) TRY(d2h(c, tot + q, dp<uint64_t>(c->j_coff3) + (size_t)q * (ntiles + 1) + ntiles));
    unsigned long long derr = 0;
    TRY(d2h(c, &derr, small + 1));
    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "js_sync");
    HIP_TRY(hipGetLastError());
    if (derr != ~0ull) return json_reject(c, info, derr);
    const uint32_t T = (uint32_t)tot[0], N = (uint32_t)tot[1], M = (uint32_t)tot[2];

    // 4. output tables
    for (DevBuf* b : {tg.ns, tg.name, tg.src, tg.netns, &c->j_tflags}) TRY(ensure(*b, (size_t)T * 4));
    TRY(ensure(*tg.flags, (size_t)T));
    TRY(ensure(*tg.roff, ((size_t)T + 1) * 4));
    TRY(ensure(*tg.noff, ((size_t)T + 1) * 4));
    TRY(link_store_alloc(c, *tg.des, N));
    TRY(link_store_alloc(c, *tg.real, M));
    const uint64_t owners = 1 + 9ull * T + 22ull * ((uint64_t)N + M);
    if (owners >= JS_NONE) {
        std::snprintf(g_last_error, sizeof(g_last_error), "ingest: too many records for one document");
        return KDTN_EINVAL;
    }
    TRY(ensure(c->j_owner, (size_t)owners * 4));
    TRY(ensure(c->j_vown, (size_t)nval * 4));
    JsTopoOut to{dp<uint32_t>(*tg.ns), dp<uint32_t>(*tg.name), dp<uint32_t>(*tg.src), dp<uint32_t>(*tg.netns),
                 dp<uint32_t>(c->j_tflags), dp<uint32_t>(*tg.roff), dp<uint32_t>(*tg.noff)};
    k_js_elems_write<<<ntiles, BLOCK, 0, s>>>(dp<uint8_t>(c->j_ecls), ntok, dp<uint64_t>(c->j_coff3), ntiles, ord, to);
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(to.real_off + T), (int)M, 1, s));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(to.des_off + T), (int)N, 1, s));
    // the values land in row-major staging (one record's 88 B written by the wave that decodes
    // it), whole tiles per side so the finalize pass reads full tiles; it writes the AoSoA tiles
    const uint64_t des_tiles = ((uint64_t)N + TILE_RECS - 1) / TILE_RECS, real_tiles = ((uint64_t)M + TILE_RECS - 1) / TILE_RECS;
    const size_t rows_bytes = (size_t)(des_tiles + real_tiles) * TILE_WORDS * 4;
    TRY(ensure(c->j_rows, std::max<size_t>(rows_bytes, 16)));
    JsStore des{dp<uint32_t>(c->j_rows)};
    JsStore real{dp<uint32_t>(c->j_rows) + (size_t)des_tiles * TILE_WORDS};

    // 5. schema values + interning; a table or heap that fills up is grown and the pass rerun
    // A table that fills up (or whose probe runs grow past JS_MAX_PROBE) is grown 4x and the
    // pass rerun. (Sized for fewer distinct strings — half a key string per record — the config-2
    // document, 12M distinct key strings, overflowed its first table after 217 ms of ever longer
    // probe runs; the decode time does not depend on the table's footprint at these sizes.)
    uint32_t kcap = std::max(c->j_kcap, next_pow2(std::max<uint64_t>(1024, 2ull * ((uint64_t)N + M) + 4ull * T)));
    uint32_t pcap = std::max(c->j_pcap, next_pow2(std::max<uint64_t>(1024, ((uint64_t)N + M) / 2 + 64)));
    uint64_t hcap = std::max<uint64_t>(1 << 20, c->j_n / 16);
    JsIntern in{};
    for (int attempt = 0;; ++attempt) {
        TRY(ensure(c->j_kslots, (size_t)kcap * sizeof(JsSlot)));
        TRY(ensure(c->j_krep, (size_t)kcap * 4));
        TRY(ensure(c->j_pslots, (size_t)pcap * sizeof(JsSlot)));
        TRY(ensure(c->j_prep, (size_t)pcap * 4));
        TRY(ensure(c->j_heap, (size_t)hcap + 64));
        TRY(ensure(c->j_kkeys, (size_t)kcap * 8));
        TRY(ensure(c->j_pkeys, (size_t)pcap * 8));
        HIP_TRY(hipMemsetAsync(c->j_kslots.p, 0, (size_t)kcap * sizeof(JsSlot), s));
        HIP_TRY(hipMemsetAsync(c->j_kkeys.p, 0, (size_t)kcap * 8, s));
        HIP_TRY(hipMemsetAsync(c->j_pkeys.p, 0, (size_t)pcap * 8, s));
        HIP_TRY(hipMemsetAsync(c->j_krep.p, 0xFF, (size_t)kcap * 4, s));
        HIP_TRY(hipMemsetAsync(c->j_pslots.p, 0, (size_t)pcap * sizeof(JsSlot), s));
        HIP_TRY(hipMemsetAsync(c->j_prep.p, 0xFF, (size_t)pcap * 4, s));
        HIP_TRY(hipMemsetAsync(small + 2, 0, J_SMALL - 16, s));
        HIP_TRY(hipMemsetAsync(small + 1, 0xFF, 8, s));
        for (DevBuf* b : {tg.ns, tg.name, tg.src, tg.netns})
            HIP_TRY(hipMemsetAsync(b->p, 0, (size_t)T * 4, s));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(to.flags), (int)(KDTN_TOPO_SPEC_NIL | KDTN_TOPO_STATUS_NIL),
                                  T, s));
        if (rows_bytes) HIP_TRY(hipMemsetAsync(c->j_rows.p, 0, rows_bytes, s));   // absent fields: id 0, uid 0
        in.doc = j.doc;
        in.heap = dp<uint8_t>(c->j_heap);
        in.heap_used = small + 2;
        in.heap_cap = hcap;
        in.status = reinterpret_cast<uint32_t*>(small + 3);
        in.owner = dp<uint32_t>(c->j_owner);
        in.vown = dp<uint32_t>(c->j_vown);
        in.own_des = 1 + 9 * T;
        in.own_real = in.own_des + 22 * N;
#if KDTN_PROFILING
        in.variant = (uint32_t)std::strtoul(std::getenv("KDTN_JS_VARIANT") ? std::getenv("KDTN_JS_VARIANT") : "0",
                                            nullptr, 0);
#else
        in.variant = 0;
#endif
        in.kd = JsDict{dp<JsSlot>(c->j_kslots), dp<unsigned long long>(c->j_kkeys), dp<uint32_t>(c->j_krep), kcap - 1};
        in.pd = JsDict{dp<JsSlot>(c->j_pslots), dp<unsigned long long>(c->j_pkeys), dp<uint32_t>(c->j_prep), pcap - 1};
        if (nval)
            k_js_values<<<nblocks(nval), BLOCK, 0, s>>>(j, tk, dp<uint32_t>(c->j_vlist), nval, par, role, ord, to,
                                                        des, real, in, small + 1);
        if (nval && !(KDTN_PROFILING && (in.variant & JSV_NO_SEEN))) {
            uint32_t* any_dup = reinterpret_cast<uint32_t*>(small + 5);   // zeroed with the small words
            k_js_dups<<<nblocks(nval), BLOCK, 0, s>>>(dp<uint32_t>(c->j_vlist), nval, dp<uint32_t>(c->j_vown),
                                                      dp<uint32_t>(c->j_owner), any_dup);
            k_js_dups_report<<<std::min<uint32_t>(nblocks(nval), 2048), BLOCK, 0, s>>>(
                tk.pos, dp<uint32_t>(c->j_vlist), nval, dp<uint32_t>(c->j_vown), dp<uint32_t>(c->j_owner), any_dup,
                small + 1);
        }
        timer_mark(c, "js_values");
        unsigned long long ctl[3];
        TRY(d2h(c, ctl, small + 1, 3));
        HIP_TRY(hipStreamSynchronize(s));
        timer_mark(c, "js_sync");
        HIP_TRY(hipGetLastError());
        const uint32_t status = (uint32_t)ctl[2];
        if (status & JS_ST_LONG) {
            std::snprintf(g_last_error, sizeof(g_last_error), "a schema string is longer than 16 MiB");
            return KDTN_EINVAL;
        }
        if (status & JS_ST_OVERFLOW) {                  // a table filled up or the heap ran out
            if (attempt >= 6) return KDTN_ENOMEM;
            if (ctl[1] > hcap) hcap = std::max<uint64_t>(hcap * 4, ctl[1] + (1 << 20));
            else { kcap = std::min<uint64_t>((uint64_t)kcap * 4, 1u << 31); pcap = std::min<uint64_t>((uint64_t)pcap * 4, 1u << 31); }
            continue;
        }
        if (ctl[0] != ~0ull) return json_reject(c, info, ctl[0]);
        break;
    }

    // 6. ids in first-occurrence order, dictionaries, id columns
    uint64_t kbytes = 0, pbytes = 0;
    uint32_t D = 0, P = 0;
    TRY(json_dict(c, in.kd, in, ntok, c->j_kslot_id, *tg.kd_bytes, *tg.kd_offs, &D, &kbytes));
    TRY(json_dict(c, in.pd, in, ntok, c->j_pslot_id, *tg.pd_bytes, *tg.pd_offs, &P, &pbytes));
    // keep the intern tables at most half full for the next document of this shape
    c->j_kcap = std::max(kcap, next_pow2(2ull * D));
    c->j_pcap = std::max(pcap, next_pow2(2ull * P));
    if (N) k_js_finalize_links<<<(uint32_t)des_tiles, BLOCK, 0, s>>>(des.base, dp<uint32_t>(tg.des->buf),
                                                                       dp<uint32_t>(c->j_kslot_id), dp<uint32_t>(c->j_pslot_id));
    if (M) k_js_finalize_links<<<(uint32_t)real_tiles, BLOCK, 0, s>>>(real.base, dp<uint32_t>(tg.real->buf),
                                                                        dp<uint32_t>(c->j_kslot_id), dp<uint32_t>(c->j_pslot_id));
    if (T) k_js_finalize_topos<<<nblocks(T), BLOCK, 0, s>>>(to, T, dp<uint32_t>(c->j_kslot_id), dp<uint8_t>(*tg.flags));
    timer_mark(c, "js_intern");
    HIP_TRY(hipGetLastError());
    *o = JsCounts{T, N, M, D, P, kbytes, pbytes};
    return KDTN_OK;
}

}  // namespace host
}  // namespace kdtn

extern "C" {

// A full ingest (JSON or wire) replaces the context's tables: what it resets first, where it
// decodes to, and (ingest_install) what kdtn_epoch_upload would set up around the decoded tables.
static void ingest_reset(kdtn_ctx* c) {
    c->sh_T = 0;
    g_last_error[0] = 0;
    c->uploaded = false;
    c->ran = false;
    c->kd_valid = c->pd_valid = c->kd_from = c->pd_from = 0;   // the document's dictionaries are new
    c->si_k = c->si_p = c->se_k = c->se_p = 0;
    c->ix_k.n = c->ix_k.mask = c->ix_p.n = c->ix_p.mask = 0;     // (their string indexes too)
}
static JsTargets ingest_targets(kdtn_ctx* c) {
    return JsTargets{&c->t_ns, &c->t_name, &c->t_src, &c->t_netns, &c->t_flags, &c->t_roff, &c->t_noff,
                     &c->des, &c->real, &c->kd_bytes, &c->kd_offs, &c->pd_bytes, &c->pd_offs};
}
static int ingest_install(kdtn_ctx* c, const JsCounts& k, const kdtn_vni_table* vnis, kdtn_ingest_info* info);

static int json_ingest_full(kdtn_ctx* c, const kdtn_vni_table* vnis, kdtn_ingest_info* info) {
    if (!c || !c->j_loaded) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    ingest_reset(c);
    const JsTargets tg = ingest_targets(c);
    JsCounts k{};
    TRY(json_decode(c, tg, &k, info));
    return ingest_install(c, k, vnis, info);
}

static int ingest_install(kdtn_ctx* c, const JsCounts& k, const kdtn_vni_table* vnis, kdtn_ingest_info* info) {
    hipStream_t s = c->stream;
    const uint32_t T = k.T, N = k.N, M = k.M;
    const uint64_t kbytes = k.kbytes, pbytes = k.pbytes;
    c->T = T;
    c->D = k.D;
    c->P = k.P;

    // 7. the epoch inputs are in place: finish what kdtn_epoch_upload would set up
    TRY(prepare_dicts(c));
    const kdtn_vni_table none{0, nullptr, nullptr, nullptr};
    const kdtn_vni_table& vn = vnis ? *vnis : none;
    TRY(check_vnis(c, vn, c->D, 0u));             // the engine's own dictionary: no kept prefix
    TRY(prepare_epoch(c, vn, T, M, N));
    HIP_TRY(hipStreamSynchronize(s));
    c->j_info.n_topos = T;
    c->j_info.n_desired = N;
    c->j_info.n_realised = M;
    c->j_info.n_kdict = c->D;
    c->j_info.n_pdict = c->P;
    c->j_info.kdict_bytes = kbytes;
    c->j_info.pdict_bytes = pbytes;
    c->kd_arena = kbytes;
    c->pd_arena = pbytes;
    if (info) *info = c->j_info;
    c->j_done = true;
    c->uploaded = true;
    c->pods_ready = false;
    c->pods_delta = false;
    return KDTN_OK;
}

int kdtn_json_ingest(kdtn_ctx* c, const kdtn_vni_table* vnis, kdtn_ingest_info* info) {
    if (c) end_shard_ingest(c);
    if (c && c->nranks > 1) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "kdtn_json_ingest: single-shard contexts (kdtn_json_ingest_shard for a rank of several)");
        return KDTN_EINVAL;
    }
    return json_ingest_full(c, vnis, info);
}

// The frame pass of a stream of LinksBatchQuery messages (k_uw_frame<0/1>, kdtn_unwire.hip), for
// kdtn_wire_ingest and kdtn_update_ingest: the message table up, the count pass and its scans,
// one host round trip for the frame totals, the lists sized and written. Leaves the views of
// the stream and of the lists in *ui / *fr (merr holds the top-level faults).
static int wire_frames(kdtn_ctx* c, const char* who, uint32_t T, const uint64_t* off, const uint8_t* kind_dev, UwIn* ui,
                       UwFrames* fr, uint32_t* n_link_frames, uint32_t* n_pod_frames) {
    hipStream_t s = c->stream;
    TRY(ensure(c->u_off, ((size_t)T + 1) * 8));
    for (DevBuf* b : {&c->u_nl, &c->u_np}) TRY(ensure(*b, (size_t)T * 4));
    for (DevBuf* b : {&c->u_loff, &c->u_poff, &c->u_merr}) TRY(ensure(*b, ((size_t)T + 1) * 8));
    TRY(ensure(c->u_ctl, UW_CTL_WORDS * 8));
    if (T) HIP_TRY(hipMemcpyAsync(c->u_off.p, off, ((size_t)T + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c->u_merr.p, 0xFF, ((size_t)T + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(c->u_ctl.p, 0, UW_CTL_WORDS * 8, s));
    HIP_TRY(hipMemsetAsync(dp<unsigned long long>(c->u_ctl) + UW_CTL_FIRST_LONG, 0xFF, 8, s));
    *ui = UwIn{dp<uint8_t>(c->j_doc), (uint32_t)c->j_n, (uint32_t)((size_t)c->j_nb * 64 + 128), T,
               dp<uint64_t>(c->u_off), kind_dev};
    *fr = UwFrames{dp<uint32_t>(c->u_nl), dp<uint32_t>(c->u_np), dp<uint64_t>(c->u_loff), dp<uint64_t>(c->u_poff),
                   nullptr, nullptr, nullptr, dp<unsigned long long>(c->u_merr), dp<unsigned long long>(c->u_ctl)};
    const uint32_t nwave = nblocks(T, 64);
    if (T) k_uw_frame<false><<<nwave, UW_BLOCK, 0, s>>>(*ui, *fr);
    TRY(scan_u32(c, fr->nl, T, dp<uint64_t>(c->u_loff)));
    TRY(scan_u32(c, fr->np, T, dp<uint64_t>(c->u_poff)));
    timer_mark(c, "uw_frame_count");
    uint64_t nlf64 = 0, npf64 = 0;
    TRY(d2h(c, &nlf64, fr->loff + T));
    TRY(d2h(c, &npf64, fr->poff + T));
    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "uw_sync");
    HIP_TRY(hipGetLastError());
    if (nlf64 >= 0xFFFFFFFFull || npf64 >= 0xFFFFFFFFull) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: too many links for one stream", who);
        return KDTN_EINVAL;
    }
    const uint32_t NF = (uint32_t)nlf64, NP = (uint32_t)npf64;
    TRY(ensure(c->u_lfr, (size_t)NF * 8));
    TRY(ensure(c->u_lmsg, (size_t)NF * 4));
    TRY(ensure(c->u_pfr, (size_t)NP * 8));
    fr->lfr = dp<uint2>(c->u_lfr);
    fr->lmsg = dp<uint32_t>(c->u_lmsg);
    fr->pfr = dp<uint2>(c->u_pfr);
    if (T) k_uw_frame<true><<<nwave, UW_BLOCK, 0, s>>>(*ui, *fr);
    timer_mark(c, "uw_frame_write");
    *n_link_frames = NF;
    *n_pod_frames = NP;
    return KDTN_OK;
}

// LinksBatchQuery streams → the context's epoch tables (kdtn_unwire.hip). Host round trips:
// the frame totals (to size the frame lists), the record totals with the error bytes (to size
// the stores), the intern status (again only when a table is grown), then the dictionary finish's.
int kdtn_wire_ingest(kdtn_ctx* c, const kdtn_wire_in* in, kdtn_ingest_info* info) {
    if (!c || !in || !c->j_loaded || (in->n_msgs && (!in->off || !in->kind))) return KDTN_EINVAL;
    end_shard_ingest(c);
    if (c->nranks > 1) {
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_wire_ingest: single-shard contexts");
        return KDTN_EINVAL;
    }
    const uint32_t T = in->n_msgs;
    for (uint32_t m = 0; m < T; ++m) {
        if (in->off[m + 1] < in->off[m] || in->off[m + 1] > c->j_n || in->kind[m] > KDTN_BATCH_UPD) {
            std::snprintf(g_last_error, sizeof(g_last_error),
                          "kdtn_wire_ingest: message %u: offsets must ascend within the uploaded %llu bytes, kind <= 2",
                          m, (unsigned long long)c->j_n);
            return KDTN_EINVAL;
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    ingest_reset(c);
    hipStream_t s = c->stream;
    c->u_done = false;
    c->j_done = false;
    c->j_info = kdtn_ingest_info{};
    stage_begin(c);
    const JsTargets tg = ingest_targets(c);

    // 1. the message table and the frame pass
    for (DevBuf* b : {&c->u_cdes, &c->u_creal, &c->u_rbase}) TRY(ensure(*b, (size_t)T * 4));
    for (DevBuf* b : {&c->u_des64, &c->u_real64}) TRY(ensure(*b, ((size_t)T + 1) * 8));
    TRY(ensure(c->u_kind, (size_t)T));
    TRY(ensure(c->u_err8, (size_t)T));
    TRY(ensure(c->j_small, J_SMALL));
    if (T) HIP_TRY(hipMemcpyAsync(c->u_kind.p, in->kind, T, hipMemcpyHostToDevice, s));
    UwIn ui{};
    UwFrames fr{};
    uint32_t NF = 0, NP = 0;
    TRY(wire_frames(c, "kdtn_wire_ingest", T, in->off, dp<uint8_t>(c->u_kind), &ui, &fr, &NF, &NP));

    // 2. the nested decode for its errors; record counts per side
    for (DevBuf* b : {tg.ns, tg.name, tg.src, tg.netns, &c->j_tflags}) TRY(ensure(*b, (size_t)T * 4));
    TRY(ensure(*tg.flags, (size_t)T));
    TRY(ensure(*tg.roff, ((size_t)T + 1) * 4));
    TRY(ensure(*tg.noff, ((size_t)T + 1) * 4));
    JsTopoOut to{dp<uint32_t>(*tg.ns), dp<uint32_t>(*tg.name), dp<uint32_t>(*tg.src), dp<uint32_t>(*tg.netns),
                 dp<uint32_t>(c->j_tflags), dp<uint32_t>(*tg.roff), dp<uint32_t>(*tg.noff)};
    JsIntern it{};
    const JsStore none{nullptr};
    if (NF) k_uw_links<false><<<nblocks(NF, 64), UW_BLOCK, 0, s>>>(ui, fr, NF, nullptr, none, none, it);
    if (T) k_uw_pods<false><<<nblocks(T), BLOCK, 0, s>>>(ui, fr, to, it);
    timer_mark(c, "uw_check");
    if (T) k_uw_counts<<<nblocks(T), BLOCK, 0, s>>>(ui, fr, dp<uint32_t>(c->u_cdes), dp<uint32_t>(c->u_creal),
                                                   dp<uint8_t>(c->u_err8));
    TRY(scan_u32(c, dp<uint32_t>(c->u_cdes), T, dp<uint64_t>(c->u_des64)));
    TRY(scan_u32(c, dp<uint32_t>(c->u_creal), T, dp<uint64_t>(c->u_real64)));
    k_uw_offsets<<<nblocks((uint64_t)T + 1), BLOCK, 0, s>>>(ui, dp<uint64_t>(c->u_des64), dp<uint64_t>(c->u_real64), to,
                                                            dp<uint32_t>(c->u_rbase));
    timer_mark(c, "uw_counts");
    uint64_t n64 = 0, m64 = 0;
    unsigned long long ctl[UW_CTL_WORDS] = {};
    TRY(d2h(c, &n64, dp<uint64_t>(c->u_des64) + T));
    TRY(d2h(c, &m64, dp<uint64_t>(c->u_real64) + T));
    TRY(d2h(c, ctl, c->u_ctl.p, UW_CTL_WORDS));
    std::vector<uint8_t> herr(T);
    if (T) HIP_TRY(hipMemcpyAsync(herr.data(), c->u_err8.p, T, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    timer_mark(c, "uw_sync");
    HIP_TRY(hipGetLastError());
    const uint32_t N = (uint32_t)n64, M = (uint32_t)m64;
    uint32_t nrej = 0;
    for (uint32_t m = 0; m < T; ++m) nrej += herr[m] != 0;
    if (in->err && T) std::memcpy(in->err, herr.data(), T);
    c->j_info.n_tokens = ctl[UW_CTL_FIELDS];

    // 3. stores, intern tables; the intern pass, rerun with larger tables when one fills up
    TRY(link_store_alloc(c, *tg.des, N));
    TRY(link_store_alloc(c, *tg.real, M));
    const uint64_t des_tiles = ((uint64_t)N + TILE_RECS - 1) / TILE_RECS, real_tiles = ((uint64_t)M + TILE_RECS - 1) / TILE_RECS;
    const size_t rows_bytes = (size_t)(des_tiles + real_tiles) * TILE_WORDS * 4;
    TRY(ensure(c->j_rows, std::max<size_t>(rows_bytes, 16)));
    const JsStore des{dp<uint32_t>(c->j_rows)};
    const JsStore real{dp<uint32_t>(c->j_rows) + (size_t)des_tiles * TILE_WORDS};
    uint32_t kcap = std::max(c->j_kcap, next_pow2(std::max<uint64_t>(1024, 2ull * ((uint64_t)N + M) + 4ull * T)));
    uint32_t pcap = std::max(c->j_pcap, next_pow2(std::max<uint64_t>(1024, ((uint64_t)N + M) / 2 + 64)));
    unsigned long long* small = dp<unsigned long long>(c->j_small);
    TRY(ensure(c->j_heap, 64));                          // (no decoded strings: wire strings are raw bytes)
    uint32_t passes = 0;
    for (int attempt = 0;; ++attempt) {
        TRY(ensure(c->j_kslots, (size_t)kcap * sizeof(JsSlot)));
        TRY(ensure(c->j_krep, (size_t)kcap * 4));
        TRY(ensure(c->j_pslots, (size_t)pcap * sizeof(JsSlot)));
        TRY(ensure(c->j_prep, (size_t)pcap * 4));
        TRY(ensure(c->j_kkeys, (size_t)kcap * 8));
        TRY(ensure(c->j_pkeys, (size_t)pcap * 8));
        HIP_TRY(hipMemsetAsync(c->j_kslots.p, 0, (size_t)kcap * sizeof(JsSlot), s));
        HIP_TRY(hipMemsetAsync(c->j_kkeys.p, 0, (size_t)kcap * 8, s));
        HIP_TRY(hipMemsetAsync(c->j_pkeys.p, 0, (size_t)pcap * 8, s));
        HIP_TRY(hipMemsetAsync(c->j_krep.p, 0xFF, (size_t)kcap * 4, s));
        HIP_TRY(hipMemsetAsync(c->j_pslots.p, 0, (size_t)pcap * sizeof(JsSlot), s));
        HIP_TRY(hipMemsetAsync(c->j_prep.p, 0xFF, (size_t)pcap * 4, s));
        HIP_TRY(hipMemsetAsync(small, 0, J_SMALL, s));
        for (DevBuf* b : {tg.ns, tg.name, tg.src, tg.netns, &c->j_tflags})   // rejected messages: "" and no flags
            if (T) HIP_TRY(hipMemsetAsync(b->p, 0, (size_t)T * 4, s));
        if (rows_bytes) HIP_TRY(hipMemsetAsync(c->j_rows.p, 0, rows_bytes, s));
        it = JsIntern{};
        it.doc = ui.doc;
        it.heap = dp<uint8_t>(c->j_heap);
        it.heap_used = small + 2;
        it.status = reinterpret_cast<uint32_t*>(small + 3);
        it.kd = JsDict{dp<JsSlot>(c->j_kslots), dp<unsigned long long>(c->j_kkeys), dp<uint32_t>(c->j_krep), kcap - 1};
        it.pd = JsDict{dp<JsSlot>(c->j_pslots), dp<unsigned long long>(c->j_pkeys), dp<uint32_t>(c->j_prep), pcap - 1};
        if (NF) k_uw_links<true><<<nblocks(NF, 64), UW_BLOCK, 0, s>>>(ui, fr, NF, dp<uint32_t>(c->u_rbase), des, real, it);
        if (T) k_uw_pods<true><<<nblocks(T), BLOCK, 0, s>>>(ui, fr, to, it);
        timer_mark(c, "uw_intern");
        unsigned long long st = 0;
        TRY(d2h(c, &st, small + 3));
        HIP_TRY(hipStreamSynchronize(s));
        timer_mark(c, "uw_sync");
        HIP_TRY(hipGetLastError());
        ++passes;
        if ((uint32_t)st & JS_ST_LONG) {
            std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_wire_ingest: a string is longer than 16 MiB");
            return KDTN_EINVAL;
        }
        if ((uint32_t)st & JS_ST_OVERFLOW) {
            if (attempt >= 6) return KDTN_ENOMEM;
            kcap = (uint32_t)std::min<uint64_t>((uint64_t)kcap * 4, 1u << 31);
            pcap = (uint32_t)std::min<uint64_t>((uint64_t)pcap * 4, 1u << 31);
            continue;
        }
        break;
    }

    // 4. the ingest's finish: first-occurrence ids (occurrence = stream offset / 2), dictionaries
    uint64_t kbytes = 0, pbytes = 0;
    uint32_t D = 0, P = 0;
    const uint32_t nocc = (uint32_t)(c->j_n / 2 + 1);
    TRY(json_dict(c, it.kd, it, nocc, c->j_kslot_id, *tg.kd_bytes, *tg.kd_offs, &D, &kbytes));
    TRY(json_dict(c, it.pd, it, nocc, c->j_pslot_id, *tg.pd_bytes, *tg.pd_offs, &P, &pbytes));
    c->j_kcap = std::max(kcap, next_pow2(2ull * D));
    c->j_pcap = std::max(pcap, next_pow2(2ull * P));
    if (N) k_js_finalize_links<<<(uint32_t)des_tiles, BLOCK, 0, s>>>(des.base, dp<uint32_t>(tg.des->buf),
                                                                       dp<uint32_t>(c->j_kslot_id), dp<uint32_t>(c->j_pslot_id));
    if (M) k_js_finalize_links<<<(uint32_t)real_tiles, BLOCK, 0, s>>>(real.base, dp<uint32_t>(tg.real->buf),
                                                                        dp<uint32_t>(c->j_kslot_id), dp<uint32_t>(c->j_pslot_id));
    if (T) k_js_finalize_topos<<<nblocks(T), BLOCK, 0, s>>>(to, T, dp<uint32_t>(c->j_kslot_id), dp<uint8_t>(*tg.flags));
    timer_mark(c, "js_intern");
    HIP_TRY(hipGetLastError());
    c->u_plan = kdtn_wire_plan{UW_WIN, (uint32_t)ctl[UW_CTL_N_LONG], (uint32_t)ctl[UW_CTL_FIRST_LONG], NF, NP, nrej, passes, 0u};
    const JsCounts k{T, N, M, D, P, kbytes, pbytes};
    TRY(ingest_install(c, k, nullptr, info));
    c->u_done = true;
    return KDTN_OK;
}

int kdtn_wire_ingest_plan(kdtn_ctx* c, kdtn_wire_plan* out) {
    if (!c || !out || !c->u_done) return KDTN_EINVAL;
    *out = c->u_plan;
    return KDTN_OK;
}

// RemotePod bodies → Remote.Update plans (kdtn_remote.hip). Two launches and one
// synchronisation: the report block and the records come back together. Touches only its own
// buffers and the uploaded bytes, so the context's epoch state stays as it was.
int kdtn_remote_ingest(kdtn_ctx* c, const kdtn_remote_in* in, kdtn_remote_plan* plan, kdtn_qdisc* qdisc) {
    if (!c || !in || !c->j_loaded) return KDTN_EINVAL;
    const uint32_t n = in->n_msgs, nv = in->n_vni;
    if ((n && (!in->start || !in->size || !plan)) || (nv && (!in->vni || !in->vni_ns.offs || in->vni_ns.n != nv)))
        return KDTN_EINVAL;
    g_last_error[0] = 0;
    for (uint32_t m = 0; m < n; ++m) {
        if (in->start[m] > c->j_n || in->size[m] > c->j_n - in->start[m]) {
            std::snprintf(g_last_error, sizeof(g_last_error),
                          "kdtn_remote_ingest: body %u reaches past the uploaded %llu bytes", m, (unsigned long long)c->j_n);
            return KDTN_EINVAL;
        }
    }
    for (uint32_t i = 0; i < nv; ++i) {
        if (in->vni_ns.offs[i + 1] < in->vni_ns.offs[i] || (!in->vni_ns.bytes && in->vni_ns.offs[nv])) {
            std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_remote_ingest: vni_ns offsets must ascend");
            return KDTN_EINVAL;
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->ri_done = false;
    const uint32_t cap = next_pow2(2ull * nv);               // a power of two >= 2 n_vni (and >= 64)
    uint32_t bits = 0;
    while ((1u << bits) < cap) ++bits;
    StreamsDrain drain{s, s};                                // (the copies below read caller memory)
    TRY(upload(c, c->ri_start, in->start, (size_t)n * 8));
    TRY(upload(c, c->ri_size, in->size, (size_t)n * 4));
    TRY(upload(c, c->ri_vni, in->vni, (size_t)nv * 4));
    TRY(upload(c, c->ri_nso, in->vni_ns.offs, nv ? ((size_t)nv + 1) * 4 : 0));
    TRY(upload(c, c->ri_nsb, in->vni_ns.bytes, nv ? in->vni_ns.offs[nv] : 0));
    TRY(ensure(c->ri_slots, (size_t)cap * 4));
    TRY(ensure(c->ri_plan, (size_t)n * sizeof(kdtn_remote_plan)));
    TRY(ensure(c->ri_qd, (size_t)n * sizeof(kdtn_qdisc)));
    TRY(ensure(c->ri_ctl, RP_CTL_WORDS * 4));
    HIP_TRY(hipMemsetAsync(c->ri_slots.p, 0xFF, (size_t)cap * 4, s));
    HIP_TRY(hipMemsetAsync(c->ri_ctl.p, 0, RP_CTL_WORDS * 4, s));
    stage_begin(c);
    if (nv) k_rp_vni_build<<<nblocks(nv), BLOCK, 0, s>>>(dp<int32_t>(c->ri_vni), nv, dp<uint32_t>(c->ri_slots), cap - 1, 32u - bits);
    timer_mark(c, "rp_vni_build");
    const RpIn ri{dp<uint8_t>(c->j_doc), n, dp<uint64_t>(c->ri_start), dp<uint32_t>(c->ri_size), nv, dp<int32_t>(c->ri_vni),
                  dp<uint8_t>(c->ri_nsb), dp<uint32_t>(c->ri_nso), dp<uint32_t>(c->ri_slots), cap - 1, 32u - bits,
                  c->cfg.tick_in_usec};
    if (n) k_rp_plan<<<nblocks(n, 64), UW_BLOCK, 0, s>>>(ri, dp<uint4>(c->ri_plan), qdisc ? dp<uint2>(c->ri_qd) : nullptr,
                                                        dp<uint32_t>(c->ri_ctl));
    timer_mark(c, "rp_plan");
    HIP_TRY(hipGetLastError());
    uint32_t ctl[RP_CTL_WORDS] = {};
    TRY(d2h(c, ctl, c->ri_ctl.p, RP_CTL_WORDS));
    if (n) HIP_TRY(hipMemcpyAsync(plan, c->ri_plan.p, (size_t)n * sizeof(kdtn_remote_plan), hipMemcpyDeviceToHost, s));
    if (n && qdisc) HIP_TRY(hipMemcpyAsync(qdisc, c->ri_qd.p, (size_t)n * sizeof(kdtn_qdisc), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    c->ri_report = kdtn_remote_ingest_plan_t{UW_WIN, ctl[RP_CTL_DIRECT], ctl[RP_CTL_REJECTED], ctl[RP_CTL_CONFLICT]};
    c->ri_done = true;
    return KDTN_OK;
}

int kdtn_remote_ingest_plan(kdtn_ctx* c, kdtn_remote_ingest_plan_t* out) {
    if (!c || !out || !c->ri_done) return KDTN_EINVAL;
    *out = c->ri_report;
    return KDTN_OK;
}

// Copies of the last batch's records to the caller (the records stay in ul_msg / ul_link / ul_qd)
static int update_fetch(kdtn_ctx* c, kdtn_update_out* out, uint32_t n_links) {
    hipStream_t s = c->stream;
    const uint32_t T = c->ul_T;
    if (T) HIP_TRY(hipMemcpyAsync(out->msg, c->ul_msg.p, (size_t)T * sizeof(kdtn_update_msg), hipMemcpyDeviceToHost, s));
    if (n_links && out->link)
        HIP_TRY(hipMemcpyAsync(out->link, c->ul_link.p, (size_t)n_links * sizeof(kdtn_update_link), hipMemcpyDeviceToHost, s));
    if (n_links && out->link && out->qdisc)
        HIP_TRY(hipMemcpyAsync(out->qdisc, c->ul_qd.p, (size_t)n_links * sizeof(kdtn_qdisc), hipMemcpyDeviceToHost, s));
    return KDTN_OK;
}

// UpdateLinks bodies → per-link plans (kdtn_update.hip). One host round trip inside the call,
// the frame totals that size the lists; the report block and the records come back together at
// the end. The placed records hold at most one per link frame, so their copies are enqueued
// before the surviving count is known. Touches only the frame pass's lists, its own buffers
// and the uploaded bytes: the context's epoch state stays as it was.
int kdtn_update_ingest(kdtn_ctx* c, const kdtn_update_in* in, kdtn_update_out* out) {
    if (!c || !out) return KDTN_EINVAL;
    g_last_error[0] = 0;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!in) {                                               // the last batch's records again
        if (!c->ul_done || (c->ul_T && !out->msg)) return KDTN_EINVAL;
        out->n_links = c->ul_report.n_links;
        StreamsDrain drain{s, s};
        TRY(update_fetch(c, out, out->link_cap >= out->n_links ? out->n_links : 0u));
        HIP_TRY(hipStreamSynchronize(s));
        drain.armed = false;
        return KDTN_OK;
    }
    const uint32_t T = in->n_msgs;
    if (!c->j_loaded || (T && (!in->off || !out->msg))) return KDTN_EINVAL;
    for (uint32_t m = 0; m < T; ++m) {
        if (in->off[m + 1] < in->off[m] || in->off[m + 1] > c->j_n) {
            std::snprintf(g_last_error, sizeof(g_last_error),
                          "kdtn_update_ingest: message %u: offsets must ascend within the uploaded %llu bytes", m,
                          (unsigned long long)c->j_n);
            return KDTN_EINVAL;
        }
    }
    c->ul_done = false;
    StreamsDrain drain{s, s};                                // (the copies below read caller memory)
    stage_begin(c);
    UwIn ui{};
    UwFrames fr{};
    uint32_t NF = 0, NP = 0;
    TRY(wire_frames(c, "kdtn_update_ingest", T, in->off, nullptr, &ui, &fr, &NF, &NP));

    TRY(ensure(c->ul_cut, (size_t)T * 8));
    TRY(ensure(c->ul_cnt, (size_t)T * 4));
    TRY(ensure(c->ul_base64, ((size_t)T + 1) * 8));
    TRY(ensure(c->ul_msg, (size_t)T * sizeof(kdtn_update_msg)));
    for (DevBuf* b : {&c->ul_link0, &c->ul_link}) TRY(ensure(*b, (size_t)NF * sizeof(kdtn_update_link)));
    for (DevBuf* b : {&c->ul_qd0, &c->ul_qd}) TRY(ensure(*b, (size_t)NF * sizeof(kdtn_qdisc)));
    TRY(ensure(c->ul_ctl, UL_CTL_WORDS * 4));
    if (T) HIP_TRY(hipMemsetAsync(c->ul_cut.p, 0xFF, (size_t)T * 8, s));
    HIP_TRY(hipMemsetAsync(c->ul_ctl.p, 0, UL_CTL_WORDS * 4, s));
    const UlOut uo{dp<uint4>(c->ul_link0), dp<uint2>(c->ul_qd0), dp<unsigned long long>(c->ul_cut), dp<uint32_t>(c->ul_ctl)};
    if (NF) k_ul_plan<<<nblocks(NF, 64), UW_BLOCK, 0, s>>>(ui, fr, NF, c->cfg.tick_in_usec, uo);
    timer_mark(c, "ul_plan");
    if (T) k_ul_msgs<<<nblocks(T), BLOCK, 0, s>>>(ui, fr, uo, dp<uint4>(c->ul_msg), dp<uint32_t>(c->ul_cnt));
    TRY(scan_u32(c, dp<uint32_t>(c->ul_cnt), T, dp<uint64_t>(c->ul_base64)));
    const uint64_t nthr = std::max<uint64_t>(13ull * NF, T);
    if (nthr) k_ul_pack<<<nblocks(nthr), BLOCK, 0, s>>>(fr, T, NF, dp<uint64_t>(c->ul_base64), uo, dp<uint4>(c->ul_msg),
                                                       dp<uint2>(c->ul_link), dp<uint2>(c->ul_qd));
    timer_mark(c, "ul_msgs");
    HIP_TRY(hipGetLastError());
    uint32_t ctl[UL_CTL_WORDS] = {};
    unsigned long long wctl[UW_CTL_WORDS] = {};
    uint64_t nl64 = 0;
    TRY(d2h(c, ctl, c->ul_ctl.p, UL_CTL_WORDS));
    TRY(d2h(c, wctl, c->u_ctl.p, UW_CTL_WORDS));
    TRY(d2h(c, &nl64, dp<uint64_t>(c->ul_base64) + T));
    c->ul_T = T;
    TRY(update_fetch(c, out, std::min(NF, out->link_cap)));
    HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    out->n_links = (uint32_t)nl64;
    c->ul_report = kdtn_update_ingest_plan_t{UW_WIN, (uint32_t)wctl[UW_CTL_N_LONG], ctl[UL_CTL_DIRECT], ctl[UL_CTL_REJECTED],
                                             (uint32_t)nl64, ctl[UL_CTL_CUT]};
    c->ul_done = true;
    return KDTN_OK;
}

int kdtn_update_ingest_plan(kdtn_ctx* c, kdtn_update_ingest_plan_t* out) {
    if (!c || !out || !c->ul_done) return KDTN_EINVAL;
    *out = c->ul_report;
    return KDTN_OK;
}

// The whole document decoded as for one GPU, then the epoch cut down to this shard's
// Topologies on the GPU: the full table fills the pod-status rows of every Topology (pod
// index = document index), the shard's topology rows and records are compacted into fresh
// tables that are swapped in, and the context is left as a rank whose pod table is in place.
int kdtn_json_ingest_shard(kdtn_ctx* c, const kdtn_vni_table* vnis, uint32_t nshards, uint32_t shard,
                           kdtn_ingest_info* info) {
    if (!c || nshards < 1 || shard >= nshards || nshards > 0x7FFFFFFFu) return KDTN_EINVAL;
    if (c->comm) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "kdtn_json_ingest_shard: the context has an RCCL communicator (no exchange is needed)");
        return KDTN_EINVAL;
    }
    end_shard_ingest(c);
    const int saved_nranks = c->nranks, saved_rank = c->rank;
    c->nranks = 1;
    c->rank = 0;
    const int rc = json_ingest_full(c, vnis, info);
    if (rc != KDTN_OK || nshards == 1) {
        c->nranks = saved_nranks;
        c->rank = saved_rank;
        return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint32_t Tf = c->T, Mf = c->real.n, Nf = c->des.n;
    const DevTopos full = topo_view(c);
    // 1. selection and the shard's offsets
    for (DevBuf* b : {&c->sh_keep, &c->sh_kreal, &c->sh_kdes}) TRY(ensure(*b, ((size_t)Tf + 1) * 4));
    for (DevBuf* b : {&c->sh_tidx, &c->sh_roff64, &c->sh_noff64}) TRY(ensure(*b, ((size_t)Tf + 1) * 8));
    if (Tf)
        k_shard_mark<<<nblocks(Tf), BLOCK, 0, s>>>(full, dp<uint8_t>(c->kd_bytes), dp<uint32_t>(c->kd_offs), nshards,
                                                   shard, dp<uint32_t>(c->sh_keep), dp<uint32_t>(c->sh_kreal),
                                                   dp<uint32_t>(c->sh_kdes));
    TRY(scan_u32(c, dp<uint32_t>(c->sh_keep), Tf, dp<uint64_t>(c->sh_tidx)));
    TRY(scan_u32(c, dp<uint32_t>(c->sh_kreal), Tf, dp<uint64_t>(c->sh_roff64)));
    TRY(scan_u32(c, dp<uint32_t>(c->sh_kdes), Tf, dp<uint64_t>(c->sh_noff64)));
    uint64_t cnt[3] = {0, 0, 0};
    TRY(d2h(c, cnt, dp<uint64_t>(c->sh_tidx) + Tf));
    TRY(d2h(c, cnt + 1, dp<uint64_t>(c->sh_roff64) + Tf));
    TRY(d2h(c, cnt + 2, dp<uint64_t>(c->sh_noff64) + Tf));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    const uint32_t Ts = (uint32_t)cnt[0], Ms = (uint32_t)cnt[1], Ns = (uint32_t)cnt[2];
    // 2. the shard's tables
    for (DevBuf* b : {&c->sh_ns, &c->sh_name, &c->sh_src, &c->sh_netns, &c->sh_doc}) TRY(ensure(*b, ((size_t)Ts + 1) * 4));
    TRY(ensure(c->sh_flags, (size_t)Ts + 1));
    TRY(ensure(c->sh_roff, ((size_t)Ts + 1) * 4));
    TRY(ensure(c->sh_noff, ((size_t)Ts + 1) * 4));
    TRY(link_store_alloc(c, c->sh_real, Ms));
    TRY(link_store_alloc(c, c->sh_des, Ns));
    HIP_TRY(hipMemsetAsync(c->sh_real.buf.p, 0, c->sh_real.buf.cap, s));   // tile padding as an upload leaves it
    HIP_TRY(hipMemsetAsync(c->sh_des.buf.p, 0, c->sh_des.buf.cap, s));
    DevTopos out{dp<uint32_t>(c->sh_ns), dp<uint32_t>(c->sh_name), dp<uint32_t>(c->sh_src), dp<uint32_t>(c->sh_netns),
                 dp<uint8_t>(c->sh_flags), dp<uint32_t>(c->sh_roff), dp<uint32_t>(c->sh_noff), Ts};
    k_shard_topos<<<nblocks((uint64_t)Tf + 1), BLOCK, 0, s>>>(full, dp<uint32_t>(c->sh_keep), dp<uint64_t>(c->sh_tidx),
                                                              dp<uint64_t>(c->sh_roff64), dp<uint64_t>(c->sh_noff64), out,
                                                              dp<uint32_t>(c->sh_doc));
    if (Mf)
        k_shard_links<<<nblocks(Mf), BLOCK, 0, s>>>(c->real.view, full.real_off, Tf, dp<uint32_t>(c->sh_keep),
                                                    dp<uint64_t>(c->sh_roff64), dp<uint32_t>(c->sh_real.buf));
    if (Nf)
        k_shard_links<<<nblocks(Nf), BLOCK, 0, s>>>(c->des.view, full.des_off, Tf, dp<uint32_t>(c->sh_keep),
                                                    dp<uint64_t>(c->sh_noff64), dp<uint32_t>(c->sh_des.buf));
    HIP_TRY(hipGetLastError());
    // 3. a rank of nshards with every Topology's pod-status row: pod index = document index
    const uint32_t slice = (Tf + nshards - 1) / nshards;
    c->sh_active = true;
    c->sh_saved_nranks = saved_nranks;
    c->sh_saved_rank = saved_rank;
    c->nranks = (int)nshards;
    c->pods_rank_major = false;                         // pod index = document index
    c->rank = (int)shard;
    c->T = Ts;
    const kdtn_vni_table none{0, nullptr, nullptr, nullptr};
    TRY(prepare_epoch(c, vnis ? *vnis : none, slice, Ms, Ns));
    if (c->pod_total)
        k_pods_fill<<<nblocks(c->pod_total), BLOCK, 0, s>>>(full, c->pod_total, 0u, dp<uint4>(c->pods));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                // the full tables are read until here
    std::swap(c->t_ns, c->sh_ns);
    std::swap(c->t_name, c->sh_name);
    std::swap(c->t_src, c->sh_src);
    std::swap(c->t_netns, c->sh_netns);
    std::swap(c->t_flags, c->sh_flags);
    std::swap(c->t_roff, c->sh_roff);
    std::swap(c->t_noff, c->sh_noff);
    std::swap(c->real, c->sh_real);
    std::swap(c->des, c->sh_des);
    c->sh_T = Ts;
    c->pods_imported = true;
    c->j_info.n_topos = Ts;
    c->j_info.n_desired = Ns;
    c->j_info.n_realised = Ms;
    if (info) *info = c->j_info;
    return KDTN_OK;
}

int kdtn_ingest_shard_topos(kdtn_ctx* c, uint32_t* doc_index) {
    if (!c || !c->j_done || (c->sh_T && !doc_index)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (c->nranks == 1) {                            // unsharded: the identity
        for (uint32_t t = 0; t < c->T; ++t) doc_index[t] = t;
        return KDTN_OK;
    }
    if (c->sh_T)
        HIP_TRY(hipMemcpyAsync(doc_index, c->sh_doc.p, (size_t)c->sh_T * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KDTN_OK;
}

int kdtn_ingest_download(kdtn_ctx* c, kdtn_ingest_tables* o) {
    if (!c || !o || !(c->j_done || c->tables_cur)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const kdtn_ingest_info& I = c->j_info;
    auto get = [&](void* dst, const DevBuf& b, size_t bytes) -> int {
        if (dst && bytes) HIP_TRY(hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, s));
        return KDTN_OK;
    };
    TRY(get(o->kd_bytes, c->kd_bytes, I.kdict_bytes));
    TRY(get(o->kd_offs, c->kd_offs, ((size_t)I.n_kdict + 1) * 4));
    TRY(get(o->pd_bytes, c->pd_bytes, I.pdict_bytes));
    TRY(get(o->pd_offs, c->pd_offs, ((size_t)I.n_pdict + 1) * 4));
    const size_t T = I.n_topos;
    TRY(get(o->ns, c->t_ns, T * 4));
    TRY(get(o->name, c->t_name, T * 4));
    TRY(get(o->src_ip, c->t_src, T * 4));
    TRY(get(o->net_ns, c->t_netns, T * 4));
    TRY(get(o->flags, c->t_flags, T));
    TRY(get(o->real_off, c->t_roff, (T + 1) * 4));
    TRY(get(o->des_off, c->t_noff, (T + 1) * 4));
    // AoSoA tiles → SoA columns
    auto cols = [&](const DevLinkStore& st, uint32_t* key, uint32_t* prop, uint32_t* gap, int64_t* uid) -> int {
        const uint32_t n = st.n;
        if (!n) return KDTN_OK;
        const size_t full = n / TILE_RECS, tail = n % TILE_RECS, tile_bytes = (size_t)TILE_WORDS * 4;
        const uint8_t* base = reinterpret_cast<const uint8_t*>(st.view.base);   // (des may read real's buffer)
        auto col = [&](int cidx, void* dst, size_t esz) -> int {
            if (!dst) return KDTN_OK;
            const size_t run = TILE_RECS * esz;
            const uint8_t* src = base + (size_t)cidx * TILE_RECS * 4;
            if (full) HIP_TRY(hipMemcpy2DAsync(dst, run, src, tile_bytes, run, full, hipMemcpyDeviceToHost, s));
            if (tail)
                HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(dst) + full * run, src + full * tile_bytes, tail * esz,
                                       hipMemcpyDeviceToHost, s));
            return KDTN_OK;
        };
        for (int k = 0; k < KDTN_NKEY; ++k) TRY(col(COL_KEY0 + k, key ? key + (size_t)k * n : nullptr, 4));
        for (int k = 0; k < KDTN_NPROP; ++k) TRY(col(COL_PROP0 + k, prop ? prop + (size_t)k * n : nullptr, 4));
        TRY(col(COL_GAP, gap, 4));
        TRY(col(COL_UID, uid, 8));
        return KDTN_OK;
    };
    TRY(cols(c->des, o->des_key, o->des_prop, o->des_gap, o->des_uid));
    TRY(cols(c->real, o->real_key, o->real_prop, o->real_gap, o->real_uid));
    HIP_TRY(hipStreamSynchronize(s));
    return KDTN_OK;
}

}  // extern "C"
