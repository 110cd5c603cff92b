// kdtn_engine.h — private to the host side of libkdtn.so (the kdtn_engine*.hip translation
// units): the context, its owning device buffers, and the helpers more than one of them uses.
// Not installed; the C-ABI is include/kdtn.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kdtn.h"
#include "kdtn_kernels.h"

namespace kdtn {
namespace host {

constexpr int kMaxTimers = 32;

extern thread_local char g_last_error[512];

// Replaced or destroyed device buffers are retired, not freed at once (kdtn_engine.hip).
void retire(void* p, size_t bytes);

// A device allocation and its owner: the destructor and move-assignment retire the pointer
// (never hipFree directly: it synchronises the whole device), a moved-from buffer is null.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            retire(p, cap);
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { retire(p, cap); }
};

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            std::snprintf(g_last_error, sizeof(g_last_error), "%s: %s (%s:%d)", #expr,   \
                          hipGetErrorString(_e), __FILE__, __LINE__);                    \
            return KDTN_EIO;                                                             \
        }                                                                                \
    } while (0)

#define TRY(expr)                   \
    do {                            \
        int _r = (expr);            \
        if (_r != KDTN_OK) return _r; \
    } while (0)

// Link table storage: one allocation in 64-record tiles (AoSoA, kdtn_kernels.h), so kernels
// receive one base pointer per table.
struct DevLinkStore {
    DevBuf buf;
    uint32_t n = 0;
    DevLinks view{};
};

}  // namespace host
}  // namespace kdtn

using namespace kdtn;
using namespace kdtn::host;

// The context's streams, events, SDMA and RCCL handles and pinned host words. A base of kdtn_ctx,
// so its destructor runs after the context's members — every DevBuf — have been retired: it
// frees the retired buffers (retired_flush) and then tears these down. kdtn_destroy
// synchronises every stream before it deletes the context.
struct kdtn_ctx_handles {
    kdtn_ctx_handles() = default;
    kdtn_ctx_handles(const kdtn_ctx_handles&) = delete;
    kdtn_ctx_handles& operator=(const kdtn_ctx_handles&) = delete;
    ~kdtn_ctx_handles();
    int device = 0;
    uint32_t n_cus = 256;
    kdtn_config cfg{};
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;          // RCCL pod-status exchange (nranks > 1)
    hipStream_t copy_stream = nullptr;          // delta uploads: host-to-device copies beside the kernels
    hipEvent_t ev_cp[4] = {};
    hipEvent_t ev_col[LINK_COLS32 + 1] = {};   // a delta's staged column copies (+ uid), each placed on arrival
    hipStream_t d2h_stream = nullptr;           // kdtn_epoch_download_async: the outputs' copies
    hipEvent_t ev_dl_ready = nullptr, ev_dl_done = nullptr;
    bool dl_pending = false;                    // an async download's copies may still be reading outputs
    // Downloads on one SDMA engine (hsa_amd_memory_async_copy_on_engine): the copy engine alone
    // reaches the host link's rate (56 GB/s D2H, profiles/r05d_sdma_probe.jsonl) and takes no
    // CUs, where the runtime's device-to-host copies in this process run as blit kernels. Used
    // when every destination is page-locked host memory, else the HIP copies.
    bool sdma_tried = false, sdma_ok = false, dl_sdma = false;
    bool sdma_inited = false;   // hsa_init held and dl_sig created (outlives sdma_ok after a failed issue)
    hsa_agent_t sdma_gpu{}, sdma_cpu{};
    uint32_t sdma_engine[2] = {0, 0};   // the download's engines (bit masks; [1] = 0: one engine)
    hsa_signal_t dl_sig{};
    hipEvent_t ev_fill = nullptr, ev_ag = nullptr;
    // host-visible counters
    hipEvent_t ev_done = nullptr;  // the epoch's last command (kdtn_epoch_sync polls it)
    uint32_t* h_misc = nullptr;   // pinned: [1]=del, [2]=upd, [3]=add, [4]=look-back error (sync header words)
    // coherent page-locked words the epoch's last kernel writes itself ([0..2] list totals, [3]
    // look-back error): no readback copy per epoch (a 16-B blit kernel, 5.6 µs + a dispatch);
    // kdtn_epoch_sync moves them to h_misc[1..4]
    uint32_t* h_tot = nullptr;
    ncclComm_t comm = nullptr;     // multi-GPU
    hipEvent_t ev[kMaxTimers + 1] = {};   // timers (kdtn_set_timing)
};

struct kdtn_ctx : kdtn_ctx_handles {
    // dictionaries; parsed tables persist across uploads for an append-only interner
    // (kdtn_epoch_in.kdict_keep / pdict_keep): *_valid strings have valid parsed tables, a run
    // parses [*_from, n) — the strings its upload added
    DevBuf kd_bytes, kd_offs, kd_bits, pd_bytes, pd_offs, pd_pct, pd_dur, pd_rate, pd_rerr, kd_special;
    uint32_t D = 0, P = 0;
    uint32_t kd_from = 0, pd_from = 0, kd_valid = 0, pd_valid = 0, kb_cap = 0;
    uint32_t si_k = 0, si_p = 0;           // leading strings whose inline encoder entries are built

    // topologies
    DevBuf t_ns, t_name, t_src, t_netns, t_flags, t_roff, t_noff;
    // sharded ingest: selection, scans, the shard's tables before they are swapped in
    DevBuf sh_keep, sh_kreal, sh_kdes, sh_tidx, sh_roff64, sh_noff64, sh_doc;
    DevBuf sh_ns, sh_name, sh_src, sh_netns, sh_flags, sh_roff, sh_noff;
    uint32_t T = 0;
    // links
    DevLinkStore real, des;
    DevLinkStore sh_real, sh_des;              // sharded ingest: the shard's link stores (swapped in)
    uint32_t sh_T = 0;                         // sharded ingest: topologies of the shard (doc index table)
    // vni table
    DevBuf v_node, v_vni, v_netns, v_ents, v_slots, v_table;
    uint32_t V = 0, vni_mask = 0;
    // kdtn_epoch_vni_apply: ops, snapshot marks, the new map's table, arrays and scan partials
    DevBuf vx_ops, vx_dead, vx_slots, vx_node, vx_vni, vx_netns, vx_part, vx_cut, vx_vis;
    // v_node/v_vni/v_netns: the snapshot of the current upload (what vni_hit is decided
    // against, re-runs included); r_*: the map kdtn_epoch_vni_apply produced, which becomes
    // the next KDTN_VNI_RESIDENT upload's snapshot. The resident map is r_* when vres_in_r.
    DevBuf r_node, r_vni, r_netns;
    bool vres_ok = false;          // a map usable as KDTN_VNI_RESIDENT exists
    bool vres_in_r = false;
    // sharded apply: every rank's ops gathered in rank order ([dels][adds]), by RCCL or imported
    DevBuf vx_cnt, vx_send, vx_recv, vx_gops;
    DevBuf vx_flag, vx_dkeys, vx_dused, vx_cpos, vx_cpart, vx_cnode, vx_cvni;   // order-dependent keys
    uint32_t vx_ncont = 0;
    bool vx_contest_ok = false;      // a vni_apply ran since the last run
    uint64_t vx_gd = 0, vx_ga = 0;
    bool vx_imported = false;
    uint32_t vres_n = 0, vres_D = 0;   // its entries; the dictionary size its ids were made for
    // pods
    DevBuf pods, pod_ovf, pod_direct;
    uint32_t slice = 0, pod_total = 0, ovf_mask = 0, kb_words = 0, pod_stamp = 0;
    // late pods (kdtn_epoch_late_pods): rows [pod_total, pod_total + n_late) of `pods`, after
    // the gathered table; cleared by the next upload, delta, ingest or commit (prepare_work)
    uint32_t n_late = 0;
    // pods_ready: pods / pod_direct / pod_ovf hold the complete tables of the current rows (a
    // full build ran and every later row change was patched). pods_delta: this upload's rows were
    // patched in kdtn_epoch_upload_delta, so its runs do no pod-table work.
    bool pods_ready = false, pods_delta = false;
    DevBuf pd_send, pd_recv, pd_cnt;
    bool traced = false;
    // work
    DevBuf otarget, sync, misc, hscratch, fscratch, trace, stage;
    uint32_t nwg = 0;
    // outputs
    DevBuf action, del_off, add_off, upd_off, del_idx, add_idx, upd_idx;
    DevBuf del_res, add_res, upd_res, add_qdisc, upd_qdisc, add_qerr;
    // wire encoding
    DevBuf kd_si, kd_len1, pd_si, pd_len1, w_rel, w_topo, w_size, w_err, w_off, w_part, w_arena, w_pinfo;
    uint64_t w_bytes = 0;
    bool encoded = false;
    // RemotePod fan-out
    DevBuf f_mark, f_send, f_node_idx, f_nodes, f_counts, f_base, f_part, f_idx, f_inv, f_reach_upd, f_cut, f_st, f_node;
    bool fan_valid = false;                    // the fan-out of the last run is in f_* (fanout_compute)
    bool lc_valid = false;                     // lc: coarse entry -> topology indexes of the last run's lists
    bool si_run = false;                       // the string tables were built since the last run
    DevBuf lc[3];
    uint32_t fan_nn = 0, fan_nsend = 0;
    // RemotePod messages (kdtn_epoch_remote_encode)
    DevBuf rp_flag, rp_pos, rp_phys, rp_msz, rp_moff, rp_tsz, rp_toff, rp_arena, rp_tc;
    uint32_t rp_n = 0, rp_nr = 0;
    uint64_t rp_bytes = 0, rp_tc_bytes = 0;
    bool rp_done = false;
    // resident state: commit / delta plans, the delta's arrays and inline records
    DevBuf st_cnt, st_len, st_base, st_mode, st_flags, st_off64, st_part, st_off32, st_mask, st_chg;
    DevBuf dl_rows;
    // delta with a topology-set change: the map, created rows' names, the realised plan
    DevBuf dl_prev, dl_dest, dl_pack, st_rlen, st_rbase, st_roff64, st_rpart, st_roff32, st_seen;
    // incremental CR ingest (kdtn_json_ingest_delta): the document's scratch tables and local
    // dictionaries, the id maps into the resident dictionaries, the topology-key match
    DevBuf ji_ns, ji_name, ji_src, ji_netns, ji_flags, ji_roff, ji_noff, ji_kb, ji_ko, ji_pb, ji_po;
    DevLinkStore ji_des, ji_real;
    DevBuf ji_kmap, ji_pmap, ji_miss, ji_mlen, ji_rank, ji_boff, ji_nil, ji_keep, ji_kpos, ji_claim, ji_res,
        ji_created, ji_cpos, ji_keys, ji_vals, ji_dkeys, ji_del, ji_ref;
    // resident string indexes (string → id) of the dictionaries' first n strings
    struct StrIndex {
        DevBuf slots;
        uint32_t n = 0, mask = 0;
    } ix_k, ix_p;
    uint64_t kd_arena = 0, pd_arena = 0;       // dictionary arena bytes (host-known: tables_info)
    DevLinkStore dl_rec;
    bool tables_cur = false;                   // j_info describes the current tables (kdtn_epoch_tables_info)
    // tc argv
    DevBuf tc_size, tc_off, tc_arena;
    uint64_t tc_bytes = 0;
    uint32_t tc_n = 0;
    bool tc_done = false;
    // status write-back bodies (kdtn_epoch_status_encode): per-dictionary escape tables with
    // their watermarks (leading strings whose words are built, like si_k / si_p), selection,
    // sizes, scans, body offsets, totals block, arena
    DevBuf kd_esc, pd_esc, sj_mask, sj_sel, sj_tsz, sj_tpos, sj_rsz, sj_rtopo, sj_rpos, sj_off, sj_tot, sj_arena;
    uint32_t se_k = 0, se_p = 0;
    bool se_run = false;                       // the escape tables were built since the last run
    uint64_t sj_bytes = 0;
    uint32_t sj_T = 0;
    bool sj_done = false;
    // CR ingest (kdtn_ingest.hip): document, block masks, token stream, decode scratch
    DevBuf j_doc, j_q, j_bs, j_hb, j_esc, j_qcnt, j_qoff, j_tok, j_open, j_close, j_gcnt, j_goff;
    DevBuf j_olist, j_vlist, j_slist;
    uint32_t j_kcap = 0, j_pcap = 0;   // intern table sizes that fit the last document
    DevBuf j_toks, j_par, j_role, j_ecls, j_odep, j_ord, j_tagg, j_gagg, j_cnt3, j_coff3, j_small, j_part;
    DevBuf j_tflags, j_owner, j_vown, j_kslots, j_krep, j_pslots, j_prep, j_heap;
    DevBuf j_kkeys, j_pkeys;     // dense key words of the intern tables
    DevBuf j_rows;               // row-major staging of the decoded link records (JS_ROW words each)
    DevBuf j_bits, j_bcnt, j_wrank, j_kslot_id, j_pslot_id, j_len, j_off64, j_sofid;
    uint64_t j_n = 0;
    uint32_t j_nb = 0;
    bool j_loaded = false, j_done = false;
    // LinksBatchQuery decode (kdtn_wire_ingest): message table, frame lists, per-message state
    DevBuf u_off, u_kind, u_nl, u_np, u_loff, u_poff, u_lfr, u_lmsg, u_pfr, u_merr, u_ctl;
    DevBuf u_cdes, u_creal, u_des64, u_real64, u_rbase, u_err8;
    kdtn_wire_plan u_plan{};
    bool u_done = false;
    // RemotePod planning (kdtn_remote_ingest): body table, VNI snapshot and table, outputs, report
    DevBuf ri_start, ri_size, ri_vni, ri_nsb, ri_nso, ri_slots, ri_plan, ri_qd, ri_ctl;
    kdtn_remote_ingest_plan_t ri_report{};
    bool ri_done = false;
    // UpdateLinks planning (kdtn_update_ingest; its frame pass works in the u_* lists above): cut
    // words, counts and their scan, staged and placed records, report
    DevBuf ul_cut, ul_cnt, ul_base64, ul_link0, ul_qd0, ul_msg, ul_link, ul_qd, ul_ctl;
    kdtn_update_ingest_plan_t ul_report{};
    uint32_t ul_T = 0;
    bool ul_done = false;
    kdtn_ingest_info j_info{};
    bool uploaded = false;
    bool ran = false;
    bool synced = false;   // h_misc[1..4] hold the last run's list totals (kdtn_epoch_sync or counts_fresh)
    uint32_t last_stages = 0;
    kdtn_plan plan{};      // what the last kdtn_epoch_run chose (kdtn_epoch_plan)
    // multi-GPU
    int nranks = 1, rank = 0;
    bool pods_imported = false;   // host transport: this epoch's global pod table is in place
    bool pods_rank_major = true;  // pod table rank-major (uploads) vs document order (sharded ingest)
    // kdtn_json_ingest_shard leaves the context as rank `shard` of `nshards` for its epoch; the
    // next upload or ingest restores the rank setup the caller had before (sh_saved_*)
    bool sh_active = false;
    int sh_saved_nranks = 1, sh_saved_rank = 0;
    // timers: 0 none, 1 k_reconcile (+ placement) only, 2 every stage (kdtn_set_timing)
    int timing = 2;
    const char* ev_name[kMaxTimers] = {};
    int n_ev = 0;
    // per-stage HIP-event times summed over the epochs synced since the last reset
    // (kdtn_timer_totals): a timed loop reads them once instead of once per epoch
    const char* acc_name[kMaxTimers] = {};
    double acc_ms[kMaxTimers] = {};
    uint32_t acc_n[kMaxTimers] = {};
    int n_acc = 0;
};

namespace kdtn {
namespace host {

template <typename T>
T* dp(DevBuf& b) { return static_cast<T*>(b.p); }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline uint32_t nblocks(uint64_t n, int block = BLOCK) { return (uint32_t)((n + block - 1) / block); }
uint32_t next_pow2(uint64_t x);

// device buffers (kdtn_engine.hip)
int ensure(DevBuf& b, size_t bytes);
int ensure_keep(DevBuf& b, size_t bytes, size_t keep, hipStream_t s);
int upload(kdtn_ctx* c, DevBuf& b, const void* src, size_t bytes);
int link_store_alloc(kdtn_ctx* c, DevLinkStore& st, uint32_t n);

template <typename T>
int d2h(kdtn_ctx* c, T* host, const void* dev, size_t count = 1) {
    HIP_TRY(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
    return KDTN_OK;
}


// Scope guard of a call that enqueued copies from caller memory: an early (error) return waits
// for the streams; the normal path disarms it once it has synchronised itself.
struct StreamsDrain {
    hipStream_t a, b;
    bool armed = true;
    ~StreamsDrain() {
        if (!armed) return;
        (void)hipStreamSynchronize(a);
        if (b != a) (void)hipStreamSynchronize(b);
    }
};

// input checks, uploads and the per-epoch buffers
int check_strtab(const kdtn_strtab& t, const char* what, uint32_t from = 0);
int check_vnis(kdtn_ctx* c, const kdtn_vni_table& vn, uint32_t D, uint32_t keep);
int upload_dicts(kdtn_ctx* c, const kdtn_strtab& kd, const kdtn_strtab& pd, uint32_t kk, uint32_t pk,
                 hipStream_t hs = nullptr);
int prepare_dicts(kdtn_ctx* c);
int prepare_vnis(kdtn_ctx* c, const kdtn_vni_table& vn);
int prepare_work(kdtn_ctx* c, uint32_t slice, uint32_t M, uint32_t N);
int prepare_epoch(kdtn_ctx* c, const kdtn_vni_table& vn, uint32_t slice, uint32_t M, uint32_t N);
int stage_columns(kdtn_ctx* c, uint8_t* st, const kdtn_link_table& L, size_t col, hipStream_t hs,
                  uint32_t (*segs)[2] = nullptr, int* nseg = nullptr);
void end_shard_ingest(kdtn_ctx* c);

// stages: timers, the last run's counts and lists, the encoders' tables, scans
void stage_begin(kdtn_ctx* c);
void timer_mark(kdtn_ctx* c, const char* name, int level = 0);
DevTopos topo_view(kdtn_ctx* c);
int counts_fresh(kdtn_ctx* c);
int list_coarse(kdtn_ctx* c);
int run_reach(kdtn_ctx* c, uint32_t* mark, uint32_t stamp);
bool fanout_stages_ok(const kdtn_ctx* c);
int str_tables(kdtn_ctx* c);
StrTab str_tab_kd(kdtn_ctx* c);
StrTab str_tab_pd(kdtn_ctx* c);
int esc_tables(kdtn_ctx* c);
int scan_u32(kdtn_ctx* c, const uint32_t* in, uint32_t n, uint64_t* out);
int scan_arena(kdtn_ctx* c, const uint32_t* sizes, uint32_t n, uint64_t* offs, const char* scanned, DevBuf& arena,
               size_t slack, uint64_t* total);

// CR ingest (kdtn_engine_ingest.hip)
// where a decode writes its tables (the context's own, or an incremental ingest's scratch)
struct JsTargets {
    DevBuf *ns, *name, *src, *netns, *flags, *roff, *noff;
    DevLinkStore *des, *real;
    DevBuf *kd_bytes, *kd_offs, *pd_bytes, *pd_offs;
};
struct JsCounts {
    uint32_t T, N, M, D, P;
    uint64_t kbytes, pbytes;
};

int json_decode(kdtn_ctx* c, const JsTargets& tg, JsCounts* o, kdtn_ingest_info* info);

}  // namespace host
}  // namespace kdtn
