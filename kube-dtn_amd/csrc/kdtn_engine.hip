// kdtn_engine.hip — host side of libkdtn.so: the C-ABI of include/kdtn.h over the
// HIP kernels of kdtn_kernels.hip. One kdtn_ctx per process/GPU; device buffers are
// owned by the context and reused across epochs (high-water-mark growth).
#include "kdtn_engine.h"

namespace kdtn {
namespace host {

constexpr int kSyncSpinUs = 2000;     // kdtn_epoch_sync: event polling before the blocking wait

thread_local char g_last_error[512] = "";

uint32_t next_pow2(uint64_t x) {
    uint64_t p = 64;
    while (p < x) p <<= 1;
    return (uint32_t)p;
}

// Replaced device buffers are retired, not freed at once: hipFree synchronises the whole
// device (measured: 1.3-1.5 ms inside a delta upload whose copies and kernels were in flight
// on two streams, every overlap lost), so they are freed together once more than
// kRetireBytes are waiting (one synchronisation for many regrowths) or when a context is
// destroyed. Retired buffers belong to no context: nothing enqueues work on them any more, and
// hipFree completes the work already in flight first. The bound is 32 GB of the 288 GB: a
// resident config-3 chain retires ≈ 8.5 GB while its rotating buffers reach their sizes, and
// at 8 GB that flush (≈ 10 frees, 5.6 ms) landed inside an epoch of the steady state
// (profiles/r04p_resident_alloc_log.txt).
constexpr size_t kRetireBytes = (size_t)32 << 30;
struct Retired {
    std::mutex m;
    std::vector<void*> p;
    size_t bytes = 0;
};
static Retired& retired() {
    static Retired r;
    return r;
}
// (profiling build, KDTN_ALLOC_LOG set) allocations of 16 MB and more and the flushes, on stderr
static void alloc_log(const char* what, size_t bytes) {
#if KDTN_PROFILING
    static const bool on = std::getenv("KDTN_ALLOC_LOG") != nullptr;
    if (on && bytes >= (16u << 20)) std::fprintf(stderr, "[kdtn alloc] %s %zu MB\n", what, bytes >> 20);
#else
    (void)what;
    (void)bytes;
#endif
}
// SDMA downloads in flight (any context): a retired buffer may be one they read
struct SdmaInflight {
    std::mutex m;
    std::vector<uint64_t> sig;
};
static SdmaInflight& sdma_inflight() {
    static SdmaInflight f;
    return f;
}
static void sdma_wait(hsa_signal_t sg) {
    while (hsa_signal_wait_scacquire(sg, HSA_SIGNAL_CONDITION_EQ, 0, UINT64_MAX, HSA_WAIT_STATE_ACTIVE) != 0) {
    }
}
static void retired_flush() {
    {
        SdmaInflight& f = sdma_inflight();
        std::lock_guard<std::mutex> lk(f.m);
        for (uint64_t h : f.sig) sdma_wait(hsa_signal_t{h});
    }
    Retired& r = retired();
    std::lock_guard<std::mutex> lk(r.m);
    alloc_log("flush", r.bytes);
    for (void* p : r.p) (void)hipFree(p);
    r.p.clear();
    r.bytes = 0;
}
void retire(void* p, size_t bytes) {
    if (!p) return;
    Retired& r = retired();
    bool flush;
    {
        std::lock_guard<std::mutex> lk(r.m);
        r.p.push_back(p);
        r.bytes += bytes;
        flush = r.bytes > kRetireBytes;
    }
    if (flush) retired_flush();
}

// hipMalloc that first gives back the retired buffers when the device is out of memory (up to
// kRetireBytes may only be waiting to be freed; hipFree waits for the work that uses them)
static hipError_t dev_malloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
        (void)hipGetLastError();
        retired_flush();
        e = hipMalloc(p, bytes);
    }
    return e;
}

int ensure(DevBuf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    if (b.cap >= bytes) return KDTN_OK;
    // grown buffers get 1/8 headroom (from 1 MB on): epoch sizes drift from epoch to epoch
    // (a churn chain's record counts); the old buffer is retired (no device synchronisation)
    if (bytes >= (1u << 20)) bytes = (bytes + bytes / 8 + 0xFFFFF) & ~(size_t)0xFFFFF;
    b = DevBuf{};
    alloc_log("ensure", bytes);
    hipError_t e = dev_malloc(&b.p, bytes);
    if (e != hipSuccess) {
        std::snprintf(g_last_error, sizeof(g_last_error), "hipMalloc(%zu): %s", bytes,
                      hipGetErrorString(e));
        b.p = nullptr;
        return KDTN_ENOMEM;
    }
    b.cap = bytes;
    return KDTN_OK;
}
// Grow b to at least `bytes`, keeping its first `keep` bytes (stream-ordered copy).
int ensure_keep(DevBuf& b, size_t bytes, size_t keep, hipStream_t s) {
    bytes = std::max<size_t>(bytes, 256);
    if (b.cap >= bytes) return KDTN_OK;
    if (!keep || !b.p) return ensure(b, bytes);
    const size_t cap = std::max(bytes, b.cap + b.cap / 2);
    alloc_log("ensure_keep", cap);
    void* np = nullptr;
    hipError_t e = dev_malloc(&np, cap);
    if (e != hipSuccess) {
        std::snprintf(g_last_error, sizeof(g_last_error), "hipMalloc(%zu): %s", cap, hipGetErrorString(e));
        return KDTN_ENOMEM;
    }
    HIP_TRY(hipMemcpyAsync(np, b.p, std::min(keep, b.cap), hipMemcpyDeviceToDevice, s));
    retire(b.p, b.cap);                  // (stream-ordered after the copy: no synchronisation)
    b.p = np;
    b.cap = cap;
    return KDTN_OK;
}

int upload(kdtn_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    TRY(ensure(b, bytes));
    if (bytes) HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return KDTN_OK;
}

// arenas get 64 B of slack: dictionary slices are staged with 16-B loads
static int upload_arena(kdtn_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    TRY(ensure(b, bytes + 64));
    if (bytes) HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return KDTN_OK;
}

// Dictionary arena + offsets, uploading only what follows the first `keep` strings (offs[keep],
// the kept prefix's end, stays the device's own: the keep checks compare it with the host's).
// The copies go on `hs` (the context stream unless a delta overlaps them with its kernels).
static int upload_dict(kdtn_ctx* c, DevBuf& bytes, DevBuf& offs, const kdtn_strtab& t, uint32_t keep, hipStream_t hs) {
    const size_t b0 = t.offs[keep], b1 = t.offs[t.n];
    TRY(ensure_keep(bytes, b1 + 64, keep ? b0 : 0, c->stream));
    TRY(ensure_keep(offs, ((size_t)t.n + 1) * 4, keep ? ((size_t)keep + 1) * 4 : 0, c->stream));
    if (b1 > b0) HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(bytes.p) + b0, t.bytes + b0, b1 - b0,
                                        hipMemcpyHostToDevice, hs));
    const uint32_t o0 = keep ? keep + 1 : 0;
    if (t.n + 1 > o0)
        HIP_TRY(hipMemcpyAsync(static_cast<uint32_t*>(offs.p) + o0, t.offs + o0, ((size_t)t.n + 1 - o0) * 4,
                               hipMemcpyHostToDevice, hs));
    return KDTN_OK;
}

// k_reconcile sync block: 16 B (ticket, error word) + 3 look-back granules per workgroup,
// padded to 16 B (memset size % 16 == 0, cdna_hip_programming.md G16)
// ticket + error word, look-back granules [nwg*3] u64, then VAR_DIFF counts and bases [nwg*3] u32 each
// (16-B aligned: k_place_scan reads and writes them as uint4)
static size_t sync_counts_at(uint32_t nwg) { return align_up(SYNC_HEADER_BYTES + (size_t)nwg * 24, 16); }
static size_t sync_bytes(uint32_t nwg) { return sync_counts_at(nwg) + 2 * align_up((size_t)nwg * 12, 16); }

// from: the kept prefix of an append-only upload (its offsets were checked when uploaded and
// check_keep compares offs[keep] with the device copy), so only [from, n] is walked
int check_strtab(const kdtn_strtab& t, const char* what, uint32_t from) {
    if (t.n == 0 || !t.offs || (!t.bytes && t.offs[t.n] != 0)) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: empty dictionary (id 0 must be \"\")", what);
        return KDTN_EINVAL;
    }
    if (t.n >= 0x7FFFFFFFu) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: too many strings", what);
        return KDTN_EINVAL;
    }
    if (t.offs[0] != 0 || t.offs[1] != 0) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: id 0 must be the empty string", what);
        return KDTN_EINVAL;
    }
    for (uint32_t i = from < t.n ? from : t.n; i < t.n; ++i)
        if (t.offs[i + 1] < t.offs[i]) {
            std::snprintf(g_last_error, sizeof(g_last_error), "%s: offsets not monotone at %u", what, i);
            return KDTN_EINVAL;
        }
    return KDTN_OK;
}

static int check_ids(const uint32_t* col, uint32_t n, uint32_t lim, const char* what) {
    if (n && !col) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: missing column", what);
        return KDTN_EINVAL;
    }
    uint32_t mx = 0;
    for (uint32_t i = 0; i < n; ++i) mx = std::max(mx, col[i]);
    if (n && mx >= lim) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: id %u out of range (%u strings)", what, mx, lim);
        return KDTN_EINVAL;
    }
    return KDTN_OK;
}

static int check_offsets(const uint32_t* off, uint32_t T, uint32_t n, const char* what) {
    if (!off) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: missing offsets", what);
        return KDTN_EINVAL;
    }
    if (off[0] != 0 || off[T] != n) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: offsets must span [0,%u]", what, n);
        return KDTN_EINVAL;
    }
    for (uint32_t t = 0; t < T; ++t)
        if (off[t + 1] < off[t]) {
            std::snprintf(g_last_error, sizeof(g_last_error), "%s: offsets not monotone at %u", what, t);
            return KDTN_EINVAL;
        }
    return KDTN_OK;
}

constexpr uint32_t STAGED_UPLOAD_MIN = 1u << 16;   // records: below it, 2-D copies straight into tiles

// A link table's columns as host runs: consecutive columns whose host arrays are adjacent (a
// caller holding key[7][n] / prop[12][n] blocks) become one copy into the staging buffer.
// segs (optional): the column ranges of the copies, in copy order, each followed by an event
// on hs (c->ev_col[k]); returns their count in *nseg
int stage_columns(kdtn_ctx* c, uint8_t* st, const kdtn_link_table& L, size_t col, hipStream_t hs,
                  uint32_t (*segs)[2], int* nseg) {
    const uint32_t* src[LINK_COLS32];
    for (int k = 0; k < KDTN_NKEY; ++k) src[COL_KEY0 + k] = L.key[k];
    for (int k = 0; k < KDTN_NPROP; ++k) src[COL_PROP0 + k] = L.prop[k];
    src[COL_GAP] = L.gap;
    int ns = 0;
    for (int a = 0; a < LINK_COLS32;) {
        int b = a + 1;
        while (b < LINK_COLS32 && reinterpret_cast<const uint8_t*>(src[b]) ==
                                      reinterpret_cast<const uint8_t*>(src[b - 1]) + col)
            ++b;
        HIP_TRY(hipMemcpyAsync(st + (size_t)a * col, src[a], (size_t)(b - a) * col, hipMemcpyHostToDevice, hs));
        if (segs) {
            segs[ns][0] = (uint32_t)a;
            segs[ns][1] = (uint32_t)b;
            HIP_TRY(hipEventRecord(c->ev_col[ns], hs));
        }
        ++ns;
        a = b;
    }
    if (nseg) *nseg = ns;
    return KDTN_OK;
}

// defer: the id-range check's column maxima stay in misc[MISC_COLMAX..] for the caller to read
// back with its own synchronisation (the staged path is then taken for any size)
static int upload_links(kdtn_ctx* c, DevLinkStore& s, const kdtn_link_table& L, uint32_t D, uint32_t P,
                 const char* what, bool defer = false) {
    const uint32_t n = L.n;
    for (int k = 0; k < KDTN_NKEY; ++k)
        if (n && !L.key[k]) return check_ids(L.key[k], n, D, what);          // missing column
    for (int k = 0; k < KDTN_NPROP; ++k)
        if (n && !L.prop[k]) return check_ids(L.prop[k], n, P, what);
    if (n && (!L.uid || !L.gap)) {
        std::snprintf(g_last_error, sizeof(g_last_error), "%s: missing uid/gap", what);
        return KDTN_EINVAL;
    }
    const size_t tiles = ((size_t)std::max<uint32_t>(n, 1) + TILE_RECS - 1) / TILE_RECS;
    const size_t tile_bytes = (size_t)TILE_WORDS * 4;
    TRY(ensure(s.buf, tiles * tile_bytes));
    uint8_t* base = static_cast<uint8_t*>(s.buf.p);
    s.view.base = reinterpret_cast<const uint32_t*>(base);
    s.view.n = n;
    s.n = n;
    if (n >= STAGED_UPLOAD_MIN || defer) {
        // large tables: one linear copy per column (full host-link rate) into a staging buffer,
        // then the tiles and the id-range check in one GPU pass (no host pass over the columns)
        const size_t col = (size_t)n * 4, uid_at = align_up(col * LINK_COLS32, 8);
        TRY(ensure(c->stage, uid_at + (size_t)n * 8 + 128));
        uint8_t* st = static_cast<uint8_t*>(c->stage.p);
        TRY(ensure(c->misc, 256));
        uint32_t* colmax = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(c->misc.p) + MISC_COLMAX * 4);
        HIP_TRY(hipMemsetAsync(colmax, 0, COL_GAP * 4, c->stream));
        if (!n) return KDTN_OK;
        TRY(stage_columns(c, st, L, col, c->stream));
        HIP_TRY(hipMemcpyAsync(st + uid_at, L.uid, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        k_soa_to_tiles<<<std::min<uint32_t>((n + BLOCK - 1) / BLOCK, 4 * c->n_cus), BLOCK, 0, c->stream>>>(
            reinterpret_cast<const uint32_t*>(st), reinterpret_cast<const int64_t*>(st + uid_at), n,
            reinterpret_cast<uint32_t*>(base), colmax);
        HIP_TRY(hipGetLastError());
        if (defer) return KDTN_OK;
        uint32_t mx[COL_GAP];
        HIP_TRY(hipMemcpyAsync(mx, colmax, sizeof(mx), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int k = 0; k < COL_GAP; ++k) {
            const uint32_t lim = k < KDTN_NKEY ? D : P;
            if (mx[k] >= lim) {
                std::snprintf(g_last_error, sizeof(g_last_error), "%s: id %u out of range (%u strings)", what, mx[k], lim);
                return KDTN_EINVAL;
            }
        }
        return KDTN_OK;
    }
    for (int k = 0; k < KDTN_NKEY; ++k) TRY(check_ids(L.key[k], n, D, what));
    for (int k = 0; k < KDTN_NPROP; ++k) TRY(check_ids(L.prop[k], n, P, what));
    // tiles of 64 records (kdtn_kernels.h DevLinks): each column is a 2-D copy with a
    // 256-B (uid: 512-B) run per tile
    auto put = [&](int col, const void* src, size_t esz) -> int {
        const size_t full = n / TILE_RECS, tail = n % TILE_RECS;
        const size_t run = TILE_RECS * esz;
        uint8_t* dst = base + (size_t)col * TILE_RECS * 4;
        if (full)
            HIP_TRY(hipMemcpy2DAsync(dst, tile_bytes, src, run, run, full, hipMemcpyHostToDevice, c->stream));
        if (tail)
            HIP_TRY(hipMemcpyAsync(dst + full * tile_bytes, static_cast<const uint8_t*>(src) + full * run,
                                   tail * esz, hipMemcpyHostToDevice, c->stream));
        return KDTN_OK;
    };
    if (n) {
        for (int k = 0; k < KDTN_NKEY; ++k) TRY(put(COL_KEY0 + k, L.key[k], 4));
        for (int k = 0; k < KDTN_NPROP; ++k) TRY(put(COL_PROP0 + k, L.prop[k], 4));
        TRY(put(COL_GAP, L.gap, 4));
        TRY(put(COL_UID, L.uid, 8));
    }
    return KDTN_OK;
}

// Each timing event costs ≈5 µs of stream time on MI355X (measured: two consecutive marks
// with nothing between them read 5.4 µs), so epoch stages are marked at a level.
void timer_mark(kdtn_ctx* c, const char* name, int level) {
    if (c->n_ev >= kMaxTimers || c->timing < level) return;
    c->ev_name[c->n_ev] = name;
    (void)hipEventRecord(c->ev[c->n_ev + 1], c->stream);
    c->n_ev++;
}

DevTopos topo_view(kdtn_ctx* c) {
    DevTopos t;
    t.ns = dp<uint32_t>(c->t_ns);
    t.name = dp<uint32_t>(c->t_name);
    t.src_ip = dp<uint32_t>(c->t_src);
    t.net_ns = dp<uint32_t>(c->t_netns);
    t.flags = dp<uint8_t>(c->t_flags);
    t.real_off = dp<uint32_t>(c->t_roff);
    t.des_off = dp<uint32_t>(c->t_noff);
    t.n = c->T;
    return t;
}

// Parse the property strings [p0, n): one thread per (string, interpretation), three
// launches' worth of waves in one grid (125k-pod config 2: 0.0374 -> 0.0341 ms against one
// thread per string; 1M: equal).
static void launch_pdict(kdtn_ctx* c, uint32_t p0, uint32_t n) {
#if KDTN_PROFILING
    if (const char* ev = std::getenv("KDTN_PD_ONLY")) {           // one interpretation alone (A/B)
        const int w = std::atoi(ev);
        auto one = [&](auto kern) {
            kern<<<nblocks(n - p0), BLOCK, 0, c->stream>>>(dp<uint8_t>(c->pd_bytes), dp<uint32_t>(c->pd_offs), p0, n,
                                                          c->cfg.tick_in_usec, dp<uint32_t>(c->pd_pct),
                                                          dp<uint2>(c->pd_dur), dp<uint2>(c->pd_rate),
                                                          dp<uint32_t>(c->pd_rerr));
        };
        if (w == PD_DUR) { one(k_pdict_only<PD_DUR>); return; }
        if (w == PD_PCT) { one(k_pdict_only<PD_PCT>); return; }
        if (w == PD_RATE) { one(k_pdict_only<PD_RATE>); return; }
    }
#endif
    k_pdict_parse<<<dim3(nblocks(n - p0), 3), BLOCK, 0, c->stream>>>(
        dp<uint8_t>(c->pd_bytes), dp<uint32_t>(c->pd_offs), p0, n, c->cfg.tick_in_usec, dp<uint32_t>(c->pd_pct),
        dp<uint2>(c->pd_dur), dp<uint2>(c->pd_rate), dp<uint32_t>(c->pd_rerr));
}

// Special key-string ids (SPECIAL_DEFAULT / SPECIAL_LOCALHOST) at or past the parse start
// are forgotten when an upload sets it; every run's k_kdict_flags re-finds them there.
static void clip_specials(kdtn_ctx* c) {
    if (c->kd_special.p) k_special_clip<<<1, 64, 0, c->stream>>>(dp<uint32_t>(c->kd_special), c->kd_from & ~63u);
}

// per-string parse tables of both dictionaries (c->D, c->P set), keeping the parsed
// tables of the first c->kd_valid / c->pd_valid strings. kbits holds KB_NSETS bitsets at a
// stride of kb_cap words; growing the stride moves each set.
int prepare_dicts(kdtn_ctx* c) {
    const uint32_t D = c->D, P = c->P;
    hipStream_t s = c->stream;
    const uint32_t need = (uint32_t)(((uint64_t)D + 63) / 64 * 2);
    if (need > c->kb_cap || !c->kd_bits.p) {
        // stride a multiple of 2 words (kdtn_kernels.h kb_words): growth by 1.5x rounded up
        const uint32_t cap = (std::max<uint32_t>(need, c->kd_valid ? c->kb_cap + c->kb_cap / 2 : 0) + 1u) & ~1u;
        DevBuf nb;
        TRY(ensure(nb, (size_t)KB_NSETS * cap * 4 + 4));
        const uint32_t keepw = (uint32_t)(((uint64_t)c->kd_valid + 63) / 64 * 2);
        if (keepw && c->kd_bits.p)
            HIP_TRY(hipMemcpy2DAsync(nb.p, (size_t)cap * 4, c->kd_bits.p, (size_t)c->kb_cap * 4, (size_t)keepw * 4,
                                     KB_NSETS, hipMemcpyDeviceToDevice, s));
        c->kd_bits = std::move(nb);          // the old table is retired: stream-ordered after the copy
        c->kb_cap = cap;
    }
    c->kb_words = c->kb_cap;
    const size_t pv = c->pd_valid;
    TRY(ensure_keep(c->pd_pct, (size_t)P * 4, pv * 4, s));
    TRY(ensure_keep(c->pd_dur, (size_t)P * 8, pv * 8, s));
    TRY(ensure_keep(c->pd_rate, (size_t)P * 8, pv * 8, s));
    TRY(ensure_keep(c->pd_rerr, (size_t)nblocks(P) * BLOCK / 8, (pv + 63) / 64 * 8, s));
    TRY(ensure(c->kd_special, 64));
    clip_specials(c);
    return KDTN_OK;
}

// VxlanManager snapshot ids valid for a dictionary of D strings. KDTN_VNI_RESIDENT needs a
// resident map whose ids still name the same strings: the upload keeps (kdict_keep) at least
// the vres_D strings the map was made for — every upload since kept that prefix, since an
// upload that kept less either replaced the map or was refused here. A dictionary the engine
// builds itself (JSON ingest) cannot keep a prefix (keep = 0).
int check_vnis(kdtn_ctx* c, const kdtn_vni_table& vn, uint32_t D, uint32_t keep) {
    if (vn.n == KDTN_VNI_RESIDENT) {
        if (!c->vres_ok || keep < c->vres_D || D < c->vres_D) {
            std::snprintf(g_last_error, sizeof(g_last_error),
                          "KDTN_VNI_RESIDENT: the resident VXLAN map's ids (%u strings) are not a kept prefix "
                          "of this dictionary (kdict_keep %u)", c->vres_D, keep);
            return KDTN_EINVAL;
        }
        return KDTN_OK;
    }
    TRY(check_ids(vn.node, vn.n, D, "vnis.node"));
    return check_ids(vn.net_ns, vn.n, D, "vnis.net_ns");
}

// Append-only dictionaries: the first *_keep strings equal the previous upload's (the arena
// offset of the kept prefix is checked against the device copy).
static int check_keep(kdtn_ctx* c, const kdtn_strtab& kd, const kdtn_strtab& pd, uint32_t kk, uint32_t pk) {
    const uint32_t D = kd.n, P = pd.n;
    uint32_t dev_off[2] = {0, 0};
    if (kk <= c->kd_valid && kk && kk <= D)
        HIP_TRY(hipMemcpyAsync(dev_off, dp<uint32_t>(c->kd_offs) + kk, 4, hipMemcpyDeviceToHost, c->stream));
    if (pk <= c->pd_valid && pk && pk <= P)
        HIP_TRY(hipMemcpyAsync(dev_off + 1, dp<uint32_t>(c->pd_offs) + pk, 4, hipMemcpyDeviceToHost, c->stream));
    if (kk || pk) HIP_TRY(hipStreamSynchronize(c->stream));
    if (kk > D || pk > P || kk > c->kd_valid || pk > c->pd_valid || (kk && kd.offs[kk] != dev_off[0]) ||
        (pk && pd.offs[pk] != dev_off[1])) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "kdict_keep %u / pdict_keep %u: not a prefix of the previous upload's parsed dictionaries "
                      "(%u / %u strings)", kk, pk, c->kd_valid, c->pd_valid);
        return KDTN_EINVAL;
    }
    return KDTN_OK;
}

// upload the dictionaries past the kept prefixes and size their parsed tables
int upload_dicts(kdtn_ctx* c, const kdtn_strtab& kd, const kdtn_strtab& pd, uint32_t kk, uint32_t pk,
                 hipStream_t hs) {
    if (!hs) hs = c->stream;
    c->D = kd.n;
    c->P = pd.n;
    // strings past the kept prefix may differ: an index that covers them is rebuilt (mask 0)
    if (kk < c->ix_k.n) c->ix_k.n = c->ix_k.mask = 0;
    if (pk < c->ix_p.n) c->ix_p.n = c->ix_p.mask = 0;
    c->kd_arena = kd.offs[kd.n];
    c->pd_arena = pd.offs[pd.n];
    c->kd_valid = kk;
    c->pd_valid = pk;
    c->kd_from = kk;
    c->pd_from = pk;
    c->si_k = std::min(c->si_k, kk);
    c->si_p = std::min(c->si_p, pk);
    c->se_k = std::min(c->se_k, kk);
    c->se_p = std::min(c->se_p, pk);
    TRY(upload_dict(c, c->kd_bytes, c->kd_offs, kd, kk, hs));
    TRY(upload_dict(c, c->pd_bytes, c->pd_offs, pd, pk, hs));
    return prepare_dicts(c);
}

// A sharded ingest's rank setup ends when the next upload or ingest starts.
void end_shard_ingest(kdtn_ctx* c) {
    if (!c->sh_active) return;
    c->nranks = c->sh_saved_nranks;
    c->rank = c->sh_saved_rank;
    c->pods_rank_major = true;
    c->pods_imported = false;
    c->pods_ready = false;                        // the pod table was in document order
    c->sh_T = 0;
    c->sh_active = false;
}

// everything an epoch needs besides its input tables: VNI snapshot, pod tables, work and
// output buffers (c->D, c->T set; shared by kdtn_epoch_upload and kdtn_json_ingest)
int prepare_vnis(kdtn_ctx* c, const kdtn_vni_table& vn) {
    const uint32_t D = c->D;
    const bool resident = vn.n == KDTN_VNI_RESIDENT;
    const uint32_t V = resident ? c->vres_n : vn.n;
    c->V = V;
    if (!resident) {
        TRY(upload(c, c->v_node, vn.node, (size_t)V * 4));
        TRY(upload(c, c->v_vni, vn.vni, (size_t)V * 4));
        TRY(upload(c, c->v_netns, vn.net_ns, (size_t)V * 4));
        c->vres_ok = true;                      // the uploaded map stays resident
        c->vres_in_r = false;
        c->vres_n = V;
        c->vres_D = D;
    } else if (c->vres_in_r) {                  // the applied map becomes this upload's snapshot
        std::swap(c->v_node, c->r_node);
        std::swap(c->v_vni, c->r_vni);
        std::swap(c->v_netns, c->r_netns);
        c->vres_in_r = false;
    }
    c->vni_mask = V ? next_pow2((uint64_t)V * 2) - 1 : 0;
    TRY(ensure(c->v_ents, (size_t)V * 16));
    TRY(ensure(c->v_slots, (size_t)(c->vni_mask + 1) * 4));
    TRY(ensure(c->v_table, (size_t)(c->vni_mask + 1) * 16));
    return KDTN_OK;
}

// pod tables, work and output buffers for T = c->T topologies, M realised and N desired records
int prepare_work(kdtn_ctx* c, uint32_t slice, uint32_t M, uint32_t N) {
    const uint32_t D = c->D;
    if (slice != c->slice) c->pods_ready = false;
    c->slice = slice;
    if ((uint64_t)slice * (uint64_t)c->nranks > POD_INDEX) {
        std::snprintf(g_last_error, sizeof(g_last_error), "pod table of %llu entries exceeds 2^30",
                      (unsigned long long)slice * (unsigned long long)c->nranks);
        return KDTN_EINVAL;
    }
    c->pod_total = slice * (uint32_t)c->nranks;
    if (c->n_late) c->pods_ready = false;
    c->n_late = 0;
    c->ovf_mask = next_pow2((uint64_t)c->pod_total * 2) - 1;
    TRY(ensure(c->pods, (size_t)c->pod_total * 16));
    if (c->pod_ovf.cap < (size_t)(c->ovf_mask + 1) * 8) {       // stamped slots start zeroed
        TRY(ensure(c->pod_ovf, (size_t)(c->ovf_mask + 1) * 8));
        HIP_TRY(hipMemsetAsync(c->pod_ovf.p, 0, c->pod_ovf.cap, c->stream));
    }
    if (c->pod_direct.cap < (size_t)D * 16) {                  // stamps start from a zeroed table
        // headroom for append-only dictionaries: slots of ids past the last build read as empty
        // (stamp 0), so a delta upload that adds strings keeps the built table
        TRY(ensure(c->pod_direct, (size_t)D * 16 + (size_t)D * 4 + 4096));
        HIP_TRY(hipMemsetAsync(c->pod_direct.p, 0, c->pod_direct.cap, c->stream));   // stamp 0 = empty
        c->pods_ready = false;
    }

    const uint32_t nwg = (c->T + TPW - 1) / TPW;
    c->nwg = nwg;
    TRY(ensure(c->otarget, (size_t)M * 4));
    TRY(ensure(c->sync, sync_bytes(nwg)));
    TRY(ensure(c->misc, 256));
    TRY(ensure(c->hscratch, ((size_t)M + N) * 4));
    TRY(ensure(c->fscratch, (size_t)M + N));
    TRY(ensure(c->action, c->T));
    TRY(ensure(c->del_off, (size_t)(c->T + 1) * 4));
    TRY(ensure(c->add_off, (size_t)(c->T + 1) * 4));
    TRY(ensure(c->upd_off, (size_t)(c->T + 1) * 4));
    // the comparison build (both lists non-empty) emits deferred chunks into upper halves
    const size_t h = (M && N) ? 2 : 1;
    TRY(ensure(c->del_idx, h * M * 4));
    TRY(ensure(c->upd_idx, h * M * 4));
    TRY(ensure(c->add_idx, h * N * 4));
    TRY(ensure(c->del_res, h * M * 16));
    TRY(ensure(c->upd_res, h * M * 16));
    TRY(ensure(c->add_res, h * N * 16));
    TRY(ensure(c->upd_qdisc, h * M * 72));
    TRY(ensure(c->add_qdisc, h * N * 72));
    TRY(ensure(c->add_qerr, h * N + 16));
    return KDTN_OK;
}

int prepare_epoch(kdtn_ctx* c, const kdtn_vni_table& vn, uint32_t slice, uint32_t M, uint32_t N) {
    TRY(prepare_vnis(c, vn));
    return prepare_work(c, slice, M, N);
}

// The last run's list totals in h_misc[1..3] (and the look-back error in [4]), from the coherent
// host words k_reconcile writes: read_totals once the run has completed (kdtn_epoch_sync);
// counts_fresh for an output stage called without kdtn_epoch_sync waits for the run first, so
// no stage sizes its passes from the counts of an earlier epoch.
static int read_totals(kdtn_ctx* c) {              // (the run has completed)
    for (int i = 0; i < 4; ++i) c->h_misc[1 + i] = __atomic_load_n(c->h_tot + i, __ATOMIC_ACQUIRE);
    if (c->h_misc[4] != 0) {
        std::snprintf(g_last_error, sizeof(g_last_error), "k_reconcile look-back timed out (0x%x)", c->h_misc[4]);
        return KDTN_EIO;
    }
    c->synced = true;
    return KDTN_OK;
}
int counts_fresh(kdtn_ctx* c) {
    if (c->synced) return KDTN_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return read_totals(c);
}

// Which batch entries the daemons reach (k_reach; include/kdtn.h): c->f_send (add) and
// c->f_reach_upd (update) flags of the last run; stamps destination daemons into `mark`.
// coarse entry -> topology indexes of the last run's del / add / upd lists (k_list_coarse),
// built by the first output stage after a run
int list_coarse(kdtn_ctx* c) {
    if (c->lc_valid) return KDTN_OK;
    const uint32_t cnt[3] = {c->h_misc[1], c->h_misc[3], c->h_misc[2]};   // del, add, upd
    DevBuf* offs[3] = {&c->del_off, &c->add_off, &c->upd_off};
    for (int l = 0; l < 3; ++l) {
        TRY(ensure(c->lc[l], ((size_t)cnt[l] / 64 + 2) * 4));
        if (c->T && cnt[l])
            k_list_coarse<<<nblocks(c->T), BLOCK, 0, c->stream>>>(dp<uint32_t>(*offs[l]), c->T, dp<uint32_t>(c->lc[l]));
    }
    HIP_TRY(hipGetLastError());
    c->lc_valid = true;
    return KDTN_OK;
}

int run_reach(kdtn_ctx* c, uint32_t* mark, uint32_t stamp) {
    const uint32_t nu = c->h_misc[2], na = c->h_misc[3];
    TRY(ensure(c->f_send, (size_t)na + 16));
    TRY(ensure(c->f_reach_upd, (size_t)nu + 16));
    ReachIn r{dp<uint32_t>(c->del_off), dp<uint4>(c->del_res), dp<uint32_t>(c->add_off), dp<uint4>(c->add_res),
              dp<uint2>(c->add_qdisc), dp<uint32_t>(c->upd_off), dp<uint4>(c->upd_res), c->T, stamp,
              dp<uint8_t>(c->add_qerr), nullptr, nullptr, nullptr};
    TRY(list_coarse(c));
    r.add_coarse = dp<uint32_t>(c->lc[1]);
    r.upd_coarse = dp<uint32_t>(c->lc[2]);
    if (mark) {                                     // the fan-out: dense node ids for its passes
        TRY(ensure(c->f_node, (size_t)na * 4 + 16));
        r.add_node = dp<uint32_t>(c->f_node);
    }
    const uint32_t nd = c->h_misc[1];
    TRY(ensure(c->f_cut, (size_t)c->T * 12 + 12));
    TRY(ensure(c->f_st, (size_t)na + 16));
    uint32_t* cut = dp<uint32_t>(c->f_cut);
    if (c->T) {
        HIP_TRY(hipMemsetAsync(cut, 0xFF, (size_t)c->T * 12, c->stream));
        if ((uint64_t)nd + na + nu)
            k_reach_cuts<<<nblocks((uint64_t)nd + na + nu), BLOCK, 0, c->stream>>>(r, nd, na, nu, cut,
                                                                                    dp<uint8_t>(c->f_st));
        if ((uint64_t)na + nu)
            k_reach<<<nblocks((uint64_t)na + nu), BLOCK, 0, c->stream>>>(r, na, nu, cut, dp<uint8_t>(c->f_st), mark,
                                                                         dp<uint8_t>(c->f_send),
                                                                         dp<uint8_t>(c->f_reach_upd));
    }
    return KDTN_OK;
}

// The encoders' inline string tables (StrTab) of both dictionaries, on the context stream,
// built by the first output stage after a run (the later stages of the epoch share them). Like
// the dictionary parses, the work is a function of the upload: the strings from the upload's
// keep index (and any never built) on; the entries before it are kept.
int str_tables(kdtn_ctx* c) {
    if (c->si_run && c->si_k == c->D && c->si_p == c->P) return KDTN_OK;
    hipStream_t s = c->stream;
    const uint32_t k0 = std::min(c->si_k, c->kd_from), p0 = std::min(c->si_p, c->pd_from);
    TRY(ensure_keep(c->kd_si, (size_t)c->D * SI_KW * 4 + 16, (size_t)k0 * SI_KW * 4, s));
    TRY(ensure_keep(c->kd_len1, (size_t)c->D + 16, k0, s));
    TRY(ensure_keep(c->pd_si, (size_t)c->P * SI_PW * 4 + 16, (size_t)p0 * SI_PW * 4, s));
    TRY(ensure_keep(c->pd_len1, (size_t)c->P + 16, p0, s));
    if (c->D > k0)
        k_str_inline<SI_KW><<<nblocks(c->D - k0), BLOCK, 0, s>>>(dp<uint8_t>(c->kd_bytes), dp<uint32_t>(c->kd_offs) + k0,
                                                                c->D - k0, dp<uint32_t>(c->kd_si) + (size_t)k0 * SI_KW,
                                                                dp<uint8_t>(c->kd_len1) + k0);
    if (c->P > p0)
        k_str_inline<SI_PW><<<nblocks(c->P - p0), BLOCK, 0, s>>>(dp<uint8_t>(c->pd_bytes), dp<uint32_t>(c->pd_offs) + p0,
                                                                c->P - p0, dp<uint32_t>(c->pd_si) + (size_t)p0 * SI_PW,
                                                                dp<uint8_t>(c->pd_len1) + p0);
    HIP_TRY(hipGetLastError());
    c->si_k = c->D;
    c->si_p = c->P;
    c->si_run = true;
    return KDTN_OK;
}

StrTab str_tab_kd(kdtn_ctx* c) {
    return StrTab{dp<uint32_t>(c->kd_si), dp<uint8_t>(c->kd_len1), dp<uint8_t>(c->kd_bytes)};
}
StrTab str_tab_pd(kdtn_ctx* c) {
    return StrTab{dp<uint32_t>(c->pd_si), dp<uint8_t>(c->pd_len1), dp<uint8_t>(c->pd_bytes)};
}

// The JSON escape tables of both dictionaries (k_status_esc), kept like the inline tables: the
// words of the strings before the upload's keep index stay, the rest are scanned.
int esc_tables(kdtn_ctx* c) {
    if (c->se_run && c->se_k == c->D && c->se_p == c->P) return KDTN_OK;
    hipStream_t s = c->stream;
    const uint32_t k0 = std::min(c->se_k, c->kd_from), p0 = std::min(c->se_p, c->pd_from);
    TRY(ensure_keep(c->kd_esc, (size_t)c->D * 4 + 16, (size_t)k0 * 4, s));
    TRY(ensure_keep(c->pd_esc, (size_t)c->P * 4 + 16, (size_t)p0 * 4, s));
    if (c->D > k0)
        k_status_esc<<<nblocks(c->D - k0), BLOCK, 0, s>>>(dp<uint8_t>(c->kd_bytes), dp<uint32_t>(c->kd_offs) + k0,
                                                         c->D - k0, dp<uint32_t>(c->kd_esc) + k0);
    if (c->P > p0)
        k_status_esc<<<nblocks(c->P - p0), BLOCK, 0, s>>>(dp<uint8_t>(c->pd_bytes), dp<uint32_t>(c->pd_offs) + p0,
                                                         c->P - p0, dp<uint32_t>(c->pd_esc) + p0);
    HIP_TRY(hipGetLastError());
    c->se_k = c->D;
    c->se_p = c->P;
    c->se_run = true;
    return KDTN_OK;
}

// exclusive scan of n u32 values into n+1 u64 offsets (out[n] = total): partial sums, a
// one-block scan of the partials, the final pass. (A single-pass decoupled look-back over
// 1024-value blocks measured slower on the output stages: 132 vs 52 us for 10M values, the
// look-back round trips of ~10k small blocks in the critical path.)
int scan_u32(kdtn_ctx* c, const uint32_t* in, uint32_t n, uint64_t* out) {
    const uint32_t nb = nblocks((uint64_t)n + 1, SCAN_CHUNK);
    TRY(ensure(c->j_part, (size_t)nb * 8));
    hipStream_t s = c->stream;
    k_scan_partial<<<nb, BLOCK, 0, s>>>(in, n, dp<uint64_t>(c->j_part));
    k_scan_top<<<1, SCAN_TOP_BLOCK, 0, s>>>(dp<uint64_t>(c->j_part), nb);
    k_scan_final<<<nb, BLOCK, 0, s>>>(in, n, dp<uint64_t>(c->j_part), out);
    HIP_TRY(hipGetLastError());
    return KDTN_OK;
}

// sizes → offsets → total → arena: scan_u32 of a size column (`scanned` names the timer mark
// after it), the total (offs[n]) brought to the host with one synchronisation, and `arena`
// grown to total + slack bytes
int scan_arena(kdtn_ctx* c, const uint32_t* sizes, uint32_t n, uint64_t* offs, const char* scanned, DevBuf& arena,
               size_t slack, uint64_t* total) {
    TRY(scan_u32(c, sizes, n, offs));
    timer_mark(c, scanned);
    HIP_TRY(hipMemcpyAsync(total, offs + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ensure(arena, (size_t)*total + slack);
}

// an output or ingest stage starts its timers: ev[0] is the stage's start
void stage_begin(kdtn_ctx* c) {
    c->n_ev = 0;
    (void)hipEventRecord(c->ev[0], c->stream);
}

}  // namespace host
}  // namespace kdtn

// ======================================================================================
// C-ABI
// ======================================================================================
extern "C" {

const char* kdtn_version(void) { return "kdtn-mi355x 0.1 (abi 1, gfx950)"; }

const char* kdtn_strerror(int code) {
    switch (code) {
    case KDTN_OK: return "ok";
    case KDTN_EINVAL: return g_last_error[0] ? g_last_error : "invalid argument";
    case KDTN_ENOMEM: return g_last_error[0] ? g_last_error : "out of memory";
    case KDTN_EIO: return g_last_error[0] ? g_last_error : "HIP/RCCL runtime error";
    case KDTN_ENOSPC: return "output capacity too small";
    case KDTN_ENODEV: return g_last_error[0] ? g_last_error : "no usable gfx950 device";
    default: return "unknown error";
    }
}

const char* kdtn_err_name(int e) {
    static const char* names[] = {"none", "veth_cidr", "veth_mac", "latency", "latency_corr",
                                  "jitter", "loss", "loss_corr", "duplicate", "duplicate_corr",
                                  "reorder_prob", "reorder_corr", "corrupt_prob", "corrupt_corr",
                                  "rate", "peer_lookup", "peer_no_links", "peer_veth_cidr",
                                  "peer_veth_mac", "remote_cidr"};
    if (e < 0 || e >= (int)(sizeof(names) / sizeof(names[0]))) return "unknown";
    return names[e];
}

double kdtn_psched_tick_in_usec(void) {
    // netlink initClock(): /proc/net/psched "t2us us2t clock_res hz" in hex
    FILE* f = std::fopen("/proc/net/psched", "r");
    if (!f) return 0.0;
    unsigned long long v[4];
    int got = std::fscanf(f, "%llx %llx %llx %llx", &v[0], &v[1], &v[2], &v[3]);
    std::fclose(f);
    if (got != 4 || v[1] == 0) return 0.0;
    if (v[2] == 1000000000ull) v[0] = v[1];
    const double clock_factor = (double)v[2] / 1000000.0;
    return (double)v[0] / (double)v[1] * clock_factor;
}

int kdtn_init(kdtn_ctx** out, const kdtn_config* cfg) {
    if (!out || !cfg) return KDTN_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        std::snprintf(g_last_error, sizeof(g_last_error), "no HIP device visible");
        return KDTN_ENODEV;
    }
    int dev = cfg->device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= ndev) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::snprintf(g_last_error, sizeof(g_last_error), "device %d is %s, libkdtn is built for gfx950",
                      dev, prop.gcnArchName);
        return KDTN_ENODEV;
    }
    kdtn_ctx* c = new kdtn_ctx();
    c->device = dev;
    c->cfg = *cfg;
    c->n_cus = (uint32_t)std::max(1, prop.multiProcessorCount);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return KDTN_EIO;
    }
    c->stream = c->own_stream;
    // words [0, 16): epoch sync header copy; [64, 128): the misc words a delta reads back
    if (hipHostMalloc(reinterpret_cast<void**>(&c->h_misc), 512, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_tot), 64, hipHostMallocCoherent) != hipSuccess) {
        delete c;
        return KDTN_ENOMEM;
    }
    std::memset(c->h_tot, 0, 64);
    // timing events only (read after a stream sync): no system-scope fence, whose L2 write-back
    // and invalidate at every mark cost the timed epoch stream time
    for (int i = 0; i <= kMaxTimers; ++i) (void)hipEventCreateWithFlags(&c->ev[i], hipEventDisableSystemFence);
    (void)hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming);
    for (hipEvent_t& e : c->ev_cp) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    for (hipEvent_t& e : c->ev_col) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) c->copy_stream = nullptr;
    if (hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking) != hipSuccess) c->d2h_stream = nullptr;
    (void)hipEventCreateWithFlags(&c->ev_dl_ready, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&c->ev_dl_done, hipEventDisableTiming);
    *out = c;
    return KDTN_OK;
}

void kdtn_destroy(kdtn_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)kdtn_epoch_download_wait(c);
    (void)hipStreamSynchronize(c->stream);
    for (hipStream_t st : {c->comm_stream, c->copy_stream, c->d2h_stream})
        if (st) (void)hipStreamSynchronize(st);
    // every stream is synchronised: the members (each DevBuf retires its memory) go first, then
    // the base's destructor frees the retired buffers and tears the handles down
    delete c;
}

}  // extern "C"

kdtn_ctx_handles::~kdtn_ctx_handles() {
    kdtn_ctx_handles* c = this;
    retired_flush();
    for (int i = 0; i <= kMaxTimers; ++i)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->ev_fill) (void)hipEventDestroy(c->ev_fill);
    if (c->ev_ag) (void)hipEventDestroy(c->ev_ag);
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
    for (hipEvent_t e : c->ev_cp)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_col)
        if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->d2h_stream) (void)hipStreamDestroy(c->d2h_stream);
    if (c->ev_dl_ready) (void)hipEventDestroy(c->ev_dl_ready);
    if (c->ev_dl_done) (void)hipEventDestroy(c->ev_dl_done);
    if (c->sdma_inited) {
        (void)hsa_signal_destroy(c->dl_sig);
        (void)hsa_shut_down();                      // (balances sdma_setup's hsa_init)
    }
    if (c->h_misc) (void)hipHostFree(c->h_misc);
    if (c->h_tot) (void)hipHostFree(c->h_tot);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
}

extern "C" {

int kdtn_set_stream(kdtn_ctx* c, void* s) {
    if (!c) return KDTN_EINVAL;
    c->stream = s ? static_cast<hipStream_t>(s) : c->own_stream;
    return KDTN_OK;
}

int kdtn_epoch_upload(kdtn_ctx* c, const kdtn_epoch_in* in) {
    if (!c || !in) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    g_last_error[0] = 0;
    end_shard_ingest(c);
    TRY(check_strtab(in->kdict, "kdict", in->kdict_keep));
    TRY(check_strtab(in->pdict, "pdict", in->pdict_keep));
    const kdtn_topo_table& T = in->topos;
    const uint32_t D = in->kdict.n, P = in->pdict.n;
    TRY(check_offsets(T.real_off, T.n, in->realised.n, "topos.real_off"));
    TRY(check_offsets(T.des_off, T.n, in->desired.n, "topos.des_off"));
    if (T.n && (!T.flags)) return KDTN_EINVAL;
    TRY(check_ids(T.ns, T.n, D, "topos.ns"));
    TRY(check_ids(T.name, T.n, D, "topos.name"));
    TRY(check_ids(T.src_ip, T.n, D, "topos.src_ip"));
    TRY(check_ids(T.net_ns, T.n, D, "topos.net_ns"));
    for (uint32_t t = 0; t < T.n; ++t) {
        if ((T.flags[t] & KDTN_TOPO_STATUS_NIL) && T.real_off[t + 1] != T.real_off[t]) {
            std::snprintf(g_last_error, sizeof(g_last_error), "topology %u: status.links nil but non-empty", t);
            return KDTN_EINVAL;
        }
        if ((T.flags[t] & KDTN_TOPO_SPEC_NIL) && T.des_off[t + 1] != T.des_off[t]) {
            std::snprintf(g_last_error, sizeof(g_last_error), "topology %u: spec.links nil but non-empty", t);
            return KDTN_EINVAL;
        }
    }
    TRY(check_vnis(c, in->vnis, D, in->kdict_keep));
    const uint32_t slice = in->pod_slice ? in->pod_slice : T.n;
    if (slice < T.n) return KDTN_EINVAL;

    TRY(check_keep(c, in->kdict, in->pdict, in->kdict_keep, in->pdict_keep));
    c->uploaded = false;                            // a failure from here on leaves no usable epoch
    c->T = T.n;
    TRY(upload_dicts(c, in->kdict, in->pdict, in->kdict_keep, in->pdict_keep));

    TRY(upload(c, c->t_ns, T.ns, (size_t)T.n * 4));
    TRY(upload(c, c->t_name, T.name, (size_t)T.n * 4));
    TRY(upload(c, c->t_src, T.src_ip, (size_t)T.n * 4));
    TRY(upload(c, c->t_netns, T.net_ns, (size_t)T.n * 4));
    TRY(upload(c, c->t_flags, T.flags, (size_t)T.n));
    TRY(upload(c, c->t_roff, T.real_off, (size_t)(T.n + 1) * 4));
    TRY(upload(c, c->t_noff, T.des_off, (size_t)(T.n + 1) * 4));

    TRY(upload_links(c, c->real, in->realised, D, P, "realised"));
    TRY(upload_links(c, c->des, in->desired, D, P, "desired"));

    c->pods_rank_major = true;
    TRY(prepare_epoch(c, in->vnis, slice, in->realised.n, in->desired.n));
    HIP_TRY(hipStreamSynchronize(c->stream));   // host arrays may be released after return
    c->uploaded = true;
    c->ran = false;
    c->pods_imported = false;
    c->j_done = false;                             // the tables are no ingest's any more
    c->tables_cur = false;
    c->pods_ready = false;                         // new rows: the next run builds the pod tables
    c->pods_delta = false;
    return KDTN_OK;
}

// The VxlanManager snapshot's lookup table on the context stream (k_vni_pack / _ht_build / _fill).
static int build_vni_table(kdtn_ctx* c) {
    hipStream_t s = c->stream;
    const size_t vcap = (size_t)c->vni_mask + 1;
    HIP_TRY(hipMemsetAsync(c->v_slots.p, 0xFF, vcap * 4, s));
    k_vni_pack<<<nblocks(c->V), BLOCK, 0, s>>>(dp<uint32_t>(c->v_node), dp<int32_t>(c->v_vni),
                                              dp<uint32_t>(c->v_netns), c->V, dp<uint4>(c->v_ents));
    k_vni_ht_build<<<nblocks(c->V), BLOCK, 0, s>>>(dp<uint4>(c->v_ents), c->V, dp<uint32_t>(c->v_slots),
                                                  c->vni_mask);
    k_vni_fill<<<nblocks(vcap), BLOCK, 0, s>>>(dp<uint4>(c->v_ents), dp<uint32_t>(c->v_slots), (uint32_t)vcap,
                                               dp<uint4>(c->v_table));
    return KDTN_OK;
}

int kdtn_epoch_run(kdtn_ctx* c, uint32_t stages) {
    if (!c || !c->uploaded) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    stages |= KDTN_STAGE_DIFF;
    c->last_stages = stages;
    c->n_ev = 0;
    hipStream_t s = c->stream;
    const DevTopos T = topo_view(c);
    const bool resolve = stages & KDTN_STAGE_RESOLVE;
    // pod tables already current (patched by kdtn_epoch_upload_delta): no fill, exchange or build
    const bool pods_cur = resolve && c->pods_delta && c->pods_ready;
    const bool host_xchg = resolve && !pods_cur && c->nranks > 1 && !c->comm;   // rows imported by the caller
    const bool exchange = resolve && !pods_cur && c->comm;                       // RCCL (a 1-rank comm too)
    if (host_xchg && !c->pods_imported) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "host transport: kdtn_pods_import the gathered pod table before kdtn_epoch_run");
        return KDTN_EINVAL;
    }
    if (c->dl_pending) {                                          // outputs still being copied out
        if (c->dl_sdma) TRY(kdtn_epoch_download_wait(c));
        else HIP_TRY(hipStreamWaitEvent(s, c->ev_dl_done, 0));
    }
    // the previous epoch's kernels are done once its sync returned, so these host stores cannot
    // race a device write; an epoch without topologies leaves them zero
    for (int i = 0; i < 4; ++i) __atomic_store_n(c->h_tot + i, 0u, __ATOMIC_RELAXED);
    if (c->timing >= 2) (void)hipEventRecord(c->ev[0], s);
    uint32_t* sync = dp<uint32_t>(c->sync);
    // Epoch front: first launch (sync header, look-back area, pod-status rows) + RCCL
    // all-gather, the dictionary parses, the pod lookup tables, in sequence. The tables need
    // nothing from the parses, but running them beside a long key-string parse did not shorten
    // the epoch (config 2): on a side stream 0.791-0.796 vs 0.789 ms (profiles/r03u_side_ab.json),
    // fused into the parse launches 0.804 vs 0.793 ms (profiles/r06ae_fuse_ab.json). When the key
    // strings to parse are few (a churn epoch's appended strings, configs 1 and 4) the five
    // launches are the cost, and one local rank fuses them into two: k_epoch_front (sync header,
    // pod rows and their lookup slots, key strings) and k_pdict_verify (slot verify, full-prefix
    // scan, property strings): config-3 churn epochs 0.762 -> 0.741 ms, config 4 0.246 -> 0.240,
    // config 1 0.223 -> 0.206 (profiles/r06ad_fuse_churn.json, r06ae_fuse_ab.json).
    constexpr uint32_t FUSE_MAX_KSTRINGS = 4u << 20;
    int fuse_mode = (c->D - std::min(c->D, c->kd_from & ~63u)) < FUSE_MAX_KSTRINGS ? 1 : 0;
#if KDTN_PROFILING
    if (const char* ev = std::getenv("KDTN_FUSE")) fuse_mode = std::atoi(ev);
#endif
    const bool fused = fuse_mode && resolve && !pods_cur && c->nranks == 1 && !c->comm && c->pod_total &&
                       c->pod_total == c->slice && !c->n_late;
    const uint32_t pod_rows = c->pod_total + c->n_late;             // gathered table + late pods
    uint32_t* special = dp<uint32_t>(c->kd_special);
    const uint32_t n16 = (uint32_t)(sync_bytes(c->nwg) / 16);
    const uint32_t nbz = std::min<uint32_t>(nblocks(n16), 256);
    c->plan = kdtn_plan{};
    c->plan.n_cus = c->n_cus;
    c->plan.nwg = c->nwg;
    c->plan.front = fused ? 1u : 0u;
    c->plan.kstrings_parsed = c->D - std::min(c->D, c->kd_from & ~63u);
    c->plan.pstrings_parsed = c->P - std::min(c->P, c->pd_from & ~63u);
    // POD_PER (4) pod rows per thread in the lookup build (every row load issued before the
    // dependent accesses): rank of 8 0.1761 / 0.1770 → 0.1735 / 0.1744 ms, N = 1 0.7895 → 0.7883 ms
    // (profiles/r05h_pod_per_ab_*)
    auto lookup_build = [&]() -> int {
        if (++c->pod_stamp >= 0x7FFFFFFFu) {                             // stamp wrap: clear once
            HIP_TRY(hipMemsetAsync(c->pod_direct.p, 0, c->pod_direct.cap, s));
            HIP_TRY(hipMemsetAsync(c->pod_ovf.p, 0, c->pod_ovf.cap, s));
            c->pod_stamp = 1;
        }
        k_pod_direct_scatter<<<nblocks(pod_rows, BLOCK * POD_PER), BLOCK, 0, s>>>(
            dp<uint4>(c->pods), pod_rows, dp<uint32_t>(c->kd_bits) + (size_t)KB_PHYSICAL * c->kb_words,
            dp<uint8_t>(c->kd_bytes), dp<uint32_t>(c->kd_offs), dp<uint4>(c->pod_direct), c->pod_stamp, c->D,
            c->pods_rank_major ? (uint32_t)c->nranks : 1u, c->pod_total);
        return KDTN_OK;
    };
    auto verify_prefix = [&]() {
        const uint32_t nbv = nblocks(pod_rows, BLOCK * POD_PER);
        const uint32_t nbp = (uint32_t)std::min<uint64_t>(4 * FP_GRID, (c->T + 4 * BLOCK - 1) / (4 * BLOCK));
        k_pod_verify_prefix<<<nbv + std::max<uint32_t>(nbp, 1), BLOCK, 0, s>>>(
            dp<uint4>(c->pods), pod_rows, dp<uint4>(c->pod_direct), c->pod_stamp,
            dp<unsigned long long>(c->pod_ovf), c->ovf_mask, c->D, T, sync + SYNC_FIRST_PARTIAL_INV, nbv,
            c->pods_rank_major ? (uint32_t)c->nranks : 1u, c->pod_total);
    };
    if (fused) {
        if (++c->pod_stamp >= 0x7FFFFFFFu) {                             // stamp wrap: clear once
            HIP_TRY(hipMemsetAsync(c->pod_direct.p, 0, c->pod_direct.cap, s));
            HIP_TRY(hipMemsetAsync(c->pod_ovf.p, 0, c->pod_ovf.cap, s));
            c->pod_stamp = 1;
        }
        const uint32_t k0 = c->kd_from & ~63u, p0 = c->pd_from & ~63u;  // (clip_specials ran at upload)
        const uint32_t nbs = nblocks(c->slice);
        const uint32_t nbk = c->D > k0 ? nblocks(c->D - k0) : 0u;
        k_epoch_front<<<nbz + nbs + nbk, BLOCK, 0, s>>>(
            reinterpret_cast<uint4*>(sync), n16, nbz, nbs, T, c->slice, dp<uint4>(c->pods), dp<uint4>(c->pod_direct),
            c->pod_stamp, dp<uint8_t>(c->kd_bytes), dp<uint32_t>(c->kd_offs), k0, c->D, dp<uint32_t>(c->kd_bits),
            c->kb_words, special);
        timer_mark(c, "epoch_front", 2);
        if (c->V) {
            TRY(build_vni_table(c));
            timer_mark(c, "hash_build", 2);
        }
        const uint32_t nbv = nblocks(c->pod_total);
        const uint32_t nbp = std::max<uint32_t>(1, (uint32_t)std::min<uint64_t>(4 * FP_GRID, (c->T + 4 * BLOCK - 1) / (4 * BLOCK)));
        const uint32_t nbd = c->P > p0 ? nblocks(c->P - p0) : 0u;
        k_pdict_verify<<<nbv + nbp + 3 * nbd, BLOCK, 0, s>>>(
            dp<uint4>(c->pods), c->pod_total, dp<uint4>(c->pod_direct), c->pod_stamp, dp<unsigned long long>(c->pod_ovf),
            c->ovf_mask, c->D, T, sync + SYNC_FIRST_PARTIAL_INV, nbv, nbp, dp<uint8_t>(c->pd_bytes),
            dp<uint32_t>(c->pd_offs), p0, c->P, nbd, c->cfg.tick_in_usec, dp<uint32_t>(c->pd_pct), dp<uint2>(c->pd_dur),
            dp<uint2>(c->pd_rate), dp<uint32_t>(c->pd_rerr));
        timer_mark(c, "pdict_verify", 2);
    } else {
        // k_epoch_begin zeroes the sync header (SYNC_*) and look-back area and fills this rank's
        // pod-status rows. With RCCL it runs on the comm stream, followed there by the
        // all-gather, beside this stream's dictionary parses; otherwise it follows the parses on
        // this stream, so the epoch's first launch is a long one and the host's later launches
        // are queued while it runs (a 2.5-µs first kernel left the GPU idle ≈ 5 µs for the next
        // launch, profiles/r05c_shardstats_trace.csv)
        const uint32_t fill = (resolve && !host_xchg && !pods_cur) ? c->slice : 0u;
        const uint32_t rank_base = c->slice * (uint32_t)c->rank;
        auto begin = [&](hipStream_t q) {
            k_epoch_begin<<<nbz + nblocks(fill), BLOCK, 0, q>>>(reinterpret_cast<uint4*>(sync), n16, nbz, T, fill,
                                                                rank_base, dp<uint4>(c->pods));
        };
        if (exchange) {
            HIP_TRY(hipEventRecord(c->ev_fill, s));                   // after the previous epoch's kernels
            HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->ev_fill, 0));
            begin(c->comm_stream);
            uint4* pods = dp<uint4>(c->pods);
            ncclResult_t r = ncclAllGather(pods + rank_base, pods, (size_t)c->slice * 4, ncclUint32, c->comm,
                                           c->comm_stream);
            if (r != ncclSuccess) {
                std::snprintf(g_last_error, sizeof(g_last_error), "ncclAllGather: %s", ncclGetErrorString(r));
                return KDTN_EIO;
            }
            HIP_TRY(hipEventRecord(c->ev_ag, c->comm_stream));
        }
        // dictionaries: the strings this upload added (all of them unless kdict_keep /
        // pdict_keep), from a multiple of 64 so every wave writes whole predicate words
        const uint32_t k0 = c->kd_from & ~63u;                            // (clip_specials ran at upload)
        if (c->D > k0) {
            const uint8_t* kb = dp<uint8_t>(c->kd_bytes);
            const uint32_t* ko = dp<uint32_t>(c->kd_offs);
            uint32_t* bits = dp<uint32_t>(c->kd_bits);
            const uint32_t nk = c->D - k0;
            auto kern = k_kdict_flags;
#if KDTN_PROFILING
            if (const char* ev = std::getenv("KDTN_KD_SUB")) {            // the kernel's floors (wrong tables)
                const int sub = std::atoi(ev);
                if (sub == 40) kern = k_kdict_null;
                else if (sub == 41) kern = k_kdict_loadonly;
            }
#endif
            kern<<<nblocks(nk), BLOCK, 0, s>>>(kb, ko, k0, c->D, bits, c->kb_words, special);
        }
        timer_mark(c, "kdict_parse", 2);
        const uint32_t p0 = c->pd_from & ~63u;
        if (c->P > p0) launch_pdict(c, p0, c->P);
        timer_mark(c, "pdict_parse", 2);
        if (!exchange) {
            begin(s);
            timer_mark(c, "pods_fill", 2);
        }
        if (resolve) {
            if (exchange) HIP_TRY(hipStreamWaitEvent(s, c->ev_ag, 0));   // exchange not hidden by the parses
            timer_mark(c, "pods_allgather", 2);
            if (pod_rows && !pods_cur) TRY(lookup_build());
            else if (!pods_cur && ++c->pod_stamp >= 0x7FFFFFFFu) {     // (no rows: the stamp still moves)
                HIP_TRY(hipMemsetAsync(c->pod_direct.p, 0, c->pod_direct.cap, s));
                HIP_TRY(hipMemsetAsync(c->pod_ovf.p, 0, c->pod_ovf.cap, s));
                c->pod_stamp = 1;
            }
            if (c->V) TRY(build_vni_table(c));
            timer_mark(c, "hash_build", 2);
        }
    }
    c->kd_valid = c->D;
    c->pd_valid = c->P;
    if (c->T) {
        DevTables tb{};
        tb.kbits = dp<uint32_t>(c->kd_bits);
        tb.kb_words = c->kb_words;
        tb.ppct = dp<uint32_t>(c->pd_pct);
        tb.pdur = dp<uint2>(c->pd_dur);
        tb.prate = dp<uint2>(c->pd_rate);
        tb.rate_err = dp<uint32_t>(c->pd_rerr);
        tb.pods = dp<uint4>(c->pods);
        tb.pod_direct = dp<uint4>(c->pod_direct);
        tb.pod_stamp = c->pod_stamp;
        tb.pod_ovf = dp<unsigned long long>(c->pod_ovf);
        tb.ovf_mask = c->ovf_mask;
        tb.vnis = dp<uint4>(c->v_table);
        tb.vni_slots = dp<uint32_t>(c->v_slots);
        tb.vni_mask = c->V ? c->vni_mask : 0;
        tb.special = special;
        tb.vxlan_base = c->cfg.vxlan_base;
        RecOut o;
        o.action = dp<uint8_t>(c->action);
        o.del_off = dp<uint32_t>(c->del_off);
        o.add_off = dp<uint32_t>(c->add_off);
        o.upd_off = dp<uint32_t>(c->upd_off);
        o.del_idx = dp<uint32_t>(c->del_idx);
        o.add_idx = dp<uint32_t>(c->add_idx);
        o.upd_idx = dp<uint32_t>(c->upd_idx);
        o.del_res = dp<uint4>(c->del_res);
        o.add_res = dp<uint4>(c->add_res);
        o.upd_res = dp<uint4>(c->upd_res);
        o.add_qdisc = dp<uint2>(c->add_qdisc);
        o.upd_qdisc = dp<uint2>(c->upd_qdisc);
        o.add_qerr = dp<uint8_t>(c->add_qerr);
        o.totals = sync + SYNC_TOTALS;
        o.htotals = c->h_tot;
        o.stages = stages;
        RecWork w;
        w.sync = sync;
        w.herr = c->h_tot + 3;
        w.status = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->sync.p) + SYNC_HEADER_BYTES);
        w.hscratch = dp<uint32_t>(c->hscratch);
        w.fscratch = dp<uint8_t>(c->fscratch);
        w.otarget = dp<uint32_t>(c->otarget);
        w.nwg = c->nwg;
        w.trace = nullptr;
        w.first_partial_inv = sync + SYNC_FIRST_PARTIAL_INV;         // 0 (none) from the memset
        w.wcount = reinterpret_cast<uint32_t*>(static_cast<char*>(c->sync.p) + sync_counts_at(c->nwg));
        w.m_cap = c->real.n;
        w.n_cap = c->des.n;
        uint32_t* wbase = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(w.wcount) + align_up((size_t)c->nwg * 12, 16));
        // several workgroups per chunk when the chunks would not fill the chip about six times
        // over (4 resident k_reconcile workgroups per CU): they share a bulk chunk's records,
        // at least ~300 records per part (measured: 125k-pod config 2, 640 records per chunk:
        // split 2 0.097 ms, 3 0.106, 4 0.115; 100k-site config 4, 1267 per chunk: split 2 / 3 /
        // 4 / 6 / 8 0.156 / 0.158 / 0.150 / 0.174 / 0.166 ms, profiles/r06v_split_sweep.json)
        // Only bulk chunks share their records; in a chunk with comparisons the other parts
        // return at once, so an epoch whose realised lists are a large share of the records
        // runs one workgroup per chunk (config 1, 1274 records per chunk: split 1 / 2 / 4
        // 0.185 / 0.186 / 0.205 ms, the same record)
        const uint64_t per_chunk = ((uint64_t)c->real.n + c->des.n) / std::max<uint32_t>(c->nwg, 1);
        const bool cmp_heavy = (uint64_t)c->real.n * 4 > c->des.n;
        w.split = cmp_heavy ? 1u
                            : std::max<uint32_t>(1, std::min<uint32_t>({4u, (6 * 4 * c->n_cus + c->nwg - 1) / c->nwg,
                                                                        (uint32_t)std::max<uint64_t>(1, per_chunk / 300)}));
#if KDTN_PROFILING
        if (const char* ev = std::getenv("KDTN_SPLIT")) if (std::atoi(ev) > 0) w.split = (uint32_t)std::atoi(ev);
#endif
        if (fused) {                                     // verify + prefix ran in k_pdict_verify
        } else if (resolve && pod_rows && !pods_cur) {   // the pod-table verify with the full-prefix scan
            verify_prefix();
            timer_mark(c, "verify_prefix", 2);
        } else {
            k_full_prefix<<<(unsigned)std::min<uint64_t>(FP_GRID, (c->T + 4 * FP_BLOCK - 1) / (4 * FP_BLOCK)), FP_BLOCK, 0, s>>>(
                T, sync + SYNC_FIRST_PARTIAL_INV);
            timer_mark(c, "full_prefix", 2);
        }
        if (c->timing == 1) (void)hipEventRecord(c->ev[0], s);
        // CalcDiff windows (both lists non-empty): the comparison-heavy build
        int variant = (c->real.n && c->des.n) ? DIFF_VARIANT : DEFAULT_VARIANT;
#if KDTN_PROFILING
        if (const char* ev = std::getenv("KDTN_VARIANT")) variant = std::atoi(ev);
        if (variant & VAR_TRACE) {
            w.split = 1;                                           // trace slots per chunk
            TRY(ensure(c->trace, (size_t)c->nwg * TRACE_WORDS * 8));
            w.trace = reinterpret_cast<unsigned long long*>(c->trace.p);
            c->traced = true;
        }
#endif
        const bool placed = (variant & VAR_DIFF) != 0;           // deferred chunks, then k_place_scan + k_place
        if (placed && ((size_t)c->real.n * 2 > c->del_idx.cap / 4 || (size_t)c->des.n * 2 > c->add_idx.cap / 4)) {
            std::snprintf(g_last_error, sizeof(g_last_error), "deferred placement without upper halves");
            return KDTN_EINVAL;
        }
        switch (variant) {
#define KDTN_VARIANT_CASE(V) \
        case V: k_reconcile<V><<<c->nwg * w.split, BLOCK, 0, s>>>(T, c->real.view, c->des.view, tb, o, w); break;
        KDTN_VARIANT_CASE(DEFAULT_VARIANT)
        KDTN_VARIANT_CASE(DIFF_VARIANT)
#if KDTN_PROFILING
        KDTN_PROFILING_VARIANTS(KDTN_VARIANT_CASE)
#endif
#undef KDTN_VARIANT_CASE
        default:
            std::snprintf(g_last_error, sizeof(g_last_error), "k_reconcile variant %d is not instantiated", variant);
            return KDTN_EINVAL;
        }
        timer_mark(c, "reconcile", 1);
        c->plan.diff_build = placed ? 1u : 0u;
        c->plan.split = w.split;
        if (placed) {
            k_place_scan<<<1, PLACE_SCAN_BLOCK, 0, s>>>(w.wcount, c->nwg, wbase, o, c->T);
            timer_mark(c, "place_scan", 1);
            if (c->nwg >= 4u * c->n_cus) {               // enough chunks for a wave each
                k_place<true><<<(c->nwg + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, s>>>(
                    T, w.wcount, wbase, w.first_partial_inv, o, w.m_cap, w.n_cap, c->nwg, 1u);
                c->plan.place = 1;
                c->plan.place_parts = 1;
            } else {                                      // workgroups per chunk to fill the chip
                const uint32_t parts = std::min<uint32_t>(16u, std::max<uint32_t>(1u, 4u * c->n_cus / std::max<uint32_t>(c->nwg, 1u)));
                k_place<false><<<c->nwg * parts, BLOCK, 0, s>>>(T, w.wcount, wbase, w.first_partial_inv, o, w.m_cap,
                                                                w.n_cap, c->nwg, parts);
                c->plan.place = 2;
                c->plan.place_parts = parts;
            }
            timer_mark(c, "place", 1);
        }
    } else {
        HIP_TRY(hipMemsetAsync(c->h_tot, 0, 16, s));   // (an earlier run may not have been synced)
        HIP_TRY(hipMemsetAsync(c->del_off.p, 0, 4, s));
        HIP_TRY(hipMemsetAsync(c->add_off.p, 0, 4, s));
        HIP_TRY(hipMemsetAsync(c->upd_off.p, 0, 4, s));
    }
    HIP_TRY(hipGetLastError());
    if (c->ev_done) HIP_TRY(hipEventRecord(c->ev_done, s));
    if (resolve && !pods_cur) c->pods_ready = true;           // the full build of this upload's rows
    c->ran = true;
    c->synced = false;
    c->encoded = false;
    c->tc_done = false;
    c->fan_valid = false;
    c->lc_valid = false;
    c->si_run = false;
    c->se_run = false;
    c->sj_done = false;
    c->rp_done = false;
    c->vx_imported = false;
    c->vx_contest_ok = false;
    return KDTN_OK;
}

int kdtn_epoch_sync(kdtn_ctx* c, kdtn_counts* counts) {
    if (!c || !c->ran) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    // poll the epoch's completion event (a host-memory signal) for a bounded time before the
    // blocking stream sync: a sub-millisecond epoch is seen ending sooner than from a sleeping
    // wait, and a long one (or a hung GPU) does not hold a host core
    if (c->ev_done) {
        const auto t0 = std::chrono::steady_clock::now();
        while (hipEventQuery(c->ev_done) == hipErrorNotReady &&
               std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(kSyncSpinUs)) {
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRY(read_totals(c));
    if (counts) {
        counts->n_del = c->h_misc[1];
        counts->n_upd = c->h_misc[2];
        counts->n_add = c->h_misc[3];
        counts->n_topos = c->T;
    }
    for (int i = 0; i < c->n_ev; ++i) {                 // this epoch's marks into the totals
        float t = 0.f;
        (void)hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]);
        int k = 0;
        while (k < c->n_acc && std::strcmp(c->acc_name[k], c->ev_name[i]) != 0) ++k;
        if (k == c->n_acc) {
            if (k == kMaxTimers) continue;
            c->acc_name[k] = c->ev_name[i];
            c->acc_ms[k] = 0.0;
            c->acc_n[k] = 0;
            ++c->n_acc;
        }
        c->acc_ms[k] += t;
        bool first = true;                              // a stage marked in pieces counts once
        for (int j = 0; j < i; ++j) first &= std::strcmp(c->ev_name[j], c->ev_name[i]) != 0;
        if (first) ++c->acc_n[k];
    }
    return KDTN_OK;
}

int kdtn_timer_totals(kdtn_ctx* c, const char** names, double* ms, uint32_t* epochs, int cap, int reset) {
    if (!c || cap < 0) return KDTN_EINVAL;
    const int n = std::min(cap, c->n_acc);
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = c->acc_name[i];
        if (ms) ms[i] = c->acc_ms[i];
        if (epochs) epochs[i] = c->acc_n[i];
    }
    if (reset) c->n_acc = 0;
    return n;
}

// the output copies of kdtn_epoch_download(_async) on stream `hs`
static int download_enqueue(kdtn_ctx* c, kdtn_batches* o, hipStream_t hs) {
    const uint32_t nd = c->h_misc[1], nu = c->h_misc[2], na = c->h_misc[3];
    o->n_del = nd;
    o->n_upd = nu;
    o->n_add = na;
    if (nd > o->del_cap || nu > o->upd_cap || na > o->add_cap) return KDTN_ENOSPC;
    auto d2h = [&](void* dst, DevBuf& b, size_t bytes) -> int {
        if (dst && bytes) HIP_TRY(hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, hs));
        return KDTN_OK;
    };
    const bool res = c->last_stages & KDTN_STAGE_RESOLVE, q = c->last_stages & KDTN_STAGE_QDISC;
    TRY(d2h(o->action, c->action, c->T));
    TRY(d2h(o->del_off, c->del_off, (size_t)(c->T + 1) * 4));
    TRY(d2h(o->add_off, c->add_off, (size_t)(c->T + 1) * 4));
    TRY(d2h(o->upd_off, c->upd_off, (size_t)(c->T + 1) * 4));
    TRY(d2h(o->del_idx, c->del_idx, (size_t)nd * 4));
    TRY(d2h(o->add_idx, c->add_idx, (size_t)na * 4));
    TRY(d2h(o->upd_idx, c->upd_idx, (size_t)nu * 4));
    if (res) {
        TRY(d2h(o->del_res, c->del_res, (size_t)nd * 16));
        TRY(d2h(o->add_res, c->add_res, (size_t)na * 16));
        TRY(d2h(o->upd_res, c->upd_res, (size_t)nu * 16));
    }
    if (q) {
        TRY(d2h(o->add_qdisc, c->add_qdisc, (size_t)na * 72));
        TRY(d2h(o->upd_qdisc, c->upd_qdisc, (size_t)nu * 72));
    }
    return KDTN_OK;
}

// HSA agents and the SDMA engine for device-to-host copies, once per context
static bool sdma_setup(kdtn_ctx* c) {
    if (c->sdma_tried) return c->sdma_ok;
    c->sdma_tried = true;
    if (hsa_init() != HSA_STATUS_SUCCESS) return false;
    hsa_amd_pointer_info_t dv{}, hv{};
    dv.size = hv.size = sizeof(hsa_amd_pointer_info_t);
    uint32_t mask = 0, pref = 0;
    bool ok = c->sync.p && hsa_amd_pointer_info(c->sync.p, &dv, nullptr, nullptr, nullptr) == HSA_STATUS_SUCCESS &&
              dv.type == HSA_EXT_POINTER_TYPE_HSA &&
              hsa_amd_pointer_info(c->h_misc, &hv, nullptr, nullptr, nullptr) == HSA_STATUS_SUCCESS &&
              hv.type == HSA_EXT_POINTER_TYPE_HSA;
    if (ok) {
        hsa_device_type_t tg = HSA_DEVICE_TYPE_CPU, th = HSA_DEVICE_TYPE_GPU;
        ok = hsa_agent_get_info(dv.agentOwner, HSA_AGENT_INFO_DEVICE, &tg) == HSA_STATUS_SUCCESS &&
             hsa_agent_get_info(hv.agentOwner, HSA_AGENT_INFO_DEVICE, &th) == HSA_STATUS_SUCCESS &&
             tg == HSA_DEVICE_TYPE_GPU && th == HSA_DEVICE_TYPE_CPU &&
             hsa_amd_memory_copy_engine_status(hv.agentOwner, dv.agentOwner, &mask) == HSA_STATUS_SUCCESS && mask;
    }
    if (ok) {
        (void)hsa_amd_memory_get_preferred_copy_engine(hv.agentOwner, dv.agentOwner, &pref);
        const uint32_t pick = (pref & mask) ? (pref & mask) : mask;
        // one engine, the lowest preferred one: beside the runtime's host-to-device copies it
        // keeps 48 GB/s where the H2D-preferred engine falls to 28 (tools/sdma_probe.cpp,
        // profiles/r06c_sdma_probe.jsonl). The download's pieces split over two engines measured
        // no faster (profiles/r06f_resident_engines.jsonl); the profiling build can still ask
        // for two (KDTN_SDMA_ENGINE = two engine bits)
        c->sdma_engine[0] = pick & (~pick + 1u);
        c->sdma_engine[1] = 0;
#if KDTN_PROFILING
        if (const char* ev = std::getenv("KDTN_SDMA_ENGINE")) {        // (A/B) engine bits of the mask
            const uint32_t e = (uint32_t)std::atoi(ev) & mask;
            if (e) {
                c->sdma_engine[0] = e & (~e + 1u);
                const uint32_t r2 = e & ~c->sdma_engine[0];
                c->sdma_engine[1] = r2 & (~r2 + 1u);
            }
        }
#endif
        c->sdma_gpu = dv.agentOwner;
        c->sdma_cpu = hv.agentOwner;
        ok = hsa_signal_create(0, 0, nullptr, &c->dl_sig) == HSA_STATUS_SUCCESS;
    }
    if (!ok) (void)hsa_shut_down();
    c->sdma_ok = c->sdma_inited = ok;
    return ok;
}

// The download's copies on the context's SDMA engine, completion on dl_sig. false (nothing
// issued) when a destination is not page-locked host memory the engine can write, or the
// setup failed: the caller takes the HIP copies. The epoch's kernels have completed (after
// kdtn_epoch_sync, whose completion event carries the system-scope release).
static bool sdma_download(kdtn_ctx* c, kdtn_batches* o) {
    if (!sdma_setup(c)) return false;
    const uint32_t nd = c->h_misc[1], nu = c->h_misc[2], na = c->h_misc[3];
    o->n_del = nd;
    o->n_upd = nu;
    o->n_add = na;
    if (nd > o->del_cap || nu > o->upd_cap || na > o->add_cap) return false;   // (the HIP path reports it)
    struct Piece { void* dst; const void* src; size_t bytes; };
    Piece pc[12];
    int n = 0;
    auto add = [&](void* dst, DevBuf& b, size_t bytes) {
        if (dst && bytes) pc[n++] = Piece{dst, b.p, bytes};
    };
    const bool res = c->last_stages & KDTN_STAGE_RESOLVE, q = c->last_stages & KDTN_STAGE_QDISC;
    add(o->action, c->action, c->T);
    add(o->del_off, c->del_off, (size_t)(c->T + 1) * 4);
    add(o->add_off, c->add_off, (size_t)(c->T + 1) * 4);
    add(o->upd_off, c->upd_off, (size_t)(c->T + 1) * 4);
    add(o->del_idx, c->del_idx, (size_t)nd * 4);
    add(o->add_idx, c->add_idx, (size_t)na * 4);
    add(o->upd_idx, c->upd_idx, (size_t)nu * 4);
    if (res) {
        add(o->del_res, c->del_res, (size_t)nd * 16);
        add(o->add_res, c->add_res, (size_t)na * 16);
        add(o->upd_res, c->upd_res, (size_t)nu * 16);
    }
    if (q) {
        add(o->add_qdisc, c->add_qdisc, (size_t)na * 72);
        add(o->upd_qdisc, c->upd_qdisc, (size_t)nu * 72);
    }
    for (int i = 0; i < n; ++i) {                   // page-locked, and the whole range inside it
        hsa_amd_pointer_info_t pi{};
        pi.size = sizeof pi;
        if (hsa_amd_pointer_info(pc[i].dst, &pi, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return false;
        if (pi.type != HSA_EXT_POINTER_TYPE_HSA && pi.type != HSA_EXT_POINTER_TYPE_LOCKED) return false;
        uint8_t* b = static_cast<uint8_t*>(pi.hostBaseAddress);
        uint8_t* d = static_cast<uint8_t*>(pc[i].dst);
        if (!b || d < b || d + pc[i].bytes > b + pi.sizeInBytes) return false;
        // Memory registered with hipHostRegister / hsa_amd_memory_lock is reached by the copy
        // engine through its agent address, which need not equal the host address: the
        // engine writes agentBaseAddress + (d - hostBaseAddress). HSA allocations map both alike.
        if (pi.type == HSA_EXT_POINTER_TYPE_LOCKED) {
            if (!pi.agentBaseAddress) return false;
            pc[i].dst = static_cast<uint8_t*>(pi.agentBaseAddress) + (d - b);
        }
    }
    if (!n) return true;
    hsa_signal_store_screlease(c->dl_sig, n);
    {
        SdmaInflight& f = sdma_inflight();
        std::lock_guard<std::mutex> lk(f.m);
        f.sig.push_back(c->dl_sig.handle);
    }
    c->dl_sdma = c->dl_pending = true;
    // pieces to the engine with fewer bytes queued, largest first (one signal counts them all)
    int order[12];
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order, order + n, [&](int a, int b) { return pc[a].bytes > pc[b].bytes; });
    size_t queued[2] = {0, 0};
    for (int k = 0; k < n; ++k) {
        const int i = order[k];
        const int e = (c->sdma_engine[1] && queued[1] < queued[0]) ? 1 : 0;
        queued[e] += pc[i].bytes;
        if (hsa_amd_memory_async_copy_on_engine(pc[i].dst, c->sdma_cpu, pc[i].src, c->sdma_gpu, pc[i].bytes, 0, nullptr,
                                                c->dl_sig, (hsa_amd_sdma_engine_id_t)c->sdma_engine[e],
                                                true) != HSA_STATUS_SUCCESS) {
            hsa_signal_subtract_screlease(c->dl_sig, n - k);       // the pieces never issued
            (void)kdtn_epoch_download_wait(c);
            c->sdma_ok = false;                                    // HIP copies from now on
            return false;
        }
    }
    return true;
}

int kdtn_epoch_download(kdtn_ctx* c, kdtn_batches* o) {
    if (!c || !o || !c->ran) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    TRY(counts_fresh(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRY(kdtn_epoch_download_wait(c));
    if (sdma_download(c, o)) return kdtn_epoch_download_wait(c);
    TRY(download_enqueue(c, o, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KDTN_OK;
}

// Asynchronous form: the copies run on a stream of their own after the epoch, beside whatever
// the caller enqueues next (commit, the next delta upload's host-to-device copies: the link is
// full duplex); the next kdtn_epoch_run waits for them on the GPU before it overwrites the
// outputs. The host buffers (page-locked, kdtn_host_alloc) hold the outputs once
// kdtn_epoch_download_wait returns. Counts are known at return (after kdtn_epoch_sync).
int kdtn_epoch_download_async(kdtn_ctx* c, kdtn_batches* o) {
    if (!c || !o || !c->ran) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    TRY(counts_fresh(c));
    TRY(kdtn_epoch_download_wait(c));
    HIP_TRY(hipStreamSynchronize(c->stream));       // (idle after kdtn_epoch_sync: returns at once)
    if (sdma_download(c, o)) return KDTN_OK;
    hipStream_t hs = c->d2h_stream ? c->d2h_stream : c->stream;
    HIP_TRY(hipEventRecord(c->ev_dl_ready, c->stream));
    HIP_TRY(hipStreamWaitEvent(hs, c->ev_dl_ready, 0));
    TRY(download_enqueue(c, o, hs));
    HIP_TRY(hipEventRecord(c->ev_dl_done, hs));
    c->dl_pending = true;
    return KDTN_OK;
}

int kdtn_epoch_download_wait(kdtn_ctx* c) {
    if (!c) return KDTN_EINVAL;
    if (!c->dl_pending) return KDTN_OK;
    if (c->dl_sdma) {
        sdma_wait(c->dl_sig);
        SdmaInflight& f = sdma_inflight();
        std::lock_guard<std::mutex> lk(f.m);
        f.sig.erase(std::remove(f.sig.begin(), f.sig.end(), c->dl_sig.handle), f.sig.end());
        c->dl_sdma = c->dl_pending = false;
        return KDTN_OK;
    }
    HIP_TRY(hipEventSynchronize(c->ev_dl_done));
    c->dl_pending = false;
    return KDTN_OK;
}

int kdtn_reconcile_epoch(kdtn_ctx* c, const kdtn_epoch_in* in, kdtn_batches* out) {
    TRY(kdtn_epoch_upload(c, in));
    TRY(kdtn_epoch_run(c, KDTN_STAGE_ALL));
    TRY(kdtn_epoch_sync(c, nullptr));
    return kdtn_epoch_download(c, out);
}

int kdtn_diff(kdtn_ctx* c, const kdtn_epoch_in* in, kdtn_batches* out) {
    TRY(kdtn_epoch_upload(c, in));
    TRY(kdtn_epoch_run(c, KDTN_STAGE_DIFF));
    TRY(kdtn_epoch_sync(c, nullptr));
    return kdtn_epoch_download(c, out);
}

// One daemon batch as a one-topology epoch: the pods become the topology table (so peer
// lookups see the informer's pods), the batch's links are the local pod's desired list
// (AddLinks: realised non-nil and empty, so every link is an add in query order) or its
// realised list (DelLinks: spec nil, so every link is a delete in query order).
int kdtn_resolve(kdtn_ctx* c, const kdtn_strtab* kdict, const kdtn_strtab* pdict, const kdtn_pod_table* pods,
                 uint32_t local, const kdtn_link_table* links, int batch_kind, const kdtn_vni_table* vnis,
                 kdtn_resolved* out, kdtn_qdisc* qout) {
    if (!c || !kdict || !pdict || !pods || !links || (links->n && !out)) return KDTN_EINVAL;
    if (local >= pods->n || (batch_kind != KDTN_BATCH_ADD && batch_kind != KDTN_BATCH_DEL)) return KDTN_EINVAL;
    if (!pods->ns || !pods->name || !pods->src_ip || !pods->net_ns || !pods->flags) return KDTN_EINVAL;
    const uint32_t P = pods->n, n = links->n;
    const bool add = batch_kind == KDTN_BATCH_ADD;
    std::vector<uint8_t> flags(pods->flags, pods->flags + P);
    std::vector<uint32_t> roff(P + 1, 0), noff(P + 1, 0);
    for (uint32_t t = 0; t < P; ++t) {
        if (t != local) flags[t] |= KDTN_TOPO_STATUS_NIL;             // no entries of their own
        else flags[t] = add ? 0u : (uint8_t)KDTN_TOPO_SPEC_NIL;
        roff[t + 1] = roff[t] + (!add && t == local ? n : 0);
        noff[t + 1] = noff[t] + (add && t == local ? n : 0);
    }
    kdtn_epoch_in in{};
    in.kdict = *kdict;
    in.pdict = *pdict;
    in.topos = kdtn_topo_table{P, pods->ns, pods->name, pods->src_ip, pods->net_ns, flags.data(), roff.data(),
                               noff.data()};
    kdtn_link_table empty{};
    in.realised = add ? empty : *links;
    in.desired = add ? *links : empty;
    if (vnis) in.vnis = *vnis;
    TRY(kdtn_epoch_upload(c, &in));
    TRY(kdtn_epoch_run(c, add ? KDTN_STAGE_ALL : (KDTN_STAGE_DIFF | KDTN_STAGE_RESOLVE)));
    kdtn_counts cnt{};
    TRY(kdtn_epoch_sync(c, &cnt));
    if ((add ? cnt.n_add : cnt.n_del) != n) {
        std::snprintf(g_last_error, sizeof(g_last_error), "kdtn_resolve: %u of %u links planned",
                      add ? cnt.n_add : cnt.n_del, n);
        return KDTN_EIO;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (n) {
        HIP_TRY(hipMemcpyAsync(out, add ? c->add_res.p : c->del_res.p, (size_t)n * 16, hipMemcpyDeviceToHost,
                               c->stream));
        if (add && qout)
            HIP_TRY(hipMemcpyAsync(qout, c->add_qdisc.p, (size_t)n * 72, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KDTN_OK;
}

void* kdtn_host_alloc(uint64_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void kdtn_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int kdtn_make_qdiscs(kdtn_ctx* c, const kdtn_strtab* pdict, const kdtn_props_table* props,
                     kdtn_qdisc* out) {
    if (!c || !pdict || !props || (!out && props->n)) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    g_last_error[0] = 0;
    TRY(check_strtab(*pdict, "pdict"));
    const uint32_t P = pdict->n, n = props->n;
    for (int k = 0; k < KDTN_NPROP; ++k) TRY(check_ids(props->prop[k], n, P, "props"));
    if (n && !props->gap) return KDTN_EINVAL;
    c->pd_valid = c->pd_from = c->si_p = c->se_p = 0;                // this call owns the property tables now
    c->ix_p.n = c->ix_p.mask = 0;
    c->uploaded = false;
    TRY(upload_arena(c, c->pd_bytes, pdict->bytes, pdict->offs[P]));
    TRY(upload(c, c->pd_offs, pdict->offs, (size_t)(P + 1) * 4));
    TRY(ensure(c->pd_pct, (size_t)P * 4));
    TRY(ensure(c->pd_dur, (size_t)P * 8));
    TRY(ensure(c->pd_rate, (size_t)P * 8));
    TRY(ensure(c->pd_rerr, (size_t)nblocks(P) * BLOCK / 8));
    // reuse the desired-link store for the property columns
    kdtn_link_table L{};
    L.n = n;
    std::vector<uint32_t> zeros((size_t)std::max<uint32_t>(n, 1), 0u);
    std::vector<int64_t> zuid((size_t)std::max<uint32_t>(n, 1), 0);
    for (int k = 0; k < KDTN_NKEY; ++k) L.key[k] = zeros.data();
    L.uid = zuid.data();
    for (int k = 0; k < KDTN_NPROP; ++k) L.prop[k] = props->prop[k];
    L.gap = props->gap;
    TRY(upload_links(c, c->des, L, 1, P, "props"));
    TRY(ensure(c->add_qdisc, (size_t)std::max<uint32_t>(n, 1) * 72));
    hipStream_t s = c->stream;
    if (P) launch_pdict(c, 0u, P);
    DevTables tb{};
    tb.ppct = dp<uint32_t>(c->pd_pct);
    tb.pdur = dp<uint2>(c->pd_dur);
    tb.prate = dp<uint2>(c->pd_rate);
    tb.rate_err = dp<uint32_t>(c->pd_rerr);
    if (n) k_qdisc_batch<<<nblocks(n), BLOCK, 0, s>>>(c->des.view, tb, dp<uint2>(c->add_qdisc));
    HIP_TRY(hipGetLastError());
    if (n) HIP_TRY(hipMemcpyAsync(out, c->add_qdisc.p, (size_t)n * 72, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->uploaded = false;   // the desired store was reused
    return KDTN_OK;
}

int kdtn_set_timing(kdtn_ctx* c, int level) {
    if (!c || level < 0 || level > 2) return KDTN_EINVAL;
    c->timing = level;
    return KDTN_OK;
}

int kdtn_epoch_plan(kdtn_ctx* c, kdtn_plan* out) {
    if (!c || !out || !c->ran || !c->synced) return KDTN_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    *out = c->plan;
    out->first_partial_chunk = 0xFFFFFFFFu;
    if (c->T) {                                      // the sync header's word, stored inverted (0: none)
        uint32_t* h = c->h_misc + 8;
        HIP_TRY(hipMemcpyAsync(h, dp<uint32_t>(c->sync) + SYNC_FIRST_PARTIAL_INV, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (*h != 0) out->first_partial_chunk = ~*h;
    }
    return KDTN_OK;
}

int kdtn_last_kernel_times(kdtn_ctx* c, const char** names, float* ms, int cap) {
    if (!c) return KDTN_EINVAL;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    int n = std::min(cap, c->n_ev);
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = c->ev_name[i];
        float t = 0.f;
        (void)hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]);
        if (ms) ms[i] = t;
    }
    return n;
}
}  // extern "C"
