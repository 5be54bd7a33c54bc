// lo_batch.hip — scan-parallel batch (one GPU): the lo_batch* entry points.
//
// B contexts advance through optimize() in lockstep: one launch per kernel per GN iteration for all jobs
// (blockIdx.y = job).  The per-job KParams live in device memory (the batched kernels read them with scalar
// loads); they are rebuilt on the host every call but uploaded only when a job's scan pointer, size or map
// table changed.  The initial poses travel in a separate 12-float-per-job array (KParams::T0p).
//
// Raw scans enter through lo_batch_filter_raw*: Estimator::preprocess_frame's FastVoxelFilter (Estimator.cpp:561-588,
// VoxelMap.h:73-104) for every job in one set of five batched launches (lo_vfilter.hip k_vf_*_b), each job on its own
// context's filter buffers and into its context's d_pts.  The counts come back to the host in one copy: the optimize
// sizes its grids and sorts the jobs into its three classes from them.
//
// One batch has one correspondence mode.  A KDTree batch (every context use_surfel_correspondence = 0) replaces the
// k_correspond_b launch of each iteration by k_knn_b, k_knn_brute_b and k_plane_b (lo_kdtree.hip): the per-point
// planes, residuals, ballots and block statistics they write are what the surfel launch writes, so everything after
// them is the same launch sequence.
#include "lo_ctx_def.h"
#include "lo_lockstep.h"

#include <climits>

static constexpr int kBatchPkoWGs = 256;    // PKO workgroups per launch over all jobs (>= 1 per job; measured best)
// one single-wave PKO workgroup per job (k_pko_tb<1, true>) is opt-in (LO_BATCH_ONE_WAVE=1): with the JS phase's
// LDS alpha table the four-wave split wins at every measured size (2048 jobs 946k vs 828k scans/s, 4096 1.039M vs
// 1.021M); the one-wave variant stays tested (tests/test_gpu_batch.py) for batches beyond the measured range
static constexpr int kBatchOneWaveMin = 0x7fffffff;
// from this many small jobs the accumulate and the solve are two launches (k_accumulate_b1<false> + k_solve_b1):
// the fused form's fp64 solve holds the 8-wave accumulate at 128 VGPRs (2 workgroups per CU; split: 70, 3 per CU).
// Measured: 4096 jobs 1.037M -> 1.090M scans/s, 1024 857k -> 875k; at 64-256 jobs the extra launch costs ~1 %.
static constexpr int kBatchSplitSolveMin = 1024;

struct lo_batch {
    std::vector<lo_ctx*> ctx;
    bool kd = false;                 // KDTree-mode contexts (all of them: one batch has one correspondence mode)
    int device = 0;
    int max_iters = 0;
    int pko_max = 1;                 // min over contexts of the single-scan PKO grid
    int pko_budget = kBatchPkoWGs;   // PKO workgroups per launch over all jobs (LO_BATCH_PKO_WGS overrides)
    int one_wave_min = kBatchOneWaveMin;   // jobs from which PKO runs one wave per job (LO_BATCH_ONE_WAVE=0/1 forces)
    int split_solve_min = kBatchSplitSolveMin;   // jobs from which k_solve_b1 solves (LO_BATCH_FUSED_SOLVE=0/1 forces)
    hipStream_t stream = nullptr;
    std::string err;
    DevBuf<KParams> d_P;
    PinnedBuf<KParams> h_P;          // staging of the active jobs' params
    DevBuf<float> d_T0;
    PinnedBuf<float> h_T0;
    DevBuf<lo_batch_rec> d_rec;
    PinnedBuf<lo_batch_rec> h_rec;
    std::vector<float> T_in;         // count x 12 (T_out of failed / skipped jobs)
    std::vector<int> act;            // active job -> job index
    std::vector<size_t> n;
    struct Sig {
        const lo_ctx* ctx; uint64_t gen; const float* pts; int n; const Slot* tab; uint32_t log2cap; int exact;
        // KDTree jobs: the grid in place of the surfel table (tab is then the context's own plane buffer) -- its point
        // and cell arrays, point count, whether it carries the kd visit order, and its geometry (zero for surfel jobs)
        const float4* kd_pts; const uint32_t* kd_start; int kd_m; bool kd_order; int kd_org[3], kd_dim[3]; float kd_h;
        // field by field: the padding after n is not initialised, so a byte compare could report a change every call
        bool operator==(const Sig& o) const {
            bool same = ctx == o.ctx && gen == o.gen && pts == o.pts && n == o.n && tab == o.tab &&
                        log2cap == o.log2cap && exact == o.exact && kd_pts == o.kd_pts && kd_start == o.kd_start &&
                        kd_m == o.kd_m && kd_order == o.kd_order && kd_h == o.kd_h;
            for (int a = 0; a < 3; ++a) same = same && kd_org[a] == o.kd_org[a] && kd_dim[a] == o.kd_dim[a];
            return same;
        }
    };
    std::vector<Sig> sig;            // what d_P currently holds, per active slot
    std::vector<const float*> act_pts;   // the active jobs' scans (a KDTree job's re-run after a distance tie)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_go = nullptr;      // reference-exact jobs: the batch's uploads done (their streams wait on it)
    std::vector<hipEvent_t> ev_ex;   //   and each exact job's scan finished (the batch stream waits on them)
    int nlock = 0;                   // jobs of the last call that ran in lockstep (the first nlock params)
    // lo_batch_filter_raw*: the jobs' filter descriptors (rebuilt and uploaded every call), their counts, and the
    // events around the five filter launches (lo_batch_filter_ms)
    DevBuf<VfJob> d_jobs;
    PinnedBuf<VfJob> h_jobs;
    DevBuf<int> d_cnt;
    PinnedBuf<int> h_cnt;
    std::vector<size_t> nf;          // lo_batch_optimize_raw: the counts handed to lo_batch_optimize_async
    hipEvent_t evf0 = nullptr, evf1 = nullptr;
    bool filt_timed = false;
    bool pending = false;
    // lo_batch_update_maps (lo_devmap.hip): its per-batch state, and how to free it
    void* map_state = nullptr;
    void (*map_state_release)(void*) = nullptr;
    // lo_batch_sync_points (lo_grid.hip): the same for the batched grid build
    void* grid_state = nullptr;
    void (*grid_state_release)(void*) = nullptr;
    // lo_batch_optimize_loop_dev (lo_batch_loop.hip): the same for the batched loop-closure ICP
    void* loop_state = nullptr;
    void (*loop_state_release)(void*) = nullptr;
};

namespace lo {
BatchView batch_view(lo_batch* b) {
    for (lo_ctx* c : b->ctx) (void)flush_hold(c);      // (the map update that asks is about to change what scans read)
    return BatchView{b->ctx.data(), static_cast<int>(b->ctx.size()), b->device, b->stream, b->pending, b->kd};
}
void batch_set_error(lo_batch* b, const char* msg) { b->err = msg; }
void** batch_map_state(lo_batch* b, void (*release)(void*)) {
    b->map_state_release = release;
    return &b->map_state;
}
void** batch_grid_state(lo_batch* b, void (*release)(void*)) {
    b->grid_state_release = release;
    return &b->grid_state;
}
void** batch_loop_state(lo_batch* b, void (*release)(void*)) {
    b->loop_state_release = release;
    return &b->loop_state;
}
}  // namespace lo

static int batch_alloc(lo_batch* b) {
    const size_t B = b->ctx.size();
    LO_HIP(b, hipSetDevice(b->device));
    LO_HIP(b, hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    LO_HIP(b, b->d_P.reserve(B));
    LO_HIP(b, b->h_P.reserve(B));
    LO_HIP(b, b->d_T0.reserve(B * 12));
    LO_HIP(b, b->h_T0.reserve(B * 12));
    LO_HIP(b, b->d_rec.reserve(B));
    LO_HIP(b, b->h_rec.reserve(B));
    LO_HIP(b, hipEventCreate(&b->ev0));
    LO_HIP(b, hipEventCreate(&b->ev1));
    LO_HIP(b, hipEventCreateWithFlags(&b->ev_go, hipEventDisableTiming));
    LO_HIP(b, b->d_jobs.reserve(B));
    LO_HIP(b, b->h_jobs.reserve(B));
    LO_HIP(b, b->d_cnt.reserve(B));
    LO_HIP(b, b->h_cnt.reserve(B));
    LO_HIP(b, hipEventCreate(&b->evf0));
    LO_HIP(b, hipEventCreate(&b->evf1));
    b->nf.assign(B, 0);
    LO_HIP(b, lockstep_prepare());                     // the lockstep kernels' dynamic-LDS attributes
    // KDTree batches: k_knn_b, k_knn_brute_b and k_plane_b use static LDS only (no attribute to set); a job that runs
    // on its own context (a large exact job, an all-pairs grid, a re-run after a tie) goes through enqueue_optimize,
    // whose kernels' attributes lo_create set for a KDTree context (kd_alloc)
    b->T_in.assign(B * 12, 0.0f);
    b->n.assign(B, 0);
    return LO_OK;
}

// The batched filter behind lo_batch_filter_raw (host = false: raw[j] is device-readable as it is) and
// lo_batch_filter_raw_host (host = true: pinned memory is read in place, pageable memory staged in the context's
// d_raw on the batch stream).  Every argument is checked before anything is enqueued.
static int batch_filter(lo_batch* b, const float* const* raw, const size_t* n_raw, int stride, float voxel_size,
                        size_t* n_out, bool host) {
    if (!b) return LO_ERR_ARG;
    if (!raw || !n_raw || !n_out) { b->err = "null argument"; return LO_ERR_ARG; }
    if (stride < 1 || !(voxel_size > 0.0f)) { b->err = "stride must be >= 1 and voxel_size > 0"; return LO_ERR_ARG; }
    if (b->pending) { b->err = "batch in flight: call lo_batch_result first"; return LO_ERR_STATE; }
    const int B = static_cast<int>(b->ctx.size());
    const size_t st = static_cast<size_t>(stride);
    for (int j = 0; j < B; ++j) {
        if (n_raw[j] > 0 && !raw[j]) { b->err = "null raw scan with n_raw > 0"; return LO_ERR_ARG; }
        if (n_raw[j] / st + (n_raw[j] % st != 0) > static_cast<size_t>(b->ctx[j]->cfg.max_points)) {
            b->err = "ceil(n_raw / stride) exceeds max_points";
            return LO_ERR_CAPACITY;
        }
    }
    LO_HIP(b, hipSetDevice(b->device));
    for (lo_ctx* c : b->ctx) {                         // a queued single scan's pending hold first (scan overlap)
        if (flush_hold(c) != LO_OK) { b->err = c->err; return LO_ERR_HIP; }
    }
    size_t max_m = 0;
    for (int j = 0; j < B; ++j) {
        lo_ctx* c = b->ctx[j];
        const size_t m = n_raw[j] / st + (n_raw[j] % st != 0);
        const float* src = n_raw[j] > 0 ? raw[j] : nullptr;
        if (host && src) {
            src = pinned_alias(raw[j]);
            if (!src) {
                LO_HIP(b, c->d_raw.reserve(n_raw[j] * 3));
                LO_HIP(b, hipMemcpyAsync(c->d_raw, raw[j], n_raw[j] * 3 * sizeof(float), hipMemcpyHostToDevice, b->stream));
                src = c->d_raw;
            }
        }
        // growth frees the old buffers: vf_reserve drains the stream it is given (the batch's), and launches on the
        // context's own stream may still read them too; the new table's k_vf_init runs on the batch stream, before
        // the batched insert
        if (c->vf.ctr != nullptr && m > c->vf.cap) LO_HIP(b, hipStreamSynchronize(c->stream));
        LO_HIP(b, vf_reserve(c->vf, m, b->stream));
        b->h_jobs[j] = vf_job(c->vf, src, m, c->d_pts);
        max_m = std::max(max_m, m);
    }
    LO_HIP(b, hipMemcpyAsync(b->d_jobs, b->h_jobs, sizeof(VfJob) * B, hipMemcpyHostToDevice, b->stream));
    LO_HIP(b, hipEventRecord(b->evf0, b->stream));
    LO_HIP(b, vf_enqueue_batch(b->d_jobs, B, max_m, stride, voxel_size, b->d_cnt, b->stream));
    LO_HIP(b, hipEventRecord(b->evf1, b->stream));
    b->filt_timed = true;
    LO_HIP(b, hipMemcpyAsync(b->h_cnt, b->d_cnt, sizeof(int) * B, hipMemcpyDeviceToHost, b->stream));
    LO_HIP(b, hipStreamSynchronize(b->stream));
    for (int j = 0; j < B; ++j) {
        lo_ctx* c = b->ctx[j];
        n_out[j] = static_cast<size_t>(b->h_cnt[j]);
        c->last_dev_count = true;                      // as after lo_voxel_filter_gpu: lo_filtered_points,
        *c->h_nf = b->h_cnt[j];                        //   ctx_filtered_device see this scan; its count is known here
        c->nf_valid = true;
    }
    return LO_OK;
}

static int knn_blocks(int n) { return static_cast<int>((static_cast<long long>(n) * kKnnGroup + kBlock - 1) / kBlock); }

extern "C" {

lo_batch* lo_batch_create(lo_ctx* const* ctxs, int count, int* err) {
    auto fail = [&](int rc, const char* msg) -> lo_batch* {
        std::fprintf(stderr, "lo_batch_create: %s\n", msg);
        if (err) *err = rc;
        return nullptr;
    };
    if (!ctxs || count < 1 || count > 65535) return fail(LO_ERR_ARG, "need 1..65535 contexts");
    for (int j = 0; j < count; ++j) {
        const lo_ctx* c = ctxs[j];
        if (!c) return fail(LO_ERR_ARG, "null context");
        if (c->kd != ctxs[0]->kd)
            return fail(LO_ERR_ARG, "surfel-mode and KDTree-mode contexts mixed: one batch has one correspondence mode");
        if (c->device != ctxs[0]->device) return fail(LO_ERR_ARG, "contexts on different devices");
        if (c->cfg.max_iterations != ctxs[0]->cfg.max_iterations) return fail(LO_ERR_ARG, "max_iterations differ");
        for (int k = 0; k < j; ++k) if (ctxs[k] == c) return fail(LO_ERR_ARG, "a context appears twice");
    }
    lo_batch* b = new lo_batch();
    b->ctx.assign(ctxs, ctxs + count);
    b->kd = ctxs[0]->kd;
    b->device = ctxs[0]->device;
    b->max_iters = ctxs[0]->cfg.max_iterations;
    b->pko_max = kPkoMaxWGs;
    for (const lo_ctx* c : b->ctx) b->pko_max = std::min(b->pko_max, pko_grid(c->cfg));
    if (const char* e = std::getenv("LO_BATCH_PKO_WGS")) b->pko_budget = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("LO_BATCH_ONE_WAVE")) b->one_wave_min = std::atoi(e) ? 1 : 0x7fffffff;
    if (const char* e = std::getenv("LO_BATCH_FUSED_SOLVE")) b->split_solve_min = std::atoi(e) ? 0x7fffffff : 1;
    const int rc = batch_alloc(b);
    if (rc != LO_OK) {
        std::fprintf(stderr, "lo_batch_create: %s\n", b->err.c_str());
        lo_batch_destroy(b);
        if (err) *err = rc;
        return nullptr;
    }
    if (err) *err = LO_OK;
    return b;
}

void lo_batch_destroy(lo_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->map_state && b->map_state_release) b->map_state_release(b->map_state);
    if (b->grid_state && b->grid_state_release) b->grid_state_release(b->grid_state);
    if (b->loop_state && b->loop_state_release) b->loop_state_release(b->loop_state);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->ev_go) (void)hipEventDestroy(b->ev_go);
    if (b->evf0) (void)hipEventDestroy(b->evf0);
    if (b->evf1) (void)hipEventDestroy(b->evf1);
    for (hipEvent_t e : b->ev_ex) (void)hipEventDestroy(e);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

const char* lo_batch_last_error(const lo_batch* b) { return b ? b->err.c_str() : "null batch"; }
int lo_batch_size(const lo_batch* b) { return b ? static_cast<int>(b->ctx.size()) : 0; }

int lo_batch_optimize_async(lo_batch* b, const float* const* d_pts, const size_t* n, const float* T_init) {
    if (!b || !n || !T_init) return LO_ERR_ARG;
    if (b->pending) { b->err = "batch in flight: call lo_batch_result first"; return LO_ERR_STATE; }
    const int B = static_cast<int>(b->ctx.size());
    for (int j = 0; j < B; ++j) {
        if (n[j] > static_cast<size_t>(b->ctx[j]->cfg.max_points)) { b->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
        if (b->ctx[j]->cfg.max_iterations != b->max_iters) {   // lo_update_config after lo_batch_create
            b->err = "a context's max_iterations no longer matches the batch's";
            return LO_ERR_STATE;
        }
    }
    LO_HIP(b, hipSetDevice(b->device));
    for (lo_ctx* c : b->ctx) {                         // a queued single scan's pending hold first (scan overlap)
        if (flush_hold(c) != LO_OK) { b->err = c->err; return LO_ERR_HIP; }
    }
    for (int j = 0; j < B; ++j) {                      // PKO / candidate buffers first (their pointers go into the params)
        if (n[j] == 0) continue;
        const int rc = ensure_acc_part(b->ctx[j]);
        if (rc != LO_OK) { b->err = b->ctx[j]->err; return rc; }
    }
    std::memcpy(b->T_in.data(), T_init, sizeof(float) * 12 * B);
    b->act.clear();
    b->act_pts.clear();
    int max_nb = 1, max_acc = 1, n_max_ex = 1, max_knn = 1;
    bool same = true;
    // job order in the device params: the fast-mode jobs, then the reference-exact ones (both in lockstep), then the
    // exact jobs too large for the one-workgroup scale (kExactMergeMax): those run their context's own exact GN loop
    // (and so does a KDTree job whose grid is the all-pairs form, which has no batched search)
    std::vector<int> fast, exl, ex;
    for (int j = 0; j < B; ++j) {
        b->n[j] = n[j];
        if (n[j] == 0) continue;
        lo_ctx* c = b->ctx[j];
        if (c->kd && c->grid.all) ex.push_back(j);
        else if (!c->exact) fast.push_back(j);
        else if (n[j] <= static_cast<size_t>(kExactMergeMax)) exl.push_back(j);
        else ex.push_back(j);
    }
    const int nfast = static_cast<int>(fast.size()), nexl = static_cast<int>(exl.size());
    for (int pass = 0; pass < 2; ++pass) {
        for (int j : pass ? exl : fast) {
            lo_ctx* c = b->ctx[j];
            const float* pts = (d_pts && d_pts[j]) ? d_pts[j] : c->d_pts;
            const int a = static_cast<int>(b->act.size());
            KParams P = make_params(c, pts, static_cast<int>(n[j]));
            P.T0p = b->d_T0 + 12 * a;
            if (pass) {                                       // the scale comes from k_exact_scale_cb (iteration 0)
                P.scale_given = 1;
                n_max_ex = std::max(n_max_ex, P.n);
            } else {
                max_acc = std::max(max_acc, P.nb_acc);
            }
            max_nb = std::max(max_nb, P.nb);
            max_knn = std::max(max_knn, knn_blocks(P.n));
            const lo_batch::Sig sg{c, c->cfg_gen, pts, P.n, P.tab, P.log2cap, pass, P.kd_pts, P.kd_start, P.kd_m,
                                   P.kd_nodes != nullptr, {P.kd_org[0], P.kd_org[1], P.kd_org[2]},
                                   {P.kd_dim[0], P.kd_dim[1], P.kd_dim[2]}, P.kd_h};
            if (a >= static_cast<int>(b->sig.size()) || !(b->sig[a] == sg)) same = false;
            if (!same) {
                if (a < static_cast<int>(b->sig.size())) b->sig[a] = sg; else b->sig.push_back(sg);
            }
            b->h_P[a] = P;
            std::memcpy(b->h_T0 + 12 * a, T_init + 12 * j, sizeof(float) * 12);
            b->act.push_back(j);
            b->act_pts.push_back(pts);
        }
    }
    const int nact = static_cast<int>(b->act.size());
    if (b->kd && static_cast<long long>(max_knn) * nact > INT_MAX) {
        b->err = "KDTree batch: the jobs' search grid exceeds 2^31 workgroups";
        return LO_ERR_CAPACITY;
    }
    b->nlock = nact;
    // large exact jobs after the lockstep ones: only their DevState pointer is read (k_export_batch)
    for (int j : ex) {
        b->h_P[b->act.size()] = make_params(b->ctx[j], b->ctx[j]->d_pts, static_cast<int>(n[j]));
        b->act.push_back(j);
        b->act_pts.push_back((d_pts && d_pts[j]) ? d_pts[j] : b->ctx[j]->d_pts);
    }
    const int ntot = static_cast<int>(b->act.size());
    if (!ex.empty()) same = false;
    if (static_cast<int>(b->sig.size()) != ntot) { same = false; b->sig.resize(ntot); }
    LO_HIP(b, hipEventRecord(b->ev0, b->stream));
    if (ntot > 0) {
        if (nact > 0) LO_HIP(b, hipMemcpyAsync(b->d_T0, b->h_T0, sizeof(float) * 12 * nact, hipMemcpyHostToDevice, b->stream));
        if (!same) LO_HIP(b, hipMemcpyAsync(b->d_P, b->h_P, sizeof(KParams) * ntot, hipMemcpyHostToDevice, b->stream));
    }
    if (!ex.empty()) {
        // large reference-exact jobs run their context's own exact GN loop (the chip-wide sequential-sum
        // reproductions; a KDTree job on an all-pairs grid its context's own launch sequence) on the context stream, ordered after the batch's uploads (lo_batch_optimize copies their
        // points on the batch stream) and before its record export; the scan pipeline stays off for them, so every
        // launch is on the context stream and the record is final when it ends
        LO_HIP(b, hipEventRecord(b->ev_go, b->stream));
        while (b->ev_ex.size() < ex.size()) {
            hipEvent_t e = nullptr;
            LO_HIP(b, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            b->ev_ex.push_back(e);
        }
        for (size_t q = 0; q < ex.size(); ++q) {
            const int j = ex[q];
            lo_ctx* c = b->ctx[j];
            const float* pts = (d_pts && d_pts[j]) ? d_pts[j] : c->d_pts;
            LO_HIP(b, hipStreamWaitEvent(c->stream, b->ev_go, 0));
            const bool pipe = c->q.pipe, sync_call = c->sync_call;
            c->q.pipe = false;
            c->sync_call = false;
            const int rc = enqueue_optimize(c, pts, n[j], T_init + 12 * j);
            c->q.pipe = pipe;
            c->sync_call = sync_call;
            c->pending = false;                               // the batch collects the record, not lo_icp_result
            if (rc != LO_OK) { b->err = std::string("exact job: ") + c->err; return rc; }
            LO_HIP(b, hipEventRecord(b->ev_ex[q], c->stream));
            LO_HIP(b, hipStreamWaitEvent(b->stream, b->ev_ex[q], 0));
        }
    }
    if (nact > 0) {
        LockstepShape sh;
        sh.nfast = nfast;
        sh.nexl = nexl;
        sh.max_nb = max_nb;
        sh.max_knn = max_knn;
        sh.max_acc = max_acc;
        sh.n_max_ex = n_max_ex;
        sh.kd = b->kd;
        sh.pko_wgs = std::max(1, std::min(b->pko_max, b->pko_budget / nact));
        sh.one_wave = nact >= b->one_wave_min;
        sh.split_solve = nfast >= b->split_solve_min;
        LO_HIP(b, launch_lockstep(b->stream, b->d_P, sh, b->max_iters));
    }
    if (ntot > 0) {
        hipLaunchKernelGGL(k_export_batch, dim3(ntot), dim3(64), 0, b->stream, b->d_P, b->d_rec);
        LO_HIP(b, hipGetLastError());
        LO_HIP(b, hipMemcpyAsync(b->h_rec, b->d_rec, sizeof(lo_batch_rec) * ntot, hipMemcpyDeviceToHost, b->stream));
    }
    LO_HIP(b, hipEventRecord(b->ev1, b->stream));
    b->pending = true;
    return LO_OK;
}

int lo_batch_result(lo_batch* b, lo_batch_rec* out, double* gpu_ms) {
    if (!b || !out) return LO_ERR_ARG;
    if (!b->pending) { b->err = "no batch in flight"; return LO_ERR_STATE; }
    LO_HIP(b, hipSetDevice(b->device));
    LO_HIP(b, hipStreamSynchronize(b->stream));
    b->pending = false;
    const int B = static_cast<int>(b->ctx.size());
    for (int j = 0; j < B; ++j) {          // skipped jobs: the reference's false on an empty cloud (:593-603)
        lo_batch_rec& R = out[j];
        std::memset(&R, 0, sizeof(R));
        R.status = LO_INSUFFICIENT;
    }
    for (size_t a = 0; a < b->act.size(); ++a) {
        const int j = b->act[a];
        lo_ctx* c = b->ctx[j];
        const bool tie = b->h_rec[a].pad != 0.0f;
        b->h_rec[a].pad = 0.0f;
        if (tie && c->kd && c->grid_dev && !c->grid.has_order) {
            // a deciding distance tie was ranked by index (a device-built grid has no kd visit order): as lo_icp_result,
            // the order built on the host from the grid's own points, then this one job again through its context (its
            // points are still the caller's), and the record of that run
            int rc = grid_add_order(c);
            if (rc != LO_OK) { b->err = std::string("tie re-run: ") + c->err; return rc; }
            const bool pipe = c->q.pipe, sync_call = c->sync_call;
            c->q.pipe = false;
            c->sync_call = false;
            rc = enqueue_optimize(c, b->act_pts[a], b->n[j], b->T_in.data() + 12 * j);
            c->q.pipe = pipe;
            c->sync_call = sync_call;
            c->pending = false;
            if (rc != LO_OK) { b->err = std::string("tie re-run: ") + c->err; return rc; }
            hipLaunchKernelGGL(k_export_batch, dim3(1), dim3(64), 0, c->stream, b->d_P + a, b->d_rec + a);
            LO_HIP(b, hipGetLastError());
            LO_HIP(b, hipMemcpyAsync(b->h_rec + a, b->d_rec + a, sizeof(lo_batch_rec), hipMemcpyDeviceToHost, c->stream));
            LO_HIP(b, hipStreamSynchronize(c->stream));
            b->h_rec[a].pad = 0.0f;
            ++c->kd_reruns;
        }
        out[j] = b->h_rec[a];
    }
    for (int j = 0; j < B; ++j)            // optimized_transform = initial unless the GN loop succeeded (:266, :301)
        if (out[j].status != LO_OK) std::memcpy(out[j].pose, b->T_in.data() + 12 * j, sizeof(float) * 12);
    if (gpu_ms) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, b->ev0, b->ev1) != hipSuccess) ms = -1.0f;
        *gpu_ms = ms;
    }
    return LO_OK;
}

int lo_batch_bench_correspond(lo_batch* b, int reps, float* avg_ms) {
    if (!b || reps < 1 || !avg_ms) return LO_ERR_ARG;
    if (b->pending) { b->err = "batch in flight: call lo_batch_result first"; return LO_ERR_STATE; }
    const int nact = b->nlock;
    if (nact == 0) { b->err = "no lockstep batch has run yet"; return LO_ERR_STATE; }
    LO_HIP(b, hipSetDevice(b->device));
    int max_nb = 1, max_knn = 1;
    for (int a = 0; a < nact; ++a) {
        max_nb = std::max(max_nb, b->h_P[a].nb);
        max_knn = std::max(max_knn, knn_blocks(b->h_P[a].n));
    }
    // every job back at its initial pose with a fresh GN state (init launch), then reps plain launches (a KDTree
    // batch: the stage's three launches each time)
    LockstepShape sh;
    sh.nexl = nact;                                     // (the correspondence stage does not tell the classes apart)
    sh.max_nb = max_nb;
    sh.max_knn = max_knn;
    sh.kd = b->kd;
    launch_lockstep_correspond(b->stream, b->d_P, sh, 1, 1);
    LO_HIP(b, hipEventRecord(b->ev0, b->stream));
    for (int r = 0; r < reps; ++r) launch_lockstep_correspond(b->stream, b->d_P, sh, 0, 0);
    LO_HIP(b, hipEventRecord(b->ev1, b->stream));
    LO_HIP(b, hipGetLastError());
    LO_HIP(b, hipEventSynchronize(b->ev1));
    float ms = 0.0f;
    LO_HIP(b, hipEventElapsedTime(&ms, b->ev0, b->ev1));
    *avg_ms = ms / reps;
    return LO_OK;
}

int lo_batch_optimize(lo_batch* b, const float* const* pts, const size_t* n, const float* T_init, lo_batch_rec* out) {
    if (!b || !pts || !n || !T_init || !out) return LO_ERR_ARG;
    if (b->pending) { b->err = "batch in flight: call lo_batch_result first"; return LO_ERR_STATE; }
    const int B = static_cast<int>(b->ctx.size());
    LO_HIP(b, hipSetDevice(b->device));
    for (lo_ctx* c : b->ctx) {                         // a queued single scan's pending hold first (scan overlap)
        if (flush_hold(c) != LO_OK) { b->err = c->err; return LO_ERR_HIP; }
    }
    for (int j = 0; j < B; ++j) {
        if (n[j] == 0) continue;
        if (!pts[j]) return LO_ERR_ARG;
        if (n[j] > static_cast<size_t>(b->ctx[j]->cfg.max_points)) { b->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
        LO_HIP(b, hipMemcpyAsync(b->ctx[j]->d_pts, pts[j], n[j] * 3 * sizeof(float), hipMemcpyHostToDevice, b->stream));
    }
    const int rc = lo_batch_optimize_async(b, nullptr, n, T_init);
    if (rc != LO_OK) return rc;
    return lo_batch_result(b, out, nullptr);
}

int lo_batch_filter_raw(lo_batch* b, const float* const* d_raw, const size_t* n_raw, int stride, float voxel_size,
                        size_t* n_out) {
    return batch_filter(b, d_raw, n_raw, stride, voxel_size, n_out, false);
}

int lo_batch_filter_raw_host(lo_batch* b, const float* const* raw, const size_t* n_raw, int stride, float voxel_size,
                             size_t* n_out) {
    return batch_filter(b, raw, n_raw, stride, voxel_size, n_out, true);
}

double lo_batch_filter_ms(const lo_batch* b) {
    float ms = -1.0f;
    if (!b || !b->filt_timed || hipEventElapsedTime(&ms, b->evf0, b->evf1) != hipSuccess) return -1.0;
    return ms;
}

int lo_batch_optimize_raw(lo_batch* b, const float* const* raw, const size_t* n_raw, int stride, float voxel_size,
                          const float* T_init, lo_batch_rec* out, size_t* n_filtered) {
    if (!b) return LO_ERR_ARG;
    if (!T_init || !out) { b->err = "null argument"; return LO_ERR_ARG; }
    int rc = batch_filter(b, raw, n_raw, stride, voxel_size, b->nf.data(), true);
    if (rc != LO_OK) return rc;
    if (n_filtered) std::copy(b->nf.begin(), b->nf.end(), n_filtered);
    rc = lo_batch_optimize_async(b, nullptr, b->nf.data(), T_init);   // NULL d_pts: each context's filtered cloud
    if (rc != LO_OK) return rc;
    return lo_batch_result(b, out, nullptr);
}

}  // extern "C"
