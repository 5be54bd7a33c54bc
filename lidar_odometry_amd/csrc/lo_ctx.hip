// lo_ctx.hip — the ICP context's life cycle: config defaults and validation, lo_create / lo_destroy, the scan and
// KDTree buffers, the PKO tables, lo_update_config and the setters.
//
// A context owns one HIP stream, the device-resident surfel hash table, scan buffers, the PKO tables and the DevState
// that carries the Gauss-Newton loop.  Every buffer is a lo::Buf member (lo_buf.h): lo_destroy frees them by deleting
// the context.
#include "lo_ctx_def.h"

namespace lo {
// All streams of the context drained (lo_sync, lo_set_stream, lo_destroy): the pending holds first, then the context
// stream and every lane's tail stream.
hipError_t sync_all(lo_ctx* c) {
    if (c->stream && flush_hold(c) != LO_OK) return hipErrorUnknown;   // (the text is in c->err)
    hipError_t e = c->stream ? hipStreamSynchronize(c->stream) : hipSuccess;
    for (hipStream_t s : c->q.s_tail)
        if (e == hipSuccess && s) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = group_sync(c);              // (the context stream already waits for them: flush_hold)
    return e;
}
}  // namespace lo

static int validate_config(const lo_config* g, std::string& err) {
    if (!g) { err = "null config"; return LO_ERR_ARG; }
    if (g->max_iterations < 1 || g->max_iterations > LO_MAX_ITERS) { err = "max_iterations out of [1, 64]"; return LO_ERR_ARG; }
    // >= 1: an iteration with no correspondence always fails (the reference would fall back to robust_loss_delta
    // with an empty system, IterativeClosestPointOptimizer.cpp:298-331; never reached with its default of 10)
    if (g->min_correspondence_points < 1) { err = "min_correspondence_points must be >= 1"; return LO_ERR_ARG; }
    if (g->gmm_sample_size < 1 || g->gmm_sample_size > kMaxS) { err = "gmm_sample_size out of [1, 256]"; return LO_ERR_ARG; }
    if (g->gmm_components < 1 || g->gmm_components > 3) { err = "gmm_components out of [1, 3]"; return LO_ERR_ARG; }
    if (g->pko_kernel < LO_PKO_HUBER || g->pko_kernel > LO_PKO_PSEUDO_HUBER) { err = "pko_kernel out of [0, 5]"; return LO_ERR_ARG; }
    if (g->num_alpha_segments < 1 || g->num_alpha_segments > kMaxAlpha) { err = "num_alpha_segments out of [1, 1000]"; return LO_ERR_ARG; }
    if (!(g->voxel_size > 0.0f)) { err = "voxel_size must be positive"; return LO_ERR_ARG; }   // VoxelMap.cpp:28-30
    if (g->hierarchy_factor <= 0 || g->hierarchy_factor % 2 == 0) { err = "hierarchy_factor must be positive and odd"; return LO_ERR_ARG; }
    if (g->max_points < 1 || g->max_points > kMaxBlocks * kBlock) { err = "max_points out of [1, 4194304]"; return LO_ERR_ARG; }
    return LO_OK;
}

extern "C" {

void lo_config_default_kitti(lo_config* c) {
    std::memset(c, 0, sizeof(*c));
    c->max_iterations = 4;
    c->translation_tolerance = 0.005;
    c->rotation_tolerance = 0.005;
    c->max_correspondence_distance = 1.0;
    c->min_correspondence_points = 10;
    c->use_robust_loss = 1;
    c->robust_loss_delta = 0.1;
    c->loss_cauchy = 0;
    c->use_adaptive_m_estimator = 1;
    c->min_scale_factor = 0.1;
    c->max_scale_factor = 10.0;
    c->num_alpha_segments = 100;
    c->truncated_threshold = 10.0;
    c->gmm_components = 3;
    c->gmm_sample_size = 100;
    c->pko_kernel = LO_PKO_HUBER;
    c->voxel_size = 0.5f;
    c->hierarchy_factor = 3;
    c->use_surfel_correspondence = 1;
    c->max_points = 1 << 17;
}

int lo_pko_kernel_from_name(const char* name) {
    if (!name) return LO_PKO_CAUCHY;
    const std::string k(name);
    if (k == "huber") return LO_PKO_HUBER;
    if (k == "cauchy") return LO_PKO_CAUCHY;
    if (k == "tukey") return LO_PKO_TUKEY;
    if (k == "welsch") return LO_PKO_WELSCH;
    if (k == "gemanMcClure") return LO_PKO_GEMAN_MCCLURE;
    if (k == "pseudoHuber") return LO_PKO_PSEUDO_HUBER;
    return LO_PKO_CAUCHY;                                  // "Default to Cauchy" (AdaptiveMEstimator.cpp:150-155)
}

void lo_config_default_mid360(lo_config* c) {
    lo_config_default_kitti(c);
    c->voxel_size = 0.4f;   // config/mid360.yaml:19
}

const char* lo_last_error(const lo_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
int lo_get_config(const lo_ctx* ctx, lo_config* out) {
    if (!ctx || !out) return LO_ERR_ARG;
    *out = ctx->cfg;
    return LO_OK;
}
int lo_device(const lo_ctx* ctx) { return ctx ? ctx->device : -1; }
// (whoever asks for the stream is about to enqueue on it: a pending hold goes first)
void* lo_stream(lo_ctx* ctx) {
    if (ctx) (void)flush_hold(ctx);
    return ctx ? static_cast<void*>(ctx->stream) : nullptr;
}

}  // extern "C"

namespace lo {
// per-point buffers of the KDTree correspondence stage (KDTree map mode, and the loop-closure ICP of any context)
int kd_alloc(lo_ctx* c) {
    if (c->d_kd_nbr) return LO_OK;
    const size_t NB = (static_cast<size_t>(c->cfg.max_points) + kBlock - 1) / kBlock;
    LO_HIP(c, c->d_kd_unres.reserve(NB * kBlock));
    LO_HIP(c, c->d_kd_res.reserve(NB * kBlock));
    LO_HIP(c, c->d_kd_plane.reserve(NB * kBlock));
    for (const void* f : {reinterpret_cast<const void*>(&k_knn_all), reinterpret_cast<const void*>(&k_pick_knn_all),
                          reinterpret_cast<const void*>(&k_inlier_all)})
        LO_HIP(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kKnnAllMax * sizeof(float4)));
    for (PointGrid* G : {&c->grid, &c->lgrid}) {          // empty grid until a point set is uploaded
        LO_HIP(c, G->d_start.reserve(2));
        LO_HIP(c, hipMemset(G->d_start, 0, 2 * sizeof(uint32_t)));
        G->h = 2.0f * c->cfg.voxel_size;
    }
    LO_HIP(c, c->d_kd_nbr.reserve(NB * kBlock * 5));     // last: the guard above reads it as "all of this succeeded"
    return LO_OK;
}
}  // namespace lo

// PKO tables (alpha grid, Z(alpha), the shuffle tables, the k-means draws), host-built for the context's config
// Built for config g into new buffers first; the context's tables and pointers change only once everything succeeded
// (a failed update leaves the old ones in place).
static int upload_pko_tables(lo_ctx* c, const lo_config& g) {
    PkoTables t;
    build_pko_tables(t, g.gmm_sample_size, g.gmm_components, g.max_points, g.min_scale_factor,
                     g.max_scale_factor, g.num_alpha_segments, g.truncated_threshold, g.pko_kernel);
    std::vector<int32_t> all;
    size_t off[6];
    auto append = [&](const std::vector<int32_t>& v, size_t& o) { o = all.size(); all.insert(all.end(), v.begin(), v.end()); all.push_back(0); };
    append(t.small_off, off[0]);
    append(t.small_perm, off[1]);
    append(t.base, off[2]);
    append(t.ev_off, off[3]);
    append(t.ev_steps, off[4]);
    append(t.km_draws, off[5]);
    DevBuf<double> a, z;
    DevBuf<int32_t> ti;
    LO_HIP(c, a.reserve(t.alphas.size()));
    LO_HIP(c, z.reserve(t.Z.size()));
    LO_HIP(c, ti.reserve(all.size()));
    LO_HIP(c, hipMemcpy(a, t.alphas.data(), t.alphas.size() * sizeof(double), hipMemcpyHostToDevice));
    LO_HIP(c, hipMemcpy(z, t.Z.data(), t.Z.size() * sizeof(double), hipMemcpyHostToDevice));
    LO_HIP(c, hipMemcpy(ti, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    c->d_alphas = std::move(a);
    c->d_Z = std::move(z);
    c->d_tabs_i = std::move(ti);
    c->off_small_off = off[0]; c->off_small_perm = off[1]; c->off_base = off[2];
    c->off_ev_off = off[3]; c->off_ev_steps = off[4]; c->off_km = off[5];
    c->tables = std::move(t);
    ++c->cfg_gen;
    return LO_OK;
}

static int ctx_alloc(lo_ctx* c) {
    const lo_config& g = c->cfg;
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const size_t N = static_cast<size_t>(g.max_points);
    LO_HIP(c, c->d_pts.reserve(N * 3));
    const int rc_l = lane_alloc_base(c, cur(c));         // (lane 0; its candidate buffers: ensure_acc_part)
    if (rc_l != LO_OK) return rc_l;
    LO_HIP(c, c->h_st.reserve(1));
    std::memset(c->h_st, 0, sizeof(DevState));
    LO_HIP(c, c->h_nf.reserve(1));
    *c->h_nf = 0;
    LO_HIP(c, hipMemset(cur(c).d_st, 0, sizeof(DevState)));
    // empty table (capacity 2) so a scan before any map upload finds nothing
    c->log2cap = 1;
    LO_HIP(c, c->d_tab.reserve(2));
    LO_HIP(c, hipMemset(c->d_tab, 0xff, 2 * sizeof(Slot)));
    const int rc_t = upload_pko_tables(c, c->cfg);
    if (rc_t != LO_OK) return rc_t;
    LO_HIP(c, hipEventCreate(&c->ev0));
    LO_HIP(c, hipEventCreate(&c->ev1));
    // k_pko_t's dynamic block-prefix LDS reaches 64 KB at the 4M-point maximum
    LO_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_pko_t<4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(kMaxBlocks * sizeof(int))));
    c->kd = g.use_surfel_correspondence == 0;
    if (c->kd) {
        int rc = kd_alloc(c);
        if (rc != LO_OK) return rc;
    }
    return LO_OK;
}

namespace lo {
// Live contexts (a host map holding a deferred-fit ticket asks whether its context still exists).
std::mutex g_live_mu;
std::unordered_set<const lo_ctx*> g_live;
uint64_t g_ticket = 0;
}  // namespace lo

extern "C" {

lo_ctx* lo_create(const lo_config* cfg, int device, int* err) {
    std::string e;
    int rc = validate_config(cfg, e);
    if (rc != LO_OK) { if (err) *err = rc; std::fprintf(stderr, "lo_create: %s\n", e.c_str()); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        if (err) *err = LO_ERR_HIP;
        std::fprintf(stderr, "lo_create: no HIP device %d (count %d)\n", device, ndev);
        return nullptr;
    }
    lo_ctx* c = new lo_ctx();
    c->cfg = *cfg;
    c->device = device;
    if (const char* pe = std::getenv("LO_PRESOLVE")) c->presolve = std::atoi(pe) != 0;   // A/B runs
    c->q.from_env();
    if (const char* pg = std::getenv("LO_PKO_GROUPS")) c->pko_groups = std::max(0, std::atoi(pg));
    if (const char* ps = std::getenv("LO_PKO_SOLO")) c->pko_solo = std::atoi(ps) != 0;
    if (const char* ex = std::getenv("LO_EXACT")) c->exact = std::atoi(ex) != 0;   // A/B runs: LO_EXACT=0 = fast mode
    rc = ctx_alloc(c);
    if (rc != LO_OK) {
        std::fprintf(stderr, "lo_create: %s\n", c->err.c_str());
        lo_destroy(c);
        if (err) *err = rc;
        return nullptr;
    }
    if (err) *err = LO_OK;
    {
        std::lock_guard<std::mutex> g(g_live_mu);
        g_live.insert(c);
    }
    return c;
}

void lo_destroy(lo_ctx* c) {
    if (!c) return;
    {
        std::lock_guard<std::mutex> g(g_live_mu);
        g_live.erase(c);
    }
    (void)hipSetDevice(c->device);
    (void)sync_all(c);
    for (hipStream_t s : c->q.s_tail)
        if (s) (void)hipStreamDestroy(s);
    group_release(c);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->st_ev) (void)hipEventDestroy(e);
    if (c->ev_patch) (void)hipEventDestroy(c->ev_patch);
    if (c->ev_fit) (void)hipEventDestroy(c->ev_fit);
    if (c->stream && c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;                                            // every buffer is a member that frees itself
}

// IterativeClosestPointOptimizer::update_config (IterativeClosestPointOptimizer.h:220) replaces the parameters and
// nothing else: the device map, the scan buffers and the stream stay.  The layout fields (voxel geometry, max_points,
// correspondence mode) size or key those and cannot change here.  New PKO parameters rebuild the PKO tables.
int lo_update_config(lo_ctx* c, const lo_config* cfg) {
    if (!c) return LO_ERR_ARG;
    std::string e;
    int rc = validate_config(cfg, e);
    if (rc != LO_OK) { c->err = e; return rc; }
    const lo_config& o = c->cfg;
    if (cfg->voxel_size != o.voxel_size || cfg->hierarchy_factor != o.hierarchy_factor || cfg->max_points != o.max_points ||
        cfg->use_surfel_correspondence != o.use_surfel_correspondence) {
        c->err = "update_config: voxel_size / hierarchy_factor / max_points / use_surfel_correspondence are fixed at lo_create";
        return LO_ERR_STATE;
    }
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, sync_all(c));
    const bool pko_changed = cfg->gmm_sample_size != o.gmm_sample_size || cfg->gmm_components != o.gmm_components ||
                             cfg->min_scale_factor != o.min_scale_factor || cfg->max_scale_factor != o.max_scale_factor ||
                             cfg->num_alpha_segments != o.num_alpha_segments ||
                             cfg->truncated_threshold != o.truncated_threshold || cfg->pko_kernel != o.pko_kernel;
    const bool na_changed = cfg->num_alpha_segments != o.num_alpha_segments;
    if (pko_changed) {                                   // the new tables first: a failure leaves the context unchanged
        rc = upload_pko_tables(c, *cfg);
        if (rc != LO_OK) return rc;
    }
    c->cfg = *cfg;
    ++c->cfg_gen;                                        // batches re-upload this context's parameters
    if (na_changed || (cfg->use_adaptive_m_estimator && !cur(c).d_acc_part)) {
        // the candidate buffers are sized by the alpha grid: the current lane's are re-made on the next optimize, every
        // other lane whole on its next use
        for (int l = 0; l < kMaxLanes; ++l) {
            ScanLane& L = c->q.lanes[l];
            if (l == c->q.lane) {
                L.d_acc_part.reset();
                L.d_cand_rec.reset();
                L.d_cand_cnt.reset();
            } else {
                L = ScanLane{};
                c->q.lane_ready[l] = false;
            }
        }
        c->q.prev_lane = -1;
    }
    return LO_OK;
}

int lo_set_exact(lo_ctx* c, int enable) {
    if (!c) return LO_ERR_ARG;
    const int rc = flush_hold(c);
    if (rc != LO_OK) return rc;
    c->exact = enable != 0;
    return LO_OK;
}

int lo_set_pko_groups(lo_ctx* c, int groups) {
    if (!c || groups < 0) return LO_ERR_ARG;
    const int rc = flush_hold(c);
    if (rc != LO_OK) return rc;
    c->pko_groups = groups;
    return LO_OK;
}

int lo_set_stream(lo_ctx* c, void* stream) {
    if (!c) return LO_ERR_ARG;
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, sync_all(c));
    if (c->own_stream) { LO_HIP(c, hipStreamDestroy(c->stream)); c->own_stream = false; }
    if (stream) c->stream = static_cast<hipStream_t>(stream);
    else { LO_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    return LO_OK;
}

int lo_icp_export_pose(lo_ctx* c, float* d_out16) {
    if (!c || !d_out16) return LO_ERR_ARG;
    const int rc = flush_hold(c);
    if (rc != LO_OK) return rc;
    hipLaunchKernelGGL(k_export_pose, dim3(1), dim3(64), 0, c->stream, cur(c).d_st, d_out16);
    LO_HIP(c, hipGetLastError());
    return LO_OK;
}

}  // extern "C"
