// lo_hooks.hip — entry points that exist for tests and measurements: the parity hooks (correspondences, kNN, PKO
// scale, normal equations, sequential sums), stage timing, the kernel benchmarks and the debug counters.
#include "lo_device.h"   // first: the HIP runtime's device memcpy has to be declared before <cstring> names std::memcpy
#include "lo_ctx_def.h"
#include "lo_exact.h"

namespace lo {

// Parity hook of the wave-cooperative solve (lo_exact.h exact_solve_step_wave): one wave per system runs the one-lane
// exact_solve_step on lane 0 and the wave form on all 64 lanes, from the same 43 totals and pose; the raw bits of
// pn[12], delta[6] and conv go to out[sys] (one lane) and out[n + sys] (wave), kSolveWords words each.
constexpr int kSolveWords = 19;
__global__ __launch_bounds__(kWave) void k_solve_both(const float* __restrict__ totals, const float* __restrict__ poses,
                                                      int n, double tol_t, double tol_r, uint32_t* __restrict__ out) {
    const int sys = blockIdx.x, lane = threadIdx.x;
    if (sys >= n) return;
    __shared__ float s_tot[kExactTerms];
    if (lane < kExactTerms) s_tot[lane] = totals[static_cast<size_t>(sys) * kExactTerms + lane];
    float pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = poses[static_cast<size_t>(sys) * 12 + k];
    __syncthreads();
    if (lane == 0) {
        float tot[kExactTerms], pn[12], delta[6];
#pragma unroll
        for (int k = 0; k < kExactTerms; ++k) tot[k] = s_tot[k];
        const bool conv = exact_solve_step(tot, pose, tol_t, tol_r, pn, delta);
        uint32_t* o = out + static_cast<size_t>(sys) * kSolveWords;
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = __float_as_uint(pn[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) o[12 + k] = __float_as_uint(delta[k]);
        o[18] = conv ? 1u : 0u;
    }
    float pn[12], delta[6];
    const bool conv = exact_solve_step_wave(s_tot, pose, tol_t, tol_r, lane, pn, delta);
    if (lane == 0) {
        uint32_t* o = out + (static_cast<size_t>(n) + sys) * kSolveWords;
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = __float_as_uint(pn[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) o[12 + k] = __float_as_uint(delta[k]);
        o[18] = conv ? 1u : 0u;
    }
}

}  // namespace lo

extern "C" {

long long lo_debug_live_bytes(void) { return g_buf_live_bytes.load(std::memory_order_relaxed); }

static int ensure_res(lo_ctx* c, size_t n) {
    const size_t cap = std::max<size_t>(n, 256);
    LO_HIP(c, c->d_res.reserve(cap));
    LO_HIP(c, c->d_u8.reserve(cap));
    return LO_OK;
}

static int reset_state(lo_ctx* c, const float T[12], double scale, double alpha) {
    Pose12 T0;
    std::memcpy(T0.v, T, sizeof(float) * 12);
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, c->stream, cur(c).d_st, T0, scale, alpha);
    LO_HIP(c, hipGetLastError());
    return LO_OK;
}

int lo_find_correspondences(lo_ctx* c, const float* pts, size_t n, const float T[12], uint8_t* valid, double* residual) {
    if (!c || !T || (n > 0 && (!pts || !valid || !residual))) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    if (n == 0) return 0;
    LO_HIP(c, hipSetDevice(c->device));
    int rc = ensure_res(c, n);
    if (rc != LO_OK) return rc;
    rc = reset_state(c, T, 1.0, 0.1);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipMemcpyAsync(c->d_pts, pts, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    KParams P = make_params(c, c->d_pts, static_cast<int>(n));
    P.res_dbg = c->d_res;
    launch_correspond(c, P, 1, c->kd);
    LO_HIP(c, hipGetLastError());
    std::vector<int32_t> slots(n);
    LO_HIP(c, hipMemcpyAsync(slots.data(), cur(c).d_slot, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipMemcpyAsync(residual, c->d_res, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    int cnt = 0;
    for (size_t i = 0; i < n; ++i) { valid[i] = slots[i] >= 0 ? 1 : 0; cnt += valid[i]; }
    return cnt;
}

int lo_knn_search(lo_ctx* c, const float* q, size_t n, int32_t* idx, float* dist) {
    if (!c || (n > 0 && (!q || !idx || !dist))) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (!c->kd) { c->err = "lo_knn_search needs use_surfel_correspondence = 0"; return LO_ERR_STATE; }
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    if (n == 0) return 0;
    LO_HIP(c, hipSetDevice(c->device));
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};       // Matrix4f * (x, y, z, 1) is exact at I
    int rc = reset_state(c, I, 1.0, 0.1);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipMemcpyAsync(c->d_pts, q, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    KParams P = make_params(c, c->d_pts, static_cast<int>(n));
    KParams Pn = P;
    Pn.init = 0;
    hipLaunchKernelGGL(k_knn, dim3((n * kKnnGroup + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, P);
    launch_brute(c, Pn);
    hipLaunchKernelGGL(k_knn_reset, dim3(1), dim3(64), 0, c->stream, Pn);
    LO_HIP(c, hipGetLastError());
    std::vector<int32_t> nb(5 * n);
    std::vector<float4> mp(static_cast<size_t>(std::max(c->grid.m, 1)));
    LO_HIP(c, hipMemcpyAsync(nb.data(), c->d_kd_nbr, nb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (c->grid.m > 0)
        LO_HIP(c, hipMemcpyAsync(mp.data(), c->grid.d_pts, c->grid.m * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    int cnt = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool ok = nb[5 * i] >= 0;
        cnt += ok ? 1 : 0;
        for (int k = 0; k < 5; ++k) {
            if (!ok) { idx[5 * i + k] = -1; dist[5 * i + k] = INFINITY; continue; }
            const float4 v = mp[nb[5 * i + k]];
            int32_t id;
            std::memcpy(&id, &v.w, sizeof(id));
            const float dx = q[3 * i] - v.x, dy = q[3 * i + 1] - v.y, dz = q[3 * i + 2] - v.z;
            idx[5 * i + k] = id;
            dist[5 * i + k] = (dx * dx + dy * dy) + dz * dz;
        }
    }
    return cnt;
}

double lo_pko_scale_factor(lo_ctx* c, const double* residuals, size_t n, double* gmm_out) {
    if (!c || (n > 0 && !residuals)) return NAN;
    if (flush_hold(c) != LO_OK) return NAN;
    if (n == 0) return 1.0;                                  // calculate_scale_factor, empty input (:66-69)
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return NAN; }
    if (hipSetDevice(c->device) != hipSuccess) return NAN;
    if (ensure_res(c, n) != LO_OK) return NAN;
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (reset_state(c, I, 1.0, 0.1) != LO_OK) return NAN;
    if (hipMemcpyAsync(c->d_res, residuals, n * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) return NAN;
    KParams P = make_params(c, c->d_pts, static_cast<int>(n));
    P.direct_res = c->d_res;
    P.use_pko = 1;
    launch_pko(c, P, 0);
    hipLaunchKernelGGL(k_pko_finish, dim3(1), dim3(64), 0, c->stream, P);
    if (hipGetLastError() != hipSuccess) return NAN;
    if (hipMemcpyAsync(c->h_st, cur(c).d_st, sizeof(DevState), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return NAN;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return NAN;
    if (gmm_out) for (int j = 0; j < 3 * c->cfg.gmm_components; ++j) gmm_out[j] = c->h_st->gmm_out[j];
    return c->h_st->alpha;
}

int lo_build_normal_equations(lo_ctx* c, const float* pts, size_t n, const float T[12], double scale, double delta,
                              double H[36], double g[6], double* cost) {
    if (!c || !T || !H || !g || !cost || (n > 0 && !pts)) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    if (n == 0) { std::memset(H, 0, 36 * sizeof(double)); std::memset(g, 0, 6 * sizeof(double)); *cost = 0; return 0; }
    LO_HIP(c, hipSetDevice(c->device));
    int rc = reset_state(c, T, scale, delta);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipMemcpyAsync(c->d_pts, pts, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    KParams P = make_params(c, c->d_pts, static_cast<int>(n));
    P.alpha_given = 1;
    launch_correspond(c, P, 0, c->kd);
    if (P.nb_acc <= kFuseMaxBlocks) {
        hipLaunchKernelGGL(k_accumulate, dim3(P.nb_acc), dim3(kBlock), 0, c->stream, P, 0, 2);
    } else {
        hipLaunchKernelGGL(k_accumulate, dim3(P.nb_acc), dim3(kBlock), 0, c->stream, P, 0, 0);
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, c->stream, P, 0, 1);
    }
    LO_HIP(c, hipGetLastError());
    std::vector<int32_t> cnt(P.nb);
    LO_HIP(c, hipMemcpyAsync(cnt.data(), cur(c).d_blk_cnt, P.nb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipMemcpyAsync(c->h_st, cur(c).d_st, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < 36; ++q) H[q] = c->h_st->H_out[q];
    for (int j = 0; j < 6; ++j) g[j] = c->h_st->g_out[j];
    *cost = c->h_st->cost_out;
    int total = 0;
    for (int v : cnt) total += v;
    return total;
}

int lo_pko_sample_indices(lo_ctx* c, size_t n, int32_t* out) {
    if (!c || !out) return LO_ERR_ARG;
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    const int k = static_cast<int>(std::min<size_t>(n, static_cast<size_t>(c->cfg.gmm_sample_size)));
    for (int s = 0; s < k; ++s) out[s] = pko_sample_host(c->tables, static_cast<int>(n), s);
    return k;
}

// start stamps ~0, end stamps 0, in every launch's record (kStageEvents + 1 records)
static int reset_spans(lo_ctx* c) {
    const size_t words = static_cast<size_t>(kSpanWords) * (kStageEvents + 1);
    LO_HIP(c, c->d_span.reserve(words));
    std::vector<unsigned long long> h(words, 0ull);
    for (size_t r = 0; r < words; r += kSpanWords)
        for (int k = 0; k < kSpanStarts; ++k) h[r + k] = ~0ull;
    LO_HIP(c, hipMemcpyAsync(c->d_span, h.data(), h.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    return LO_OK;
}

// a launch's span record: the latest end stamp minus the earliest start stamp (0 if it did not run)
static unsigned long long span_of(const unsigned long long* r) {
    unsigned long long s = ~0ull, e = 0;
    for (int k = 0; k < kSpanStarts; ++k) s = std::min(s, r[k]);
    for (int k = 0; k < kSpanEnds; ++k) e = std::max(e, r[kSpanStarts + k]);
    return e > s ? e - s : 0ull;
}

int lo_set_stage_timing(lo_ctx* c, int enable) {
    if (!c) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (enable && c->st_ev.empty()) {
        c->st_ev.resize(2 * kStageEvents, nullptr);
        for (hipEvent_t& e : c->st_ev) LO_HIP(c, hipEventCreate(&e));
    }
    if (enable) {
        LO_HIP(c, hipSetDevice(c->device));
        const int rc = reset_spans(c);
        if (rc != LO_OK) return rc;
    }
    c->stage_timing = enable != 0;
    c->st_n = 0;
    return LO_OK;
}

int lo_stage_span(lo_ctx* c, double* avg_us, int* count) {
    if (!c || !avg_us) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    *avg_us = 0.0;
    if (count) *count = 0;
    if (!c->d_span || c->st_n == 0) return LO_OK;
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> h(static_cast<size_t>(kSpanWords) * c->st_n);
    LO_HIP(c, hipMemcpy(h.data(), c->d_span, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double tot = 0.0;
    int k = 0;
    for (int i = 0; i < c->st_n; ++i) {
        const unsigned long long d = span_of(h.data() + static_cast<size_t>(kSpanWords) * i);
        if (d) { tot += static_cast<double>(d); ++k; }
    }
    *avg_us = k ? tot / k * 0.01 : 0.0;                  // s_memrealtime: 100 MHz
    if (count) *count = k;
    return LO_OK;
}

int lo_stage_time(lo_ctx* c, double* avg_us, int* count) {
    if (!c || !avg_us) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    LO_HIP(c, hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (int i = 0; i < c->st_n; ++i) {
        float ms = 0.0f;
        LO_HIP(c, hipEventElapsedTime(&ms, c->st_ev[2 * i], c->st_ev[2 * i + 1]));
        tot += ms;
    }
    *avg_us = c->st_n > 0 ? tot * 1e3 / c->st_n : 0.0;
    if (count) *count = c->st_n;
    return LO_OK;
}

int lo_pko_em_stats(lo_ctx* c, unsigned long long out[3], int reset) {
    if (!c || !out) return LO_ERR_ARG;
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, sync_all(c));
    LO_HIP(c, hipMemcpy(out, reinterpret_cast<const char*>(cur(c).d_st.get()) + offsetof(DevState, em_stat),
                        3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset)
        LO_HIP(c, hipMemset(reinterpret_cast<char*>(cur(c).d_st.get()) + offsetof(DevState, em_stat), 0, 3 * sizeof(unsigned long long)));
    return LO_OK;
}

int lo_bench_kernel(lo_ctx* c, const float* d_pts, size_t n, const float T[12], double scale, double alpha,
                    int kernel_id, int reps, float* avg_ms) {
    if (!c || !d_pts || !T || !avg_ms || n == 0 || reps < 1 || kernel_id < 0 || kernel_id > 5) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (kernel_id == 5 && c->kd) { c->err = "kernel 5: surfel correspondence only"; return LO_ERR_STATE; }
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    LO_HIP(c, hipSetDevice(c->device));
    int rc = reset_state(c, T, scale, alpha);
    if (rc != LO_OK) return rc;
    if ((rc = ensure_acc_part(c)) != LO_OK) return rc;
    KParams P = make_params(c, d_pts, static_cast<int>(n));
    P.alpha_given = 1;
    const dim3 grid(P.nb), blk(kBlock);
    // set up the inputs every kernel reads: slots / block stats (k_correspond), alpha (k_pko), partials; kernel 4 (the
    // correspondence launch with NO setup pass: its inputs not pre-read into the caches) skips it
    if (kernel_id == 5) {                                // the launches' own span (P.span), not the events'
        rc = reset_spans(c);
        if (rc != LO_OK) return rc;
        P.span = c->d_span + static_cast<size_t>(kSpanWords) * kStageEvents;
    }
    if (kernel_id < 4) {
        launch_correspond(c, P, 1, c->kd);
        hipLaunchKernelGGL(k_accumulate, dim3(P.nb_acc), blk, 0, c->stream, P, 0, 0);
    }
    LO_HIP(c, hipGetLastError());
    LO_HIP(c, hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < reps; ++r) {
        switch (kernel_id) {
            case 0: case 4: case 5: launch_correspond(c, P, 0, c->kd); break;   // KDTree: kNN + fallback + plane fit
            case 1: hipLaunchKernelGGL(k_accumulate, dim3(P.nb_acc), blk, 0, c->stream, P, 0,
                                       P.nb_acc <= kFuseMaxBlocks ? 2 : 0); break;
            case 2: if (spec_ok(P)) launch_pko_spec(c, P, 1); else launch_pko(c, P, 1); break;
            default: hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, c->stream, P, 0, 1); break;
        }
    }
    LO_HIP(c, hipEventRecord(c->ev1, c->stream));
    LO_HIP(c, hipGetLastError());
    LO_HIP(c, hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    LO_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms = ms / reps;
    if (kernel_id == 5) {
        std::vector<unsigned long long> h(kSpanWords);
        LO_HIP(c, hipMemcpy(h.data(), c->d_span + static_cast<size_t>(kSpanWords) * kStageEvents,
                            kSpanWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const unsigned long long d = span_of(h.data());
        *avg_ms = d ? static_cast<float>(static_cast<double>(d) * 1e-5) : -1.0f;   // the last launch's span
    }
    return LO_OK;
}

int lo_bench_correspond_rr(lo_ctx* const* ctxs, const float* const* d_pts, const size_t* n, const float* T, int count,
                           int rounds, float* avg_ms) {
    if (!ctxs || !d_pts || !n || !T || !avg_ms || count < 1 || rounds < 1) return LO_ERR_ARG;
    lo_ctx* c0 = ctxs[0];
    if (!c0) return LO_ERR_ARG;
    std::vector<KParams> P(count);
    for (int i = 0; i < count; ++i) {
        lo_ctx* c = ctxs[i];
        if (!c || !d_pts[i] || n[i] == 0) return LO_ERR_ARG;
        if (flush_hold(c) != LO_OK) { c0->err = c->err; return LO_ERR_HIP; }
        if (c->kd || c->device != c0->device) { c0->err = "lo_bench_correspond_rr: surfel contexts on one device"; return LO_ERR_STATE; }
        if (n[i] > static_cast<size_t>(c->cfg.max_points)) { c0->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    }
    LO_HIP(c0, hipSetDevice(c0->device));
    for (int i = 0; i < count; ++i) {                       // every context's state on its own stream, then joined
        lo_ctx* c = ctxs[i];
        int rc = reset_state(c, T + 12 * i, 1.0, 0.1);
        if (rc == LO_OK) rc = ensure_acc_part(c);
        if (rc != LO_OK) { c0->err = c->err; return rc; }
        P[i] = make_params(c, d_pts[i], static_cast<int>(n[i]));
        LO_HIP(c0, hipStreamSynchronize(c->stream));
    }
    const hipStream_t s = c0->stream;
    LO_HIP(c0, hipEventRecord(c0->ev0, s));
    for (int r = 0; r < rounds; ++r)
        for (int i = 0; i < count; ++i) hipLaunchKernelGGL(k_correspond, dim3(P[i].nb), dim3(kBlock), 0, s, P[i], 0);
    LO_HIP(c0, hipEventRecord(c0->ev1, s));
    LO_HIP(c0, hipGetLastError());
    LO_HIP(c0, hipEventSynchronize(c0->ev1));
    float ms = 0.0f;
    LO_HIP(c0, hipEventElapsedTime(&ms, c0->ev0, c0->ev1));
    *avg_ms = ms / (static_cast<float>(rounds) * count);
    return LO_OK;
}

int lo_seq_sum_f64(lo_ctx* c, const double* x, size_t n, int sort, double* out_sum, long long stats[4]) {
    if (!c || !out_sum || (n > 0 && !x) || n > static_cast<size_t>(kExactMaxPoints)) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    LO_HIP(c, hipSetDevice(c->device));
    DevBuf<double> buf;
    static_assert(sizeof(long long) == sizeof(double), "the four stats words follow the doubles");
    LO_HIP(c, buf.reserve(2 * n + 1 + 4));
    double* d = buf;
    long long* d_st = reinterpret_cast<long long*>(d + 2 * n + 1);
    if (n > 0) LO_HIP(c, hipMemcpy(d, x, n * sizeof(double), hipMemcpyHostToDevice));
    launch_seq_sum_diag(d, static_cast<int>(n), sort ? d + n : nullptr, d + 2 * n, d_st, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    long long st[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(out_sum, d + 2 * n, sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(st, d_st, sizeof(st), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->err = std::string("lo_seq_sum_f64: ") + hipGetErrorString(e); return LO_ERR_HIP; }
    if (stats) for (int k = 0; k < 4; ++k) stats[k] = st[k];
    return LO_OK;
}

int lo_seq_sum_f32(lo_ctx* c, const float* x, size_t n, float* out_sum, long long stats[4]) {
    if (!c || !out_sum || (n > 0 && !x) || n > static_cast<size_t>(kMaxBlocks) * kBlock) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    LO_HIP(c, hipSetDevice(c->device));
    const int ni = static_cast<int>(n);
    const size_t x_bytes = (n * sizeof(float) + 255) / 256 * 256, mwb = mw_bytes(1, ni);
    DevBuf<char> buf;
    LO_HIP(c, buf.reserve(x_bytes + mwb + 256));
    char* d = buf;
    float* d_x = reinterpret_cast<float*>(d);
    const MwBuf B = mw_layout(d + x_bytes, 1, ni);
    float* d_out = reinterpret_cast<float*>(d + x_bytes + mwb);
    long long* d_st = reinterpret_cast<long long*>(d + x_bytes + mwb + 64);
    hipError_t e = hipSuccess;
    if (n > 0) e = hipMemcpy(d_x, x, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mw_clear(B, 1, c->stream);
    float ms = 0.0f;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) {
        (void)hipEventRecord(e0, c->stream);
        launch_mw_sums(d_x, ni, 1, ni, nullptr, nullptr, B, d_out, d_st, c->stream, false);
        (void)hipEventRecord(e1, c->stream);
        e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    long long st[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(out_sum, d_out, sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(st, d_st, sizeof(st), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->err = std::string("lo_seq_sum_f32: ") + hipGetErrorString(e); return LO_ERR_HIP; }
    if (stats) {
        for (int k = 0; k < 3; ++k) stats[k] = st[k];
        stats[3] = static_cast<long long>(ms * 1e3);      // microseconds of the three launches
    }
    return LO_OK;
}

int lo_exact_solve_both(lo_ctx* c, const float* totals, const float* poses, size_t n, double tol_t, double tol_r,
                        uint32_t* out_lane, uint32_t* out_wave) {
    if (!c || n == 0 || n > (1u << 20) || !totals || !poses || !out_lane || !out_wave) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    LO_HIP(c, hipSetDevice(c->device));
    const size_t tb = n * kExactTerms * sizeof(float), pb = n * 12 * sizeof(float), ob = n * kSolveWords * sizeof(uint32_t);
    DevBuf<char> buf;
    LO_HIP(c, buf.reserve(tb + pb + 2 * ob));
    char* d = buf;
    float* d_tot = reinterpret_cast<float*>(d);
    float* d_pose = reinterpret_cast<float*>(d + tb);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(d + tb + pb);
    hipError_t e = hipMemcpy(d_tot, totals, tb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_pose, poses, pb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_solve_both, dim3(static_cast<unsigned>(n)), dim3(kWave), 0, c->stream, d_tot, d_pose,
                           static_cast<int>(n), tol_t, tol_r, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out_lane, d_out, ob, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_wave, d_out + n * kSolveWords, ob, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->err = std::string("lo_exact_solve_both: ") + hipGetErrorString(e); return LO_ERR_HIP; }
    return LO_OK;
}

int lo_debug_cand_records(lo_ctx* c, float* out, size_t cap_words) {
    if (!c || !out) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    const size_t cand = static_cast<size_t>(c->cfg.num_alpha_segments) + 1, words = cand * kCandWords;
    if (!cur(c).d_acc_part || cur(c).d_cand_rec.capacity() < words) { c->err = "lo_debug_cand_records: no records yet"; return LO_ERR_STATE; }
    if (cap_words < words) { c->err = "lo_debug_cand_records: output too small"; return LO_ERR_CAPACITY; }
    LO_HIP(c, sync_all(c));
    LO_HIP(c, hipMemcpy(out, cur(c).d_cand_rec, words * sizeof(float), hipMemcpyDeviceToHost));
    return static_cast<int>(cand);
}

// The 16-float record (as lo_icp_export_pose) of the scan on the OTHER lane: the scan queued before the last one, whose
// tail ran beside the last scan's head (scan overlap) -- whichever lane of the ring that was.  Drains every stream first.
int lo_debug_other_lane_record(lo_ctx* c, float out16[16]) {
    if (!c || !out16) return LO_ERR_ARG;
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, sync_all(c));
    // (two grouped scans: the one before the last has its own set of per-scan state in the group's slot)
    const ScanLane* other = (c->q.grp.cur && c->q.grp.prev) ? c->q.grp.prev
                            : c->q.prev_lane >= 0 ? &c->q.lanes[c->q.prev_lane] : nullptr;
    if (!other || !other->d_st) {
        c->err = "lo_debug_other_lane_record: no scan has overlapped yet";
        return LO_ERR_STATE;
    }
    std::vector<char> h(offsetof(DevState, logs));
    LO_HIP(c, hipMemcpy(h.data(), other->d_st.get(), h.size(), hipMemcpyDeviceToHost));
    const DevState* st = reinterpret_cast<const DevState*>(h.data());   // (header fields only)
    for (int k = 0; k < 12; ++k) out16[k] = st->pose[k];
    out16[12] = static_cast<float>(st->status);
    out16[13] = static_cast<float>(st->iter);
    out16[14] = static_cast<float>(st->n_corr);
    out16[15] = 0.0f;
    return LO_OK;
}

int lo_debug_counters(lo_ctx* c, unsigned long long out[16]) {
    if (!c || !out) return LO_ERR_ARG;
    LO_HIP(c, sync_all(c));
    const DevState* st = cur(c).d_st;
    LO_HIP(c, hipMemcpy(out, reinterpret_cast<const char*>(st) + offsetof(DevState, dbg), 16 * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost));
    return LO_OK;
}

static int debug_grid(lo_ctx* c, const PointGrid& G, float* h, int org[3], int dim[3], int* m, uint32_t* start,
                      size_t start_cap, float* pts4, size_t pts_cap) {
    LO_HIP(c, sync_all(c));
    LO_HIP(c, hipDeviceSynchronize());                   // a batch stream may have built the grid
    if (h) *h = G.h;
    for (int a = 0; a < 3; ++a) {
        if (org) org[a] = G.org[a];
        if (dim) dim[a] = G.dim[a];
    }
    if (m) *m = G.m;
    const size_t ncell = G.all ? 0 : static_cast<size_t>(G.dim[0]) * G.dim[1] * G.dim[2];
    const size_t ns = G.all ? 0 : ncell + 1, np = static_cast<size_t>(std::max(G.m, 0));
    if ((start && start_cap < ns) || (pts4 && pts_cap < np)) { c->err = "lo_debug_grid: output too small"; return LO_ERR_CAPACITY; }
    if (start && ns > 0) {
        if (G.d_start.capacity() < ns) { c->err = "lo_debug_grid: no grid yet"; return LO_ERR_STATE; }
        LO_HIP(c, hipMemcpy(start, G.d_start, ns * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (pts4 && np > 0) {
        if (G.d_pts.capacity() < np) { c->err = "lo_debug_grid: no grid yet"; return LO_ERR_STATE; }
        LO_HIP(c, hipMemcpy(pts4, G.d_pts, np * sizeof(float4), hipMemcpyDeviceToHost));
    }
    return LO_OK;
}
int lo_debug_grid(lo_ctx* c, float* h, int org[3], int dim[3], int* m, uint32_t* start, size_t start_cap, float* pts4,
                  size_t pts_cap) {
    if (!c) return LO_ERR_ARG;
    if (!c->kd) { c->err = "lo_debug_grid needs use_surfel_correspondence = 0"; return LO_ERR_STATE; }
    return debug_grid(c, c->grid, h, org, dim, m, start, start_cap, pts4, pts_cap);
}
int lo_debug_loop_grid(lo_ctx* c, float* h, int org[3], int dim[3], int* m, uint32_t* start, size_t start_cap,
                       float* pts4, size_t pts_cap) {
    if (!c) return LO_ERR_ARG;
    return debug_grid(c, c->lgrid, h, org, dim, m, start, start_cap, pts4, pts_cap);
}

int lo_debug_counters_ex(lo_ctx* c, unsigned long long* out, int n) {
    if (!c || !out || n < 1 || n > 24) return LO_ERR_ARG;
    LO_HIP(c, sync_all(c));
    LO_HIP(c, hipMemcpy(out, reinterpret_cast<const char*>(cur(c).d_st.get()) + offsetof(DevState, dbg),
                        static_cast<size_t>(n) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return LO_OK;
}

int lo_pko_sample_indices_host(size_t n, int sample_size, int32_t* out) {
    if (!out || sample_size < 1 || sample_size > kMaxS || n > static_cast<size_t>(kMaxBlocks) * kBlock) return LO_ERR_ARG;
    PkoTables t;
    build_pko_tables(t, sample_size, 1, static_cast<int>(std::max<size_t>(n, 1)), 0.1, 10.0, 1, 10.0, false);
    const int k = static_cast<int>(std::min<size_t>(n, static_cast<size_t>(sample_size)));
    for (int s = 0; s < k; ++s) out[s] = pko_sample_host(t, static_cast<int>(n), s);
    return k;
}

}  // extern "C"
