// lo_exact.h — the reference's own fp32 operation order for one GN step (reference-exact mode, lo_set_exact):
// the per-correspondence Jacobian / weight / residual terms of build_ne (IterativeClosestPointOptimizer.cpp:345-410),
// Eigen's fp32 LDLT (:418) and the SO3::Exp / SO3(Matrix3f) re-projected right-update (:420-448, MathUtils.cpp:23-39,
// :86-99), restated as the oracle states them (oracle/src/lo_oracle.cpp build_ne / ldlt6_solve / so3_exp / se3_mul).
// Shared by the sequential-sum solve (lo_exact.hip k_exact_solve) and the speculative exact candidates of the PKO
// launch (lo_pko_body.h acc_candidate_exact).
#pragma once
#include <cfloat>

#include "lo_device.h"
#include "lo_math.h"

namespace lo {

constexpr int kExactTerms = 43;        // H (36, full: the reference's H is not symmetrised), g (6), cost
constexpr int kExactFactors = 14;      // per point: J (6), w J (6), w r, r (exact_point_factors); the long sums
                                       //   (term-major) store these rows and the column sums form each term

// ---- the reference's fp32 solve and pose update (restated exactly as the oracle states them) ----
// LDLT<Matrix<float,6,6>> (Eigen ldlt_inplace<Lower>::unblocked with diagonal pivoting + LDLT::_solve_impl)
__device__ inline void ldlt6_solve_f32(const float (&Hin)[36], const float (&b)[6], float (&x)[6]) {
    float m[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) m[r][c] = Hin[r * 6 + c];
    int transp[6];
    float temp[6];
    bool zero_all = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int big = k;
        float bv = fabsf(m[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) if (fabsf(m[i][i]) > bv) { bv = fabsf(m[i][i]); big = i; }
        transp[k] = big;
        // the symmetric pivot swap with compile-time indices only (one unrolled candidate per row): a runtime index
        // into m would put the matrix in scratch memory
#pragma unroll
        for (int q = k + 1; q < 6; ++q) {
            if (q != big) continue;
#pragma unroll
            for (int j = 0; j < k; ++j) { const float t = m[k][j]; m[k][j] = m[q][j]; m[q][j] = t; }
#pragma unroll
            for (int i = q + 1; i < 6; ++i) { const float t = m[i][k]; m[i][k] = m[i][q]; m[i][q] = t; }
            { const float t = m[k][k]; m[k][k] = m[q][q]; m[q][q] = t; }
#pragma unroll
            for (int i = k + 1; i < q; ++i) { const float t = m[i][k]; m[i][k] = m[q][i]; m[q][i] = t; }
        }
        if (k > 0) {
#pragma unroll
            for (int j = 0; j < k; ++j) temp[j] = m[j][j] * m[k][j];
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < k; ++j) acc += m[k][j] * temp[j];
            m[k][k] -= acc;
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                float a = 0.0f;
#pragma unroll
                for (int j = 0; j < k; ++j) a += m[i][j] * temp[j];
                m[i][k] -= a;
            }
        }
        const float akk = m[k][k];
        const bool valid = fabsf(akk) > 0.0f;
        if (k == 0 && !valid) { zero_all = true; break; }
        if (k < 5 && valid) for (int i = k + 1; i < 6; ++i) m[i][k] /= akk;
    }
    if (zero_all) { for (int i = 0; i < 6; ++i) x[i] = 0.0f; return; }
    float d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = b[i];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q) if (transp[k] == q) { const float t = d[k]; d[k] = d[q]; d[q] = t; }
#pragma unroll
    for (int i = 0; i < 6; ++i) { float a = 0.0f; for (int j = 0; j < i; ++j) a += m[i][j] * d[j]; d[i] -= a; }
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = (fabsf(m[i][i]) > FLT_MIN) ? d[i] / m[i][i] : 0.0f;
#pragma unroll
    for (int i = 5; i >= 0; --i) { float a = 0.0f; for (int j = i + 1; j < 6; ++j) a += m[j][i] * d[j]; d[i] -= a; }
#pragma unroll
    for (int k = 5; k >= 0; --k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q) if (transp[k] == q) { const float t = d[k]; d[k] = d[q]; d[q] = t; }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = d[i];
}

__device__ inline float norm3e(const float* v) { return sqrtf(dot3e(v[0], v[1], v[2], v[0], v[1], v[2])); }

// SO3::Exp (MathUtils.cpp:23-39, kEps 1e-6f) with the SO3(Matrix3f) re-projection of its result; sin / cos are
// glibc's sinf / cosf restated (lo_math.h sincosf_ref: bit-identical to the reference's std::sin / std::cos of a
// float; r05 rounded the fp64 sin / cos instead, which differs from sinf in the last bit for 0.4 % of the floats in
// [1e-7, 0.8], and its device sin / cos took ~4.5k cycles of the solve's ~21k)
__device__ inline void so3_exp_exact(const float w[3], float R[3][3]) {
    const float theta = norm3e(w);
    float M[3][3];
    if (theta < 1e-6f) {
        const float H[3][3] = {{0.0f, -w[2], w[1]}, {w[2], 0.0f, -w[0]}, {-w[1], w[0], 0.0f}};
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = (r == c ? 1.0f : 0.0f) + H[r][c];
    } else {
        const float ti = 1.0f / theta;
        const float k[3] = {w[0] * ti, w[1] * ti, w[2] * ti};
        const float K[3][3] = {{0.0f, -k[2], k[1]}, {k[2], 0.0f, -k[0]}, {-k[1], k[0], 0.0f}};
        const float s = sincosf_ref(theta, 0);
        const float omc = 1.0f - sincosf_ref(theta, 1);
        float sK[3][3], KK[3][3];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) sK[r][c] = omc * K[r][c];
        mul33e(sK, K, KK);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = ((r == c ? 1.0f : 0.0f) + s * K[r][c]) + KK[r][c];
    }
    so3_project_svd(M, R);
}

// One correspondence's factors of the 43 terms (:364-404): J (6), w J (6), w r, r -- the terms themselves are
// H[row][col] = J[col] * (w J[row]), g[j] = (w r) * J[j], cost = (w r) * r, each one fp32 product.
__device__ __forceinline__ void exact_point_factors(const KParams& P, const float (&T)[12], double scale, float dl,
                                                    double r64, float px, float py, float pz, const Slot& sl,
                                                    float (&f)[14]) {
    const float nres = static_cast<float>(r64 / std_max(scale, 1e-6));
    const float qx = dot3f(T[0], T[1], T[2], px, py, pz) + T[3];
    const float qy = dot3f(T[4], T[5], T[6], px, py, pz) + T[7];
    const float qz = dot3f(T[8], T[9], T[10], px, py, pz) + T[11];
    const float n0 = sl.n[0], n1 = sl.n[1], n2 = sl.n[2];
    const float res = dot3f(n0, n1, n2, qx - sl.c[0], qy - sl.c[1], qz - sl.c[2]);
    float J[6];
    J[0] = dot3f(n0, n1, n2, T[0], T[4], T[8]);
    J[1] = dot3f(n0, n1, n2, T[1], T[5], T[9]);
    J[2] = dot3f(n0, n1, n2, T[2], T[6], T[10]);
    const float a0 = dot3f(-n0, -n1, -n2, T[0], T[4], T[8]);
    const float a1 = dot3f(-n0, -n1, -n2, T[1], T[5], T[9]);
    const float a2 = dot3f(-n0, -n1, -n2, T[2], T[6], T[10]);
    J[3] = dot3f(a0, a1, a2, 0.0f, pz, -py);
    J[4] = dot3f(a0, a1, a2, -pz, 0.0f, px);
    J[5] = dot3f(a0, a1, a2, py, -px, 0.0f);
    float w = 1.0f;
    if (P.robust) {
        const float an = fabsf(nres);
        if (P.cauchy_loss) { const float ratio = an / dl; w = 1.0f / (1.0f + ratio * ratio); }
        else if (an > dl) w = dl / an;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) { f[j] = J[j]; f[6 + j] = w * J[j]; }
    f[12] = w * res;
    f[13] = res;
}
// Term k of the 43 (row-major H, then g, then cost) as the product of factors fa[k] * fb[k].
__device__ __forceinline__ void exact_term_factors(int k, int& fa, int& fb) {
    if (k < 36) { fa = k % 6; fb = 6 + k / 6; }          // J[col] * wJ[row]
    else if (k < 42) { fa = 12; fb = k - 36; }           // wr * J[j]
    else { fa = 12; fb = 13; }                           // wr * r
}

// The reference's solve and right-update from the 43 sums (:417-448): pn = the new pose, delta, convergence.
__device__ inline bool exact_solve_step(const float (&tot)[kExactTerms], const float pose[12], double tol_t, double tol_r,
                                        float (&pn)[12], float (&delta)[6]) {
    float Hf[36], mg[6];
    for (int k = 0; k < 36; ++k) Hf[k] = tot[k];
    for (int j = 0; j < 6; ++j) mg[j] = -tot[36 + j];
    ldlt6_solve_f32(Hf, mg, delta);                            // :418
    const float dt[3] = {delta[0], delta[1], delta[2]}, dw[3] = {delta[3], delta[4], delta[5]};
    float Rd[3][3];
    if (norm3e(dw) < 1e-10f) {                                 // :427-431
        const float I[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
        so3_project_svd(I, Rd);
    } else {
        so3_exp_exact(dw, Rd);
    }
    float R[3][3], t[3], M[3][3], Rn[3][3];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[r][c] = pose[r * 4 + c]; t[r] = pose[r * 4 + 3]; }
    mul33e(R, Rd, M);                                           // SE3::operator* (MathUtils.h:144-147)
    so3_project_svd(M, Rn);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) pn[r * 4 + c] = Rn[r][c];
        pn[r * 4 + 3] = t[r] + dot3e(R[r][0], R[r][1], R[r][2], dt[0], dt[1], dt[2]);
    }
    return norm3e(dt) < tol_t && norm3e(dw) < tol_r;          // :443-448
}

// ---- the same solve across one wave (exact_solve_step_wave) ----
// Every fp32 operation of exact_solve_step keeps its operands, type and order; operations that do not depend on each
// other run on different lanes of one full wave (all 64 lanes call in).  What the lanes share is wave-uniform: values
// read with v_readlane from a compile-time lane, and branches on them.  The dependent scalars (pivots, the Jacobi
// rotation's divides and square roots, sin / cos) are computed once, by every lane alike, through the one-lane
// form's own functions.
__device__ __forceinline__ float wv_get(float v, int l) {            // lane l's v (l wave-uniform), as a uniform value
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// DPP row shifts within a 16-lane row: lane i reads lane i + N (wv_up) or i - N (wv_dn); lanes outside the row read 0
template <int N> __device__ __forceinline__ float wv_up(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 | N, 0xf, 0xf, true));
}
template <int N> __device__ __forceinline__ float wv_dn(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 | N, 0xf, 0xf, true));
}

// ldlt6_solve_f32 with one row per lane.  Lane i < 6 holds row i in six registers (lanes >= 6 repeat row 5 and are
// never read).  Only the lower triangle of H is ever used; the not yet factored part is kept mirrored into the upper
// triangle, so the symmetric pivot swap is a row exchange between two lanes plus a column exchange between two
// registers, all with compile-time indices.  Step k's row updates and divisions then run once for all rows; the
// substitutions run on uniform values in the one-lane form's order.
__device__ inline void ldlt6_solve_wave(const float* tot, int lane, float (&x)[6]) {
    const int i = lane < 6 ? lane : 5;
    float m[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) m[c] = tot[c <= i ? i * 6 + c : c * 6 + i];
    float dd[6];                                             // m[k][k] once step k is done (uniform)
    int transp[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float dg = m[0];                                     // this row's diagonal element
#pragma unroll
        for (int c = 1; c < 6; ++c) dg = (i == c) ? m[c] : dg;
        int big = k;
        float bv = fabsf(wv_get(dg, k));
#pragma unroll
        for (int q = k + 1; q < 6; ++q) { const float v = fabsf(wv_get(dg, q)); if (v > bv) { bv = v; big = q; } }
        transp[k] = big;
#pragma unroll
        for (int q = k + 1; q < 6; ++q) {
            if (q != big) continue;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const float rk = wv_get(m[c], k), rq = wv_get(m[c], q);
                m[c] = (i == k) ? rq : ((i == q) ? rk : m[c]);
            }
            const float t = m[k]; m[k] = m[q]; m[q] = t;
        }
        if (k > 0) {
            float temp[6];
#pragma unroll
            for (int j = 0; j < k; ++j) temp[j] = dd[j] * wv_get(m[j], k);
            float a = 0.0f;                                  // row k: m[k][k] -= acc; rows i > k: m[i][k] -= a
#pragma unroll
            for (int j = 0; j < k; ++j) a += m[j] * temp[j];
            m[k] -= a;
        }
        const float akk = wv_get(m[k], k);
        dd[k] = akk;
        const bool valid = fabsf(akk) > 0.0f;
        if (k == 0 && !valid) {
#pragma unroll
            for (int j = 0; j < 6; ++j) x[j] = 0.0f;
            return;
        }
        if (k < 5 && valid) { const float qv = m[k] / akk; m[k] = (i > k) ? qv : m[k]; }
    }
    float L[6][6];                                           // the factor's strict lower triangle, uniform
#pragma unroll
    for (int r = 1; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < r; ++c) L[r][c] = wv_get(m[c], r);
    float d[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) d[j] = -tot[36 + j];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q) if (transp[k] == q) { const float t = d[k]; d[k] = d[q]; d[q] = t; }
#pragma unroll
    for (int r = 0; r < 6; ++r) { float a = 0.0f; for (int j = 0; j < r; ++j) a += L[r][j] * d[j]; d[r] -= a; }
#pragma unroll
    for (int r = 0; r < 6; ++r) d[r] = (fabsf(dd[r]) > FLT_MIN) ? d[r] / dd[r] : 0.0f;
#pragma unroll
    for (int r = 5; r >= 0; --r) { float a = 0.0f; for (int j = r + 1; j < 6; ++j) a += L[j][r] * d[j]; d[r] -= a; }
#pragma unroll
    for (int k = 5; k >= 0; --k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q) if (transp[k] == q) { const float t = d[k]; d[k] = d[q]; d[q] = t; }
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = d[j];
}

// Element (r, c) of a uniform 3x3 for this lane (r, c < 3)
__device__ __forceinline__ float wv_pick3(int k, float a0, float a1, float a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// One Jacobi rotation of columns P, Q (P > Q) of the matrices held one element per lane (lane 3 r + c of each 16-lane
// row): rotate(M[i][P], M[i][Q], rot) for all three rows i at once
template <int P, int Q>
__device__ __forceinline__ float wv_rot_cols(float X, int c, float rc, float rs) {
    const float lf = wv_dn<P - Q>(X), rt = wv_up<P - Q>(X);
    const bool isP = c == P;
    const float xv = isP ? X : rt, yv = isP ? lf : X;
    const float c1 = isP ? rc : -rs, c2 = isP ? rs : rc;
    return c1 * xv + c2 * yv;
}
// ... and of rows P, Q: rotate(M[P][i], M[Q][i], rot) for all three columns i at once
template <int P, int Q>
__device__ __forceinline__ float wv_rot_rows(float X, int r, float rc, float rs) {
    const float lf = wv_dn<3 * (P - Q)>(X), rt = wv_up<3 * (P - Q)>(X);
    const bool isP = r == P;
    const float xv = isP ? X : rt, yv = isP ? lf : X;
    const float c1 = isP ? rc : -rs, c2 = isP ? rs : rc;
    return c1 * xv + c2 * yv;
}

// One (p, q) step of jacobi_svd3's sweep on X: U in lanes 0-8, V in lanes 16-24, W in lanes 32-40.  The 2x2 SVD and
// make_jacobi are the one-lane form's, on uniform values; the four row / column updates are two lane-parallel ones.
template <int P, int Q>
__device__ __forceinline__ void wv_jacobi_step(float& X, int grp, int r, int c, float& maxDiag, bool& done) {
    const float prec = 2.0f * FLT_EPSILON;
    const float thr = std::max(FLT_MIN, prec * maxDiag);
    const float wpq = wv_get(X, 32 + 3 * P + Q), wqp = wv_get(X, 32 + 3 * Q + P);
    if (!(std::fabs(wpq) > thr || std::fabs(wqp) > thr)) return;
    done = false;
    float m00 = wv_get(X, 32 + 4 * P), m01 = wpq, m10 = wqp, m11 = wv_get(X, 32 + 4 * Q);
    Rot r1;
    const float t = m00 + m11, d = m10 - m01;
    if (std::fabs(d) < FLT_MIN) r1 = {1.0f, 0.0f};
    else {
        const float u = t / d;
        const float tmp = std::sqrt(1.0f + u * u);
        r1 = {u / tmp, 1.0f / tmp};
    }
    rotate(m00, m10, r1);
    rotate(m01, m11, r1);
    const Rot jr = make_jacobi(m00, m01, m11);
    const Rot jl = rot_mul(r1, rot_t(jr));
    const Rot jrt = rot_t(jr);
    const float wl = wv_rot_rows<P, Q>(X, r, jl.c, jl.s);             // W.applyOnTheLeft(p,q,jl)
    X = (grp == 2 && (r == P || r == Q)) ? wl : X;
    const float xr = wv_rot_cols<P, Q>(X, c, grp == 0 ? jl.c : jrt.c, grp == 0 ? jl.s : jrt.s);
    X = (grp < 3 && (c == P || c == Q)) ? xr : X;                     // U (jl), V and W (jr^T) on the right
    maxDiag = std::max(maxDiag, std::max(std::fabs(wv_get(X, 32 + 4 * P)), std::fabs(wv_get(X, 32 + 4 * Q))));
}

// Columns I < K of U and V exchanged (the descending sort's swap)
template <int I, int K>
__device__ __forceinline__ float wv_swap_cols(float X, int grp, int c) {
    const float fromK = wv_up<K - I>(X), fromI = wv_dn<K - I>(X);
    const float v = (c == I) ? fromK : ((c == K) ? fromI : X);
    return grp < 2 ? v : X;
}

// so3_project_svd with the matrix one element per lane: a = M[r][c] in lane 3 r + c of every 16-lane row (r = c = 3
// marks the idle lanes 9-15 of a row); returns R[r][c] in the same lanes.
__device__ inline float so3_project_svd_wave(float a, int lane) {
    const int grp = lane >> 4, e = lane & 15;
    const int r = e < 9 ? e / 3 : 3, c = e < 9 ? e % 3 : 3;
    float scale = 0.0f;                                               // maxCoeff<PropagateNaN>, row-major
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float v = std::fabs(wv_get(a, k));
        scale = (std::isnan(v) || std::isnan(scale)) ? NAN : std::max(scale, v);
    }
    float X = (e < 9 && r == c) ? 1.0f : 0.0f;                        // U = V = I (W below)
    if (std::isfinite(scale)) {
        if (scale == 0.0f) scale = 1.0f;
        const float w0 = a / scale;
        X = grp == 2 ? w0 : X;
        float maxDiag = std::max(std::fabs(wv_get(X, 32)), std::max(std::fabs(wv_get(X, 36)), std::fabs(wv_get(X, 40))));
        bool done = false;
        for (int sweep = 0; !done && sweep < 1000; ++sweep) {
            done = true;
            wv_jacobi_step<1, 0>(X, grp, r, c, maxDiag, done);
            wv_jacobi_step<2, 0>(X, grp, r, c, maxDiag, done);
            wv_jacobi_step<2, 1>(X, grp, r, c, maxDiag, done);
        }
        float S[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float wd = wv_get(X, 32 + 4 * k);
            S[k] = std::fabs(wd);
            if (wd < 0.0f) X = (grp == 0 && c == k) ? -X : X;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) S[k] *= scale;
        // descending sort (first max), as jacobi_svd3's: positions 0 and 1, then nothing is left to move
        {
            int pos = 0;
            if (S[1] > S[pos]) pos = 1;
            if (S[2] > S[pos]) pos = 2;
            const float sp = pos == 0 ? S[0] : (pos == 1 ? S[1] : S[2]);
            if (sp != 0.0f) {
                if (pos == 1) { const float tq = S[0]; S[0] = S[1]; S[1] = tq; X = wv_swap_cols<0, 1>(X, grp, c); }
                if (pos == 2) { const float tq = S[0]; S[0] = S[2]; S[2] = tq; X = wv_swap_cols<0, 2>(X, grp, c); }
                if (S[2] > S[1] && S[2] != 0.0f) X = wv_swap_cols<1, 2>(X, grp, c);
            }
        }
    }
    // R = U V^T: R[r][c] = dot3e(U[r][0..2], V[c][0..2]); U.col(2) negated when det < 0
    float U[3][3], V[3][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) { U[k / 3][k % 3] = wv_get(X, k); V[k / 3][k % 3] = wv_get(X, 16 + k); }
    float vr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vr[k] = wv_pick3(c, V[0][k], V[1][k], V[2][k]);
    float ur[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ur[k] = wv_pick3(r, U[0][k], U[1][k], U[2][k]);
    float R = dot3e(ur[0], ur[1], ur[2], vr[0], vr[1], vr[2]);
    float Rm[3][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm[k / 3][k % 3] = wv_get(R, k);
    if (det3e(Rm) < 0.0f) {
        ur[2] *= -1.0f;
        R = dot3e(ur[0], ur[1], ur[2], vr[0], vr[1], vr[2]);
    }
    return R;
}

// exact_solve_step across one wave: tot = the 43 totals (LDS or global memory), read by every lane of a full wave;
// pn, delta and the return value are wave-uniform and equal exact_solve_step's bit for bit.
// Precondition: called by all 64 lanes of one wave together (lane = the lane's index, under wave-uniform control
// flow): the lanes read each other with v_readlane from fixed lanes and with DPP row shifts, so a lane that is masked
// off gives its readers undefined values.
__device__ inline bool exact_solve_step_wave(const float* tot, const float pose[12], double tol_t, double tol_r,
                                             int lane, float (&pn)[12], float (&delta)[6]) {
    static_assert(kWave == 64, "the lane layouts (rows of 16 lanes for U, V, W; readlane from lanes 0-40) assume wave64");
    ldlt6_solve_wave(tot, lane, delta);                        // :418
    const float dt[3] = {delta[0], delta[1], delta[2]}, dw[3] = {delta[3], delta[4], delta[5]};
    const int e = lane & 15;
    const int r = e < 9 ? e / 3 : 3, c = e < 9 ? e % 3 : 3;
    const bool diag = e < 9 && r == c;
    float me;                                                  // this lane's element of the matrix to project
    if (norm3e(dw) < 1e-10f) {                                 // :427-431
        me = diag ? 1.0f : 0.0f;
    } else {                                                   // so3_exp_exact
        const float theta = norm3e(dw);
        if (theta < 1e-6f) {
            const float H[3][3] = {{0.0f, -dw[2], dw[1]}, {dw[2], 0.0f, -dw[0]}, {-dw[1], dw[0], 0.0f}};
            const float h = wv_pick3(r, wv_pick3(c, H[0][0], H[0][1], H[0][2]), wv_pick3(c, H[1][0], H[1][1], H[1][2]),
                                     wv_pick3(c, H[2][0], H[2][1], H[2][2]));
            me = (diag ? 1.0f : 0.0f) + h;
        } else {
            const float ti = 1.0f / theta;
            const float k[3] = {dw[0] * ti, dw[1] * ti, dw[2] * ti};
            const float K[3][3] = {{0.0f, -k[2], k[1]}, {k[2], 0.0f, -k[0]}, {-k[1], k[0], 0.0f}};
            const float s = sincosf_ref(theta, 0);
            const float omc = 1.0f - sincosf_ref(theta, 1);
            // sK row r, K column c, K[r][c] for this lane
            const float kr[3] = {wv_pick3(r, K[0][0], K[1][0], K[2][0]), wv_pick3(r, K[0][1], K[1][1], K[2][1]),
                                 wv_pick3(r, K[0][2], K[1][2], K[2][2])};
            const float kc[3] = {wv_pick3(c, K[0][0], K[0][1], K[0][2]), wv_pick3(c, K[1][0], K[1][1], K[1][2]),
                                 wv_pick3(c, K[2][0], K[2][1], K[2][2])};
            const float krc = wv_pick3(c, kr[0], kr[1], kr[2]);
            const float kk = dot3e(omc * kr[0], omc * kr[1], omc * kr[2], kc[0], kc[1], kc[2]);
            me = ((diag ? 1.0f : 0.0f) + s * krc) + kk;
        }
    }
    const float rd = so3_project_svd_wave(me, lane);
    float Rd[3][3], R[3][3], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rd[k / 3][k % 3] = wv_get(rd, k);
#pragma unroll
    for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) R[a][b] = pose[a * 4 + b]; t[a] = pose[a * 4 + 3]; }
    // SE3::operator* (MathUtils.h:144-147): this lane's element of R Rd
    const float m2 = dot3e(wv_pick3(r, R[0][0], R[1][0], R[2][0]), wv_pick3(r, R[0][1], R[1][1], R[2][1]),
                           wv_pick3(r, R[0][2], R[1][2], R[2][2]), wv_pick3(c, Rd[0][0], Rd[0][1], Rd[0][2]),
                           wv_pick3(c, Rd[1][0], Rd[1][1], Rd[1][2]), wv_pick3(c, Rd[2][0], Rd[2][1], Rd[2][2]));
    const float rn = so3_project_svd_wave(m2, lane);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) pn[a * 4 + b] = wv_get(rn, a * 3 + b);
        pn[a * 4 + 3] = t[a] + dot3e(R[a][0], R[a][1], R[a][2], dt[0], dt[1], dt[2]);
    }
    return norm3e(dt) < tol_t && norm3e(dw) < tol_r;          // :443-448
}

}  // namespace lo
