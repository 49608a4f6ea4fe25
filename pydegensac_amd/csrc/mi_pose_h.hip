/* libmi_degensac.so — relative pose from a homography on exported correspondence lists (include/mi_degensac.h
 * mi_degensac_pose_h_lists*): per entry of a compact list (pts [cap, 4] and corr_offsets [K + 1] as the correspondence export writes
 * them, both on the device) the calibrated homography G = K2^-1 H K1 of its H under two pinhole cameras, its four (R, t / d, n)
 * solutions of G = R + (t / d) n^T, or the rotation alone when G is one, the rows each candidate triangulates in front of both cameras
 * and on the visible side of its plane, the candidate with the most of them, and per row of that candidate the midpoint, the two depths
 * and the parallax.  The sibling of mi_pose.hip for the pairs on which F is degenerate (a plane, a pure rotation).  gfx950 only, no CPU
 * path.
 *
 * One workgroup of 256 threads per entry, further entries by a grid stride; no workgroup waits for another, no atomics.  The kernel reads
 * its row range o[p], o[p + 1] itself, so the host never learns a length and the call has no synchronisation.
 *   decomposition  thread 0: G, its singular value decomposition by six sweeps of one-sided Jacobi rotations (the rule of mi_pose.hip),
 *                  the four candidates, their normals and their camera-2 centres into LDS; about a thousand flops, once per entry.
 *   counting pass  PH_STEP = 1024 rows per step, four per thread, 256 consecutive 32-byte rows per load instruction of the workgroup; both
 *                  rotations, the four centres, both normals and the eight camera numbers in registers; per load and candidate one wave
 *                  ballot whose popcount is added to a wave-uniform register; the waves' sums meet in 4 x 5 LDS words after the last step.
 *   output pass    the same steps under the chosen candidate only: front, X, depth, cosang of the used rows, the wide count likewise.
 *   rotation       an entry whose G is a rotation has one candidate and one pass: used and front rows counted, front and cosang written.
 * Integer counts only cross threads, so every output is the same bits on every call. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_host.h"
#include "mi_dev_util.h"

#define PH_T     256                      /* threads per workgroup */
#define PH_NW    (PH_T / 64)
#define PH_LOADS 4                        /* rows per thread and step */
#define PH_STEP  (PH_LOADS * PH_T)        /* rows per workgroup and step */
#define PH_GRID  256                      /* cap on the grid: further entries by the grid stride */
#define PH_SWEEPS 6                       /* one-sided Jacobi sweeps of the 3 x 3 decomposition */

struct ph_args {
    const double *pts;            /* [cap, 4] */
    const int64_t *off;           /* [K + 1] */
    const uint8_t *keep;          /* [cap] or null */
    const double *H;              /* [K * 9] */
    const double *cams;           /* [n_cams, 4] */
    const int32_t *cam_idx;       /* [K, 2] or null */
    double *pose;                 /* [K, 12] */
    uint8_t *front;               /* [cap] */
    int32_t *info;                /* [K, 5] */
    double *normal, *tod;         /* [K, 3], [K] */
    double *X, *depth, *cosang;   /* [cap, 3], [cap, 2], [cap] or null */
    double *cand, *cand_normal;   /* [K, 4, 12], [K, 4, 3] or null */
    int32_t *cand_front;          /* [K, 4] or null */
    int K, n_cams; int64_t cap;
    double cos_min, rot_eps;
};

struct ph_shared {
    double cand[4][12];           /* R row-major, t */
    double nrm[4][3];             /* the plane normal in the frame of camera 1 */
    double tod[4];                /* |t / d| */
    double c2[4][3];              /* -R^T t */
    double cam[8];                /* fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2 */
    int status;
    int cnt[PH_NW][5];
};

__device__ __forceinline__ double ph_det(const double *R)
{
    return (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

/* the candidates of H under the two cameras of S->cam into S->cand / nrm / tod / c2 (one thread); returns the status (OK: four
 * candidates; ROTATION: candidate 0 is (R, 0), the rest zeros; anything else: all zeros) */
__device__ __forceinline__ int ph_decompose(ph_shared *S, const double *H, double rot_eps)
{
    const double fx1 = S->cam[0], fy1 = S->cam[1], cx1 = S->cam[2], cy1 = S->cam[3], fx2 = S->cam[4], fy2 = S->cam[5], cx2 = S->cam[6], cy2 = S->cam[7];
    for (int q = 0; q < 4; q++) {
        for (int i = 0; i < 12; i++) S->cand[q][i] = 0.0;
        for (int j = 0; j < 3; j++) { S->nrm[q][j] = 0.0; S->c2[q][j] = 0.0; }
        S->tod[q] = 0.0;
    }
    if (!(mi_finite(fx1) && mi_finite(fy1) && mi_finite(fx2) && mi_finite(fy2)) || fx1 == 0.0 || fy1 == 0.0 || fx2 == 0.0 || fy2 == 0.0)
        return MI_DEGENSAC_POSE_BAD_CAMERA;
    double L[9], G[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {                                     /* L = H K1 */
        L[3 * i] = H[3 * i] * fx1; L[3 * i + 1] = H[3 * i + 1] * fy1;
        L[3 * i + 2] = (H[3 * i] * cx1 + H[3 * i + 1] * cy1) + H[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {                                     /* G = K2^-1 L */
        G[j] = (L[j] - cx2 * L[6 + j]) / fx2; G[3 + j] = (L[3 + j] - cy2 * L[6 + j]) / fy2; G[6 + j] = L[6 + j];
    }
    double m = 0.0; bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; i++) { const double x = fabs(G[i]); fin = fin && x <= MI_DBL_MAX; if (x > m) m = x; }
    if (!fin || !(m > 0.0)) return MI_DEGENSAC_POSE_BAD_MODEL;
    double A[9];
#pragma unroll
    for (int i = 0; i < 9; i++) A[i] = G[i] / m;
    /* the one-sided Jacobi rule of mi_pose.hip (its comment there has the convergence figures): V = I, B = A, PH_SWEEPS sweeps over the
     * column pairs (0 1) (0 2) (1 2), B = A V throughout, sigma_i = |b_i| */
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    double b0[3] = {A[0], A[3], A[6]}, b1[3] = {A[1], A[4], A[7]}, b2[3] = {A[2], A[5], A[8]};
#define PH_DOT(x, y) ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2])
#define PH_ROT(bi, vi, bj, vj) { const double al_ = PH_DOT(bi, bi), be_ = PH_DOT(bj, bj), ga_ = PH_DOT(bi, bj); \
        if (ga_ != 0.0) { const double z_ = (be_ - al_) / (2.0 * ga_), t_ = (z_ >= 0.0 ? 1.0 : -1.0) / (fabs(z_) + sqrt(1.0 + z_ * z_)), \
                          c_ = 1.0 / sqrt(1.0 + t_ * t_), s_ = c_ * t_; \
            for (int k_ = 0; k_ < 3; k_++) { const double x_ = bi[k_], y_ = bj[k_], p_ = vi[k_], q_ = vj[k_]; \
                bi[k_] = c_ * x_ - s_ * y_; bj[k_] = s_ * x_ + c_ * y_; vi[k_] = c_ * p_ - s_ * q_; vj[k_] = s_ * p_ + c_ * q_; } } }
    for (int sweep = 0; sweep < PH_SWEEPS; sweep++) { PH_ROT(b0, v0, b1, v1) PH_ROT(b0, v0, b2, v2) PH_ROT(b1, v1, b2, v2) }
#undef PH_ROT
    double s0 = sqrt(PH_DOT(b0, b0)), s1 = sqrt(PH_DOT(b1, b1)), s2 = sqrt(PH_DOT(b2, b2));
#undef PH_DOT
    /* sigma descending, ties keep the lower index in front: three compare-exchanges (0 1) (1 2) (0 1) on (sigma, column of V, column of B) */
#define PH_CX(sa, va, ba, sb, vb, bb) if (sb > sa) { double t_ = sa; sa = sb; sb = t_; \
        for (int k_ = 0; k_ < 3; k_++) { t_ = va[k_]; va[k_] = vb[k_]; vb[k_] = t_; t_ = ba[k_]; ba[k_] = bb[k_]; bb[k_] = t_; } }
    PH_CX(s0, v0, b0, s1, v1, b1) PH_CX(s1, v1, b1, s2, v2, b2) PH_CX(s0, v0, b0, s1, v1, b1)
#undef PH_CX
    if (!(s2 > 0.0)) return MI_DEGENSAC_POSE_BAD_MODEL;               /* a homography has full rank */
    const double sg = ph_det(A) < 0.0 ? -1.0 : 1.0;                   /* both cameras on one side of the plane */
    if (s0 - s2 <= rot_eps * s1) {                                    /* a rotation: R = U V^T */
        double u0[3], u1[3], u2[3], Rm[9];
#pragma unroll
        for (int r = 0; r < 3; r++) { u0[r] = b0[r] / s0; u1[r] = b1[r] / s1; u2[r] = b2[r] / s2; }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) Rm[3 * r + c] = (u0[r] * v0[c] + u1[r] * v1[c]) + u2[r] * v2[c];
        const double det = ph_det(Rm);
#pragma unroll
        for (int i = 0; i < 9; i++) { if (det < 0.0) Rm[i] = -Rm[i]; fin = fin && mi_finite(Rm[i]); }
        if (!fin) return MI_DEGENSAC_POSE_BAD_MODEL;
#pragma unroll
        for (int i = 0; i < 9; i++) S->cand[0][i] = Rm[i];
        return MI_DEGENSAC_POSE_ROTATION;
    }
    /* G <- sg G / sigma2 has the singular values (k1, 1, k3) and maps v_i to h_i; the two unit vectors a = (p v1 +- q v3) / w keep their
     * length under it as v2 does, so R is the rotation that takes (v2, a, v2 x a) to (h2, G a, h2 x G a) and n = v2 x a */
    double Gn[9], h0[3], h1[3], h2[3];
#pragma unroll
    for (int i = 0; i < 9; i++) Gn[i] = sg * (A[i] / s1);
#pragma unroll
    for (int r = 0; r < 3; r++) { h0[r] = sg * (b0[r] / s1); h1[r] = sg * (b1[r] / s1); h2[r] = sg * (b2[r] / s1); }
    const double k1 = s0 / s1, k3 = s2 / s1;
    const double pp = sqrt((1.0 - k3) * (1.0 + k3)), qq = sqrt((k1 - 1.0) * (k1 + 1.0)), ww = sqrt((k1 - k3) * (k1 + k3));
#pragma unroll
    for (int k = 0; k < 2; k++) {
        double a[3], g[3], n[3], rn[3], Rm[9], T[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            a[c] = k == 0 ? (pp * v0[c] + qq * v2[c]) / ww : (pp * v0[c] - qq * v2[c]) / ww;
            g[c] = k == 0 ? (pp * h0[c] + qq * h2[c]) / ww : (pp * h0[c] - qq * h2[c]) / ww;
        }
        n[0] = v1[1] * a[2] - v1[2] * a[1]; n[1] = v1[2] * a[0] - v1[0] * a[2]; n[2] = v1[0] * a[1] - v1[1] * a[0];
        rn[0] = h1[1] * g[2] - h1[2] * g[1]; rn[1] = h1[2] * g[0] - h1[0] * g[2]; rn[2] = h1[0] * g[1] - h1[1] * g[0];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) Rm[3 * r + c] = (h1[r] * v1[c] + g[r] * a[c]) + rn[r] * n[c];
            T[r] = ((Gn[3 * r] * n[0] + Gn[3 * r + 1] * n[1]) + Gn[3 * r + 2] * n[2]) - rn[r];
        }
        const double tod = sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2]);
        double t[3];
#pragma unroll
        for (int r = 0; r < 3; r++) { t[r] = T[r] / tod; fin = fin && mi_finite(t[r]) && mi_finite(n[r]); }
        fin = fin && mi_finite(tod);
#pragma unroll
        for (int i = 0; i < 9; i++) fin = fin && mi_finite(Rm[i]);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int q = k + 2 * h; const double sn = h ? -1.0 : 1.0;  /* (a product with +-1 is exact) */
#pragma unroll
            for (int i = 0; i < 9; i++) S->cand[q][i] = Rm[i];
            const double tq[3] = {sn * t[0], sn * t[1], sn * t[2]};
#pragma unroll
            for (int j = 0; j < 3; j++) {
                S->cand[q][9 + j] = tq[j]; S->nrm[q][j] = sn * n[j];
                S->c2[q][j] = -((Rm[j] * tq[0] + Rm[3 + j] * tq[1]) + Rm[6 + j] * tq[2]);
            }
            S->tod[q] = tod;
        }
    }
    if (!fin) {
        for (int q = 0; q < 4; q++) {
            for (int i = 0; i < 12; i++) S->cand[q][i] = 0.0;
            for (int j = 0; j < 3; j++) { S->nrm[q][j] = 0.0; S->c2[q][j] = 0.0; }
            S->tod[q] = 0.0;
        }
        return MI_DEGENSAC_POSE_BAD_MODEL;
    }
    return MI_DEGENSAC_POSE_OK;
}

/* the midpoint rule of one row under (R, c2), the rule of mi_pose.hip: lambda1, lambda2, cosang and, with WITH_X, the midpoint */
template <bool WITH_X>
__device__ __forceinline__ void ph_row(const double *R, const double *c2, double d1x, double d1y, double d2x, double d2y, double &l1, double &l2,
                                       double &cosang, double *X)
{
    const double r2x = (R[0] * d2x + R[3] * d2y) + R[6], r2y = (R[1] * d2x + R[4] * d2y) + R[7], r2z = (R[2] * d2x + R[5] * d2y) + R[8];
    const double a = (d1x * d1x + d1y * d1y) + 1.0;
    const double b = (d1x * r2x + d1y * r2y) + r2z;
    const double c = (r2x * r2x + r2y * r2y) + r2z * r2z;
    const double d = (d1x * c2[0] + d1y * c2[1]) + c2[2];
    const double e = (r2x * c2[0] + r2y * c2[1]) + r2z * c2[2];
    const double den = a * c - b * b;
    l1 = (c * d - b * e) / den;
    l2 = (b * d - a * e) / den;
    if (WITH_X) {
        cosang = b / sqrt(a * c);
        X[0] = 0.5 * ((l1 * d1x + c2[0]) + l2 * r2x);
        X[1] = 0.5 * ((l1 * d1y + c2[1]) + l2 * r2y);
        X[2] = 0.5 * ((l1 + c2[2]) + l2 * r2z);
    }
}

enum { PH_COUNT = 0, PH_FINAL = 1, PH_ROTATION = 2 };

/* One pass over the n rows at b0.  PH_COUNT: out[0] = used rows, out[1 + q] = front rows of candidate q.  PH_FINAL: the outputs of the
 * used rows under candidate `chosen`, out[0] = wide rows.  PH_ROTATION: front and cosang of the used rows under the rotation in
 * candidate 0, out[0] = used rows, out[1] = front rows.  All threads of the workgroup, uniform control flow. */
template <int MODE>
__device__ __forceinline__ void ph_pass(ph_shared *S, const ph_args &a, int64_t b0, int n, int chosen, int *out)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NR = MODE == PH_COUNT ? 2 : 1, NC = MODE == PH_COUNT ? 4 : 1, NCNT = MODE == PH_COUNT ? 5 : MODE == PH_FINAL ? 1 : 2;
    double R[NR][9], c2[NC][3], nr[NR][3], cam[8];
#pragma unroll
    for (int i = 0; i < 8; i++) cam[i] = S->cam[i];
#pragma unroll
    for (int h = 0; h < NR; h++) {                                    /* candidates 0 and 1 hold the two rotations and normals; 2 and 3 negate n */
#pragma unroll
        for (int i = 0; i < 9; i++) R[h][i] = S->cand[MODE == PH_COUNT ? h : chosen][i];
#pragma unroll
        for (int j = 0; j < 3; j++) nr[h][j] = S->nrm[MODE == PH_COUNT ? h : chosen][j];
    }
#pragma unroll
    for (int q = 0; q < NC; q++)
#pragma unroll
        for (int j = 0; j < 3; j++) c2[q][j] = S->c2[MODE == PH_COUNT ? q : chosen][j];
    const __attribute__((address_space(1))) double *G = (const __attribute__((address_space(1))) double *)(a.pts + 4 * (size_t)b0);
    int cnt[NCNT];
#pragma unroll
    for (int k = 0; k < NCNT; k++) cnt[k] = 0;
    for (int base = 0; base < n; base += PH_STEP) {
        double p[PH_LOADS][4]; bool use[PH_LOADS];
#pragma unroll
        for (int k = 0; k < PH_LOADS; k++) {                          /* the step's loads back to back; a row past the end reads row n - 1 */
            const int i = base + k * PH_T + tid, j = i < n ? i : n - 1;
#pragma unroll
            for (int c = 0; c < 4; c++) p[k][c] = G[4 * (size_t)j + c];
            use[k] = i < n && (a.keep == nullptr || a.keep[b0 + j] != 0);
        }
#pragma unroll
        for (int k = 0; k < PH_LOADS; k++) {
            const int i = base + k * PH_T + tid;
            const double d1x = (p[k][0] - cam[2]) / cam[0], d1y = (p[k][1] - cam[3]) / cam[1];
            const double d2x = (p[k][2] - cam[6]) / cam[4], d2y = (p[k][3] - cam[7]) / cam[5];
            if constexpr (MODE == PH_COUNT) {
                cnt[0] += __popcll(__ballot(use[k]));
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    double l1, l2, cs;
                    ph_row<false>(R[q & 1], c2[q], d1x, d1y, d2x, d2y, l1, l2, cs, nullptr);
                    const double side = (nr[q & 1][0] * d1x + nr[q & 1][1] * d1y) + nr[q & 1][2];      /* n . d1 of candidates 0, 1 */
                    const bool vis = q < 2 ? side > 0.0 : -side > 0.0;
                    cnt[1 + q] += __popcll(__ballot(use[k] && l1 > 0.0 && l2 > 0.0 && vis));      /* a NaN is not front */
                }
            } else if constexpr (MODE == PH_FINAL) {
                double l1, l2, cs, X[3];
                ph_row<true>(R[0], c2[0], d1x, d1y, d2x, d2y, l1, l2, cs, X);
                const double side = (nr[0][0] * d1x + nr[0][1] * d1y) + nr[0][2];
                const bool fr = use[k] && l1 > 0.0 && l2 > 0.0 && side > 0.0;
                cnt[0] += __popcll(__ballot(fr && cs <= a.cos_min));
                if (use[k]) {
                    const size_t g = (size_t)b0 + (size_t)i;
                    a.front[g] = fr ? 1 : 0;
                    if (a.X) { a.X[3 * g] = X[0]; a.X[3 * g + 1] = X[1]; a.X[3 * g + 2] = X[2]; }
                    if (a.depth) { a.depth[2 * g] = l1; a.depth[2 * g + 1] = l2; }
                    if (a.cosang) a.cosang[g] = cs;
                }
            } else {
                double l1, l2, cs, X[3];
                ph_row<true>(R[0], c2[0], d1x, d1y, d2x, d2y, l1, l2, cs, X);                 /* c2 = 0: only cosang is used */
                const bool fr = use[k] && (R[0][6] * d1x + R[0][7] * d1y) + R[0][8] > 0.0;
                cnt[0] += __popcll(__ballot(use[k]));
                cnt[1] += __popcll(__ballot(fr));
                if (use[k]) {
                    const size_t g = (size_t)b0 + (size_t)i;
                    a.front[g] = fr ? 1 : 0;
                    if (a.cosang) a.cosang[g] = cs;
                }
            }
        }
    }
    __syncthreads();                                                  /* the previous pass's words are read */
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NCNT; k++) S->cnt[wv][k] = cnt[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NCNT; k++) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < PH_NW; w++) s += S->cnt[w][k];
        out[k] = s;
    }
}

__global__ __launch_bounds__(PH_T) void ph_pose_kernel(ph_args a)
{
    __shared__ ph_shared S;
    const int tid = threadIdx.x;
    for (int p = (int)blockIdx.x; p < a.K; p += (int)gridDim.x) {
        const int64_t b = a.off[p], e = a.off[p + 1];
        const bool whole = b >= 0 && b <= e && e <= a.cap;            /* else a truncated export, or offsets that are not a list */
        __syncthreads();                                              /* the previous entry's epilogue has read S */
        if (tid == 0) {
            int st = MI_DEGENSAC_POSE_TRUNCATED;
            if (whole) {
                const int64_t i1 = a.cam_idx ? (int64_t)a.cam_idx[2 * (size_t)p] : 2 * (int64_t)p;
                const int64_t i2 = a.cam_idx ? (int64_t)a.cam_idx[2 * (size_t)p + 1] : 2 * (int64_t)p + 1;
                if (i1 < 0 || i1 >= a.n_cams || i2 < 0 || i2 >= a.n_cams) st = MI_DEGENSAC_POSE_BAD_CAMERA;
                else {
#pragma unroll
                    for (int i = 0; i < 4; i++) { S.cam[i] = a.cams[4 * (size_t)i1 + i]; S.cam[4 + i] = a.cams[4 * (size_t)i2 + i]; }
                    double H[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) H[i] = a.H[9 * (size_t)p + i];
                    st = ph_decompose(&S, H, a.rot_eps);
                }
            }
            S.status = st;
        }
        __syncthreads();
        int status = S.status, used = 0, chosen = 0, best = 0, second = 0, wide = 0;
        int c[5] = {0, 0, 0, 0, 0};
        const bool rotation = status == MI_DEGENSAC_POSE_ROTATION;
        const bool model = status == MI_DEGENSAC_POSE_OK || rotation;  /* the candidates stand in LDS */
        const int n = whole ? (int)(e - b) : 0;
        if (rotation) {
            int r2[2] = {0, 0};
            if (n > 0) ph_pass<PH_ROTATION>(&S, a, b, n, 0, r2);
            used = r2[0]; best = r2[1]; c[1] = r2[1];
            if (used == 0) status = MI_DEGENSAC_POSE_EMPTY;
        } else if (model) {
            if (n > 0) ph_pass<PH_COUNT>(&S, a, b, n, 0, c);
            used = c[0];
            if (used == 0) status = MI_DEGENSAC_POSE_EMPTY;
            else {
                best = c[1];
#pragma unroll
                for (int q = 1; q < 4; q++) if (c[1 + q] > best) { best = c[1 + q]; chosen = q; }      /* ties: the first */
                second = -1;
#pragma unroll
                for (int q = 0; q < 4; q++) if (q != chosen && c[1 + q] > second) second = c[1 + q];
                int w1[1];
                ph_pass<PH_FINAL>(&S, a, b, n, chosen, w1);
                wide = w1[0];
            }
        }
        const bool ok = status == MI_DEGENSAC_POSE_OK || status == MI_DEGENSAC_POSE_ROTATION;
        if (tid < 12) a.pose[12 * (size_t)p + tid] = ok ? S.cand[chosen][tid] : 0.0;
        if (tid < 3) a.normal[3 * (size_t)p + tid] = ok ? S.nrm[chosen][tid] : 0.0;
        if (tid == 3) a.tod[p] = ok ? S.tod[chosen] : 0.0;
        if (a.cand && tid < 48) a.cand[48 * (size_t)p + tid] = model ? S.cand[tid / 12][tid % 12] : 0.0;
        if (a.cand_normal && tid < 12) a.cand_normal[12 * (size_t)p + tid] = model ? S.nrm[tid / 3][tid % 3] : 0.0;
        if (a.cand_front && tid < 4) a.cand_front[4 * (size_t)p + tid] = ok ? c[1 + tid] : 0;
        if (tid == 0) {
            int32_t *o = a.info + 5 * (size_t)p;
            o[0] = ok ? used : 0; o[1] = ok ? best : 0; o[2] = ok ? second : 0; o[3] = ok ? wide : 0; o[4] = status;
        }
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_pose_h_tile(int which) { return which == 0 ? PH_STEP : which == 1 ? PH_GRID : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int ph_check(const void *pts, const void *off, const void *H, const void *cams, int n_cams, int K, int64_t cap, double cos_min, double rot_eps,
                    const void *pose, const void *front, const void *info, const void *normal, const void *tod)
{
    if (K < 0) return mi_einval("n_entries < 0");
    if (cap < 0) return mi_einval("cap < 0");
    if (cap > 0x3fffffff) return mi_einval("too many rows in one list (cap > 0x3fffffff)");
    if (n_cams < 0) return mi_einval("n_cams < 0");
    if (!(cos_min >= -1.0 && cos_min <= 1.0)) return mi_einval("cos_min should lie in [-1, 1]");
    if (!(rot_eps >= 0.0)) return mi_einval("rotation_eps should be >= 0 (and not NaN)");
    if (!off) return mi_einval("NULL argument: corr_offsets");
    if (K > 0 && (!H || !cams)) return mi_einval("NULL argument: H and cams");
    if (K > 0 && (!pose || !info || !normal || !tod)) return mi_einval("NULL argument: pose, info, normal and t_over_d");
    if (cap > 0 && (!pts || !front)) return mi_einval("NULL argument: pts and front");
    return 0;
}

extern "C" int mi_degensac_pose_h_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep, const double *d_H,
                                            const double *d_cams, int n_cams, const int32_t *d_cam_idx, int n_entries, int64_t cap, double cos_min,
                                            double rotation_eps, int device, void *stream, double *d_pose, uint8_t *d_front, int32_t *d_info,
                                            double *d_normal, double *d_t_over_d, double *d_X, double *d_depth, double *d_cosang, double *d_cand,
                                            double *d_cand_normal, int32_t *d_cand_front)
{
    int rc = ph_check(d_pts, d_corr_offsets, d_H, d_cams, n_cams, n_entries, cap, cos_min, rotation_eps, d_pose, d_front, d_info, d_normal, d_t_over_d);
    if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (cap > 0) {                                                    /* positions that no entry owns, and rows that are not used, keep 0 / NaN */
        MICHK(hipMemsetAsync(d_front, 0, (size_t)cap, s));
        if (d_X) MICHK(hipMemsetAsync(d_X, 0xff, (size_t)cap * 24, s));              /* all bits set: a NaN */
        if (d_depth) MICHK(hipMemsetAsync(d_depth, 0xff, (size_t)cap * 16, s));
        if (d_cosang) MICHK(hipMemsetAsync(d_cosang, 0xff, (size_t)cap * 8, s));
    }
    if (n_entries == 0) return 0;
    ph_args a;
    memset(&a, 0, sizeof a);
    a.pts = d_pts; a.off = d_corr_offsets; a.keep = d_keep; a.H = d_H; a.cams = d_cams; a.cam_idx = d_cam_idx; a.pose = d_pose; a.front = d_front;
    a.info = d_info; a.normal = d_normal; a.tod = d_t_over_d; a.X = d_X; a.depth = d_depth; a.cosang = d_cosang; a.cand = d_cand;
    a.cand_normal = d_cand_normal; a.cand_front = d_cand_front;
    a.K = n_entries; a.n_cams = n_cams; a.cap = cap; a.cos_min = cos_min; a.rot_eps = rotation_eps;
    const dim3 grid((unsigned)std::min(n_entries, PH_GRID)), block(PH_T);
    hipLaunchKernelGGL(ph_pose_kernel, grid, block, 0, s, a);
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_pose_h_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep, const double *H, const double *cams,
                                        int n_cams, const int32_t *cam_idx, int n_entries, int64_t cap, double cos_min, double rotation_eps, int device,
                                        double *pose, uint8_t *front, int32_t *info, double *normal, double *t_over_d, double *X, double *depth,
                                        double *cosang, double *cand, double *cand_normal, int32_t *cand_front)
{
    int rc = ph_check(pts, corr_offsets, H, cams, n_cams, n_entries, cap, cos_min, rotation_eps, pose, front, info, normal, t_over_d); if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t K = (size_t)n_entries, C = (size_t)cap, NC = (size_t)n_cams;
    MiStage st;
    const int i_pts = st.in(pts, C * 32), i_off = st.in(corr_offsets, (K + 1) * 8), i_keep = st.in(keep, C), i_H = st.in(H, K * 72),
              i_cams = st.in(cams, NC * 32), i_idx = st.in(cam_idx, K * 8), o_pose = st.out(pose, K * 96), o_front = st.out(front, C),
              o_info = st.out(info, K * 20), o_nrm = st.out(normal, K * 24), o_tod = st.out(t_over_d, K * 8), o_X = st.out(X, C * 24),
              o_depth = st.out(depth, C * 16), o_cos = st.out(cosang, C * 8), o_cand = st.out(cand, K * 384), o_cn = st.out(cand_normal, K * 96),
              o_cf = st.out(cand_front, K * 16);
    rc = st.upload(); if (rc) return rc;
    rc = mi_degensac_pose_h_lists_dev(st.dev<double>(i_pts), st.dev<int64_t>(i_off), st.dev<uint8_t>(i_keep), st.dev<double>(i_H),
                                      st.dev<double>(i_cams), n_cams, st.dev<int32_t>(i_idx), n_entries, cap, cos_min, rotation_eps, device, nullptr,
                                      st.dev<double>(o_pose), st.dev<uint8_t>(o_front), st.dev<int32_t>(o_info), st.dev<double>(o_nrm),
                                      st.dev<double>(o_tod), st.dev<double>(o_X), st.dev<double>(o_depth), st.dev<double>(o_cos),
                                      st.dev<double>(o_cand), st.dev<double>(o_cn), st.dev<int32_t>(o_cf));
    if (rc) return rc;
    return st.finish();
}
