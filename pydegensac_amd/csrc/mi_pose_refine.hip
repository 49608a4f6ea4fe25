/* libmi_degensac.so — refinement of relative poses on exported correspondence lists (include/mi_degensac.h
 * mi_degensac_pose_refine_lists*): per entry of a compact list (pts [cap, 4] and corr_offsets [K + 1] as the correspondence export writes
 * them, a pose [12] as the pose call writes it, all on the device) a Levenberg-Marquardt refinement of the five degrees of freedom of
 * (R, t / |t|) on the Sampson distance of the used rows, in pixels.  gfx950 only, no CPU path.
 *
 * One workgroup of 256 threads per entry, further entries by a grid stride; no workgroup waits for another, no atomics.  The kernel reads
 * its row range o[p], o[p + 1] itself, so the host never learns a length and the call has no synchronisation.
 *   thread 0    between the passes: the 5 x 5 Cholesky solve, the Cayley retraction, E and the five generators of the trial pose into
 *               LDS; a few hundred flops per trial, every small array indexed by constants only (registers, no scratch).
 *   row pass    PR_STEP = 1024 rows per step, four per thread, 256 consecutive 32-byte rows per load instruction of the workgroup, the
 *               step's loads back to back; E, the generators and the eight camera numbers are read from LDS once per pass (every lane
 *               the same address: a broadcast) and held in registers; 21 float64 accumulators per thread.
 *   sums        inside a wave six shuffle steps (lane l takes v[l] + v[l + m]), then 4 x 21 LDS words that thread 0 adds in wave order.
 * The order of every sum is fixed by the header, so every output is the same bits on every call. */
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
#include "mi_pose_dev.h"

#define PR_T     256                      /* threads per workgroup */
#define PR_NW    (PR_T / 64)
#define PR_LOADS 4                        /* rows per thread and step */
#define PR_STEP  (PR_LOADS * PR_T)        /* rows per workgroup and step */
#define PR_GRID  256                      /* cap on the grid: further entries by the grid stride */
#define PR_NS    21                       /* sums of a pass: cost, g[5], A[15] */
#define PR_RUNNING (-1)

struct pr_args {
    const double *pts;            /* [cap, 4] */
    const int64_t *off;           /* [K + 1] */
    const uint8_t *keep;          /* [cap] or null */
    const double *pose;           /* [K, 12] */
    const double *cams;           /* [n_cams, 4] */
    const int32_t *cam_idx;       /* [K, 2] or null */
    double *pose_out;             /* [K, 12] */
    double *cost;                 /* [K, 2] */
    int32_t *info;                /* [K, 4] */
    double *resid;                /* [cap] or null */
    double *F;                    /* [K, 9] or null */
    int K, n_cams; int64_t cap;
    int max_trials; double ftol;
};

struct pr_shared {
    double M[6][9];               /* E and G_0 .. G_4 of the pose of the next pass */
    double cam[8];                /* fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2 */
    double cur[18];               /* the current pose: R [9], t [3], u [3], v [3] */
    double tri[18];               /* the trial pose likewise */
    double sum[PR_NS];            /* the sums at the current pose */
    double part[PR_NW][PR_NS];    /* the waves' sums of the last pass */
    double Fm[9];
    double lambda, cost0;
    int cnt[PR_NW];
    int status, go, trials, accepted;
};

/* column j of X = cross(x, column j of R) */
__device__ __forceinline__ void pr_cross_mat(const double *x, const double *R, double *X)
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        X[j] = x[1] * R[6 + j] - x[2] * R[3 + j];
        X[3 + j] = x[2] * R[j] - x[0] * R[6 + j];
        X[6 + j] = x[0] * R[3 + j] - x[1] * R[j];
    }
}

/* E alone of the pose P (R, t, ..) into S->M[0] (one thread) */
__device__ __forceinline__ void pr_essential(pr_shared *S, const double *P)
{
    double R[9], t[3], E[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = P[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = P[9 + i];
    pr_cross_mat(t, R, E);
#pragma unroll
    for (int i = 0; i < 9; i++) S->M[0][i] = E[i];
}

/* E, u, v and the five generators of the pose (R, t) in P[0 .. 12) into S->M and P[12 .. 18) (one thread) */
__device__ __forceinline__ void pr_model(pr_shared *S, double *P)
{
    double R[9], t[3], E[9], G[9], c[3], u[3], v[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = P[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = P[9 + i];
    pr_cross_mat(t, R, E);
    const double m0 = fabs(t[0]), m1 = fabs(t[1]), m2 = fabs(t[2]);
    const int ax = (m1 < m0) ? ((m2 < m1) ? 2 : 1) : ((m2 < m0) ? 2 : 0);          /* the smallest |t[i]|, ties to the lowest index */
    c[0] = ax == 0 ? 0.0 : ax == 1 ? t[2] : -t[1];
    c[1] = ax == 0 ? -t[2] : ax == 1 ? 0.0 : t[0];
    c[2] = ax == 0 ? t[1] : ax == 1 ? -t[0] : 0.0;
    const double nc = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    u[0] = c[0] / nc; u[1] = c[1] / nc; u[2] = c[2] / nc;
    v[0] = t[1] * u[2] - t[2] * u[1]; v[1] = t[2] * u[0] - t[0] * u[2]; v[2] = t[0] * u[1] - t[1] * u[0];
#pragma unroll
    for (int i = 0; i < 3; i++) { P[12 + i] = u[i]; P[15 + i] = v[i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) {                                     /* rows of E; G_k = E [e_k]x by columns */
        const double e0 = E[3 * i], e1 = E[3 * i + 1], e2 = E[3 * i + 2];
        S->M[0][3 * i] = e0; S->M[0][3 * i + 1] = e1; S->M[0][3 * i + 2] = e2;
        S->M[1][3 * i] = 0.0; S->M[1][3 * i + 1] = e2; S->M[1][3 * i + 2] = -e1;
        S->M[2][3 * i] = -e2; S->M[2][3 * i + 1] = 0.0; S->M[2][3 * i + 2] = e0;
        S->M[3][3 * i] = e1; S->M[3][3 * i + 1] = -e0; S->M[3][3 * i + 2] = 0.0;
    }
    pr_cross_mat(u, R, G);
#pragma unroll
    for (int i = 0; i < 9; i++) S->M[4][i] = G[i];
    pr_cross_mat(v, R, G);
#pragma unroll
    for (int i = 0; i < 9; i++) S->M[5][i] = G[i];
}

/* the sums of the last pass in wave order (one thread) */
__device__ __forceinline__ double pr_sum(const pr_shared *S, int k) { return ((S->part[0][k] + S->part[1][k]) + S->part[2][k]) + S->part[3][k]; }

/* The next trial that has a pass (one thread): solve, retract, model of the trial pose into S->M.  Trials whose Cholesky meets a pivot
 * that is not > 0 are rejected here.  Returns 1 with a trial pose to pass over, 0 with S->status set. */
__device__ __forceinline__ int pr_next(pr_shared *S, int max_trials)
{
    for (;;) {
        if (S->trials >= max_trials) { S->status = MI_DEGENSAC_REFINE_MAX_TRIALS; return 0; }
        S->trials = S->trials + 1;
        const double lam = S->lambda;
        double g[5], A[15], L[5][5], y[5], dl[5];
#pragma unroll
        for (int k = 0; k < 5; k++) g[k] = S->sum[1 + k];
#pragma unroll
        for (int k = 0; k < 15; k++) A[k] = S->sum[6 + k];
        /* A[k][l], k <= l, at 5 k - k (k - 1) / 2 + (l - k): 0 1 2 3 4 | 5 6 7 8 | 9 10 11 | 12 13 | 14 */
#define PR_A(k, l) A[5 * (k) - (k) * ((k) - 1) / 2 + ((l) - (k))]
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            double x = PR_A(j, j) + lam * PR_A(j, j);
#pragma unroll
            for (int k = 0; k < j; k++) x = x - L[j][k] * L[j][k];
            ok = ok && (x > 0.0);
            L[j][j] = sqrt(x);
#pragma unroll
            for (int i = j + 1; i < 5; i++) {
                double z = PR_A(j, i);
#pragma unroll
                for (int k = 0; k < j; k++) z = z - L[i][k] * L[j][k];
                L[i][j] = z / L[j][j];
            }
        }
#undef PR_A
        if (!ok) {
            S->lambda = 10.0 * lam;
            if (S->lambda > 1e12) { S->status = MI_DEGENSAC_REFINE_STALLED; return 0; }
            continue;
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            double x = -g[i];
#pragma unroll
            for (int k = 0; k < i; k++) x = x - L[i][k] * y[k];
            y[i] = x / L[i][i];
        }
#pragma unroll
        for (int i = 4; i >= 0; i--) {
            double x = y[i];
#pragma unroll
            for (int k = i + 1; k < 5; k++) x = x - L[k][i] * dl[k];
            dl[i] = x / L[i][i];
        }
        const double w0 = dl[0], w1 = dl[1], w2 = dl[2], a0 = 0.5 * w0, a1 = 0.5 * w1, a2 = 0.5 * w2;
        const double aa = (a0 * a0 + a1 * a1) + a2 * a2, p = 1.0 - aa, d = 1.0 + aa;
        double Cm[9];
        Cm[0] = (p + w0 * a0) / d; Cm[1] = (w0 * a1 - w2) / d; Cm[2] = (w0 * a2 + w1) / d;
        Cm[3] = (w1 * a0 + w2) / d; Cm[4] = (p + w1 * a1) / d; Cm[5] = (w1 * a2 - w0) / d;
        Cm[6] = (w2 * a0 - w1) / d; Cm[7] = (w2 * a1 + w0) / d; Cm[8] = (p + w2 * a2) / d;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                S->tri[3 * i + j] = (S->cur[3 * i] * Cm[j] + S->cur[3 * i + 1] * Cm[3 + j]) + S->cur[3 * i + 2] * Cm[6 + j];
        double z[3];
#pragma unroll
        for (int j = 0; j < 3; j++) z[j] = (S->cur[9 + j] + dl[3] * S->cur[12 + j]) + dl[4] * S->cur[15 + j];
        const double nz = sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
#pragma unroll
        for (int j = 0; j < 3; j++) S->tri[9 + j] = z[j] / nz;
        pr_model(S, S->tri);
        return 1;
    }
}

/* the verdict on the trial pose after its pass (one thread): returns 1 when the run goes on, 0 with S->status set */
__device__ __forceinline__ int pr_judge(pr_shared *S, double ftol)
{
    const double cost = S->sum[0], cnew = pr_sum(S, 0);
    if (cnew < cost) {                                                /* a NaN is not accepted */
#pragma unroll
        for (int i = 0; i < 18; i++) S->cur[i] = S->tri[i];
#pragma unroll
        for (int k = 0; k < PR_NS; k++) S->sum[k] = pr_sum(S, k);
        S->accepted = S->accepted + 1;
        S->lambda = fmax(S->lambda / 10.0, 1e-12);
        if ((cost - cnew) <= ftol * cost) { S->status = MI_DEGENSAC_REFINE_CONVERGED; return 0; }
        return 1;
    }
    S->lambda = 10.0 * S->lambda;
    if (S->lambda > 1e12) { S->status = MI_DEGENSAC_REFINE_STALLED; return 0; }
    return 1;
}

struct pr_epi { double n, a0, a1, b0, b1; };
__device__ __forceinline__ pr_epi pr_epi_of(const double *M, const double *cam, double d1x, double d1y, double d2x, double d2y)
{
    const double A0 = (M[0] * d1x + M[1] * d1y) + M[2], A1 = (M[3] * d1x + M[4] * d1y) + M[5], A2 = (M[6] * d1x + M[7] * d1y) + M[8];
    const double B0 = (M[0] * d2x + M[3] * d2y) + M[6], B1 = (M[1] * d2x + M[4] * d2y) + M[7];
    pr_epi e;
    e.n = (d2x * A0 + d2y * A1) + A2;
    e.a0 = A0 / cam[4]; e.a1 = A1 / cam[5]; e.b0 = B0 / cam[0]; e.b1 = B1 / cam[1];
    return e;
}

/* One pass over the n rows at b0 under the matrices of S->M.  RESID = false: the 21 sums of the waves into S->part, the used rows into
 * S->cnt.  RESID = true: r of the used rows into a.resid.  All threads of the workgroup, uniform control flow. */
template <bool RESID>
__device__ __forceinline__ void pr_pass(pr_shared *S, const pr_args &a, int64_t b0, int n)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NM = RESID ? 1 : 6;
    double M[NM][9], cam[8];
#pragma unroll
    for (int i = 0; i < 8; i++) cam[i] = S->cam[i];
#pragma unroll
    for (int g = 0; g < NM; g++)
#pragma unroll
        for (int i = 0; i < 9; i++) M[g][i] = S->M[g][i];
    const __attribute__((address_space(1))) double *G = (const __attribute__((address_space(1))) double *)(a.pts + 4 * (size_t)b0);
    double acc[PR_NS];
#pragma unroll
    for (int k = 0; k < PR_NS; k++) acc[k] = 0.0;
    int cnt = 0;
    for (int base = 0; base < n; base += PR_STEP) {
        double p[PR_LOADS][4]; bool use[PR_LOADS];
#pragma unroll
        for (int k = 0; k < PR_LOADS; k++) {                          /* the step's loads back to back; a row past the end reads row n - 1 */
            const int i = base + k * PR_T + tid, j = i < n ? i : n - 1;
#pragma unroll
            for (int c = 0; c < 4; c++) p[k][c] = G[4 * (size_t)j + c];
            use[k] = i < n && (a.keep == nullptr || a.keep[b0 + j] != 0);
        }
#pragma unroll
        for (int k = 0; k < PR_LOADS; k++) {
            const double d1x = (p[k][0] - cam[2]) / cam[0], d1y = (p[k][1] - cam[3]) / cam[1];
            const double d2x = (p[k][2] - cam[6]) / cam[4], d2y = (p[k][3] - cam[7]) / cam[5];
            const pr_epi e = pr_epi_of(M[0], cam, d1x, d1y, d2x, d2y);
            const double s = ((e.a0 * e.a0 + e.a1 * e.a1) + e.b0 * e.b0) + e.b1 * e.b1, q = sqrt(s), r = e.n / q;
            if constexpr (RESID) {
                if (use[k]) a.resid[(size_t)b0 + (size_t)(base + k * PR_T + tid)] = r;
            } else {
                cnt += __popcll(__ballot(use[k]));
                double J[5];
                const double sq = s * q;
#pragma unroll
                for (int g = 0; g < 5; g++) {
                    const pr_epi f = pr_epi_of(M[1 + g], cam, d1x, d1y, d2x, d2y);
                    const double h = ((e.a0 * f.a0 + e.a1 * f.a1) + e.b0 * f.b0) + e.b1 * f.b1;
                    J[g] = f.n / q - (e.n * h) / sq;
                }
                const bool u = use[k];                                /* a row that is not used adds nothing */
                acc[0] = u ? acc[0] + r * r : acc[0];
                int at = 6;
#pragma unroll
                for (int g = 0; g < 5; g++) {
                    acc[1 + g] = u ? acc[1 + g] + J[g] * r : acc[1 + g];
#pragma unroll
                    for (int l = g; l < 5; l++, at++) acc[at] = u ? acc[at] + J[g] * J[l] : acc[at];
                }
            }
        }
    }
    if constexpr (!RESID) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int k = 0; k < PR_NS; k++) acc[k] = acc[k] + __shfl_down(acc[k], m, 64);          /* lanes >= m hold what nobody reads */
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < PR_NS; k++) S->part[wv][k] = acc[k];
            S->cnt[wv] = cnt;
        }
    }
}

__global__ __launch_bounds__(PR_T) void pr_refine_kernel(pr_args a)
{
    __shared__ pr_shared S;
    const int tid = threadIdx.x;
    for (int p = (int)blockIdx.x; p < a.K; p += (int)gridDim.x) {
        const int64_t b = a.off[p], e = a.off[p + 1];
        const bool whole = b >= 0 && b <= e && e <= a.cap;
        const int n = whole ? (int)(e - b) : 0;
        double mine = 0.0;
        if (tid < 12) mine = a.pose[12 * (size_t)p + tid];            /* read before pose_out, which may be the same array, is written */
        __syncthreads();                                              /* the previous entry's epilogue has read S */
        if (tid < 12) S.tri[tid] = mine;
        __syncthreads();
        if (tid == 0) {
            int st = MI_DEGENSAC_REFINE_TRUNCATED;
            if (whole) {
                st = MI_DEGENSAC_REFINE_BAD_CAMERA;
                if (mi_pose_cameras(a.cams, a.n_cams, a.cam_idx, p, S.cam)) {
                    bool fin = true;
#pragma unroll
                    for (int i = 0; i < 12; i++) fin = fin && mi_finite(S.tri[i]);
                    const double tt = (S.tri[9] * S.tri[9] + S.tri[10] * S.tri[10]) + S.tri[11] * S.tri[11];
                    st = MI_DEGENSAC_REFINE_BAD_POSE;
                    if (fin && tt > 0.0) { st = PR_RUNNING; pr_model(&S, S.tri); }
                }
            }
            S.status = st; S.trials = 0; S.accepted = 0; S.lambda = 1e-3; S.cost0 = mi_nan(); S.go = 0;
        }
        __syncthreads();
        int used = 0;
        if (S.status == PR_RUNNING) {                                 /* (uniform: every thread reads the same word) */
            pr_pass<false>(&S, a, b, n);
            __syncthreads();
            used = ((S.cnt[0] + S.cnt[1]) + S.cnt[2]) + S.cnt[3];
            if (tid == 0) {
                const double c0 = pr_sum(&S, 0);
#pragma unroll
                for (int i = 0; i < 18; i++) S.cur[i] = S.tri[i];
                if (used < 5) S.status = MI_DEGENSAC_REFINE_SHORT;
                else if (!mi_finite(c0)) S.status = MI_DEGENSAC_REFINE_NOT_FINITE;
                else {
#pragma unroll
                    for (int k = 0; k < PR_NS; k++) S.sum[k] = pr_sum(&S, k);
                    S.cost0 = c0;
                    S.go = pr_next(&S, a.max_trials);
                }
            }
            __syncthreads();
            while (S.go) {
                pr_pass<false>(&S, a, b, n);
                __syncthreads();
                if (tid == 0) S.go = pr_judge(&S, a.ftol) ? pr_next(&S, a.max_trials) : 0;
                __syncthreads();
            }
        }
        const int status = S.status;
        const bool ran = status <= MI_DEGENSAC_REFINE_MAX_TRIALS;     /* CONVERGED, STALLED, MAX_TRIALS */
        const bool posed = ran || status == MI_DEGENSAC_REFINE_SHORT || status == MI_DEGENSAC_REFINE_NOT_FINITE;
        if (posed && (a.F || (ran && a.resid))) {                     /* E of the final pose: S.M may hold a rejected trial's */
            if (tid == 0) {
                pr_essential(&S, S.cur);
                double H[9];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    H[3 * i] = S.M[0][3 * i] / S.cam[0]; H[3 * i + 1] = S.M[0][3 * i + 1] / S.cam[1];
                    H[3 * i + 2] = (S.M[0][3 * i + 2] - H[3 * i] * S.cam[2]) - H[3 * i + 1] * S.cam[3];
                }
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const double f0 = H[j] / S.cam[4], f1 = H[3 + j] / S.cam[5];
                    S.Fm[j] = f0; S.Fm[3 + j] = f1; S.Fm[6 + j] = (H[6 + j] - f0 * S.cam[6]) - f1 * S.cam[7];
                }
            }
            __syncthreads();
            if (ran && a.resid) pr_pass<true>(&S, a, b, n);
        }
        if (tid < 12) a.pose_out[12 * (size_t)p + tid] = status == MI_DEGENSAC_REFINE_BAD_POSE ? 0.0 : posed ? S.cur[tid] : mine;
        if (a.F && tid < 9) a.F[9 * (size_t)p + tid] = posed ? S.Fm[tid] : 0.0;
        if (tid == 0) {
            a.cost[2 * (size_t)p] = ran ? S.cost0 : mi_nan(); a.cost[2 * (size_t)p + 1] = ran ? S.sum[0] : mi_nan();
            int32_t *o = a.info + 4 * (size_t)p;
            o[0] = posed ? used : 0; o[1] = ran ? S.trials : 0; o[2] = ran ? S.accepted : 0; o[3] = status;
        }
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_pose_refine_tile(int which) { return which == 0 ? PR_STEP : which == 1 ? PR_GRID : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int pr_check(const void *pts, const void *off, const void *pose, const void *cams, int n_cams, int K, int64_t cap, int max_trials, double ftol,
                    const void *pose_out, const void *cost, const void *info)
{
    if (K < 0) return mi_einval("n_entries < 0");
    if (cap < 0) return mi_einval("cap < 0");
    if (cap > 0x3fffffff) return mi_einval("too many rows in one list (cap > 0x3fffffff)");
    if (n_cams < 0) return mi_einval("n_cams < 0");
    if (max_trials < 0 || max_trials > 100) return mi_einval("max_trials should lie in 0 .. 100");
    if (!(ftol >= 0.0)) return mi_einval("ftol should be a number >= 0");
    if (!off) return mi_einval("NULL argument: corr_offsets");
    if (K > 0 && (!pose || !cams)) return mi_einval("NULL argument: pose and cams");
    if (K > 0 && (!pose_out || !cost || !info)) return mi_einval("NULL argument: pose_out, cost and info");
    if (cap > 0 && !pts) return mi_einval("NULL argument: pts");
    return 0;
}

extern "C" int mi_degensac_pose_refine_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep, const double *d_pose,
                                                 const double *d_cams, int n_cams, const int32_t *d_cam_idx, int n_entries, int64_t cap,
                                                 int max_trials, double ftol, int device, void *stream, double *d_pose_out, double *d_cost,
                                                 int32_t *d_info, double *d_resid, double *d_F)
{
    int rc = pr_check(d_pts, d_corr_offsets, d_pose, d_cams, n_cams, n_entries, cap, max_trials, ftol, d_pose_out, d_cost, d_info); if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (cap > 0 && d_resid) MICHK(hipMemsetAsync(d_resid, 0xff, (size_t)cap * 8, s));      /* all bits set: a NaN where no used row is written */
    if (n_entries == 0) return 0;
    pr_args a;
    memset(&a, 0, sizeof a);
    a.pts = d_pts; a.off = d_corr_offsets; a.keep = d_keep; a.pose = d_pose; a.cams = d_cams; a.cam_idx = d_cam_idx; a.pose_out = d_pose_out;
    a.cost = d_cost; a.info = d_info; a.resid = d_resid; a.F = d_F;
    a.K = n_entries; a.n_cams = n_cams; a.cap = cap; a.max_trials = max_trials; a.ftol = ftol;
    const dim3 grid((unsigned)std::min(n_entries, PR_GRID)), block(PR_T);
    hipLaunchKernelGGL(pr_refine_kernel, grid, block, 0, s, a);
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_pose_refine_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep, const double *pose,
                                             const double *cams, int n_cams, const int32_t *cam_idx, int n_entries, int64_t cap, int max_trials,
                                             double ftol, int device, double *pose_out, double *cost, int32_t *info, double *resid, double *F)
{
    int rc = pr_check(pts, corr_offsets, pose, cams, n_cams, n_entries, cap, max_trials, ftol, pose_out, cost, info); if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t K = (size_t)n_entries, C = (size_t)cap, NC = (size_t)n_cams;
    MiStage st;
    const int i_pts = st.in(pts, C * 32), i_off = st.in(corr_offsets, (K + 1) * 8), i_keep = st.in(keep, C), i_pose = st.in(pose, K * 96),
              i_cams = st.in(cams, NC * 32), i_idx = st.in(cam_idx, K * 8), o_pose = st.out(pose_out, K * 96), o_cost = st.out(cost, K * 16),
              o_info = st.out(info, K * 16), o_res = st.out(resid, C * 8), o_F = st.out(F, K * 72);
    rc = st.upload(); if (rc) return rc;
    rc = mi_degensac_pose_refine_lists_dev(st.dev<double>(i_pts), st.dev<int64_t>(i_off), st.dev<uint8_t>(i_keep), st.dev<double>(i_pose),
                                           st.dev<double>(i_cams), n_cams, st.dev<int32_t>(i_idx), n_entries, cap, max_trials, ftol, device, nullptr,
                                           st.dev<double>(o_pose), st.dev<double>(o_cost), st.dev<int32_t>(o_info), st.dev<double>(o_res),
                                           st.dev<double>(o_F));
    if (rc) return rc;
    return st.finish();
}
