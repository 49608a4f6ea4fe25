/* libmi_degensac.so — relative pose and triangulation on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_lists*):
 * per entry of a compact list (pts [cap, 4] and corr_offsets [K + 1] as the correspondence export writes them, both on the device) the
 * essential matrix of its F under two pinhole cameras, its four (R, t) candidates, the rows each candidate triangulates in front of both
 * cameras, the candidate with the most of them, and per row of that candidate the midpoint, the two depths and the parallax.
 * gfx950 only, no CPU path.
 *
 * One workgroup of 256 threads per entry, further entries by a grid stride; no workgroup waits for another, no atomics.  The kernel reads
 * its row range o[p], o[p + 1] itself, so the host never learns a length and the call has no synchronisation.
 *   decomposition  thread 0: E, its singular value decomposition by six sweeps of one-sided Jacobi rotations, the four candidates and
 *                  their camera-2 centres into LDS; about a thousand flops, once per entry.
 *   counting pass  PS_STEP = 1024 rows per step, four per thread, 256 consecutive 32-byte rows per load instruction of the workgroup; both
 *                  rotations, the four centres and the eight camera numbers in registers; per load and candidate one wave ballot whose
 *                  popcount is added to a wave-uniform register; the waves' sums meet in 4 x 5 LDS words after the last step.
 *   output pass    the same steps under the chosen candidate only: front, X, depth, cosang of the used rows, the wide count likewise.
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

#define PS_T     256                      /* threads per workgroup */
#define PS_NW    (PS_T / 64)
#define PS_LOADS 4                        /* rows per thread and step */
#define PS_STEP  (PS_LOADS * PS_T)        /* rows per workgroup and step */
#define PS_GRID  256                      /* cap on the grid: further entries by the grid stride */
#define PS_SWEEPS 6                       /* one-sided Jacobi sweeps of the 3 x 3 decomposition */

struct ps_args {
    const double *pts;            /* [cap, 4] */
    const int64_t *off;           /* [K + 1] */
    const uint8_t *keep;          /* [cap] or null */
    const double *F;              /* [K * 9] */
    const double *cams;           /* [n_cams, 4] */
    const int32_t *cam_idx;       /* [K, 2] or null */
    double *pose;                 /* [K, 12] */
    uint8_t *front;               /* [cap] */
    int32_t *info;                /* [K, 5] */
    double *X, *depth, *cosang;   /* [cap, 3], [cap, 2], [cap] or null */
    double *cand;                 /* [K, 4, 12] or null */
    int32_t *cand_front;          /* [K, 4] or null */
    int K, n_cams; int64_t cap;
    double cos_min;
};

struct ps_shared {
    double cand[4][12];           /* R row-major, t */
    double c2[4][3];              /* -R^T t */
    double cam[8];                /* fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2 */
    int status;
    int cnt[PS_NW][5];
};

/* the candidates of F under the two cameras of S->cam into S->cand / S->c2 (one thread); returns the status */
__device__ __forceinline__ int ps_decompose(ps_shared *S, const double *F)
{
    const double fx1 = S->cam[0], fy1 = S->cam[1], cx1 = S->cam[2], cy1 = S->cam[3], fx2 = S->cam[4], fy2 = S->cam[5], cx2 = S->cam[6], cy2 = S->cam[7];
    if (!(mi_finite(fx1) && mi_finite(fy1) && mi_finite(fx2) && mi_finite(fy2)) || fx1 == 0.0 || fy1 == 0.0 || fx2 == 0.0 || fy2 == 0.0)
        return MI_DEGENSAC_POSE_BAD_CAMERA;
    double G[9], E[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {                                     /* G = F K1 */
        G[3 * i] = F[3 * i] * fx1; G[3 * i + 1] = F[3 * i + 1] * fy1;
        G[3 * i + 2] = (F[3 * i] * cx1 + F[3 * i + 1] * cy1) + F[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {                                     /* E = K2^T G */
        E[j] = fx2 * G[j]; E[3 + j] = fy2 * G[3 + j];
        E[6 + j] = (cx2 * G[j] + cy2 * G[3 + j]) + G[6 + j];
    }
    double m = 0.0; bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; i++) { const double x = fabs(E[i]); fin = fin && x <= MI_DBL_MAX; if (x > m) m = x; }
    if (!fin || !(m > 0.0)) return MI_DEGENSAC_POSE_BAD_MODEL;
    double A[9];
#pragma unroll
    for (int i = 0; i < 9; i++) A[i] = E[i] / m;
    /* The singular value decomposition by one-sided Jacobi rotations from V = I, B = A: PS_SWEEPS sweeps over the column pairs (0 1) (0 2)
     * (1 2), each rotation applied to B and V alike, so V stays orthogonal to rounding whatever A is and B = A V throughout; afterwards the
     * columns of B are orthogonal, sigma_i = |b_i| and u_i = b_i / sigma_i.  On 100000 matrices of each class (general, rank 2, rank 2
     * with sigma2 / sigma1 down to 1e-8, sigma1 == sigma2, sigma1 ~ sigma2 of rank 2 and of rank 3 by a hair), scaled like A, three
     * sweeps leave up to 3e-5 between two columns of B, four leave 7e-16 and sigma within 2e-15 of LAPACK's; PS_SWEEPS has two to spare.
     * (dg_svd3_right, the reference's 3 x 3 routine of the DEGENSAC branch, is not used: its V is not orthogonal on every input and
     * its d are not the singular values when sigma1 ~ sigma2.) */
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    double b0[3] = {A[0], A[3], A[6]}, b1[3] = {A[1], A[4], A[7]}, b2[3] = {A[2], A[5], A[8]};
#define PS_DOT(x, y) ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2])
#define PS_ROT(bi, vi, bj, vj) { const double al_ = PS_DOT(bi, bi), be_ = PS_DOT(bj, bj), ga_ = PS_DOT(bi, bj); \
        if (ga_ != 0.0) { const double z_ = (be_ - al_) / (2.0 * ga_), t_ = (z_ >= 0.0 ? 1.0 : -1.0) / (fabs(z_) + sqrt(1.0 + z_ * z_)), \
                          c_ = 1.0 / sqrt(1.0 + t_ * t_), s_ = c_ * t_; \
            for (int k_ = 0; k_ < 3; k_++) { const double x_ = bi[k_], y_ = bj[k_], p_ = vi[k_], q_ = vj[k_]; \
                bi[k_] = c_ * x_ - s_ * y_; bj[k_] = s_ * x_ + c_ * y_; vi[k_] = c_ * p_ - s_ * q_; vj[k_] = s_ * p_ + c_ * q_; } } }
    for (int sweep = 0; sweep < PS_SWEEPS; sweep++) { PS_ROT(b0, v0, b1, v1) PS_ROT(b0, v0, b2, v2) PS_ROT(b1, v1, b2, v2) }
#undef PS_ROT
    double s0 = sqrt(PS_DOT(b0, b0)), s1 = sqrt(PS_DOT(b1, b1)), s2 = sqrt(PS_DOT(b2, b2));
#undef PS_DOT
    /* sigma descending, ties keep the lower index in front: three compare-exchanges (0 1) (1 2) (0 1) on (sigma, column of V, column of B) */
#define PS_CX(sa, va, ba, sb, vb, bb) if (sb > sa) { double t_ = sa; sa = sb; sb = t_; \
        for (int k_ = 0; k_ < 3; k_++) { t_ = va[k_]; va[k_] = vb[k_]; vb[k_] = t_; t_ = ba[k_]; ba[k_] = bb[k_]; bb[k_] = t_; } }
    PS_CX(s0, v0, b0, s1, v1, b1) PS_CX(s1, v1, b1, s2, v2, b2) PS_CX(s0, v0, b0, s1, v1, b1)
#undef PS_CX
    if (!(s1 > 0.0)) return MI_DEGENSAC_POSE_BAD_MODEL;
    double u1[3], u2[3], t[3];
#pragma unroll
    for (int r = 0; r < 3; r++) { u1[r] = b0[r] / s0; u2[r] = b1[r] / s1; }
    t[0] = u1[1] * u2[2] - u1[2] * u2[1]; t[1] = u1[2] * u2[0] - u1[0] * u2[2]; t[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double nrm = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    t[0] = t[0] / nrm; t[1] = t[1] / nrm; t[2] = t[2] / nrm;
    double Ra[9], Rb[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            Ra[3 * r + c] = (u2[r] * v0[c] - u1[r] * v1[c]) + t[r] * v2[c];
            Rb[3 * r + c] = (u1[r] * v1[c] - u2[r] * v0[c]) + t[r] * v2[c];
        }
    fin = mi_finite(t[0]) && mi_finite(t[1]) && mi_finite(t[2]);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        double *R = h ? Rb : Ra;
        const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
#pragma unroll
        for (int i = 0; i < 9; i++) { if (det < 0.0) R[i] = -R[i]; fin = fin && mi_finite(R[i]); }
    }
    if (!fin) return MI_DEGENSAC_POSE_BAD_MODEL;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double *R = q < 2 ? Ra : Rb; const double sg = (q & 1) ? -1.0 : 1.0;
#pragma unroll
        for (int i = 0; i < 9; i++) S->cand[q][i] = R[i];
        const double tq[3] = {sg * t[0], sg * t[1], sg * t[2]};       /* (a product with +-1 is exact) */
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S->cand[q][9 + j] = tq[j];
            S->c2[q][j] = -((R[j] * tq[0] + R[3 + j] * tq[1]) + R[6 + j] * tq[2]);
        }
    }
    return MI_DEGENSAC_POSE_OK;
}

/* the midpoint rule of one row under (R, c2): lambda1, lambda2, cosang and, with WITH_X, the midpoint */
template <bool WITH_X>
__device__ __forceinline__ void ps_row(const double *R, const double *c2, double d1x, double d1y, double d2x, double d2y, double &l1, double &l2,
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

/* One pass over the n rows at b0.  FINAL = false: out[0] = used rows, out[1 + q] = front rows of candidate q.  FINAL = true: the outputs
 * of the used rows under candidate `chosen`, out[0] = wide rows.  All threads of the workgroup, uniform control flow. */
template <bool FINAL>
__device__ __forceinline__ void ps_pass(ps_shared *S, const ps_args &a, int64_t b0, int n, int chosen, int *out)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NR = FINAL ? 1 : 2, NC = FINAL ? 1 : 4, NCNT = FINAL ? 1 : 5;
    double R[NR][9], c2[NC][3], cam[8];
#pragma unroll
    for (int i = 0; i < 8; i++) cam[i] = S->cam[i];
#pragma unroll
    for (int h = 0; h < NR; h++)
#pragma unroll
        for (int i = 0; i < 9; i++) R[h][i] = S->cand[FINAL ? chosen : 2 * h][i];
#pragma unroll
    for (int q = 0; q < NC; q++)
#pragma unroll
        for (int j = 0; j < 3; j++) c2[q][j] = S->c2[FINAL ? chosen : q][j];
    const __attribute__((address_space(1))) double *G = (const __attribute__((address_space(1))) double *)(a.pts + 4 * (size_t)b0);
    int cnt[NCNT];
#pragma unroll
    for (int k = 0; k < NCNT; k++) cnt[k] = 0;
    for (int base = 0; base < n; base += PS_STEP) {
        double p[PS_LOADS][4]; bool use[PS_LOADS];
#pragma unroll
        for (int k = 0; k < PS_LOADS; k++) {                          /* the step's loads back to back; a row past the end reads row n - 1 */
            const int i = base + k * PS_T + tid, j = i < n ? i : n - 1;
#pragma unroll
            for (int c = 0; c < 4; c++) p[k][c] = G[4 * (size_t)j + c];
            use[k] = i < n && (a.keep == nullptr || a.keep[b0 + j] != 0);
        }
#pragma unroll
        for (int k = 0; k < PS_LOADS; k++) {
            const int i = base + k * PS_T + tid;
            const double d1x = (p[k][0] - cam[2]) / cam[0], d1y = (p[k][1] - cam[3]) / cam[1];
            const double d2x = (p[k][2] - cam[6]) / cam[4], d2y = (p[k][3] - cam[7]) / cam[5];
            if constexpr (!FINAL) {
                cnt[0] += __popcll(__ballot(use[k]));
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    double l1, l2, cs;
                    ps_row<false>(R[q >> 1], c2[q], d1x, d1y, d2x, d2y, l1, l2, cs, nullptr);
                    cnt[1 + q] += __popcll(__ballot(use[k] && l1 > 0.0 && l2 > 0.0));      /* a NaN is not front */
                }
            } else {
                double l1, l2, cs, X[3];
                ps_row<true>(R[0], c2[0], d1x, d1y, d2x, d2y, l1, l2, cs, X);
                const bool fr = use[k] && l1 > 0.0 && l2 > 0.0;
                cnt[0] += __popcll(__ballot(fr && cs <= a.cos_min));
                if (use[k]) {
                    const size_t g = (size_t)b0 + (size_t)i;
                    a.front[g] = fr ? 1 : 0;
                    if (a.X) { a.X[3 * g] = X[0]; a.X[3 * g + 1] = X[1]; a.X[3 * g + 2] = X[2]; }
                    if (a.depth) { a.depth[2 * g] = l1; a.depth[2 * g + 1] = l2; }
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
        for (int w = 0; w < PS_NW; w++) s += S->cnt[w][k];
        out[k] = s;
    }
}

__global__ __launch_bounds__(PS_T) void ps_pose_kernel(ps_args a)
{
    __shared__ ps_shared S;
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
                    double F[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) F[i] = a.F[9 * (size_t)p + i];
                    st = ps_decompose(&S, F);
                }
            }
            S.status = st;
        }
        __syncthreads();
        int status = S.status, used = 0, chosen = 0, best = 0, second = 0, wide = 0;
        int c[5] = {0, 0, 0, 0, 0};
        const bool model = status == MI_DEGENSAC_POSE_OK;             /* the candidates stand in LDS */
        if (model) {
            const int n = (int)(e - b);
            if (n > 0) ps_pass<false>(&S, a, b, n, 0, c);
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
                ps_pass<true>(&S, a, b, n, chosen, w1);
                wide = w1[0];
            }
        }
        const bool ok = status == MI_DEGENSAC_POSE_OK;
        if (tid < 12) a.pose[12 * (size_t)p + tid] = ok ? S.cand[chosen][tid] : 0.0;
        if (a.cand && tid < 48) a.cand[48 * (size_t)p + tid] = model ? S.cand[tid / 12][tid % 12] : 0.0;
        if (a.cand_front && tid < 4) a.cand_front[4 * (size_t)p + tid] = ok ? c[1 + tid] : 0;
        if (tid == 0) {
            int32_t *o = a.info + 5 * (size_t)p;
            o[0] = ok ? used : 0; o[1] = ok ? best : 0; o[2] = ok ? second : 0; o[3] = ok ? wide : 0; o[4] = status;
        }
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_pose_tile(int which) { return which == 0 ? PS_STEP : which == 1 ? PS_GRID : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int ps_check(const void *pts, const void *off, const void *F, const void *cams, int n_cams, int K, int64_t cap, double cos_min, const void *pose,
                    const void *front, const void *info)
{
    if (K < 0) return mi_einval("n_entries < 0");
    if (cap < 0) return mi_einval("cap < 0");
    if (cap > 0x3fffffff) return mi_einval("too many rows in one list (cap > 0x3fffffff)");
    if (n_cams < 0) return mi_einval("n_cams < 0");
    if (!(cos_min >= -1.0 && cos_min <= 1.0)) return mi_einval("cos_min should lie in [-1, 1]");
    if (!off) return mi_einval("NULL argument: corr_offsets");
    if (K > 0 && (!F || !cams)) return mi_einval("NULL argument: F and cams");
    if (K > 0 && (!pose || !info)) return mi_einval("NULL argument: pose and info");
    if (cap > 0 && (!pts || !front)) return mi_einval("NULL argument: pts and front");
    return 0;
}

extern "C" int mi_degensac_pose_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep, const double *d_F,
                                          const double *d_cams, int n_cams, const int32_t *d_cam_idx, int n_entries, int64_t cap, double cos_min,
                                          int device, void *stream, double *d_pose, uint8_t *d_front, int32_t *d_info, double *d_X, double *d_depth,
                                          double *d_cosang, double *d_cand, int32_t *d_cand_front)
{
    int rc = ps_check(d_pts, d_corr_offsets, d_F, d_cams, n_cams, n_entries, cap, cos_min, d_pose, d_front, d_info); if (rc) return rc;
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
    ps_args a;
    memset(&a, 0, sizeof a);
    a.pts = d_pts; a.off = d_corr_offsets; a.keep = d_keep; a.F = d_F; a.cams = d_cams; a.cam_idx = d_cam_idx; a.pose = d_pose; a.front = d_front;
    a.info = d_info; a.X = d_X; a.depth = d_depth; a.cosang = d_cosang; a.cand = d_cand; a.cand_front = d_cand_front;
    a.K = n_entries; a.n_cams = n_cams; a.cap = cap; a.cos_min = cos_min;
    const dim3 grid((unsigned)std::min(n_entries, PS_GRID)), block(PS_T);
    hipLaunchKernelGGL(ps_pose_kernel, grid, block, 0, s, a);
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_pose_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep, const double *F, const double *cams,
                                      int n_cams, const int32_t *cam_idx, int n_entries, int64_t cap, double cos_min, int device, double *pose,
                                      uint8_t *front, int32_t *info, double *X, double *depth, double *cosang, double *cand, int32_t *cand_front)
{
    int rc = ps_check(pts, corr_offsets, F, cams, n_cams, n_entries, cap, cos_min, pose, front, info); if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t K = (size_t)n_entries, C = (size_t)cap, NC = (size_t)n_cams;
    MiStage st;
    const int i_pts = st.in(pts, C * 32), i_off = st.in(corr_offsets, (K + 1) * 8), i_keep = st.in(keep, C), i_F = st.in(F, K * 72),
              i_cams = st.in(cams, NC * 32), i_idx = st.in(cam_idx, K * 8), o_pose = st.out(pose, K * 96), o_front = st.out(front, C),
              o_info = st.out(info, K * 20), o_X = st.out(X, C * 24), o_depth = st.out(depth, C * 16), o_cos = st.out(cosang, C * 8),
              o_cand = st.out(cand, K * 384), o_cf = st.out(cand_front, K * 16);
    rc = st.upload(); if (rc) return rc;
    rc = mi_degensac_pose_lists_dev(st.dev<double>(i_pts), st.dev<int64_t>(i_off), st.dev<uint8_t>(i_keep), st.dev<double>(i_F), st.dev<double>(i_cams),
                                    n_cams, st.dev<int32_t>(i_idx), n_entries, cap, cos_min, device, nullptr, st.dev<double>(o_pose),
                                    st.dev<uint8_t>(o_front), st.dev<int32_t>(o_info), st.dev<double>(o_X), st.dev<double>(o_depth),
                                    st.dev<double>(o_cos), st.dev<double>(o_cand), st.dev<int32_t>(o_cf));
    if (rc) return rc;
    return st.finish();
}
