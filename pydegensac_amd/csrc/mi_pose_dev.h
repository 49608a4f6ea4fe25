/* Device code that the pose kernels share (mi_pose.hip from F, mi_pose_h.hip from H; the camera lookup also mi_pose_refine.hip): the
 * camera pair of an entry, the singular value decomposition of a 3 x 3 matrix by one-sided Jacobi rotations, the closed-form midpoint
 * rule of one row, the row pass and the kernel's loop over the entries.  All __forceinline__; every step is one IEEE float64 operation
 * per written operator in the order of include/mi_degensac.h, which tests/pose_ref.py and tests/pose_h_ref.py restate bit for bit.
 *
 * The pass and the entry loop are templates over a model policy P, one struct per kernel:
 *   struct P::extra                     further LDS fields of the model: the base of mi_pose_shared<P> (empty for F)
 *   P::ROTATION                         whether decompose can answer MI_DEGENSAC_POSE_ROTATION (one candidate, one pass)
 *   P::rot_slot(h), P::rot_of(q)        the cand slot of the h-th of the two distinct rotations, and which of them candidate q has
 *   template <int NR> struct P::side    the model's further front test in registers: load(S, h, slot) and
 *                                       vis(h, negated, d1x, d1y) -> bool (constant true for F)
 *   P::decompose(S, M, a)               thread 0: the candidates of the model M [9] under S->cam into S; returns the status
 *   P::epilogue(S, a, p, ok, model, chosen)   the model's further outputs of entry p */
#ifndef MI_POSE_DEV_H
#define MI_POSE_DEV_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/mi_degensac.h"
#include "mi_dev_util.h"

#define MI_POSE_T      256                        /* threads per workgroup */
#define MI_POSE_NW     (MI_POSE_T / 64)
#define MI_POSE_LOADS  4                          /* rows per thread and step */
#define MI_POSE_STEP   (MI_POSE_LOADS * MI_POSE_T) /* rows per workgroup and step */
#define MI_POSE_GRID   256                        /* cap on the grid: further entries by the grid stride */
#define MI_POSE_SWEEPS 6                          /* one-sided Jacobi sweeps of the 3 x 3 decomposition */

struct mi_pose_args {
    const double *pts;            /* [cap, 4] */
    const int64_t *off;           /* [K + 1] */
    const uint8_t *keep;          /* [cap] or null */
    const double *M;              /* [K * 9]: F or H */
    const double *cams;           /* [n_cams, 4] */
    const int32_t *cam_idx;       /* [K, 2] or null */
    double *pose;                 /* [K, 12] */
    uint8_t *front;               /* [cap] */
    int32_t *info;                /* [K, 5] */
    double *normal, *tod;         /* [K, 3], [K] (H only) */
    double *X, *depth, *cosang;   /* [cap, 3], [cap, 2], [cap] or null */
    double *cand, *cand_normal;   /* [K, 4, 12], [K, 4, 3] (H only) or null */
    int32_t *cand_front;          /* [K, 4] or null */
    int K, n_cams; int64_t cap;
    double cos_min, rot_eps;      /* (rot_eps: H only) */
};

template <class P>
struct mi_pose_shared : P::extra {
    double cand[4][12];           /* R row-major, t */
    double c2[4][3];              /* -R^T t */
    double cam[8];                /* fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2 */
    int status;
    int cnt[MI_POSE_NW][5];
};

/* The two cameras of entry p, rows (cam_idx[2 p], cam_idx[2 p + 1]) or (2 p, 2 p + 1) of cams [n_cams, 4], into cam[8].  False, with cam
 * untouched, when a row lies outside the table; false, with cam written, when a focal length is zero or not finite. */
__device__ __forceinline__ bool mi_pose_cameras(const double *cams, int n_cams, const int32_t *cam_idx, int p, double *cam)
{
    const int64_t i1 = cam_idx ? (int64_t)cam_idx[2 * (size_t)p] : 2 * (int64_t)p;
    const int64_t i2 = cam_idx ? (int64_t)cam_idx[2 * (size_t)p + 1] : 2 * (int64_t)p + 1;
    if (i1 < 0 || i1 >= n_cams || i2 < 0 || i2 >= n_cams) return false;
    double cm[8];
#pragma unroll
    for (int i = 0; i < 4; i++) { cm[i] = cams[4 * (size_t)i1 + i]; cm[4 + i] = cams[4 * (size_t)i2 + i]; }
#pragma unroll
    for (int i = 0; i < 8; i++) cam[i] = cm[i];
    return mi_finite(cm[0]) && mi_finite(cm[1]) && mi_finite(cm[4]) && mi_finite(cm[5]) && cm[0] != 0.0 && cm[1] != 0.0 && cm[4] != 0.0 && cm[5] != 0.0;
}

__device__ __forceinline__ double mi_det3(const double *R)
{
    return (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

__device__ __forceinline__ double mi_dot3(const double *x, const double *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

/* one Jacobi rotation of the column pair (bi, bj) of B, applied to (vi, vj) of V alike */
__device__ __forceinline__ void mi_jacobi_rot(double *bi, double *vi, double *bj, double *vj)
{
    const double al = mi_dot3(bi, bi), be = mi_dot3(bj, bj), ga = mi_dot3(bi, bj);
    if (ga != 0.0) {
        const double z = (be - al) / (2.0 * ga), t = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(1.0 + z * z)), c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double x = bi[k], y = bj[k], p = vi[k], q = vj[k];
            bi[k] = c * x - s * y; bj[k] = s * x + c * y; vi[k] = c * p - s * q; vj[k] = s * p + c * q;
        }
    }
}

/* one compare-exchange of the sigma sort on (sigma, column of V, column of B) */
__device__ __forceinline__ void mi_sigma_cx(double &sa, double *va, double *ba, double &sb, double *vb, double *bb)
{
    if (sb > sa) {
        double t = sa; sa = sb; sb = t;
#pragma unroll
        for (int k = 0; k < 3; k++) { t = va[k]; va[k] = vb[k]; vb[k] = t; t = ba[k]; ba[k] = bb[k]; bb[k] = t; }
    }
}

/* The singular value decomposition of A (row-major) by one-sided Jacobi rotations from V = I, B = A: MI_POSE_SWEEPS sweeps over the column
 * pairs (0 1) (0 2) (1 2), each rotation applied to B and V alike, so V stays orthogonal to rounding whatever A is and B = A V throughout;
 * afterwards the columns of B are orthogonal, sigma_i = |b_i| and u_i = b_i / sigma_i.  On 100000 matrices of each class (general, rank 2,
 * rank 2 with sigma2 / sigma1 down to 1e-8, sigma1 == sigma2, sigma1 ~ sigma2 of rank 2 and of rank 3 by a hair), scaled like A, three
 * sweeps leave up to 3e-5 between two columns of B, four leave 7e-16 and sigma within 2e-15 of LAPACK's; MI_POSE_SWEEPS has two to spare.
 * (dg_svd3_right, the reference's 3 x 3 routine of the DEGENSAC branch, is not used: its V is not orthogonal on every input and its d
 * are not the singular values when sigma1 ~ sigma2.)
 * Then sigma descending, ties keep the lower index in front: three compare-exchanges (0 1) (1 2) (0 1).  Columns of V in v0, v1, v2, of B
 * in b0, b1, b2, sigma in s[3]. */
__device__ __forceinline__ void mi_jacobi_svd3(const double *A, double *v0, double *v1, double *v2, double *b0, double *b1, double *b2, double *s)
{
    v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0; v1[0] = 0.0; v1[1] = 1.0; v1[2] = 0.0; v2[0] = 0.0; v2[1] = 0.0; v2[2] = 1.0;
    b0[0] = A[0]; b0[1] = A[3]; b0[2] = A[6]; b1[0] = A[1]; b1[1] = A[4]; b1[2] = A[7]; b2[0] = A[2]; b2[1] = A[5]; b2[2] = A[8];
    for (int sweep = 0; sweep < MI_POSE_SWEEPS; sweep++) { mi_jacobi_rot(b0, v0, b1, v1); mi_jacobi_rot(b0, v0, b2, v2); mi_jacobi_rot(b1, v1, b2, v2); }
    s[0] = sqrt(mi_dot3(b0, b0)); s[1] = sqrt(mi_dot3(b1, b1)); s[2] = sqrt(mi_dot3(b2, b2));
    mi_sigma_cx(s[0], v0, b0, s[1], v1, b1); mi_sigma_cx(s[1], v1, b1, s[2], v2, b2); mi_sigma_cx(s[0], v0, b0, s[1], v1, b1);
}

/* the midpoint rule of one row under (R, c2): lambda1, lambda2, cosang and, with WITH_X, the midpoint */
template <bool WITH_X>
__device__ __forceinline__ void mi_pose_row(const double *R, const double *c2, double d1x, double d1y, double d2x, double d2y, double &l1, double &l2,
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

enum { MI_POSE_COUNT = 0, MI_POSE_FINAL = 1, MI_POSE_ROTPASS = 2 };

/* One pass over the n rows at b0.  COUNT: out[0] = used rows, out[1 + q] = front rows of candidate q.  FINAL: the outputs of the used rows
 * under candidate `chosen`, out[0] = wide rows.  ROTPASS: front and cosang of the used rows under the rotation in candidate 0, out[0] =
 * used rows, out[1] = front rows.  All threads of the workgroup, uniform control flow. */
template <class P, int MODE>
__device__ __forceinline__ void mi_pose_pass(mi_pose_shared<P> *S, const mi_pose_args &a, int64_t b0, int n, int chosen, int *out)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NR = MODE == MI_POSE_COUNT ? 2 : 1, NC = MODE == MI_POSE_COUNT ? 4 : 1, NCNT = MODE == MI_POSE_COUNT ? 5 : MODE == MI_POSE_FINAL ? 1 : 2;
    double R[NR][9], c2[NC][3], cam[8];
    typename P::template side<NR> sd;
#pragma unroll
    for (int i = 0; i < 8; i++) cam[i] = S->cam[i];
#pragma unroll
    for (int h = 0; h < NR; h++) {
        const int slot = MODE == MI_POSE_COUNT ? P::rot_slot(h) : chosen;
#pragma unroll
        for (int i = 0; i < 9; i++) R[h][i] = S->cand[slot][i];
        sd.load(S, h, slot);
    }
#pragma unroll
    for (int q = 0; q < NC; q++)
#pragma unroll
        for (int j = 0; j < 3; j++) c2[q][j] = S->c2[MODE == MI_POSE_COUNT ? q : chosen][j];
    const __attribute__((address_space(1))) double *G = (const __attribute__((address_space(1))) double *)(a.pts + 4 * (size_t)b0);
    int cnt[NCNT];
#pragma unroll
    for (int k = 0; k < NCNT; k++) cnt[k] = 0;
    for (int base = 0; base < n; base += MI_POSE_STEP) {
        double p[MI_POSE_LOADS][4]; bool use[MI_POSE_LOADS];
#pragma unroll
        for (int k = 0; k < MI_POSE_LOADS; k++) {                     /* the step's loads back to back; a row past the end reads row n - 1 */
            const int i = base + k * MI_POSE_T + tid, j = i < n ? i : n - 1;
#pragma unroll
            for (int c = 0; c < 4; c++) p[k][c] = G[4 * (size_t)j + c];
            use[k] = i < n && (a.keep == nullptr || a.keep[b0 + j] != 0);
        }
#pragma unroll
        for (int k = 0; k < MI_POSE_LOADS; k++) {
            const int i = base + k * MI_POSE_T + tid;
            const double d1x = (p[k][0] - cam[2]) / cam[0], d1y = (p[k][1] - cam[3]) / cam[1];
            const double d2x = (p[k][2] - cam[6]) / cam[4], d2y = (p[k][3] - cam[7]) / cam[5];
            if constexpr (MODE == MI_POSE_COUNT) {
                cnt[0] += __popcll(__ballot(use[k]));
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    double l1, l2, cs;
                    mi_pose_row<false>(R[P::rot_of(q)], c2[q], d1x, d1y, d2x, d2y, l1, l2, cs, nullptr);
                    const bool vis = sd.vis(P::rot_of(q), q >= 2, d1x, d1y);
                    cnt[1 + q] += __popcll(__ballot(use[k] && l1 > 0.0 && l2 > 0.0 && vis));      /* a NaN is not front */
                }
            } else if constexpr (MODE == MI_POSE_FINAL) {
                double l1, l2, cs, X[3];
                mi_pose_row<true>(R[0], c2[0], d1x, d1y, d2x, d2y, l1, l2, cs, X);
                const bool fr = use[k] && l1 > 0.0 && l2 > 0.0 && sd.vis(0, false, d1x, d1y);
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
                mi_pose_row<true>(R[0], c2[0], d1x, d1y, d2x, d2y, l1, l2, cs, X);             /* c2 = 0: only cosang is used */
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
        for (int w = 0; w < MI_POSE_NW; w++) s += S->cnt[w][k];
        out[k] = s;
    }
}

/* the body of a pose kernel: the entries of the list by a grid stride, one workgroup of MI_POSE_T threads per entry */
template <class P>
__device__ __forceinline__ void mi_pose_entries(const mi_pose_args &a)
{
    __shared__ mi_pose_shared<P> S;
    const int tid = threadIdx.x;
    for (int p = (int)blockIdx.x; p < a.K; p += (int)gridDim.x) {
        const int64_t b = a.off[p], e = a.off[p + 1];
        const bool whole = b >= 0 && b <= e && e <= a.cap;            /* else a truncated export, or offsets that are not a list */
        __syncthreads();                                              /* the previous entry's epilogue has read S */
        if (tid == 0) {
            int st = MI_DEGENSAC_POSE_TRUNCATED;
            if (whole) {
                st = MI_DEGENSAC_POSE_BAD_CAMERA;
                if (mi_pose_cameras(a.cams, a.n_cams, a.cam_idx, p, S.cam)) {
                    double M[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) M[i] = a.M[9 * (size_t)p + i];
                    st = P::decompose(&S, M, a);
                }
            }
            S.status = st;
        }
        __syncthreads();
        int status = S.status, used = 0, chosen = 0, best = 0, second = 0, wide = 0;
        int c[5] = {0, 0, 0, 0, 0};
        const bool rotation = P::ROTATION && status == MI_DEGENSAC_POSE_ROTATION;
        const bool model = status == MI_DEGENSAC_POSE_OK || rotation;  /* the candidates stand in LDS */
        const int n = (int)(e - b);                                   /* (read under a model only, which a whole range precedes) */
        if (rotation) {
            int r2[2] = {0, 0};
            if (n > 0) mi_pose_pass<P, MI_POSE_ROTPASS>(&S, a, b, n, 0, r2);
            used = r2[0]; best = r2[1]; c[1] = r2[1];
            if (used == 0) status = MI_DEGENSAC_POSE_EMPTY;
        } else if (model) {
            if (n > 0) mi_pose_pass<P, MI_POSE_COUNT>(&S, a, b, n, 0, c);
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
                mi_pose_pass<P, MI_POSE_FINAL>(&S, a, b, n, chosen, w1);
                wide = w1[0];
            }
        }
        const bool ok = status == MI_DEGENSAC_POSE_OK || (P::ROTATION && status == MI_DEGENSAC_POSE_ROTATION);
        if (tid < 12) a.pose[12 * (size_t)p + tid] = ok ? S.cand[chosen][tid] : 0.0;
        P::epilogue(&S, a, p, ok, model, chosen);
        if (a.cand && tid < 48) a.cand[48 * (size_t)p + tid] = model ? S.cand[tid / 12][tid % 12] : 0.0;
        if (a.cand_front && tid < 4) a.cand_front[4 * (size_t)p + tid] = ok ? c[1 + tid] : 0;
        if (tid == 0) {
            int32_t *o = a.info + 5 * (size_t)p;
            o[0] = ok ? used : 0; o[1] = ok ? best : 0; o[2] = ok ? second : 0; o[3] = ok ? wide : 0; o[4] = status;
        }
    }
}
#endif /* MI_POSE_DEV_H */
