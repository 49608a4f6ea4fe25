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
 *   counting pass  MI_POSE_STEP = 1024 rows per step, four per thread, 256 consecutive 32-byte rows per load instruction of the workgroup; both
 *                  rotations, the four centres and the eight camera numbers in registers; per load and candidate one wave ballot whose
 *                  popcount is added to a wave-uniform register; the waves' sums meet in 4 x 5 LDS words after the last step.
 *   output pass    the same steps under the chosen candidate only: front, X, depth, cosang of the used rows, the wide count likewise.
 * Integer counts only cross threads, so every output is the same bits on every call.
 *
 * This file holds what is the F call's own: the candidates of E behind the singular value decomposition, its model policy and its
 * entries.  The decomposition, the row rule, the passes and the entry loop are mi_pose_dev.h's, the host path is mi_pose_host.h's; both
 * are shared with mi_pose_h.hip. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_pose_host.h"

struct ps_model;
typedef mi_pose_shared<ps_model> ps_shared;

__device__ __forceinline__ int ps_decompose(ps_shared *S, const double *F);

struct ps_model {
    struct extra {};
    static constexpr bool ROTATION = false;
    /* slots 0, 1 hold Ra and slots 2, 3 Rb */
    static __device__ __forceinline__ constexpr int rot_slot(int h) { return 2 * h; }
    static __device__ __forceinline__ constexpr int rot_of(int q) { return q >> 1; }
    template <int NR> struct side {
        __device__ __forceinline__ void load(const ps_shared *, int, int) {}
        __device__ __forceinline__ bool vis(int, bool, double, double) const { return true; }
    };
    static __device__ __forceinline__ int decompose(ps_shared *S, const double *F, const mi_pose_args &) { return ps_decompose(S, F); }
    static __device__ __forceinline__ void epilogue(const ps_shared *, const mi_pose_args &, int, bool, bool, int) {}
};

/* the candidates of F under the two cameras of S->cam (focal lengths finite and not zero) into S->cand / S->c2 (one thread); returns the
 * status */
__device__ __forceinline__ int ps_decompose(ps_shared *S, const double *F)
{
    const double fx1 = S->cam[0], fy1 = S->cam[1], cx1 = S->cam[2], cy1 = S->cam[3], fx2 = S->cam[4], fy2 = S->cam[5], cx2 = S->cam[6], cy2 = S->cam[7];
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
    double v0[3], v1[3], v2[3], b0[3], b1[3], b2[3], sg[3];
    mi_jacobi_svd3(A, v0, v1, v2, b0, b1, b2, sg);
    const double s0 = sg[0], s1 = sg[1];
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
        const double det = mi_det3(R);
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


__global__ __launch_bounds__(MI_POSE_T) void ps_pose_kernel(mi_pose_args a) { mi_pose_entries<ps_model>(a); }

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_pose_tile(int which) { return which == 0 ? MI_POSE_STEP : which == 1 ? MI_POSE_GRID : -1; }

extern "C" int mi_degensac_pose_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep, const double *d_F,
                                          const double *d_cams, int n_cams, const int32_t *d_cam_idx, int n_entries, int64_t cap, double cos_min,
                                          int device, void *stream, double *d_pose, uint8_t *d_front, int32_t *d_info, double *d_X, double *d_depth,
                                          double *d_cosang, double *d_cand, int32_t *d_cand_front)
{
    return mi_pose_dev(ps_pose_kernel, d_pts, d_corr_offsets, d_keep, d_F, d_cams, n_cams, d_cam_idx, n_entries, cap, cos_min, device, stream, d_pose,
                       d_front, d_info, d_X, d_depth, d_cosang, d_cand, d_cand_front, mi_pose_extras());
}

extern "C" int mi_degensac_pose_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep, const double *F, const double *cams,
                                      int n_cams, const int32_t *cam_idx, int n_entries, int64_t cap, double cos_min, int device, double *pose,
                                      uint8_t *front, int32_t *info, double *X, double *depth, double *cosang, double *cand, int32_t *cand_front)
{
    return mi_pose_staged(ps_pose_kernel, pts, corr_offsets, keep, F, cams, n_cams, cam_idx, n_entries, cap, cos_min, device, pose, front, info, X,
                          depth, cosang, cand, cand_front, mi_pose_extras());
}
