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
 *   decomposition  thread 0: G, its singular value decomposition by six sweeps of one-sided Jacobi rotations (the rule of the F call),
 *                  the four candidates, their normals and their camera-2 centres into LDS; about a thousand flops, once per entry.
 *   counting pass  MI_POSE_STEP = 1024 rows per step, four per thread, 256 consecutive 32-byte rows per load instruction of the workgroup; both
 *                  rotations, the four centres, both normals and the eight camera numbers in registers; per load and candidate one wave
 *                  ballot whose popcount is added to a wave-uniform register; the waves' sums meet in 4 x 5 LDS words after the last step.
 *   output pass    the same steps under the chosen candidate only: front, X, depth, cosang of the used rows, the wide count likewise.
 *   rotation       an entry whose G is a rotation has one candidate and one pass: used and front rows counted, front and cosang written.
 * Integer counts only cross threads, so every output is the same bits on every call.
 *
 * This file holds what is the H call's own: the four solutions and the rotation case behind the singular value decomposition, its model
 * policy (normals and t / d in LDS, the plane-side test, the rotation pass, two more outputs) and its entries.  The decomposition, the row
 * rule, the passes and the entry loop are mi_pose_dev.h's, the host path is mi_pose_host.h's; both are shared with mi_pose.hip. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_pose_host.h"

struct ph_model;
struct ph_extra {
    double nrm[4][3];             /* the plane normal in the frame of camera 1 */
    double tod[4];                /* |t / d| */
};
typedef mi_pose_shared<ph_model> ph_shared;

__device__ __forceinline__ int ph_decompose(ph_shared *S, const double *H, double rot_eps);

struct ph_model {
    typedef ph_extra extra;
    static constexpr bool ROTATION = true;
    /* slots 0 and 1 hold the two rotations and normals; 2 and 3 negate t and n */
    static __device__ __forceinline__ constexpr int rot_slot(int h) { return h; }
    static __device__ __forceinline__ constexpr int rot_of(int q) { return q & 1; }
    /* the plane is seen from its visible side: n . d1 > 0 */
    template <int NR> struct side {
        double nr[NR][3];
        __device__ __forceinline__ void load(const ph_shared *S, int h, int slot)
        {
#pragma unroll
            for (int j = 0; j < 3; j++) nr[h][j] = S->nrm[slot][j];
        }
        __device__ __forceinline__ bool vis(int h, bool negated, double d1x, double d1y) const
        {
            const double s = (nr[h][0] * d1x + nr[h][1] * d1y) + nr[h][2];
            return negated ? -s > 0.0 : s > 0.0;
        }
    };
    static __device__ __forceinline__ int decompose(ph_shared *S, const double *H, const mi_pose_args &a) { return ph_decompose(S, H, a.rot_eps); }
    static __device__ __forceinline__ void epilogue(const ph_shared *S, const mi_pose_args &a, int p, bool ok, bool model, int chosen)
    {
        const int tid = threadIdx.x;
        if (tid < 3) a.normal[3 * (size_t)p + tid] = ok ? S->nrm[chosen][tid] : 0.0;
        if (tid == 3) a.tod[p] = ok ? S->tod[chosen] : 0.0;
        if (a.cand_normal && tid < 12) a.cand_normal[12 * (size_t)p + tid] = model ? S->nrm[tid / 3][tid % 3] : 0.0;
    }
};

/* the candidates of H under the two cameras of S->cam (focal lengths finite and not zero) into S->cand / nrm / tod / c2 (one thread);
 * returns the status (OK: four candidates; ROTATION: candidate 0 is (R, 0), the rest zeros; anything else: all zeros) */
__device__ __forceinline__ int ph_decompose(ph_shared *S, const double *H, double rot_eps)
{
    const double fx1 = S->cam[0], fy1 = S->cam[1], cx1 = S->cam[2], cy1 = S->cam[3], fx2 = S->cam[4], fy2 = S->cam[5], cx2 = S->cam[6], cy2 = S->cam[7];
    for (int q = 0; q < 4; q++) {
        for (int i = 0; i < 12; i++) S->cand[q][i] = 0.0;
        for (int j = 0; j < 3; j++) { S->nrm[q][j] = 0.0; S->c2[q][j] = 0.0; }
        S->tod[q] = 0.0;
    }
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
    double v0[3], v1[3], v2[3], b0[3], b1[3], b2[3], sg3[3];
    mi_jacobi_svd3(A, v0, v1, v2, b0, b1, b2, sg3);
    const double s0 = sg3[0], s1 = sg3[1], s2 = sg3[2];
    if (!(s2 > 0.0)) return MI_DEGENSAC_POSE_BAD_MODEL;               /* a homography has full rank */
    const double sg = mi_det3(A) < 0.0 ? -1.0 : 1.0;                   /* both cameras on one side of the plane */
    if (s0 - s2 <= rot_eps * s1) {                                    /* a rotation: R = U V^T */
        double u0[3], u1[3], u2[3], Rm[9];
#pragma unroll
        for (int r = 0; r < 3; r++) { u0[r] = b0[r] / s0; u1[r] = b1[r] / s1; u2[r] = b2[r] / s2; }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) Rm[3 * r + c] = (u0[r] * v0[c] + u1[r] * v1[c]) + u2[r] * v2[c];
        const double det = mi_det3(Rm);
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

__global__ __launch_bounds__(MI_POSE_T) void ph_pose_kernel(mi_pose_args a) { mi_pose_entries<ph_model>(a); }

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_pose_h_tile(int which) { return which == 0 ? MI_POSE_STEP : which == 1 ? MI_POSE_GRID : -1; }

static mi_pose_extras ph_extras(double rotation_eps, double *normal, double *t_over_d, double *cand_normal)
{
    mi_pose_extras x;
    x.from_h = true; x.rot_eps = rotation_eps; x.normal = normal; x.tod = t_over_d; x.cand_normal = cand_normal;
    return x;
}

extern "C" int mi_degensac_pose_h_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep, const double *d_H,
                                            const double *d_cams, int n_cams, const int32_t *d_cam_idx, int n_entries, int64_t cap, double cos_min,
                                            double rotation_eps, int device, void *stream, double *d_pose, uint8_t *d_front, int32_t *d_info,
                                            double *d_normal, double *d_t_over_d, double *d_X, double *d_depth, double *d_cosang, double *d_cand,
                                            double *d_cand_normal, int32_t *d_cand_front)
{
    return mi_pose_dev(ph_pose_kernel, d_pts, d_corr_offsets, d_keep, d_H, d_cams, n_cams, d_cam_idx, n_entries, cap, cos_min, device, stream, d_pose,
                       d_front, d_info, d_X, d_depth, d_cosang, d_cand, d_cand_front, ph_extras(rotation_eps, d_normal, d_t_over_d, d_cand_normal));
}

extern "C" int mi_degensac_pose_h_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep, const double *H, const double *cams,
                                        int n_cams, const int32_t *cam_idx, int n_entries, int64_t cap, double cos_min, double rotation_eps, int device,
                                        double *pose, uint8_t *front, int32_t *info, double *normal, double *t_over_d, double *X, double *depth,
                                        double *cosang, double *cand, double *cand_normal, int32_t *cand_front)
{
    return mi_pose_staged(ph_pose_kernel, pts, corr_offsets, keep, H, cams, n_cams, cam_idx, n_entries, cap, cos_min, device, pose, front, info, X,
                          depth, cosang, cand, cand_front, ph_extras(rotation_eps, normal, t_over_d, cand_normal));
}
