/* Host code that the two pose calls share (mi_pose.hip from F, mi_pose_h.hip from H): the refusals of include/mi_degensac.h, the device
 * entry (guard, fills, arguments, launch) and the staged entry on host pointers.  A call from F passes mi_pose_extras() for what only the
 * call from H has. */
#ifndef MI_POSE_HOST_H
#define MI_POSE_HOST_H
#include <string.h>
#include <algorithm>
#include "mi_host.h"
#include "mi_pose_dev.h"

typedef void (*mi_pose_kernel_t)(mi_pose_args);

struct mi_pose_extras {           /* of the call from H; from_h false: none of them is looked at */
    bool from_h = false;
    double rot_eps = 0.0;
    double *normal = nullptr, *tod = nullptr, *cand_normal = nullptr;
};

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static inline int mi_pose_check(const void *pts, const void *off, const void *M, const void *cams, int n_cams, int K, int64_t cap, double cos_min,
                                const void *pose, const void *front, const void *info, const mi_pose_extras &x)
{
    if (K < 0) return mi_einval("n_entries < 0");
    if (cap < 0) return mi_einval("cap < 0");
    if (cap > 0x3fffffff) return mi_einval("too many rows in one list (cap > 0x3fffffff)");
    if (n_cams < 0) return mi_einval("n_cams < 0");
    if (!(cos_min >= -1.0 && cos_min <= 1.0)) return mi_einval("cos_min should lie in [-1, 1]");
    if (x.from_h && !(x.rot_eps >= 0.0)) return mi_einval("rotation_eps should be >= 0 (and not NaN)");
    if (!off) return mi_einval("NULL argument: corr_offsets");
    if (K > 0 && (!M || !cams)) return mi_einval(x.from_h ? "NULL argument: H and cams" : "NULL argument: F and cams");
    if (K > 0 && (!pose || !info || (x.from_h && (!x.normal || !x.tod))))
        return mi_einval(x.from_h ? "NULL argument: pose, info, normal and t_over_d" : "NULL argument: pose and info");
    if (cap > 0 && (!pts || !front)) return mi_einval("NULL argument: pts and front");
    return 0;
}

static inline int mi_pose_dev(mi_pose_kernel_t kernel, const double *d_pts, const int64_t *d_off, const uint8_t *d_keep, const double *d_M,
                              const double *d_cams, int n_cams, const int32_t *d_cam_idx, int n_entries, int64_t cap, double cos_min, int device,
                              void *stream, double *d_pose, uint8_t *d_front, int32_t *d_info, double *d_X, double *d_depth, double *d_cosang,
                              double *d_cand, int32_t *d_cand_front, const mi_pose_extras &x)
{
    int rc = mi_pose_check(d_pts, d_off, d_M, d_cams, n_cams, n_entries, cap, cos_min, d_pose, d_front, d_info, x); if (rc) return rc;
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
    mi_pose_args a;
    memset(&a, 0, sizeof a);
    a.pts = d_pts; a.off = d_off; a.keep = d_keep; a.M = d_M; a.cams = d_cams; a.cam_idx = d_cam_idx; a.pose = d_pose; a.front = d_front;
    a.info = d_info; a.normal = x.normal; a.tod = x.tod; a.X = d_X; a.depth = d_depth; a.cosang = d_cosang; a.cand = d_cand;
    a.cand_normal = x.cand_normal; a.cand_front = d_cand_front;
    a.K = n_entries; a.n_cams = n_cams; a.cap = cap; a.cos_min = cos_min; a.rot_eps = x.rot_eps;
    const dim3 grid((unsigned)std::min(n_entries, MI_POSE_GRID)), block(MI_POSE_T);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
    MICHK(hipGetLastError());
    return 0;
}

/* the same on host pointers (blocking): the inputs go to the device once, every output that is asked for comes back whole */
static inline int mi_pose_staged(mi_pose_kernel_t kernel, const double *pts, const int64_t *corr_offsets, const uint8_t *keep, const double *M,
                                 const double *cams, int n_cams, const int32_t *cam_idx, int n_entries, int64_t cap, double cos_min, int device,
                                 double *pose, uint8_t *front, int32_t *info, double *X, double *depth, double *cosang, double *cand,
                                 int32_t *cand_front, const mi_pose_extras &x)
{
    int rc = mi_pose_check(pts, corr_offsets, M, cams, n_cams, n_entries, cap, cos_min, pose, front, info, x); if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t K = (size_t)n_entries, C = (size_t)cap, NC = (size_t)n_cams;
    MiStage st;
    const int i_pts = st.in(pts, C * 32), i_off = st.in(corr_offsets, (K + 1) * 8), i_keep = st.in(keep, C), i_M = st.in(M, K * 72),
              i_cams = st.in(cams, NC * 32), i_idx = st.in(cam_idx, K * 8), o_pose = st.out(pose, K * 96), o_front = st.out(front, C),
              o_info = st.out(info, K * 20), o_nrm = st.out(x.normal, K * 24), o_tod = st.out(x.tod, K * 8), o_X = st.out(X, C * 24),
              o_depth = st.out(depth, C * 16), o_cos = st.out(cosang, C * 8), o_cand = st.out(cand, K * 384), o_cn = st.out(x.cand_normal, K * 96),
              o_cf = st.out(cand_front, K * 16);
    rc = st.upload(); if (rc) return rc;
    mi_pose_extras d = x;
    d.normal = st.dev<double>(o_nrm); d.tod = st.dev<double>(o_tod); d.cand_normal = st.dev<double>(o_cn);
    rc = mi_pose_dev(kernel, st.dev<double>(i_pts), st.dev<int64_t>(i_off), st.dev<uint8_t>(i_keep), st.dev<double>(i_M), st.dev<double>(i_cams),
                     n_cams, st.dev<int32_t>(i_idx), n_entries, cap, cos_min, device, nullptr, st.dev<double>(o_pose), st.dev<uint8_t>(o_front),
                     st.dev<int32_t>(o_info), st.dev<double>(o_X), st.dev<double>(o_depth), st.dev<double>(o_cos), st.dev<double>(o_cand),
                     st.dev<int32_t>(o_cf), d);
    if (rc) return rc;
    return st.finish();
}
#endif /* MI_POSE_HOST_H */
