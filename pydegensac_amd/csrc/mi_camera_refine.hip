/* libmi_degensac.so — refinement of camera poses against triangulated tracks (include/mi_degensac.h mi_degensac_camera_refine_tracks*):
 * per image a Levenberg-Marquardt refinement of the six degrees of freedom of its world-to-camera pose on the reprojection error, in
 * pixels, of its used observations, the points of the tracks held fixed.  The tables are the track-major ones the tracks call writes
 * (track_offsets, obs, obs_image, n_tracks, all on the device); the call regroups them by image itself.  gfx950 only, no CPU path.
 *   fill, mark  every position gets the sentinel key n_images and itself as the value; then a group of CR_G lanes walks a track (tracks by
 *               a grid stride, the range check of the triangulation) and writes per owned position the key (its image when the
 *               observation is used) and track_of[p];
 *   group       rocprim::radix_sort_pairs of (key, position) over the key bits: stable, so the positions of an image come out ascending
 *               without an atomic;
 *   bounds      img_offsets[m] = the lower bound of m in the sorted keys, one thread per image; the same launch writes img_obs;
 *   refine      one workgroup of 256 threads per image, further images by a grid stride; no workgroup waits for another, no atomics.
 *               row pass: CR_STEP = 512 observations per step, two per thread, their gathers (position -> row and track -> keypoint
 *               and point) issued back to back; the pose and the camera are read from LDS once per pass and held in registers; 28
 *               float64 accumulators per thread.  Inside a wave six shuffle steps, then 4 x 28 LDS words that thread 0 adds in wave
 *               order.  Thread 0 does the 6 x 6 Cholesky solve and the Cayley update between the passes.
 * The order of every sum is fixed by the header, so every output is the same bits on every call. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_host.h"
#include "mi_dev_util.h"

#define CR_T     256                      /* threads per workgroup */
#define CR_NW    (CR_T / 64)
#define CR_LOADS 2                        /* observations per thread and step */
#define CR_STEP  (CR_LOADS * CR_T)        /* observations per workgroup and step */
#define CR_GRID  256                      /* cap on the grid of the refinement: further images by the grid stride */
#define CR_G     16                       /* lanes per track of the mark kernel */
#define CR_MGRID 1024                     /* cap on the grid of the mark kernel */
#define CR_NS    28                       /* sums of a pass: cost, g[6], A[21] */
#define CR_RUNNING (-1)

struct cr_args {
    const int64_t *off;           /* [T + 1] */
    const int32_t *obs, *img;     /* [M] */
    const int64_t *nt;            /* [1] or null */
    const double *kps;            /* [rows, 2] */
    const double *cams;           /* [n_images, 4] */
    const double *poses;          /* [n_images, 12] */
    const double *X;              /* [T, 3] */
    const uint8_t *keep;          /* [M] or null */
    const uint8_t *refine;        /* [n_images] or null */
    uint32_t *key;                /* [M] the keys before the sort */
    int32_t *track_of;            /* [M] */
    const uint32_t *skey;         /* [M] the sorted keys */
    const int32_t *spos;          /* [M] the positions in the order of the sorted keys */
    int64_t *io;                  /* [n_images + 1] */
    int32_t *img_obs;             /* [M] or null */
    double *poses_out;            /* [n_images, 12] */
    double *cost;                 /* [n_images, 2] */
    int32_t *info;                /* [n_images, 4] */
    double *err;                  /* [M] or null */
    int64_t T, M, rows;
    int n_images, max_trials;
    double ftol;
};

/* ---- the table --------------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void cr_fill_kernel(uint32_t *key, int32_t *val, int64_t M, uint32_t sentinel)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < M) { key[p] = sentinel; val[p] = (int32_t)p; }
}

__global__ __launch_bounds__(256) void cr_mark_kernel(cr_args a)
{
    const int lane = (int)threadIdx.x % CR_G, grp = (int)threadIdx.x / CR_G;
    int64_t nt = a.T;
    if (a.nt) { const int64_t v = a.nt[0]; nt = v < 0 ? 0 : v < a.T ? v : a.T; }
    for (int64_t k = (int64_t)blockIdx.x * (256 / CR_G) + grp; k < nt; k += (int64_t)gridDim.x * (256 / CR_G)) {
        const int64_t b = a.off[k], e = a.off[k + 1];
        if (!(b >= 0 && b <= e && e <= a.M)) continue;                 /* a track with a bad range owns nothing */
        const double *Xk = a.X + 3 * (size_t)k;
        const bool point = mi_finite(Xk[0]) && mi_finite(Xk[1]) && mi_finite(Xk[2]);
        for (int64_t p = b + lane; p < e; p += CR_G) {
            const int m = a.img[p], r = a.obs[p];
            bool u = point && m >= 0 && m < a.n_images && r >= 0 && (int64_t)r < a.rows && (a.keep == nullptr || a.keep[p] != 0);
            if (u) u = mi_finite(a.kps[2 * (size_t)r]) && mi_finite(a.kps[2 * (size_t)r + 1]);
            a.key[p] = u ? (uint32_t)m : (uint32_t)a.n_images;
            a.track_of[p] = (int32_t)k;
        }
    }
}

/* thread i <= n_images: io[i] = the number of sorted keys below i; thread i < M: img_obs[i] = the position behind the i-th sorted key, -1
 * behind the used ones */
__global__ __launch_bounds__(256) void cr_bounds_kernel(cr_args a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= a.n_images) {
        int64_t lo = 0, hi = a.M;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.skey[mid] < (uint32_t)i) lo = mid + 1; else hi = mid;
        }
        a.io[i] = lo;
    }
    if (a.img_obs && i < a.M) a.img_obs[i] = a.skey[i] < (uint32_t)a.n_images ? a.spos[i] : -1;
}

/* ---- the refinement ---------------------------------------------------------------------------------------------------------------- */
struct cr_shared {
    double cur[12];               /* the current pose: R [9], t [3] */
    double tri[12];               /* the pose of the next pass */
    double cam[4];                /* fx fy cx cy */
    double sum[CR_NS];            /* the sums at the current pose */
    double part[CR_NW][CR_NS];    /* the waves' sums of the last pass */
    double lambda, cost0;
    int behind[CR_NW];
    int status, go, trials, accepted;
};

/* the sums of the last pass in wave order (one thread) */
__device__ __forceinline__ double cr_sum(const cr_shared *S, int k) { return ((S->part[0][k] + S->part[1][k]) + S->part[2][k]) + S->part[3][k]; }

/* The next trial that has a pass (one thread): solve, update, the trial pose into S->tri.  Trials whose Cholesky meets a pivot that is
 * not > 0 are rejected here.  Returns 1 with a trial pose to pass over, 0 with S->status set. */
__device__ __forceinline__ int cr_next(cr_shared *S, int max_trials)
{
    for (;;) {
        if (S->trials >= max_trials) { S->status = MI_DEGENSAC_CAMREF_MAX_TRIALS; return 0; }
        S->trials = S->trials + 1;
        const double lam = S->lambda;
        double g[6], A[21], L[6][6], y[6], dl[6];
#pragma unroll
        for (int k = 0; k < 6; k++) g[k] = S->sum[1 + k];
#pragma unroll
        for (int k = 0; k < 21; k++) A[k] = S->sum[7 + k];
        /* A[k][l], k <= l, at 6 k - k (k - 1) / 2 + (l - k): 0 .. 5 | 6 .. 10 | 11 .. 14 | 15 16 17 | 18 19 | 20 */
#define CR_A(k, l) A[6 * (k) - (k) * ((k) - 1) / 2 + ((l) - (k))]
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double x = CR_A(j, j) + lam * CR_A(j, j);
#pragma unroll
            for (int k = 0; k < j; k++) x = x - L[j][k] * L[j][k];
            ok = ok && (x > 0.0);
            L[j][j] = sqrt(x);
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double z = CR_A(j, i);
#pragma unroll
                for (int k = 0; k < j; k++) z = z - L[i][k] * L[j][k];
                L[i][j] = z / L[j][j];
            }
        }
#undef CR_A
        if (!ok) {
            S->lambda = 10.0 * lam;
            if (S->lambda > 1e12) { S->status = MI_DEGENSAC_CAMREF_STALLED; return 0; }
            continue;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double x = -g[i];
#pragma unroll
            for (int k = 0; k < i; k++) x = x - L[i][k] * y[k];
            y[i] = x / L[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; i--) {
            double x = y[i];
#pragma unroll
            for (int k = i + 1; k < 6; k++) x = x - L[k][i] * dl[k];
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
                S->tri[3 * i + j] = (Cm[3 * i] * S->cur[j] + Cm[3 * i + 1] * S->cur[3 + j]) + Cm[3 * i + 2] * S->cur[6 + j];
#pragma unroll
        for (int j = 0; j < 3; j++) S->tri[9 + j] = S->cur[9 + j] + dl[3 + j];
        return 1;
    }
}

/* the verdict on the trial pose after its pass (one thread): returns 1 when the run goes on, 0 with S->status set */
__device__ __forceinline__ int cr_judge(cr_shared *S, double ftol)
{
    const double cost = S->sum[0], cnew = cr_sum(S, 0);
    const int behind = ((S->behind[0] + S->behind[1]) + S->behind[2]) + S->behind[3];
    if (cnew < cost && behind == 0) {                                 /* a NaN is not accepted */
#pragma unroll
        for (int i = 0; i < 12; i++) S->cur[i] = S->tri[i];
#pragma unroll
        for (int k = 0; k < CR_NS; k++) S->sum[k] = cr_sum(S, k);
        S->accepted = S->accepted + 1;
        S->lambda = fmax(S->lambda / 10.0, 1e-12);
        if ((cost - cnew) <= ftol * cost) { S->status = MI_DEGENSAC_CAMREF_CONVERGED; return 0; }
        return 1;
    }
    S->lambda = 10.0 * S->lambda;
    if (S->lambda > 1e12) { S->status = MI_DEGENSAC_CAMREF_STALLED; return 0; }
    return 1;
}

/* One pass over the n used observations of the image, whose positions start at sp, under the pose Q[12] of LDS.  ERR = false: the 28
 * sums of the waves into S->part, the observations that are not in front into S->behind.  ERR = true: the error of every observation
 * into a.err at its track-major position.  All threads of the workgroup, uniform control flow. */
template <bool ERR>
__device__ __forceinline__ void cr_pass(cr_shared *S, const cr_args &a, const double *Q, const int32_t *sp, int n)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = Q[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = Q[9 + i];
    const double fx = S->cam[0], fy = S->cam[1], cx = S->cam[2], cy = S->cam[3];
    double acc[CR_NS];
#pragma unroll
    for (int k = 0; k < CR_NS; k++) acc[k] = 0.0;
    int behind = 0;
    for (int base = 0; base < n; base += CR_STEP) {
        int32_t pos[CR_LOADS], row[CR_LOADS], trk[CR_LOADS]; bool use[CR_LOADS];
        double xy[CR_LOADS][2], X[CR_LOADS][3];
#pragma unroll
        for (int k = 0; k < CR_LOADS; k++) {                          /* an observation past the end reads the last one */
            const int i = base + k * CR_T + tid;
            use[k] = i < n;
            pos[k] = sp[use[k] ? i : n - 1];
        }
#pragma unroll
        for (int k = 0; k < CR_LOADS; k++) { row[k] = a.obs[pos[k]]; trk[k] = a.track_of[pos[k]]; }
#pragma unroll
        for (int k = 0; k < CR_LOADS; k++) {
            xy[k][0] = a.kps[2 * (size_t)row[k]]; xy[k][1] = a.kps[2 * (size_t)row[k] + 1];
#pragma unroll
            for (int c = 0; c < 3; c++) X[k][c] = a.X[3 * (size_t)trk[k] + c];
        }
#pragma unroll
        for (int k = 0; k < CR_LOADS; k++) {
            const double P0 = (R[0] * X[k][0] + R[1] * X[k][1]) + R[2] * X[k][2];
            const double P1 = (R[3] * X[k][0] + R[4] * X[k][1]) + R[5] * X[k][2];
            const double P2 = (R[6] * X[k][0] + R[7] * X[k][1]) + R[8] * X[k][2];
            const double xc = P0 + t[0], yc = P1 + t[1], zc = P2 + t[2];
            const double uu = xc / zc, vv = yc / zc;
            const double rx = (fx * uu + cx) - xy[k][0], ry = (fy * vv + cy) - xy[k][1];
            const bool u = use[k];
            if constexpr (ERR) {
                if (u) a.err[pos[k]] = sqrt(rx * rx + ry * ry);
            } else {
                const double ax = fx / zc, ex = (fx * uu) / zc, ay = fy / zc, ey = (fy * vv) / zc;
                double jx[6], jy[6];
                jx[0] = -(ex * P1); jx[1] = ax * P2 + ex * P0; jx[2] = -(ax * P1); jx[3] = ax; jx[4] = 0.0; jx[5] = -ex;
                jy[0] = -(ay * P2 + ey * P1); jy[1] = ey * P0; jy[2] = ay * P0; jy[3] = 0.0; jy[4] = ay; jy[5] = -ey;
                behind += __popcll(__ballot(u && !(zc > 0.0)));
                const double c = rx * rx + ry * ry;
                acc[0] = u ? acc[0] + c : acc[0];                     /* an observation past the end adds nothing */
                int at = 7;
#pragma unroll
                for (int g = 0; g < 6; g++) {
                    const double gg = jx[g] * rx + jy[g] * ry;
                    acc[1 + g] = u ? acc[1 + g] + gg : acc[1 + g];
#pragma unroll
                    for (int l = g; l < 6; l++, at++) {
                        const double h = jx[g] * jx[l] + jy[g] * jy[l];
                        acc[at] = u ? acc[at] + h : acc[at];
                    }
                }
            }
        }
    }
    if constexpr (!ERR) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int k = 0; k < CR_NS; k++) acc[k] = acc[k] + __shfl_down(acc[k], m, 64);          /* lanes >= m hold what nobody reads */
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < CR_NS; k++) S->part[wv][k] = acc[k];
            S->behind[wv] = behind;
        }
    }
}

__global__ __launch_bounds__(CR_T) void cr_refine_kernel(cr_args a)
{
    __shared__ cr_shared S;
    const int tid = threadIdx.x;
    for (int m = (int)blockIdx.x; m < a.n_images; m += (int)gridDim.x) {
        const int64_t b = a.io[m];
        const int n = (int)(a.io[m + 1] - b);
        const int32_t *sp = a.spos + b;
        double mine = 0.0;
        if (tid < 12) mine = a.poses[12 * (size_t)m + tid];           /* read before poses_out, which may be the same array, is written */
        __syncthreads();                                              /* the previous image's epilogue has read S */
        if (tid < 12) S.tri[tid] = mine;
        __syncthreads();
        if (tid == 0) {
            double cm[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { cm[i] = a.cams[4 * (size_t)m + i]; S.cam[i] = cm[i]; }
            int st = MI_DEGENSAC_CAMREF_BAD_CAMERA;
            if (mi_finite(cm[0]) && mi_finite(cm[1]) && cm[0] != 0.0 && cm[1] != 0.0) {
                bool fin = true;
#pragma unroll
                for (int i = 0; i < 12; i++) fin = fin && mi_finite(S.tri[i]);
                st = !fin ? MI_DEGENSAC_CAMREF_BAD_POSE : n < 3 ? MI_DEGENSAC_CAMREF_SHORT : CR_RUNNING;
            }
            S.status = st; S.trials = 0; S.accepted = 0; S.lambda = 1e-3; S.cost0 = mi_nan(); S.go = 0;
        }
        __syncthreads();
        if (S.status == CR_RUNNING) {                                 /* (uniform: every thread reads the same word) */
            cr_pass<false>(&S, a, S.tri, sp, n);
            __syncthreads();
            if (tid == 0) {
                const double c0 = cr_sum(&S, 0);
                const int behind = ((S.behind[0] + S.behind[1]) + S.behind[2]) + S.behind[3];
#pragma unroll
                for (int i = 0; i < 12; i++) S.cur[i] = S.tri[i];
#pragma unroll
                for (int k = 0; k < CR_NS; k++) S.sum[k] = cr_sum(&S, k);
                if (!mi_finite(c0)) S.status = MI_DEGENSAC_CAMREF_NOT_FINITE;
                else if (behind != 0) { S.status = MI_DEGENSAC_CAMREF_BEHIND; S.cost0 = c0; }
                else if (a.refine && a.refine[m] == 0) { S.status = MI_DEGENSAC_CAMREF_FIXED; S.cost0 = c0; }
                else { S.cost0 = c0; S.go = cr_next(&S, a.max_trials); }
            }
            __syncthreads();
            while (S.go) {
                cr_pass<false>(&S, a, S.tri, sp, n);
                __syncthreads();
                if (tid == 0) S.go = cr_judge(&S, a.ftol) ? cr_next(&S, a.max_trials) : 0;
                __syncthreads();
            }
        }
        const int status = S.status;
        const bool scored = status <= MI_DEGENSAC_CAMREF_FIXED;       /* CONVERGED, STALLED, MAX_TRIALS, FIXED */
        if (scored && a.err) cr_pass<true>(&S, a, S.cur, sp, n);
        if (tid < 12) a.poses_out[12 * (size_t)m + tid] = scored ? S.cur[tid] : mine;
        if (tid == 0) {
            const bool costs = scored || status == MI_DEGENSAC_CAMREF_BEHIND;
            a.cost[2 * (size_t)m] = costs ? S.cost0 : mi_nan(); a.cost[2 * (size_t)m + 1] = costs ? S.sum[0] : mi_nan();
            int32_t *o = a.info + 4 * (size_t)m;
            o[0] = n; o[1] = S.trials; o[2] = S.accepted; o[3] = status;
        }
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_camera_refine_tile(int which) { return which == 0 ? CR_STEP : which == 1 ? CR_GRID : which == 2 ? CR_G : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int cr_check(const void *off, const void *obs, const void *img, const void *kps, int64_t rows, const void *cams, const void *poses, int n_images,
                    const void *X, int64_t T, int64_t M, int max_trials, double ftol, const void *poses_out, const void *cost, const void *info)
{
    if (T < 0) return mi_einval("n_tracks_max < 0");
    if (T > 0x3fffffff) return mi_einval("too many tracks (n_tracks_max > 0x3fffffff)");
    if (M < 0) return mi_einval("n_obs_max < 0");
    if (M > 0x3fffffff) return mi_einval("too many observations (n_obs_max > 0x3fffffff)");
    if (rows < 0 || rows > 0x7fffffff) return mi_einval("rows should lie in 0 .. 0x7fffffff");
    if (n_images < 0) return mi_einval("n_images < 0");
    if (max_trials < 0 || max_trials > 100) return mi_einval("max_trials should lie in 0 .. 100");
    if (!(ftol >= 0.0)) return mi_einval("ftol should be a number >= 0");
    if (!off) return mi_einval("NULL argument: track_offsets");
    if (M > 0 && (!obs || !img)) return mi_einval("NULL argument: obs and obs_image");
    if (rows > 0 && !kps) return mi_einval("NULL argument: kps");
    if (T > 0 && !X) return mi_einval("NULL argument: X");
    if (n_images > 0 && (!cams || !poses)) return mi_einval("NULL argument: cams and poses");
    if (n_images > 0 && (!poses_out || !cost || !info)) return mi_einval("NULL argument: poses_out, cost and info");
    return 0;
}

extern "C" int mi_degensac_camera_refine_tracks_dev(const int64_t *d_track_offsets, const int32_t *d_obs, const int32_t *d_obs_image,
                                                    const int64_t *d_n_tracks, const double *d_kps, int64_t rows, const double *d_cams,
                                                    const double *d_poses, int n_images, const double *d_X, const uint8_t *d_obs_keep,
                                                    const uint8_t *d_refine, int64_t n_tracks_max, int64_t n_obs_max, int max_trials, double ftol,
                                                    int device, void *stream, double *d_poses_out, double *d_cost, int32_t *d_info, double *d_err,
                                                    int64_t *d_img_offsets, int32_t *d_img_obs)
{
    const int64_t T = n_tracks_max, M = n_obs_max;
    int rc = cr_check(d_track_offsets, d_obs, d_obs_image, d_kps, rows, d_cams, d_poses, n_images, d_X, T, M, max_trials, ftol, d_poses_out, d_cost, d_info);
    if (rc) return rc;
    if (M == 0 && n_images == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (M > 0 && d_err) MICHK(hipMemsetAsync(d_err, 0xff, (size_t)M * 8, s));          /* all bits set: a NaN where no used observation is written */
    if (n_images == 0) {                                              /* no image uses anything */
        if (d_img_offsets) MICHK(hipMemsetAsync(d_img_offsets, 0, 8, s));
        if (M > 0 && d_img_obs) MICHK(hipMemsetAsync(d_img_obs, 0xff, (size_t)M * 4, s));
        return 0;
    }
    unsigned bits = 1;
    while (((uint32_t)n_images >> bits) != 0) bits++;                 /* the keys are <= n_images */
    size_t sort_bytes = 0;
    if (M > 0)
        MICHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (unsigned)M,
                                        0u, bits, s));
    const size_t w = mi_up256((size_t)M * 4);
    const size_t a_k1 = w, a_v0 = a_k1 + w, a_v1 = a_v0 + w, a_trk = a_v1 + w, a_io = a_trk + w, a_sort = a_io + mi_up256(((size_t)n_images + 1) * 8),
                 a_all = a_sort + mi_up256(sort_bytes) + 256;
    MiScratch scr; rc = scr.alloc(a_all, s); if (rc) return rc;
    char *blk = scr.p;
    uint32_t *k0 = (uint32_t *)blk, *k1 = (uint32_t *)(blk + a_k1);
    int32_t *v0 = (int32_t *)(blk + a_v0), *v1 = (int32_t *)(blk + a_v1);
    cr_args a;
    memset(&a, 0, sizeof a);
    a.off = d_track_offsets; a.obs = d_obs; a.img = d_obs_image; a.nt = d_n_tracks; a.kps = d_kps; a.cams = d_cams; a.poses = d_poses; a.X = d_X;
    a.keep = d_obs_keep; a.refine = d_refine; a.key = k0; a.track_of = (int32_t *)(blk + a_trk); a.skey = k1; a.spos = v1;
    a.io = d_img_offsets ? d_img_offsets : (int64_t *)(blk + a_io); a.img_obs = d_img_obs;
    a.poses_out = d_poses_out; a.cost = d_cost; a.info = d_info; a.err = d_err;
    a.T = T; a.M = M; a.rows = rows; a.n_images = n_images; a.max_trials = max_trials; a.ftol = ftol;
    if (M > 0) {
        hipLaunchKernelGGL(cr_fill_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, k0, v0, M, (uint32_t)n_images);
        MICHK(hipGetLastError());
        if (T > 0) {
            const int64_t wgs = (T + 256 / CR_G - 1) / (256 / CR_G);
            hipLaunchKernelGGL(cr_mark_kernel, dim3((unsigned)std::min<int64_t>(wgs, CR_MGRID)), dim3(256), 0, s, a);
            MICHK(hipGetLastError());
        }
        MICHK(rocprim::radix_sort_pairs((void *)(blk + a_sort), sort_bytes, k0, k1, v0, v1, (unsigned)M, 0u, bits, s));
    }
    const int64_t nb = std::max<int64_t>((int64_t)n_images + 1, d_img_obs ? M : 0);
    hipLaunchKernelGGL(cr_bounds_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, a);
    MICHK(hipGetLastError());
    hipLaunchKernelGGL(cr_refine_kernel, dim3((unsigned)std::min(n_images, CR_GRID)), dim3(CR_T), 0, s, a);
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_camera_refine_tracks(const int64_t *track_offsets, const int32_t *obs, const int32_t *obs_image, int64_t n_tracks,
                                                const double *kps, int64_t rows, const double *cams, const double *poses, int n_images, const double *X,
                                                const uint8_t *obs_keep, const uint8_t *refine, int64_t n_tracks_max, int64_t n_obs_max, int max_trials,
                                                double ftol, int device, double *poses_out, double *cost, int32_t *info, double *err, int64_t *img_offsets,
                                                int32_t *img_obs)
{
    const int64_t T = n_tracks_max, M = n_obs_max;
    int rc = cr_check(track_offsets, obs, obs_image, kps, rows, cams, poses, n_images, X, T, M, max_trials, ftol, poses_out, cost, info);
    if (rc) return rc;
    if (M == 0 && n_images == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t t = (size_t)T, m = (size_t)M, r = (size_t)rows, ni = (size_t)n_images;
    MiStage st;
    const int i_off = st.in(track_offsets, (t + 1) * 8), i_obs = st.in(obs, m * 4), i_img = st.in(obs_image, m * 4),
              i_nt = st.in(n_tracks >= 0 ? &n_tracks : nullptr, 8), i_kps = st.in(kps, r * 16), i_cams = st.in(cams, ni * 32), i_poses = st.in(poses, ni * 96),
              i_X = st.in(X, t * 24), i_keep = st.in(obs_keep, m), i_ref = st.in(refine, ni), o_pose = st.out(poses_out, ni * 96),
              o_cost = st.out(cost, ni * 16), o_info = st.out(info, ni * 16), o_err = st.out(err, m * 8), o_io = st.out(img_offsets, (ni + 1) * 8),
              o_obs = st.out(img_obs, m * 4);
    rc = st.upload(); if (rc) return rc;
    rc = mi_degensac_camera_refine_tracks_dev(st.dev<int64_t>(i_off), st.dev<int32_t>(i_obs), st.dev<int32_t>(i_img), st.dev<int64_t>(i_nt),
                                              st.dev<double>(i_kps), rows, st.dev<double>(i_cams), st.dev<double>(i_poses), n_images, st.dev<double>(i_X),
                                              st.dev<uint8_t>(i_keep), st.dev<uint8_t>(i_ref), T, M, max_trials, ftol, device, nullptr,
                                              st.dev<double>(o_pose), st.dev<double>(o_cost), st.dev<int32_t>(o_info), st.dev<double>(o_err),
                                              st.dev<int64_t>(o_io), st.dev<int32_t>(o_obs));
    if (rc) return rc;
    return st.finish();
}
