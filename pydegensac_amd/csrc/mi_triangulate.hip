/* libmi_degensac.so — triangulation of tracks under known camera poses (include/mi_degensac.h mi_degensac_triangulate_tracks*): per
 * track of the tables the tracks call writes (track_offsets, obs, obs_image, n_tracks, all on the device) the N-view midpoint of its
 * used observations, a Gauss-Newton refinement on the reprojection error in pixels, the flags of the observations at the final point
 * and the smallest cosine between two of its rays.  gfx950 only, no CPU path.
 *
 * A group of TR_G lanes handles one track, TR_T / TR_G groups share a workgroup, further tracks by a grid stride; no group waits for
 * another (no workgroup barrier at all: the lanes of a group lie inside one wave), no atomics.  The kernel reads its range o[k],
 * o[k + 1] and n_tracks itself, so the host never learns a length and the call has no synchronisation.
 *   row passes  lane l takes the observations l, l + G, l + 2 G, .. of the track; per observation two int32, the keypoint, the camera's
 *               four numbers and its pose are gathered (18 float64: the tables are small and stay in the caches) and 9 (linear pass) or
 *               10 (Gauss-Newton pass) float64 accumulators are kept; every small array is indexed by constants only.
 *   sums        log2(G) butterfly steps, lane l takes v[l] + v[l xor m]: IEEE addition commutes, so every lane of the group ends with
 *               the same bits and solves the 3 x 3 system itself; nothing is broadcast.
 *   pair pass   the unit rays of TR_CH observations are staged in LDS (NaN for one that is not used) and every lane takes the minimum
 *               of its rays' products with the staged rays before them; a track longer than TR_CH is walked chunk against chunk with a
 *               second staging area, the rays recomputed per chunk.
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

#ifndef TR_G
/* lanes per track.  Measured (profiles/triangulate.log, kernel alone): 64 lanes take 0.052 ms against 0.095 ms on the benchmark collection
 * (tracks of 39 in the median) and 0.219 ms against 0.069 ms on the same observations cut into tracks of 2 .. 5, the lengths that
 * dominate real collections: 16 loses 0.04 ms where it loses and wins 0.15 ms where it wins, so 16 it is.  `make g64` builds the other. */
#define TR_G     16
#endif
#define TR_T     256                      /* threads per workgroup */
#define TR_GPW   (TR_T / TR_G)            /* tracks per workgroup and stride step */
#define TR_CH    64                       /* rays per staging area of the pair pass */
#define TR_GRID  1024                     /* cap on the grid: further tracks by the grid stride */
static_assert(TR_G >= 2 && TR_G <= 64 && (TR_G & (TR_G - 1)) == 0 && TR_CH % TR_G == 0, "a group is a power of two inside one wave");

struct tr_args {
    const int64_t *off;           /* [T + 1] */
    const int32_t *obs, *img;     /* [M] */
    const int64_t *nt;            /* [1] or null */
    const double *kps;            /* [rows, 2] */
    const double *cams;           /* [n_images, 4] */
    const double *poses;          /* [n_images, 12] */
    double *X;                    /* [T, 3] */
    int32_t *info;                /* [T, 5] */
    double *cost;                 /* [T, 2] */
    double *cosang;               /* [T] */
    double *err;                  /* [M] or null */
    uint8_t *ok;                  /* [M] or null */
    double *depth;                /* [M] or null */
    int64_t T, M, rows;
    int n_images, max_iters;
    double cos_min, max_px, ftol;
};

struct tr_ob { double x, y, fx, fy, cx, cy, R[9], t[3]; };

/* the observation at position p of the tables: true when it is used; an index out of range is never used as one */
__device__ __forceinline__ bool tr_load(const tr_args &a, int64_t p, bool valid, tr_ob &o)
{
    o.x = o.y = o.fx = o.fy = o.cx = o.cy = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) o.R[i] = 0.0;
    o.t[0] = o.t[1] = o.t[2] = 0.0;
    if (!valid) return false;
    const int m = a.img[p], r = a.obs[p];
    if (m < 0 || m >= a.n_images || r < 0 || (int64_t)r >= a.rows) return false;
    o.x = a.kps[2 * (size_t)r]; o.y = a.kps[2 * (size_t)r + 1];
    const double *c = a.cams + 4 * (size_t)m, *q = a.poses + 12 * (size_t)m;
    o.fx = c[0]; o.fy = c[1]; o.cx = c[2]; o.cy = c[3];
    bool fin = mi_finite(o.x) && mi_finite(o.y) && mi_finite(o.fx) && mi_finite(o.fy) && o.fx != 0.0 && o.fy != 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) { o.R[i] = q[i]; fin = fin && mi_finite(o.R[i]); }
#pragma unroll
    for (int i = 0; i < 3; i++) { o.t[i] = q[9 + i]; fin = fin && mi_finite(o.t[i]); }
    return fin;
}

/* w = R^T d / |R^T d| */
__device__ __forceinline__ void tr_ray(const tr_ob &o, double *w)
{
    const double d0 = (o.x - o.cx) / o.fx, d1 = (o.y - o.cy) / o.fy;
    double v[3];
#pragma unroll
    for (int j = 0; j < 3; j++) v[j] = (o.R[j] * d0 + o.R[3 + j] * d1) + o.R[6 + j];
    const double nn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = v[j] / nn;
}

/* every lane of the group takes the group's sum: the same bits in all of them */
template <int N>
__device__ __forceinline__ void tr_sum(double *v)
{
#pragma unroll
    for (int m = TR_G / 2; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = v[k] + __shfl_xor(v[k], m, TR_G);
}
__device__ __forceinline__ int tr_isum(int v)
{
#pragma unroll
    for (int m = TR_G / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, TR_G);
    return v;
}

/* x of M x = r by an unpivoted Cholesky factor; M = (00 01 02 11 12 22).  False when a pivot is not > 0. */
__device__ __forceinline__ bool tr_solve(const double *M, const double *r, double *x)
{
    double p = M[0];
    bool ok = p > 0.0;
    const double L00 = sqrt(p), L10 = M[1] / L00, L20 = M[2] / L00;
    p = M[3] - L10 * L10;
    ok = ok && (p > 0.0);
    const double L11 = sqrt(p), L21 = (M[4] - L20 * L10) / L11;
    p = M[5] - L20 * L20; p = p - L21 * L21;
    ok = ok && (p > 0.0);
    const double L22 = sqrt(p);
    const double y0 = r[0] / L00, y1 = (r[1] - L10 * y0) / L11, y2 = ((r[2] - L20 * y0) - L21 * y1) / L22;
    x[2] = y2 / L22;
    x[1] = (y1 - L21 * x[2]) / L11;
    x[0] = ((y0 - L10 * x[1]) - L20 * x[2]) / L00;
    return ok;
}

/* the linear pass: A (00 01 02 11 12 22), b of the used observations into s[0 .. 9), their number is returned */
__device__ __forceinline__ int tr_linear(const tr_args &a, int64_t b0, int n, int lane, double *s)
{
#pragma unroll
    for (int k = 0; k < 9; k++) s[k] = 0.0;
    int cnt = 0;
    for (int base = 0; base < n; base += TR_G) {
        const int i = base + lane;
        tr_ob o;
        const bool u = tr_load(a, b0 + i, i < n, o);
        double w[3], c[3], P[6], t[9];
        tr_ray(o, w);
#pragma unroll
        for (int j = 0; j < 3; j++) c[j] = -((o.R[j] * o.t[0] + o.R[3 + j] * o.t[1]) + o.R[6 + j] * o.t[2]);
        P[0] = 1.0 - w[0] * w[0]; P[1] = -(w[0] * w[1]); P[2] = -(w[0] * w[2]);
        P[3] = 1.0 - w[1] * w[1]; P[4] = -(w[1] * w[2]); P[5] = 1.0 - w[2] * w[2];
#pragma unroll
        for (int k = 0; k < 6; k++) t[k] = P[k];
        t[6] = (P[0] * c[0] + P[1] * c[1]) + P[2] * c[2];
        t[7] = (P[1] * c[0] + P[3] * c[1]) + P[4] * c[2];
        t[8] = (P[2] * c[0] + P[4] * c[1]) + P[5] * c[2];
#pragma unroll
        for (int k = 0; k < 9; k++) s[k] = u ? s[k] + t[k] : s[k];      /* an observation that is not used adds nothing */
        cnt += u ? 1 : 0;
    }
    tr_sum<9>(s);
    return tr_isum(cnt);
}

struct tr_res { double rx, ry, zc, jx[3], jy[3]; };
__device__ __forceinline__ tr_res tr_residual(const tr_ob &o, const double *X)
{
    tr_res q;
    const double xc = ((o.R[0] * X[0] + o.R[1] * X[1]) + o.R[2] * X[2]) + o.t[0];
    const double yc = ((o.R[3] * X[0] + o.R[4] * X[1]) + o.R[5] * X[2]) + o.t[1];
    const double zc = ((o.R[6] * X[0] + o.R[7] * X[1]) + o.R[8] * X[2]) + o.t[2];
    const double uu = xc / zc, vv = yc / zc;
    q.rx = (o.fx * uu + o.cx) - o.x; q.ry = (o.fy * vv + o.cy) - o.y; q.zc = zc;
    const double ax = o.fx / zc, ex = (o.fx * uu) / zc, ay = o.fy / zc, ey = (o.fy * vv) / zc;
#pragma unroll
    for (int j = 0; j < 3; j++) { q.jx[j] = ax * o.R[j] - ex * o.R[6 + j]; q.jy[j] = ay * o.R[3 + j] - ey * o.R[6 + j]; }
    return q;
}

/* one Gauss-Newton pass at X: cost, H (00 01 02 11 12 22), g into s[0 .. 10) */
__device__ __forceinline__ void tr_pass(const tr_args &a, int64_t b0, int n, int lane, const double *X, double *s)
{
#pragma unroll
    for (int k = 0; k < 10; k++) s[k] = 0.0;
    for (int base = 0; base < n; base += TR_G) {
        const int i = base + lane;
        tr_ob o;
        const bool u = tr_load(a, b0 + i, i < n, o);
        const tr_res q = tr_residual(o, X);
        double t[10];
        t[0] = q.rx * q.rx + q.ry * q.ry;
        t[1] = q.jx[0] * q.jx[0] + q.jy[0] * q.jy[0]; t[2] = q.jx[0] * q.jx[1] + q.jy[0] * q.jy[1]; t[3] = q.jx[0] * q.jx[2] + q.jy[0] * q.jy[2];
        t[4] = q.jx[1] * q.jx[1] + q.jy[1] * q.jy[1]; t[5] = q.jx[1] * q.jx[2] + q.jy[1] * q.jy[2]; t[6] = q.jx[2] * q.jx[2] + q.jy[2] * q.jy[2];
#pragma unroll
        for (int j = 0; j < 3; j++) t[7 + j] = q.jx[j] * q.rx + q.jy[j] * q.ry;
#pragma unroll
        for (int k = 0; k < 10; k++) s[k] = u ? s[k] + t[k] : s[k];
    }
    tr_sum<10>(s);
}

/* the flags of the used observations at X: err, ok and depth into the tables when they are asked for (WRITE); the ok count is returned */
__device__ __forceinline__ int tr_flags(const tr_args &a, int64_t b0, int n, int lane, const double *X)
{
    int cnt = 0;
    for (int base = 0; base < n; base += TR_G) {
        const int i = base + lane;
        tr_ob o;
        const bool u = tr_load(a, b0 + i, i < n, o);
        const tr_res q = tr_residual(o, X);
        const double e = sqrt(q.rx * q.rx + q.ry * q.ry);
        const bool ok = u && q.zc > 0.0 && e <= a.max_px;              /* a NaN is neither front nor within the bound */
        cnt += ok ? 1 : 0;
        if (u) {
            if (a.err) a.err[b0 + i] = e;
            if (a.ok) a.ok[b0 + i] = ok ? 1 : 0;
            if (a.depth) a.depth[b0 + i] = q.zc;
        }
    }
    return tr_isum(cnt);
}

/* What one lane wrote to LDS is read by the other lanes of its group.  This relies on two things: the lanes of a group lie in one wave,
 * whose LDS operations keep their order, and every lane of a group takes the same branch everywhere (n, the chunk counters, used, the
 * solves and the verdicts are the same bits in all of them: that is what the butterfly of tr_sum guarantees), so the whole group is
 * active at every shuffle and at every staging.  Groups of one wave may diverge from each other: a group never reads another's lanes. */
__device__ __forceinline__ void tr_group_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* the unit rays of the observations c0 .. c0 + TR_CH of the track into W [3][TR_CH]; NaN for one that is not used or past the end */
__device__ __forceinline__ void tr_stage(const tr_args &a, int64_t b0, int n, int lane, int c0, double (*W)[TR_CH])
{
    for (int k = lane; k < TR_CH; k += TR_G) {
        const int i = c0 + k;
        tr_ob o;
        const bool u = tr_load(a, b0 + i, i < n, o);
        double w[3];
        tr_ray(o, w);
#pragma unroll
        for (int j = 0; j < 3; j++) W[j][k] = u ? w[j] : mi_nan();
    }
}

/* the smallest product of two rays of used observations (all of them finite here: the linear system was positive definite) */
__device__ __forceinline__ double tr_cosang(const tr_args &a, int64_t b0, int n, int lane, double (*WA)[TR_CH], double (*WB)[TR_CH])
{
    double mn = mi_inf();
    for (int a0 = 0; a0 < n; a0 += TR_CH) {
        tr_group_fence();                                              /* the readers of the previous round are through */
        tr_stage(a, b0, n, lane, a0, WA);
        tr_group_fence();
        const int na = n - a0 < TR_CH ? n - a0 : TR_CH;
        for (int c0 = 0; c0 <= a0; c0 += TR_CH) {
            const bool self = c0 == a0;
            double (*B)[TR_CH] = WA;
            if (!self) {
                tr_group_fence();
                tr_stage(a, b0, n, lane, c0, WB);
                tr_group_fence();
                B = WB;
            }
            for (int i = lane; i < na; i += TR_G) {
                const double w0 = WA[0][i], w1 = WA[1][i], w2 = WA[2][i];
                const int lim = self ? i : TR_CH;                      /* an earlier chunk is full */
                for (int j = 0; j < lim; j++) {
                    const double d = (w0 * B[0][j] + w1 * B[1][j]) + w2 * B[2][j];
                    mn = d < mn ? d : mn;                              /* a NaN (a ray that is not used) is passed over */
                }
            }
        }
    }
#pragma unroll
    for (int m = TR_G / 2; m >= 1; m >>= 1) {
        const double o = __shfl_xor(mn, m, TR_G);
        mn = o < mn ? o : mn;
    }
    return mn;
}

__global__ __launch_bounds__(TR_T) void tr_triangulate_kernel(tr_args a)
{
    __shared__ double S[TR_GPW][2][3][TR_CH];
    const int lane = (int)threadIdx.x % TR_G, grp = (int)threadIdx.x / TR_G;
    int64_t nt = a.T;
    if (a.nt) { const int64_t v = a.nt[0]; nt = v < 0 ? 0 : v < a.T ? v : a.T; }
    for (int64_t k = (int64_t)blockIdx.x * TR_GPW + grp; k < a.T; k += (int64_t)gridDim.x * TR_GPW) {
        int status = MI_DEGENSAC_TRI_SHORT, used = 0, n_ok = 0, accepted = 0, trials = 0;
        double X[3] = {mi_nan(), mi_nan(), mi_nan()}, cost0 = mi_nan(), cost1 = mi_nan(), cosang = mi_nan();
        if (k < nt) {                                                  /* a track beyond n_tracks gets the outputs of an empty one */
            const int64_t b = a.off[k], e = a.off[k + 1];
            const bool whole = b >= 0 && b <= e && e <= a.M;
            const int n = whole ? (int)(e - b) : 0;
            if (!whole) status = MI_DEGENSAC_TRI_TRUNCATED;
            else {
                double s[10], Y[3];
                used = tr_linear(a, b, n, lane, s);
                if (used >= 2) {
                    const bool pd = tr_solve(s, s + 6, Y);
                    if (!pd || !(mi_finite(Y[0]) && mi_finite(Y[1]) && mi_finite(Y[2]))) status = MI_DEGENSAC_TRI_DEGENERATE;
                    else {
                        tr_pass(a, b, n, lane, Y, s);
                        cost0 = s[0];
                        double cur = s[0];
                        while (trials < a.max_iters) {
                            double dl[3], Z[3], s2[10];
                            if (!tr_solve(s + 1, s + 7, dl)) break;
                            trials++;
#pragma unroll
                            for (int j = 0; j < 3; j++) Z[j] = Y[j] - dl[j];
                            tr_pass(a, b, n, lane, Z, s2);
                            if (!(mi_finite(s2[0]) && s2[0] < cur)) break;          /* the first rejected trial ends the run */
                            accepted++;
                            const bool done = (cur - s2[0]) <= a.ftol * cur;
#pragma unroll
                            for (int j = 0; j < 3; j++) Y[j] = Z[j];
#pragma unroll
                            for (int j = 0; j < 10; j++) s[j] = s2[j];
                            cur = s2[0];
                            if (done) break;
                        }
                        cost1 = cur;
#pragma unroll
                        for (int j = 0; j < 3; j++) X[j] = Y[j];
                        n_ok = tr_flags(a, b, n, lane, X);
                        cosang = tr_cosang(a, b, n, lane, S[grp][0], S[grp][1]);
                        status = cosang > a.cos_min ? MI_DEGENSAC_TRI_NARROW : MI_DEGENSAC_TRI_OK;
                    }
                }
            }
        }
        if (lane == 0) {
            a.X[3 * (size_t)k] = X[0]; a.X[3 * (size_t)k + 1] = X[1]; a.X[3 * (size_t)k + 2] = X[2];
            a.cost[2 * (size_t)k] = cost0; a.cost[2 * (size_t)k + 1] = cost1;
            a.cosang[k] = cosang;
            int32_t *o = a.info + 5 * (size_t)k;
            o[0] = used; o[1] = n_ok; o[2] = accepted; o[3] = trials; o[4] = status;
        }
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_triangulate_tile(int which) { return which == 0 ? TR_G : which == 1 ? TR_GRID : which == 2 ? TR_GPW : which == 3 ? TR_CH : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int tr_check(const void *off, const void *obs, const void *img, const void *kps, int64_t rows, const void *cams, const void *poses, int n_images,
                    int64_t T, int64_t M, double min_angle_deg, double max_reproj_px, int max_iters, double ftol, const void *X, const void *info,
                    const void *cost, const void *cosang)
{
    if (T < 0) return mi_einval("n_tracks_max < 0");
    if (T > 0x3fffffff) return mi_einval("too many tracks (n_tracks_max > 0x3fffffff)");
    if (M < 0) return mi_einval("n_obs_max < 0");
    if (M > 0x3fffffff) return mi_einval("too many observations (n_obs_max > 0x3fffffff)");
    if (rows < 0 || rows > 0x7fffffff) return mi_einval("rows should lie in 0 .. 0x7fffffff");
    if (n_images < 0) return mi_einval("n_images < 0");
    if (!(min_angle_deg >= 0.0 && min_angle_deg <= 180.0)) return mi_einval("min_angle_deg should be a number in [0, 180]");
    if (!(max_reproj_px >= 0.0)) return mi_einval("max_reproj_px should be a number >= 0");
    if (max_iters < 0 || max_iters > 100) return mi_einval("max_iters should lie in 0 .. 100");
    if (!(ftol >= 0.0)) return mi_einval("ftol should be a number >= 0");
    if (!off) return mi_einval("NULL argument: track_offsets");
    if (M > 0 && (!obs || !img)) return mi_einval("NULL argument: obs and obs_image");
    if (T > 0 && (!X || !info || !cost || !cosang)) return mi_einval("NULL argument: X, info, cost and cosang");
    if (rows > 0 && !kps) return mi_einval("NULL argument: kps");
    if (n_images > 0 && (!cams || !poses)) return mi_einval("NULL argument: cams and poses");
    return 0;
}

extern "C" int mi_degensac_triangulate_tracks_dev(const int64_t *d_track_offsets, const int32_t *d_obs, const int32_t *d_obs_image,
                                                  const int64_t *d_n_tracks, const double *d_kps, int64_t rows, const double *d_cams,
                                                  const double *d_poses, int n_images, int64_t n_tracks_max, int64_t n_obs_max,
                                                  double min_angle_deg, double max_reproj_px, int max_iters, double ftol, int device, void *stream,
                                                  double *d_X, int32_t *d_info, double *d_cost, double *d_cosang, double *d_err, uint8_t *d_ok,
                                                  double *d_depth)
{
    const int64_t T = n_tracks_max, M = n_obs_max;
    int rc = tr_check(d_track_offsets, d_obs, d_obs_image, d_kps, rows, d_cams, d_poses, n_images, T, M, min_angle_deg, max_reproj_px, max_iters, ftol,
                      d_X, d_info, d_cost, d_cosang);
    if (rc) return rc;
    if (T == 0 && M == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (M > 0 && d_err) MICHK(hipMemsetAsync(d_err, 0xff, (size_t)M * 8, s));          /* all bits set: a NaN where no used observation is written */
    if (M > 0 && d_depth) MICHK(hipMemsetAsync(d_depth, 0xff, (size_t)M * 8, s));
    if (M > 0 && d_ok) MICHK(hipMemsetAsync(d_ok, 0, (size_t)M, s));
    if (T == 0) return 0;
    tr_args a;
    memset(&a, 0, sizeof a);
    a.off = d_track_offsets; a.obs = d_obs; a.img = d_obs_image; a.nt = d_n_tracks; a.kps = d_kps; a.cams = d_cams; a.poses = d_poses;
    a.X = d_X; a.info = d_info; a.cost = d_cost; a.cosang = d_cosang; a.err = d_err; a.ok = d_ok; a.depth = d_depth;
    a.T = T; a.M = M; a.rows = rows; a.n_images = n_images; a.max_iters = max_iters;
    a.cos_min = cos(min_angle_deg * (3.141592653589793 / 180.0)); a.max_px = max_reproj_px; a.ftol = ftol;
    const int64_t wgs = (T + TR_GPW - 1) / TR_GPW;
    const dim3 grid((unsigned)std::min<int64_t>(wgs, TR_GRID)), block(TR_T);
    hipLaunchKernelGGL(tr_triangulate_kernel, grid, block, 0, s, a);
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_triangulate_tracks(const int64_t *track_offsets, const int32_t *obs, const int32_t *obs_image, int64_t n_tracks,
                                              const double *kps, int64_t rows, const double *cams, const double *poses, int n_images,
                                              int64_t n_tracks_max, int64_t n_obs_max, double min_angle_deg, double max_reproj_px, int max_iters,
                                              double ftol, int device, double *X, int32_t *info, double *cost, double *cosang, double *err, uint8_t *ok,
                                              double *depth)
{
    const int64_t T = n_tracks_max, M = n_obs_max;
    int rc = tr_check(track_offsets, obs, obs_image, kps, rows, cams, poses, n_images, T, M, min_angle_deg, max_reproj_px, max_iters, ftol, X, info, cost,
                      cosang);
    if (rc) return rc;
    if (T == 0 && M == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t t = (size_t)T, m = (size_t)M, r = (size_t)rows, ni = (size_t)n_images;
    MiStage st;
    const int i_off = st.in(track_offsets, (t + 1) * 8), i_obs = st.in(obs, m * 4), i_img = st.in(obs_image, m * 4),
              i_nt = st.in(n_tracks >= 0 ? &n_tracks : nullptr, 8), i_kps = st.in(kps, r * 16), i_cams = st.in(cams, ni * 32), i_poses = st.in(poses, ni * 96),
              o_X = st.out(X, t * 24), o_info = st.out(info, t * 20), o_cost = st.out(cost, t * 16), o_cos = st.out(cosang, t * 8), o_err = st.out(err, m * 8),
              o_ok = st.out(ok, m), o_depth = st.out(depth, m * 8);
    rc = st.upload(); if (rc) return rc;
    rc = mi_degensac_triangulate_tracks_dev(st.dev<int64_t>(i_off), st.dev<int32_t>(i_obs), st.dev<int32_t>(i_img), st.dev<int64_t>(i_nt), st.dev<double>(i_kps),
                                            rows, st.dev<double>(i_cams), st.dev<double>(i_poses), n_images, T, M, min_angle_deg, max_reproj_px, max_iters,
                                            ftol, device, nullptr, st.dev<double>(o_X), st.dev<int32_t>(o_info), st.dev<double>(o_cost),
                                            st.dev<double>(o_cos), st.dev<double>(o_err), st.dev<uint8_t>(o_ok), st.dev<double>(o_depth));
    if (rc) return rc;
    return st.finish();
}
