/* libmi_degensac.so — rotation averaging (include/mi_degensac.h mi_degensac_rotation_average*): one world-to-camera rotation per image
 * from the relative rotations of a pair list, and one residual cosine per pair.  gfx950 only, no CPU path.
 *   mark     every half-edge h = 2 e + side gets the key of its camera (the sentinel n_images when the edge is unused) and itself as value;
 *   group    rocprim::radix_sort_pairs of (key, half-edge) over the key bits: stable, so the half-edges of a camera come out ascending
 *            without an atomic;
 *   init     off[c] = the lower bound of c in the sorted keys, one thread per camera; the same launch writes the start state;
 *   sweep    one launch per sweep.  A group of RA_G lanes handles one camera, RA_T / RA_G groups share a workgroup, further cameras by a
 *            grid stride; no barrier, no group waits for another (the lanes of a group lie inside one wave).  Lane l takes the camera's
 *            half-edges at positions l, l + G, ..; per half-edge two matrices of 72 bytes are gathered (the edge's and the other end's:
 *            nothing is reused inside a group, so nothing is staged in LDS).  The sums meet by log2(G) butterfly steps v[l] + v[l xor m]:
 *            IEEE addition commutes, so every lane ends with the same bits and applies the update itself; lane 0 writes.  Sweep s reads
 *            the state sweep s - 1 wrote and writes the other buffer (Jacobi); a sweep whose predecessor changed nothing returns at once;
 *   finish   the outputs from the buffer of the last sweep that ran.
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

#define RA_G     16                       /* lanes per camera */
#define RA_T     256                      /* threads per workgroup */
#define RA_CPW   (RA_T / RA_G)            /* cameras per workgroup and stride step */
#define RA_GRID  1024                     /* cap on the grid of a sweep: further cameras by the grid stride */
#define RA_NONE  0x7fffffff               /* the position of "no half-edge" */
static_assert(RA_G >= 2 && RA_G <= 64 && (RA_G & (RA_G - 1)) == 0 && RA_T % RA_G == 0, "a group is a power of two inside one wave");

struct ra_args {
    const int32_t *pairs;         /* [K, 2] */
    const double *Rrel;           /* [K, 9] */
    const double *weight;         /* [K] or null */
    const uint8_t *keep;          /* [K] or null */
    const double *R0;             /* [n, 9] or null */
    const uint8_t *known;         /* [n] or null */
    uint32_t *key;                /* [2 K] the keys before the sort */
    int32_t *val;                 /* [2 K] the half-edges before the sort */
    const uint32_t *skey;         /* [2 K] the sorted keys */
    const int32_t *shalf;         /* [2 K] the half-edges in the order of the sorted keys */
    int32_t *off;                 /* [n + 1] */
    double *Rs[2];                /* [n, 9] the two state buffers */
    double *steps[2];             /* [n] */
    int32_t *meta[2];             /* [n, 2] = (the sweep in which the camera was set, -1 = not set; opposed edges) */
    int32_t *ctl;                 /* [2 + sweeps + 1] = the last sweep that ran, a known camera exists, changed[0 .. sweeps] */
    double *R;                    /* [n, 9] */
    int32_t *info;                /* [n, 4] */
    double *step;                 /* [n] */
    int64_t *summary;             /* [4] */
    double *edge_cos;             /* [K] or null */
    int64_t K;
    int n, root, sweeps, robust;
    double damping, sigma2, tol2;
};

/* whether edge e is used (the header's five conditions); an index out of range is never used as one */
__device__ __forceinline__ bool ra_used(const ra_args &a, int64_t e)
{
    if (a.keep && a.keep[e] == 0) return false;
    const int i = a.pairs[2 * e], j = a.pairs[2 * e + 1];
    if (i < 0 || i >= a.n || j < 0 || j >= a.n || i == j) return false;
    if (a.weight) { const double w = a.weight[e]; if (!(w > 0.0 && mi_finite(w))) return false; }
    const double *r = a.Rrel + 9 * e;
    double s = r[0] * r[0];
#pragma unroll
    for (int k = 1; k < 9; k++) s = s + r[k] * r[k];
    return fabs(s - 3.0) <= 1e-6;                                     /* false for a NaN */
}

__device__ __forceinline__ bool ra_known(const ra_args &a, int c) { return a.known ? a.known[c] != 0 : c == a.root; }

/* ---- the adjacency ----------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void ra_mark_kernel(ra_args a)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= 2 * a.K) return;
    const int64_t e = h >> 1;
    a.key[h] = ra_used(a, e) ? (uint32_t)a.pairs[2 * e + (h & 1)] : (uint32_t)a.n;
    a.val[h] = (int32_t)h;
}

/* thread i <= n: off[i] = the number of sorted keys below i; thread i < n: the start state of camera i in buffer 0; thread 0: the flags */
__global__ __launch_bounds__(256) void ra_init_kernel(ra_args a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= a.n) {
        int64_t lo = 0, hi = 2 * a.K;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.skey[mid] < (uint32_t)i) lo = mid + 1; else hi = mid;
        }
        a.off[i] = (int32_t)lo;
    }
    if (i < a.n) {
        const int c = (int)i;
        const bool kn = ra_known(a, c);
        double *R = a.Rs[0] + 9 * (size_t)c;
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = !kn ? 0.0 : a.R0 ? a.R0[9 * (size_t)c + k] : (k % 4 == 0 ? 1.0 : 0.0);
        a.steps[0][c] = mi_nan();
        a.meta[0][2 * (size_t)c] = kn ? 0 : -1; a.meta[0][2 * (size_t)c + 1] = 0;
        if (kn) atomicOr(&a.ctl[1], 1);
    }
    if (i == 0) a.ctl[2] = 1;                                         /* changed[0]: the first sweep runs */
}

/* ---- one sweep --------------------------------------------------------------------------------------------------------------------- */
/* P = A B, or A^T B with tr: P[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j] */
__device__ __forceinline__ void ra_mul(const double *A, const double *B, bool tr, double *P)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double x0 = tr ? A[i] : A[3 * i], x1 = tr ? A[3 + i] : A[3 * i + 1], x2 = tr ? A[6 + i] : A[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; j++) P[3 * i + j] = (x0 * B[j] + x1 * B[3 + j]) + x2 * B[6 + j];
    }
}

/* the prediction of the camera of half-edge h from its other end o under the state Rp */
__device__ __forceinline__ void ra_predict(const ra_args &a, const double *Rp, int h, int o, double *P)
{
    double A[9], B[9];
    const double *pa = a.Rrel + 9 * (size_t)(h >> 1), *pb = Rp + 9 * (size_t)o;
#pragma unroll
    for (int k = 0; k < 9; k++) { A[k] = pa[k]; B[k] = pb[k]; }
    ra_mul(A, B, (h & 1) == 0, P);                                    /* the first image of the edge takes the transpose */
}

__global__ __launch_bounds__(RA_T) void ra_sweep_kernel(ra_args a, int s)
{
    int32_t *changed = a.ctl + 2;
    if (changed[s - 1] == 0) return;                                  /* (uniform over the grid) the state stays where it is */
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[0] = s;
    const int lane = (int)threadIdx.x % RA_G, grp = (int)threadIdx.x / RA_G;
    const double *Rp = a.Rs[(s - 1) & 1], *stp = a.steps[(s - 1) & 1];
    const int32_t *mp = a.meta[(s - 1) & 1];
    double *Rn = a.Rs[s & 1], *stn = a.steps[s & 1];
    int32_t *mn = a.meta[s & 1];
    for (int c = (int)blockIdx.x * RA_CPW + grp; c < a.n; c += (int)gridDim.x * RA_CPW) {
        const int b = a.off[c], deg = a.off[c + 1] - b;
        double Rc[9];
#pragma unroll
        for (int k = 0; k < 9; k++) Rc[k] = Rp[9 * (size_t)c + k];
        int setsw = mp[2 * (size_t)c], opp = 0;
        double step = stp[c];
        bool chg = false;
        const bool known = ra_known(a, c);
        if (!known && setsw < 0) {                                    /* the start: the heaviest half-edge whose other end is set */
            double bw = 0.0; int bp = RA_NONE;
            for (int base = 0; base < deg; base += RA_G) {
                const int pos = base + lane;
                if (pos < deg) {
                    const int h = a.shalf[b + pos], o = a.pairs[2 * (size_t)(h >> 1) + (1 - (h & 1))];
                    if (mp[2 * (size_t)o] >= 0) {
                        const double w = a.weight ? a.weight[h >> 1] : 1.0;
                        if (w > bw) { bw = w; bp = pos; }               /* a tie keeps the lower position */
                    }
                }
            }
#pragma unroll
            for (int m = RA_G / 2; m >= 1; m >>= 1) {
                const double ow = __shfl_xor(bw, m, RA_G); const int op = __shfl_xor(bp, m, RA_G);
                if (ow > bw || (ow == bw && op < bp)) { bw = ow; bp = op; }
            }
            if (bp != RA_NONE) {
                const int h = a.shalf[b + bp], o = a.pairs[2 * (size_t)(h >> 1) + (1 - (h & 1))];
                ra_predict(a, Rp, h, o, Rc);
                setsw = s; chg = true;
            }
        } else if (!known) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int base = 0; base < deg; base += RA_G) {
                const int pos = base + lane;
                if (pos < deg) {
                    const int h = a.shalf[b + pos], o = a.pairs[2 * (size_t)(h >> 1) + (1 - (h & 1))];
                    if (mp[2 * (size_t)o] >= 0) {
                        double P[9], Q[9];
                        ra_predict(a, Rp, h, o, P);
#pragma unroll
                        for (int i = 0; i < 3; i++)
#pragma unroll
                            for (int j = 0; j < 3; j++) Q[3 * i + j] = (P[3 * i] * Rc[3 * j] + P[3 * i + 1] * Rc[3 * j + 1]) + P[3 * i + 2] * Rc[3 * j + 2];
                        const double q = 1.0 + ((Q[0] + Q[4]) + Q[8]);
                        if (!(q > 0.0009765625)) opp++;                 /* 2^-10; a NaN is opposed */
                        else {
                            const double w0 = (Q[7] - Q[5]) / q, w1 = (Q[2] - Q[6]) / q, w2 = (Q[3] - Q[1]) / q;
                            double f = a.weight ? a.weight[h >> 1] : 1.0;
                            if (a.robust) {
                                const double m = (w0 * w0 + w1 * w1) + w2 * w2, g = a.sigma2 / (a.sigma2 + m);
                                f = f * (g * g);
                            }
                            acc[0] = acc[0] + f; acc[1] = acc[1] + f * w0; acc[2] = acc[2] + f * w1; acc[3] = acc[3] + f * w2;
                        }
                    }
                }
            }
#pragma unroll
            for (int m = RA_G / 2; m >= 1; m >>= 1) {
#pragma unroll
                for (int k = 0; k < 4; k++) acc[k] = acc[k] + __shfl_xor(acc[k], m, RA_G);
                opp = opp + __shfl_xor(opp, m, RA_G);
            }
            if (acc[0] > 0.0) {
                const double u0 = acc[1] / acc[0], u1 = acc[2] / acc[0], u2 = acc[3] / acc[0];
                step = (u0 * u0 + u1 * u1) + u2 * u2;
                const double a0 = a.damping * u0, a1 = a.damping * u1, a2 = a.damping * u2, w0 = a0 + a0, w1 = a1 + a1, w2 = a2 + a2;
                const double aa = (a0 * a0 + a1 * a1) + a2 * a2, p = 1.0 - aa, d = 1.0 + aa;
                double Cm[9], N[9];
                Cm[0] = (p + w0 * a0) / d; Cm[1] = (w0 * a1 - w2) / d; Cm[2] = (w0 * a2 + w1) / d;
                Cm[3] = (w1 * a0 + w2) / d; Cm[4] = (p + w1 * a1) / d; Cm[5] = (w1 * a2 - w0) / d;
                Cm[6] = (w2 * a0 - w1) / d; Cm[7] = (w2 * a1 + w0) / d; Cm[8] = (p + w2 * a2) / d;
                ra_mul(Cm, Rc, false, N);
#pragma unroll
                for (int k = 0; k < 9; k++) Rc[k] = N[k];
                chg = step > a.tol2;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) Rn[9 * (size_t)c + k] = Rc[k];
            stn[c] = step;
            mn[2 * (size_t)c] = setsw; mn[2 * (size_t)c + 1] = opp;
            if (chg) atomicOr(&changed[s], 1);
        }
    }
}

/* ---- the outputs ------------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void ra_finish_kernel(ra_args a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int last = a.ctl[0];
    const double *Rf = a.Rs[last & 1];
    const int32_t *mf = a.meta[last & 1];
    bool isset = false;
    if (i < a.n) {
        const int c = (int)i, setsw = mf[2 * (size_t)c], deg = a.off[c + 1] - a.off[c];
        isset = setsw >= 0;
#pragma unroll
        for (int k = 0; k < 9; k++) a.R[9 * (size_t)c + k] = Rf[9 * (size_t)c + k];
        a.step[c] = a.steps[last & 1][c];
        int32_t *o = a.info + 4 * (size_t)c;
        o[0] = deg; o[1] = setsw; o[2] = mf[2 * (size_t)c + 1];
        o[3] = ra_known(a, c) ? MI_DEGENSAC_ROTAVG_KNOWN : isset ? MI_DEGENSAC_ROTAVG_OK : deg > 0 ? MI_DEGENSAC_ROTAVG_UNREACHED : MI_DEGENSAC_ROTAVG_ISOLATED;
    }
    const unsigned long long bal = __ballot(isset);
    if ((threadIdx.x & 63) == 0 && bal != 0) atomicAdd((unsigned long long *)&a.summary[1], (unsigned long long)__popcll(bal));
    if (a.edge_cos && i < a.K) {
        double v = mi_nan();
        if (ra_used(a, i)) {
            const int ci = a.pairs[2 * i], cj = a.pairs[2 * i + 1];
            if (mf[2 * (size_t)ci] >= 0 && mf[2 * (size_t)cj] >= 0) {
                double T[9], B[9];
                ra_predict(a, Rf, (int)(2 * i + 1), ci, T);               /* R_rel R_i */
#pragma unroll
                for (int k = 0; k < 9; k++) B[k] = Rf[9 * (size_t)cj + k];
                const double d0 = (T[0] * B[0] + T[1] * B[1]) + T[2] * B[2], d1 = (T[3] * B[3] + T[4] * B[4]) + T[5] * B[5],
                             d2 = (T[6] * B[6] + T[7] * B[7]) + T[8] * B[8];
                v = (((d0 + d1) + d2) - 1.0) / 2.0;
            }
        }
        a.edge_cos[i] = v;
    }
    if (i == 0) {
        const int32_t *changed = a.ctl + 2;
        const bool still = changed[last] != 0;                        /* the last sweep that ran changed something (or none ran) */
        a.summary[0] = last == 0 ? 0 : last - (still ? 0 : 1);
        a.summary[2] = a.off[a.n] / 2;
        a.summary[3] = a.ctl[1] == 0 ? MI_DEGENSAC_ROTAVG_NO_ROOT : still ? MI_DEGENSAC_ROTAVG_MAX_SWEEPS : MI_DEGENSAC_ROTAVG_CONVERGED;
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_rotation_average_tile(int which) { return which == 0 ? RA_G : which == 1 ? RA_GRID : which == 2 ? RA_CPW : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int ra_check(const void *pairs, const void *Rrel, int n_images, int64_t K, const void *R0, const void *known, int root, int sweeps, double damping,
                    double robust_deg, double tol, const void *R, const void *info, const void *step, const void *summary)
{
    if (n_images < 1 || n_images > (1 << 24)) return mi_einval("n_images should lie in 1 .. 2^24");
    if (K < 0) return mi_einval("n_pairs < 0");
    if (K > 0x3fffffff) return mi_einval("too many pairs (n_pairs > 0x3fffffff)");
    if (sweeps < 0 || sweeps > 4096) return mi_einval("sweeps should lie in 0 .. 4096");
    if (!(damping > 0.0 && damping <= 1.0)) return mi_einval("damping should be a number in (0, 1]");
    if (!(robust_deg >= 0.0 && robust_deg < 180.0)) return mi_einval("robust_deg should be a number in (0, 180), or 0 for no robust factor");
    if (!(tol >= 0.0)) return mi_einval("tol should be a number >= 0");
    if (root < 0 || root >= n_images) return mi_einval("root should lie in 0 .. n_images - 1");
    if (K > 0 && (!pairs || !Rrel)) return mi_einval("NULL argument: pairs and R_rel");
    if ((R0 == nullptr) != (known == nullptr)) return mi_einval("R0 and known go together: both or neither");
    if (!R || !info || !step || !summary) return mi_einval("NULL argument: R, info, step and summary");
    return 0;
}

extern "C" int mi_degensac_rotation_average_dev(const int32_t *d_pairs, const double *d_R_rel, const double *d_weight, const uint8_t *d_edge_keep,
                                                int64_t n_pairs, int n_images, const double *d_R0, const uint8_t *d_known, int root, int sweeps,
                                                double damping, double robust_deg, double tol, int device, void *stream, double *d_R, int32_t *d_info,
                                                double *d_step, int64_t *d_summary, double *d_edge_cos)
{
    const int64_t K = n_pairs, M = 2 * n_pairs;
    int rc = ra_check(d_pairs, d_R_rel, n_images, K, d_R0, d_known, root, sweeps, damping, robust_deg, tol, d_R, d_info, d_step, d_summary);
    if (rc) return rc;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)n_images;
    unsigned bits = 1;
    while (((uint32_t)n_images >> bits) != 0) bits++;                 /* the keys are <= n_images */
    size_t sort_bytes = 0;
    if (M > 0)
        MICHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (unsigned)M,
                                        0u, bits, s));
    const size_t w = mi_up256((size_t)M * 4), sR = mi_up256(n * 72), sS = mi_up256(n * 8), nctl = (size_t)sweeps + 3;
    const size_t a_k1 = w, a_v0 = a_k1 + w, a_v1 = a_v0 + w, a_off = a_v1 + w, a_R0 = a_off + mi_up256((n + 1) * 4), a_R1 = a_R0 + sR, a_s0 = a_R1 + sR,
                 a_s1 = a_s0 + sS, a_m0 = a_s1 + sS, a_m1 = a_m0 + sS, a_ctl = a_m1 + sS, a_sort = a_ctl + mi_up256(nctl * 4),
                 a_all = a_sort + mi_up256(sort_bytes) + 256;
    MiScratch scr; rc = scr.alloc(a_all, s); if (rc) return rc;
    char *blk = scr.p;
    ra_args a;
    memset(&a, 0, sizeof a);
    a.pairs = d_pairs; a.Rrel = d_R_rel; a.weight = d_weight; a.keep = d_edge_keep; a.R0 = d_R0; a.known = d_known;
    a.key = (uint32_t *)blk; a.skey = (uint32_t *)(blk + a_k1); a.val = (int32_t *)(blk + a_v0); a.shalf = (int32_t *)(blk + a_v1);
    a.off = (int32_t *)(blk + a_off);
    a.Rs[0] = (double *)(blk + a_R0); a.Rs[1] = (double *)(blk + a_R1); a.steps[0] = (double *)(blk + a_s0); a.steps[1] = (double *)(blk + a_s1);
    a.meta[0] = (int32_t *)(blk + a_m0); a.meta[1] = (int32_t *)(blk + a_m1); a.ctl = (int32_t *)(blk + a_ctl);
    a.R = d_R; a.info = d_info; a.step = d_step; a.summary = d_summary; a.edge_cos = d_edge_cos;
    a.K = K; a.n = n_images; a.root = root; a.sweeps = sweeps; a.robust = robust_deg > 0.0 ? 1 : 0;
    a.damping = damping; a.tol2 = tol * tol;
    if (a.robust) { const double sg = tan(robust_deg * (3.141592653589793 / 360.0)); a.sigma2 = sg * sg; }
    MICHK(hipMemsetAsync(a.ctl, 0, nctl * 4, s));
    MICHK(hipMemsetAsync(d_summary, 0, 32, s));
    if (M > 0) {
        hipLaunchKernelGGL(ra_mark_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, a);
        MICHK(hipGetLastError());
        MICHK(rocprim::radix_sort_pairs((void *)(blk + a_sort), sort_bytes, a.key, (uint32_t *)(blk + a_k1), a.val, (int32_t *)(blk + a_v1), (unsigned)M, 0u,
                                        bits, s));
    }
    hipLaunchKernelGGL(ra_init_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, a);
    MICHK(hipGetLastError());
    const dim3 grid((unsigned)std::min<int64_t>(((int64_t)n_images + RA_CPW - 1) / RA_CPW, RA_GRID));
    for (int sw = 1; sw <= sweeps; sw++) {
        hipLaunchKernelGGL(ra_sweep_kernel, grid, dim3(RA_T), 0, s, a, sw);
        MICHK(hipGetLastError());
    }
    const int64_t nf = std::max<int64_t>(n_images, d_edge_cos ? K : 0);
    hipLaunchKernelGGL(ra_finish_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, a);
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_rotation_average(const int32_t *pairs, const double *R_rel, const double *weight, const uint8_t *edge_keep, int64_t n_pairs,
                                            int n_images, const double *R0, const uint8_t *known, int root, int sweeps, double damping, double robust_deg,
                                            double tol, int device, double *R, int32_t *info, double *step, int64_t *summary, double *edge_cos)
{
    const int64_t K = n_pairs;
    int rc = ra_check(pairs, R_rel, n_images, K, R0, known, root, sweeps, damping, robust_deg, tol, R, info, step, summary);
    if (rc) return rc;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t k = (size_t)K, n = (size_t)n_images;
    MiStage st;
    const int i_pr = st.in(pairs, k * 8), i_rr = st.in(R_rel, k * 72), i_w = st.in(weight, k * 8), i_kp = st.in(edge_keep, k), i_R0 = st.in(R0, n * 72),
              i_kn = st.in(known, n), o_R = st.out(R, n * 72), o_info = st.out(info, n * 16), o_step = st.out(step, n * 8), o_sum = st.out(summary, 32),
              o_cos = st.out(edge_cos, k * 8);
    rc = st.upload(); if (rc) return rc;
    rc = mi_degensac_rotation_average_dev(st.dev<int32_t>(i_pr), st.dev<double>(i_rr), st.dev<double>(i_w), st.dev<uint8_t>(i_kp), K, n_images,
                                          st.dev<double>(i_R0), st.dev<uint8_t>(i_kn), root, sweeps, damping, robust_deg, tol, device, nullptr,
                                          st.dev<double>(o_R), st.dev<int32_t>(o_info), st.dev<double>(o_step), st.dev<int64_t>(o_sum), st.dev<double>(o_cos));
    if (rc) return rc;
    return st.finish();
}
