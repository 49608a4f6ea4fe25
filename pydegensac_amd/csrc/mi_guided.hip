/* libmi_degensac.so — guided matching (include/mi_degensac.h mi_degensac_match_guided_*): the batched 2-NN of mi_matcher.hip
 * restricted, per pair p, to the train rows that are inliers of a given model M_p ("guided matching" after RANSAC, Hartley &
 * Zisserman; COLMAP).  gfx950 only, no CPU path.
 *
 * Semantics, for pair p with model M_p (9 doubles in the driver's form) and threshold th_p (as fill_params derives th: F px_th^2;
 * H px_th^2 for error_type 0 / 1 / 3, px_th for 2 / 4):
 *   gate(q, t) := r(M_p; x1_q, y1_q, x2_t, y2_t) <= th_p with r the estimator's own residual of the error type (F: 0 dg_FDs,
 *                 1 dg_FDsSym; H: 0 dg_HDs, 1..4 dg_Hsym on dg_hsym_prepare(M_p)), fp64 without contraction.  `<=` is the
 *                 reference's inlier rule (rtools.c inlidxs); a NaN residual fails.  A model of nine zeros (a short or failed
 *                 pair) passes nothing.  The estimators' symmetric check and LAF check are NOT part of the gate: both judge a
 *                 correspondence that is already chosen (a second metric with its own threshold; the affine frames of both
 *                 keypoints), they do not describe the model's inlier band that the search is restricted to.
 *   guided 2-NN  the two nearest train rows of the query's own pair among those that pass the gate, in the matcher's distance
 *                (L2 = sqrt of the fp32 sum over ascending dimension, Hamming = popcount, L2 over uint8 rows = sqrt of the exact
 *                integer sum) and (distance, index) order, ties to
 *                the lower index (mt_push); -1 / inf where fewer than two rows pass.
 *
 * Cost follows the candidates, not n1 n2 dim: a workgroup owns MG_Q queries of one pair (MG_QPW per wave) and streams the pair's
 * train keypoints through LDS MG_TC rows at a time.  Per 64-row step every lane tests the gate of one train row for each of its
 * wave's queries — a division-free screen that never rejects a row the exact residual accepts, then the exact residual for the
 * survivors — and the rows that pass go, by ballot and popcount, to the query's candidate list in LDS (ascending train order).
 * Whenever a list holds 64 rows, and once at the end, the 64 lanes each take one candidate, form its distance in the matcher's
 * order (the query row is wave-uniform) and push it into a lane-local top-2; a butterfly over the wave merges the 64 top-2s.
 * Memory is bounded (two fixed LDS blocks per workgroup) whatever the gate passes.  A gate that passes everything is correct,
 * and slower than the dense matcher (one distance per lane instead of a 4 x 4 register block over LDS tiles). */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "dg_geom.h"

#define MG_W    4                 /* waves per workgroup */
#define MG_QPW  4                 /* queries per wave */
#define MG_Q    (MG_W * MG_QPW)   /* queries per workgroup, all of one pair */
#define MG_TC   1024              /* train keypoints per LDS chunk */
#define MG_LIST 128               /* per-query candidate list: < 64 pending + one 64-row step */

enum { MG_F_SAMPSON = 0, MG_F_SYM = 1, MG_H_SAMPSON = 2, MG_H_SYM = 3 };

/* gate(x1, y1, x2, y2) of model M.  The screens: F forms the exact residual's numerator and denominator in its own operation order
 * and compares them without the division (whose rounding lies far inside tb = 1.01 th); H Sampson is dg_HDs_maybe_below; the four
 * symmetric H errors are each bounded below by the forward transfer error d1 (kind <= th implies d1 <= th, or <= th^2 for the
 * square-root kinds), screened as |x2 a - n|^2 <= tb a^2.  screen = 0 (th == 0) takes the exact residual of every row. */
template <int GK>
__device__ __forceinline__ bool mg_gate(const double *M, const double *Hinv, const double *H1, int hk, double th, double tb, int screen,
                                        double x1, double y1, double x2, double y2)
{
    if (GK == MG_F_SAMPSON || GK == MG_F_SYM) {
        if (screen) {
            DG_F_COMMON(M, x1, y1, x2, y2);
            const double rr = r * r, a = rxc*rxc + ryc*ryc;
            if (GK == MG_F_SAMPSON) { if (rr > tb * (a + rx*rx + ry*ry)) return false; }
            else { const double b = rx*rx + ry*ry; if (rr * (a + b) > tb * (a * b)) return false; }
        }
        return (GK == MG_F_SAMPSON ? dg_FDs(M, x1, y1, x2, y2) : dg_FDsSym(M, x1, y1, x2, y2)) <= th;
    } else if (GK == MG_H_SAMPSON) {
        if (screen && !dg_HDs_maybe_below(M, x1, y1, x2, y2, tb)) return false;
        return dg_HDs(M, x1, y1, x2, y2) <= th;
    } else {
        if (screen) {
            double a = H1[6]*x1 + H1[7]*y1 + H1[8];
            if (hk >= 3) a = a + 1e-10;
            const double e0 = x2 * a - (H1[0]*x1 + H1[1]*y1 + H1[2]), e1 = y2 * a - (H1[3]*x1 + H1[4]*y1 + H1[5]);
            if (e0*e0 + e1*e1 > tb * (a * a)) return false;
        }
        return dg_Hsym(Hinv, H1, x1, y1, x2, y2, hk, hk >= 3) <= th;
    }
}

/* the first n (<= 64) entries of a wave's candidate list: lane l takes entry l, forms its distance to the query row in the order of
 * mt_knn2_tile (fp32 sum of squared differences over ascending words / popcount) and pushes it into b.  NORM 2 (uint8 rows under
 * L2): the integer sum of the squared byte differences, at most 256 * 255^2 < 2^24 and so exact as the float it is pushed as (the
 * value the dense matcher's matrix-core form gives) */
template <int NORM>
__device__ __forceinline__ void mg_flush(const uint32_t *qrow, const uint32_t *dt, int words, int t_b, const int *lst, int n, int lane, mt_best &b)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          /* other lanes' list entries are written before they are read */
    __builtin_amdgcn_wave_barrier();
    if (lane < n) {
        const int c = lst[lane];
        const uint32_t *trow = dt + (size_t)(t_b + c) * words;
        float acc = 0.f; unsigned h = 0u;
        for (int w = 0; w < words; w++) {
            const uint32_t a = qrow[w], t = trow[w];
            if (NORM == 0) { const float df = __uint_as_float(a) - __uint_as_float(t); acc = acc + df * df; }
            else if (NORM == 1) h += (unsigned)__popc(a ^ t);
            else {
#pragma unroll
                for (int k = 0; k < 32; k += 8) { const int d = (int)((a >> k) & 255u) - (int)((t >> k) & 255u); h += (unsigned)(d * d); }
            }
        }
        mt_push(b, NORM == 0 ? acc : (float)h, c);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

/* grid = one workgroup per tile of MG_Q queries of one pair.  tab = [toff | oq | ot], each [K + 1] int32: pair p owns tiles
 * toff[p] .. toff[p+1] - 1, query rows oq[p] .. oq[p+1] - 1 and train rows ot[p] .. ot[p+1] - 1 (relative, global over the batch).
 * Every branch around a barrier or a ballot is uniform: the chunk loop over the workgroup, query slots and list counts over the wave. */
template <int NORM, int GK>
__global__ __launch_bounds__(256) void mg_guided_kernel(const uint32_t *dq, const uint32_t *dt, int words, const double *kq, const double *kt, int kd,
                                                        const int32_t *tab, int n_pairs, const double *models, int hk, double th, double tb, int screen,
                                                        int swap, int32_t *idx, float *dist)
{
    __shared__ double2 ts[MG_TC];
    __shared__ int lists[MG_W][MG_QPW][MG_LIST];
    const int32_t *toff = tab, *oq = tab + (n_pairs + 1), *ot = tab + 2 * (n_pairs + 1);
    const int b = (int)blockIdx.x;
    int lo = 0, hi = n_pairs - 1;                                    /* the last pair p with toff[p] <= b (empty pairs own no tile) */
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (toff[mid] <= b) lo = mid; else hi = mid - 1; }
    const int pair = lo, q0 = oq[pair] + (b - toff[pair]) * MG_Q, q_end = oq[pair + 1], t_b = ot[pair];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double M[9], Hinv[9], H1[9];
    bool any = false;
#pragma unroll
    for (int i = 0; i < 9; i++) { M[i] = models[(size_t)pair * 9 + i]; any = any || M[i] != 0.0; }
    if (GK == MG_H_SYM) dg_hsym_prepare(M, Hinv, H1);
    const int t_e = any ? ot[pair + 1] : t_b;                        /* a zero model has no candidates */
    double qx[MG_QPW], qy[MG_QPW]; int cnt[MG_QPW]; mt_best best[MG_QPW];
#pragma unroll
    for (int j = 0; j < MG_QPW; j++) {
        const int q = q0 + wv + MG_W * j;
        qx[j] = q < q_end ? kq[(size_t)q * kd] : 0.0; qy[j] = q < q_end ? kq[(size_t)q * kd + 1] : 0.0;
        cnt[j] = 0; best[j].d0 = best[j].d1 = __builtin_inff(); best[j].i0 = best[j].i1 = -1;
    }
    for (int c0 = t_b; c0 < t_e; c0 += MG_TC) {
        const int c_end = c0 + MG_TC < t_e ? c0 + MG_TC : t_e;
        __syncthreads();
        for (int i = threadIdx.x; i < c_end - c0; i += 256) ts[i] = make_double2(kt[(size_t)(c0 + i) * kd], kt[(size_t)(c0 + i) * kd + 1]);
        __syncthreads();
        for (int s0 = c0; s0 < c_end; s0 += 64) {
            const int t = s0 + lane;
            const bool in = t < c_end;
            const double2 p = ts[in ? t - c0 : 0];
#pragma unroll
            for (int j = 0; j < MG_QPW; j++) {
                const int q = q0 + wv + MG_W * j;
                if (q >= q_end) continue;                                          /* wave-uniform */
                const bool pass = in && (swap ? mg_gate<GK>(M, Hinv, H1, hk, th, tb, screen, p.x, p.y, qx[j], qy[j])
                                              : mg_gate<GK>(M, Hinv, H1, hk, th, tb, screen, qx[j], qy[j], p.x, p.y));
                const unsigned long long bal = __ballot(pass);
                int *lst = lists[wv][j];
                if (pass) lst[cnt[j] + __popcll(bal & ((1ull << lane) - 1ull))] = t - t_b;
                cnt[j] += __popcll(bal);
                if (cnt[j] >= 64) {                                                /* wave-uniform */
                    mg_flush<NORM>(dq + (size_t)q * words, dt, words, t_b, lst, 64, lane, best[j]);
                    if (lane < cnt[j] - 64) lst[lane] = lst[64 + lane];
                    cnt[j] -= 64;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MG_QPW; j++) {
        const int q = q0 + wv + MG_W * j;
        if (q >= q_end) continue;
        if (cnt[j] > 0) mg_flush<NORM>(dq + (size_t)q * words, dt, words, t_b, lists[wv][j], cnt[j], lane, best[j]);
        mt_best m = best[j];
        /* butterfly: after the step of mask k every lane holds the top-2 of 2k lanes' disjoint candidate sets */
        for (int k = 1; k < 64; k <<= 1) {
            const float d0 = __shfl_xor(m.d0, k), d1 = __shfl_xor(m.d1, k);
            const int i0 = __shfl_xor(m.i0, k), i1 = __shfl_xor(m.i1, k);
            if (i0 >= 0) mt_push(m, d0, i0);
            if (i1 >= 0) mt_push(m, d1, i1);
        }
        if (lane == 0) {
            idx[2 * (size_t)q] = m.i0; idx[2 * (size_t)q + 1] = m.i1;
            dist[2 * (size_t)q] = NORM != 1 ? sqrtf(m.d0) : m.d0; dist[2 * (size_t)q + 1] = NORM != 1 ? sqrtf(m.d1) : m.d1;
        }
    }
}

/* one workgroup per pair: every query's decision and the pair's number of guided matches */
__global__ __launch_bounds__(256) void mg_decide_kernel(const int32_t *idx, const float *dist, const int32_t *off1, const int32_t *off2, float ratio,
                                                        const int32_t *back, int32_t *match, int32_t *count)
{
    __shared__ int wsum[4];
    const int p = blockIdx.x, lo = off1[p], hi = off1[p + 1], b2 = off2[p];
    int c = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const int j = idx[2 * i];
        bool ok = j >= 0 && dist[2 * i] < ratio * dist[2 * i + 1];     /* one candidate: dist[1] = inf, the query passes */
        if (ok && back) ok = back[2 * (b2 + j)] == i - lo;
        match[i] = ok ? j : -1;
        c += ok ? 1 : 0;
    }
    for (int k = 32; k >= 1; k >>= 1) c += __shfl_xor(c, k);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0 && count) count[p] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
#define MGCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { char b_[256]; snprintf(b_, sizeof b_, "%s failed: %s", #x, hipGetErrorString(e_)); \
    mt_set_error(b_); (void)hipGetLastError(); return MI_DEGENSAC_EHIP; } } while (0)
static int mg_einval(const char *msg) { mt_set_error(msg); return MI_DEGENSAC_EINVAL; }

struct MgDevGuard {
    int prev = -1; bool armed = false;
    int enter(int device)
    {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { (void)hipGetLastError(); mt_set_error("no HIP device: this library has no CPU path");
            return MI_DEGENSAC_ENODEV; }
        if (device < 0 || device >= n) { mt_set_error("device index out of range"); return MI_DEGENSAC_ENODEV; }
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != device) { MGCHK(hipSetDevice(device)); armed = prev >= 0; }
        return 0;
    }
    ~MgDevGuard() { if (armed) (void)hipSetDevice(prev); }
};

int mt_guided_gate(int homography, int error_type, double px_th, mt_gate *g)
{
    if (!(px_th >= 0)) return mg_einval("px_th must be >= 0 (not NaN)");
    if (!homography) {
        if (error_type != 0 && error_type != 1) return mg_einval("error_type must be 0 or 1 for the fundamental matrix");
        g->gk = error_type; g->hk = 0; g->th = px_th * px_th;
    } else {
        if (error_type < 0 || error_type > 4) return mg_einval("error_type must be 0..4 for the homography");
        g->gk = error_type == 0 ? MG_H_SAMPSON : MG_H_SYM; g->hk = error_type;
        g->th = (error_type == 2 || error_type == 4) ? px_th : px_th * px_th;
    }
    /* the screens' bound: 1 % above th (the symmetric H kinds screen d1: th, or th^2 for the square-root kinds 2 and 4) */
    const double t1 = (homography && (error_type == 2 || error_type == 4)) ? g->th * g->th : g->th;
    g->tb = t1 * 1.01; g->screen = g->th > 0 ? 1 : 0;
    return 0;
}

int mt_batch_guided_knn2(int norm, int words, const void *dq, const void *dt, const double *kq, const double *kt, int kd, const int64_t *oq,
                         const int64_t *ot, int n_pairs, const double *d_models, const mt_gate &g, int swap, int device, hipStream_t s,
                         int32_t *idx, float *dist)
{
    if (n_pairs <= 0 || oq[n_pairs] == 0) return 0;
    std::vector<int32_t> tab(3 * (size_t)(n_pairs + 1));
    int64_t tiles = 0;
    for (int p = 0; p <= n_pairs; p++) {
        tab[p] = (int32_t)tiles; tab[n_pairs + 1 + p] = (int32_t)oq[p]; tab[2 * (n_pairs + 1) + p] = (int32_t)ot[p];
        if (p < n_pairs) tiles += (oq[p + 1] - oq[p] + MG_Q - 1) / MG_Q;
    }
    int32_t *d_tab = nullptr;
    MGCHK(hipMallocAsync((void **)&d_tab, tab.size() * 4, s));
    int rc = mt_batch_upload(device, s, tab.data(), tab.size() * 4, d_tab);
    if (rc) { (void)hipFreeAsync(d_tab, s); return rc; }
    const dim3 grid((unsigned)tiles), block(256);
#define MG_LAUNCH(N, G) hipLaunchKernelGGL((mg_guided_kernel<N, G>), grid, block, 0, s, (const uint32_t *)dq, (const uint32_t *)dt, words, kq, kt, kd, \
        d_tab, n_pairs, d_models, g.hk, g.th, g.tb, g.screen, swap, idx, dist)
    switch (4 * mt_norm_index(norm) + g.gk) {
    case 0: MG_LAUNCH(0, MG_F_SAMPSON); break;
    case 1: MG_LAUNCH(0, MG_F_SYM); break;
    case 2: MG_LAUNCH(0, MG_H_SAMPSON); break;
    case 3: MG_LAUNCH(0, MG_H_SYM); break;
    case 4: MG_LAUNCH(1, MG_F_SAMPSON); break;
    case 5: MG_LAUNCH(1, MG_F_SYM); break;
    case 6: MG_LAUNCH(1, MG_H_SAMPSON); break;
    case 7: MG_LAUNCH(1, MG_H_SYM); break;
    case 8: MG_LAUNCH(2, MG_F_SAMPSON); break;
    case 9: MG_LAUNCH(2, MG_F_SYM); break;
    case 10: MG_LAUNCH(2, MG_H_SAMPSON); break;
    default: MG_LAUNCH(2, MG_H_SYM); break;
    }
#undef MG_LAUNCH
    const hipError_t le = hipGetLastError();
    (void)hipFreeAsync(d_tab, s);
    MGCHK(le);
    return 0;
}

int mt_batch_guided_decide(const int32_t *d_idx, const float *d_dist, const int32_t *d_off1, const int32_t *d_off2, int n_pairs, float ratio,
                           const int32_t *d_back, hipStream_t s, int32_t *d_match, int32_t *d_count)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(mg_decide_kernel, dim3(n_pairs), dim3(256), 0, s, d_idx, d_dist, d_off1, d_off2, ratio, d_back, d_match, d_count);
    MGCHK(hipGetLastError());
    return 0;
}

/* ---- C-ABI ----------------------------------------------------------------------------------------------------------- */
static int mg_check(int norm, int dim, int kp_dim, const mi_degensac_guide_params *gp, const int64_t *o1, const int64_t *o2, int n_pairs, mt_gate *g)
{
    if (!mt_norm_known(norm) || dim <= 0) return mg_einval("bad norm or descriptor dim");
    if (const char *e = mt_norm_dim_error(norm, dim)) return mg_einval(e);
    if (kp_dim != 2 && kp_dim != 6) return mg_einval("keypoint rows must be [n,2] or [n,6]");
    if (!gp) return mg_einval("guide params are NULL");
    if (gp->struct_size != 0 && gp->struct_size < (int32_t)sizeof(mi_degensac_guide_params)) return mg_einval("guide params: struct_size too small");
    if (gp->homography != 0 && gp->homography != 1) return mg_einval("homography must be 0 or 1");
    int rc = mt_guided_gate(gp->homography, gp->error_type, gp->px_th, g); if (rc) return rc;
    if (n_pairs < 0) return mg_einval("n_pairs < 0");
    if (n_pairs == 0) return 0;
    for (const int64_t *o : {o1, o2}) {
        if (!o || o[0] < 0) return mg_einval("offsets must be given and start at >= 0");
        for (int p = 0; p < n_pairs; p++) if (o[p + 1] < o[p]) return mg_einval("offsets must be non-decreasing");
        if (o[n_pairs] - o[0] > 0x3fffffff) return mg_einval("too many descriptor rows in one batch");
    }
    return 0;
}

static int mg_words(int norm, int dim) { return mt_row_words(norm, dim); }

extern "C" int mi_degensac_match_guided_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                       const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp1, const double *d_kp2,
                                                       int kp_dim, const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream,
                                                       int32_t *d_idx, float *d_dist)
{
    mt_gate g; int rc = mg_check(norm, dim, kp_dim, gp, offsets1_host, offsets2_host, n_pairs, &g); if (rc) return rc;
    if (n_pairs == 0) return 0;
    const int64_t n1 = offsets1_host[n_pairs] - offsets1_host[0], n2 = offsets2_host[n_pairs] - offsets2_host[0];
    if (!d_models || (n1 > 0 && (!d_desc1 || !d_kp1 || !d_idx || !d_dist)) || (n2 > 0 && (!d_desc2 || !d_kp2))) return mg_einval("NULL argument");
    MgDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const int words = mg_words(norm, dim);
    std::vector<int64_t> o1(n_pairs + 1), o2(n_pairs + 1);
    for (int p = 0; p <= n_pairs; p++) { o1[p] = offsets1_host[p] - offsets1_host[0]; o2[p] = offsets2_host[p] - offsets2_host[0]; }
    return mt_batch_guided_knn2(norm, words, (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words,
                                (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words, d_kp1 + (size_t)offsets1_host[0] * kp_dim,
                                d_kp2 + (size_t)offsets2_host[0] * kp_dim, kp_dim, o1.data(), o2.data(), n_pairs, d_models, g, 0, device,
                                (hipStream_t)stream, d_idx + 2 * offsets1_host[0], d_dist + 2 * offsets1_host[0]);
}

static int mg_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *off1, const int64_t *off2,
                        const double *d_kp1, const double *d_kp2, int kd, int K, const double *d_models, const mi_degensac_guide_params *gp, int device,
                        hipStream_t s, int32_t *d_idx, float *d_dist, int32_t *d_match, int32_t *d_counts, int32_t *h_counts)
{
    if (!mp) return mg_einval("match params are NULL");
    if (!(isfinite(mp->ratio) && mp->ratio > 0.f)) return mg_einval("ratio must be finite and > 0");
    mt_gate g; int rc = mg_check(mp->norm, mp->dim, kd, gp, off1, off2, K, &g); if (rc) return rc;
    if (K == 0) return 0;
    const int64_t n1 = off1[K] - off1[0], n2 = off2[K] - off2[0];
    if (!d_models || (n1 > 0 && (!d_desc1 || !d_kp1 || !d_idx || !d_dist || !d_match)) || (n2 > 0 && (!d_desc2 || !d_kp2))) return mg_einval("NULL argument");
    MgDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const int words = mg_words(mp->norm, mp->dim);
    const bool mutual = mp->mutual != 0;
    std::vector<int64_t> o1(K + 1), o2(K + 1); std::vector<int32_t> o32(2 * (size_t)(K + 1));
    for (int p = 0; p <= K; p++) { o1[p] = off1[p] - off1[0]; o2[p] = off2[p] - off2[0]; o32[p] = (int32_t)o1[p]; o32[K + 1 + p] = (int32_t)o2[p]; }
    const uint32_t *q1 = (const uint32_t *)d_desc1 + (size_t)off1[0] * words, *q2 = (const uint32_t *)d_desc2 + (size_t)off2[0] * words;
    const double *kp1 = d_kp1 + (size_t)off1[0] * kd, *kp2 = d_kp2 + (size_t)off2[0] * kd;
    int32_t *idx = d_idx + 2 * off1[0], *match = d_match + off1[0]; float *dist = d_dist + 2 * off1[0];
    /* one stream-ordered block: offsets | reverse idx | reverse dist | counts (when the caller gives none on the device) */
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t a_bidx = up(o32.size() * 4), a_bdist = a_bidx + (mutual ? up((size_t)n2 * 8) : 0), a_cnt = a_bdist + (mutual ? up((size_t)n2 * 8) : 0),
                 a_all = a_cnt + up((size_t)K * 4);
    char *blk = nullptr;
    MGCHK(hipMallocAsync((void **)&blk, a_all, s));
    struct Free { char *p; hipStream_t s; ~Free() { (void)hipFreeAsync(p, s); } } fr{blk, s};
    const int32_t *d_o1 = (const int32_t *)blk, *d_o2 = d_o1 + (K + 1);
    int32_t *bidx = mutual ? (int32_t *)(blk + a_bidx) : nullptr, *cnt = d_counts ? d_counts : (int32_t *)(blk + a_cnt);
    float *bdist = (float *)(blk + a_bdist);
    rc = mt_batch_upload(device, s, o32.data(), o32.size() * 4, blk); if (rc) return rc;
    rc = mt_batch_guided_knn2(mp->norm, words, q1, q2, kp1, kp2, kd, o1.data(), o2.data(), K, d_models, g, 0, device, s, idx, dist); if (rc) return rc;
    if (mutual) { rc = mt_batch_guided_knn2(mp->norm, words, q2, q1, kp2, kp1, kd, o2.data(), o1.data(), K, d_models, g, 1, device, s, bidx, bdist);
        if (rc) return rc; }
    rc = mt_batch_guided_decide(idx, dist, d_o1, d_o2, K, mp->ratio, bidx, s, match, cnt); if (rc) return rc;
    if (h_counts) {                                                  /* the only synchronisation, and only when asked for */
        MGCHK(hipMemcpyAsync(h_counts, cnt, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        MGCHK(hipStreamSynchronize(s));
    }
    return 0;
}

extern "C" int mi_degensac_match_guided_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                  const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2, int kp_dim, int n_pairs,
                                                  const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx,
                                                  float *d_dist, int32_t *d_match, int32_t *d_counts, int32_t *h_counts)
{
    return mg_batch_dev(mp, d_desc1, d_desc2, offsets1_host, offsets2_host, d_kp1, d_kp2, kp_dim, n_pairs, d_models, gp, device, (hipStream_t)stream,
                        d_idx, d_dist, d_match, d_counts, h_counts);
}

/* host pointers: stage, run the device path on the null stream, copy back */
extern "C" int mi_degensac_match_guided_batch(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                              const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim, int n_pairs, const double *models,
                                              const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist, int32_t *match, int32_t *counts)
{
    if (!mp) return mg_einval("match params are NULL");
    if (!(isfinite(mp->ratio) && mp->ratio > 0.f)) return mg_einval("ratio must be finite and > 0");
    mt_gate g; int rc = mg_check(mp->norm, mp->dim, kp_dim, gp, offsets1, offsets2, n_pairs, &g); if (rc) return rc;
    const int K = n_pairs;
    if (K == 0) return 0;
    if (!desc1 || !desc2 || !kp1 || !kp2 || !models || !idx || !dist || !match) return mg_einval("NULL argument");
    MgDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const int64_t n1 = offsets1[K] - offsets1[0], n2 = offsets2[K] - offsets2[0];
    const size_t row = mt_row_bytes(mp->norm, mp->dim);
    std::vector<int64_t> o1(K + 1), o2(K + 1);
    for (int p = 0; p <= K; p++) { o1[p] = offsets1[p] - offsets1[0]; o2[p] = offsets2[p] - offsets2[0]; }
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t a_d2 = up(n1 * row), a_k1 = a_d2 + up(n2 * row), a_k2 = a_k1 + up((size_t)n1 * kp_dim * 8), a_mo = a_k2 + up((size_t)n2 * kp_dim * 8),
                 a_ix = a_mo + up((size_t)K * 72), a_ds = a_ix + up((size_t)n1 * 8), a_ma = a_ds + up((size_t)n1 * 8), a_all = a_ma + up((size_t)n1 * 4);
    char *D = nullptr;
    struct Free { char *&p; ~Free() { (void)hipFree(p); } } fr{D};
    MGCHK(hipMalloc((void **)&D, a_all));
    MGCHK(hipMemcpy(D, (const char *)desc1 + offsets1[0] * row, n1 * row, hipMemcpyHostToDevice));
    MGCHK(hipMemcpy(D + a_d2, (const char *)desc2 + offsets2[0] * row, n2 * row, hipMemcpyHostToDevice));
    MGCHK(hipMemcpy(D + a_k1, kp1 + offsets1[0] * kp_dim, (size_t)n1 * kp_dim * 8, hipMemcpyHostToDevice));
    MGCHK(hipMemcpy(D + a_k2, kp2 + offsets2[0] * kp_dim, (size_t)n2 * kp_dim * 8, hipMemcpyHostToDevice));
    MGCHK(hipMemcpy(D + a_mo, models, (size_t)K * 72, hipMemcpyHostToDevice));
    std::vector<int32_t> cnt(K);
    rc = mg_batch_dev(mp, D, D + a_d2, o1.data(), o2.data(), (const double *)(D + a_k1), (const double *)(D + a_k2), kp_dim, K, (const double *)(D + a_mo),
                      gp, device, nullptr, (int32_t *)(D + a_ix), (float *)(D + a_ds), (int32_t *)(D + a_ma), nullptr, cnt.data());
    if (rc) return rc;
    MGCHK(hipStreamSynchronize(nullptr));
    MGCHK(hipMemcpy(idx + 2 * offsets1[0], D + a_ix, (size_t)n1 * 8, hipMemcpyDeviceToHost));
    MGCHK(hipMemcpy(dist + 2 * offsets1[0], D + a_ds, (size_t)n1 * 8, hipMemcpyDeviceToHost));
    MGCHK(hipMemcpy(match + offsets1[0], D + a_ma, (size_t)n1 * 4, hipMemcpyDeviceToHost));
    if (counts) memcpy(counts, cnt.data(), (size_t)K * 4);
    return 0;
}
