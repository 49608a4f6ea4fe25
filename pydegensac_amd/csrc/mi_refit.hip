/* libmi_degensac.so — refit F / H on exported correspondence lists (include/mi_degensac.h mi_degensac_refit_lists*): per entry of a
 * compact list (pts [cap, 4] and corr_offsets [K + 1] as the correspondence export writes them, both on the device) the members of the
 * start model under the estimator's own residual, then at most max_fits rounds of "non-minimal fit on the members, members of the fit".
 * gfx950 only, no CPU path.
 *
 * One workgroup of 256 threads per entry, further entries by a grid stride; no workgroup waits for another, no atomics.  The kernel reads
 * its row range o[p], o[p + 1] itself, so the host never learns a length and the call has no synchronisation.
 *   scoring pass   RF_STEP = 1024 rows per step, four per thread, 256 consecutive 32-byte rows per load instruction of the workgroup; the
 *                  residual of dg_geom.h in registers (the model is read from LDS once per pass); membership by wave ballot, the
 *                  positions from the per-(load, wave) popcounts through 2 x 16 LDS words and one barrier per step, so the member list is
 *                  in row order.  While a pass overwrites the list, the thread that owns position j compares the id it writes with the
 *                  id that stood there: with equal counts that is set equality.
 *   fit            the reference's non-minimal solvers as the drivers pick them (dg_kernel_f.h dg_u2f_list, dg_kernel_h.h dg_u2h_list):
 *                  F <= 16 members dg_u2f_small_w on wave 0, beyond dg_u2f_big; H <= 12 dg_u2h_small_w, beyond dg_u2h_big.  The big
 *                  variants gather the members into the entry's slice [2 o[p], 2 o[p + 1]) of a staging array of 2 cap dg_pt.
 *   final pass     inlier / resid of the entry's rows under the model that is kept, then the model (driver form, and for H the
 *                  user-facing inv(H_c^T) through dg_hsym_prepare, zeros when H_c is singular) and the info row. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#define DG_T 256
#include "dg_dev_small.h"
#include "dg_wg.h"
#include "dg_geom.h"
#include "dg_kernel_common.h"
#include "dg_lsq.h"
#include "dg_kernel_f.h"
#include "dg_kernel_f_main.h"
#include "dg_kernel_h.h"
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_host.h"

#define RF_LOADS 4                        /* rows per thread and step */
#define RF_STEP  (RF_LOADS * DG_T)        /* rows per workgroup and step */
#define RF_GRID  256                      /* cap on the grid: further entries by the grid stride */

enum { RF_F_SAMPSON = 0, RF_F_SYM = 1, RF_H_SAMPSON = 2, RF_H_SYM = 3 };      /* the gate kinds of mi_guided.hip */

struct rf_args {
    const dg_pt *pts;             /* [cap] */
    const int64_t *off;           /* [K + 1] */
    const double *models;         /* [K * 9] */
    double *models_out;           /* [K * 9] */
    double *models_user;          /* [K * 9] or null */
    uint8_t *inlier;              /* [cap] */
    int32_t *info;                /* [K * 4] or null */
    double *resid;                /* [cap] or null */
    dg_pt *stage;                 /* [2 * cap] */
    int32_t *list;                /* [cap] */
    int K; int64_t cap;
    double th; int hk, max_fits;
};

struct rf_shared {
    dg_lsq_scratch lsq;
    double best[9], cand[9], prep[18];     /* prep = Hinv | H1 of the model a pass scores (RF_H_SYM) */
    int cnt[2][RF_LOADS][DG_NW];
    int diff[DG_NW];
};

/* does the model pass anything at all: nine finite numbers, not all zero */
__device__ __forceinline__ bool rf_model_ok(const double *M)
{
    bool any = false, fin = true;
#pragma unroll
    for (int i = 0; i < 9; i++) { any = any || M[i] != 0.0; fin = fin && fabs(M[i]) <= 1.7976931348623157e308; }
    return any && fin;
}

template <int GK>
__device__ __forceinline__ double rf_resid(const double *M, const double *Hinv, const double *H1, int hk, const dg_pt &p)
{
    if (GK == RF_F_SAMPSON) return dg_FDs(M, p.x1, p.y1, p.x2, p.y2);
    if (GK == RF_F_SYM) return dg_FDsSym(M, p.x1, p.y1, p.x2, p.y2);
    if (GK == RF_H_SAMPSON) return dg_HDs(M, p.x1, p.y1, p.x2, p.y2);
    return dg_Hsym(Hinv, H1, p.x1, p.y1, p.x2, p.y2, hk, hk >= 3);
}

/* One pass over the n rows P of an entry under model Ms (LDS).  LIST: the members' row ids go to list[0 ..] in row order and *same says
 * whether they are the ids that stood there (meaningful where the count equals old_cnt).  FINAL: inl / res of every row instead.  Returns
 * the member count.  All threads of the workgroup, uniform control flow. */
template <int GK, bool FINAL>
__device__ __forceinline__ int rf_pass(rf_shared *S, const double *Ms, const dg_pt *P, int n, double th, int hk, int32_t *list, int old_cnt, bool *same,
                                       uint8_t *inl, double *res)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __syncthreads();                                                 /* Ms is written, the previous pass's LDS words are read */
    if (GK == RF_H_SYM && tid == 0) dg_hsym_prepare(Ms, S->prep, S->prep + 9);
    if (tid < DG_NW) S->diff[tid] = 0;
    __syncthreads();
    double M[9], Hinv[9], H1[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { M[i] = Ms[i]; Hinv[i] = GK == RF_H_SYM ? S->prep[i] : 0.0; H1[i] = GK == RF_H_SYM ? S->prep[9 + i] : 0.0; }
    const bool ok = rf_model_ok(M);
    const __attribute__((address_space(1))) double *G = (const __attribute__((address_space(1))) double *)(const double *)P;
    const unsigned long long below = (1ull << lane) - 1ull;
    int running = 0, buf = 0; bool differ = false;
    for (int base = 0; base < n; base += RF_STEP, buf ^= 1) {
        dg_pt p[RF_LOADS];
#pragma unroll
        for (int k = 0; k < RF_LOADS; k++) {                          /* the step's loads back to back; a row past the end reads row n - 1 */
            const int i = base + k * DG_T + tid, j = i < n ? i : n - 1;
            p[k].x1 = G[4 * (size_t)j]; p[k].y1 = G[4 * (size_t)j + 1]; p[k].x2 = G[4 * (size_t)j + 2]; p[k].y2 = G[4 * (size_t)j + 3];
        }
        unsigned f = 0u; int before[RF_LOADS];
#pragma unroll
        for (int k = 0; k < RF_LOADS; k++) {
            const int i = base + k * DG_T + tid;
            const double d = rf_resid<GK>(M, Hinv, H1, hk, p[k]);
            const bool m = i < n && ok && d <= th;                    /* a NaN residual is not a member */
            if (FINAL && i < n) { inl[i] = m ? 1 : 0; if (res) res[i] = d; }
            const unsigned long long bal = __ballot(m);
            before[k] = __popcll(bal & below);
            if (lane == 0) S->cnt[buf][k][wv] = __popcll(bal);
            f |= m ? 1u << k : 0u;
        }
        __syncthreads();
        /* position = the members before the step + those of the earlier loads and, in this load, of the lower waves + the ballot prefix */
        int pre = running;
#pragma unroll
        for (int k = 0; k < RF_LOADS; k++) {
            int mine = pre;
#pragma unroll
            for (int w = 0; w < DG_NW; w++) { const int c = S->cnt[buf][k][w]; if (w < wv) mine += c; pre += c; }
            if (!FINAL && ((f >> k) & 1u)) {
                const int pos = mine + before[k], id = base + k * DG_T + tid;
                if (pos < old_cnt && list[pos] != id) differ = true;
                list[pos] = id;
            }
        }
        running = pre;
    }
    if (!FINAL) {
        const unsigned long long any = __ballot(differ);
        if (lane == 0) S->diff[wv] = any != 0ull;
        __syncthreads();                                              /* also: the list is complete before the fit's gather reads it */
        int dsum = 0;
#pragma unroll
        for (int w = 0; w < DG_NW; w++) dsum += S->diff[w];
        *same = dsum == 0 && running == old_cnt;
    }
    return running;
}

/* the non-minimal fit on the listed rows of P into S->cand, the variant the drivers pick for that length */
template <int GK>
__device__ __forceinline__ void rf_fit(rf_shared *S, const dg_pt *P, const int32_t *list, int len, dg_pt *stage)
{
    const int tid = threadIdx.x;
    constexpr bool HOMOG = GK == RF_H_SAMPSON || GK == RF_H_SYM;
    if (len <= (HOMOG ? 12 : 16)) {
        __syncthreads();
        if (tid < 64) {
            if (tid < len) { const dg_pt q = dg_ldpt<0>(P, list[tid]); double *px = S->lsq.px + 4 * tid; px[0] = q.x1; px[1] = q.y1; px[2] = q.x2; px[3] = q.y2; }
            DG_WSYNC();
            if (HOMOG) dg_u2h_small_w(&S->lsq, S->lsq.px, len, S->cand, tid);
            else dg_u2f_small_w(&S->lsq, S->lsq.px, (const double *)0, len, S->cand, tid);
        }
        __syncthreads();
    } else {
        auto pt = [&](int i) { return dg_ldpt<0>(P, i); };
        if (HOMOG) dg_u2h_big((dg_red *)0, &S->lsq, pt, (const int *)list, len, tid, S->cand, stage, 2 * len, (double *)0);
        else dg_u2f_big((dg_red *)0, &S->lsq, pt, (const int *)list, len, tid, S->cand, stage, 2 * len);
    }
}

template <int GK>
__global__ __launch_bounds__(DG_T) void rf_refit_kernel(rf_args a)
{
    __shared__ rf_shared S;
    constexpr bool HOMOG = GK == RF_H_SAMPSON || GK == RF_H_SYM;
    constexpr int MINN = HOMOG ? 4 : 8;
    const int tid = threadIdx.x;
    for (int p = (int)blockIdx.x; p < a.K; p += (int)gridDim.x) {
        const int64_t b = a.off[p], e = a.off[p + 1];
        __syncthreads();                                              /* the previous entry's epilogue has read S.best */
        if (tid < 9) S.best[tid] = a.models[(size_t)p * 9 + tid];
        int n0 = 0, cnt = 0, fits = 0, status = MI_DEGENSAC_REFIT_MAX_FITS;
        const bool whole = b >= 0 && b <= e && e <= a.cap;            /* else a truncated export, or offsets that are not a list */
        if (!whole) status = MI_DEGENSAC_REFIT_TRUNCATED;
        else {
            const int n = (int)(e - b);
            const dg_pt *P = a.pts + b;
            int32_t *list = a.list + b;
            bool same = false;
            n0 = cnt = rf_pass<GK, false>(&S, S.best, P, n, a.th, a.hk, list, 0, &same, nullptr, nullptr);
            for (int it = 0; it < a.max_fits; it++) {
                if (cnt < MINN) { status = MI_DEGENSAC_REFIT_SHORT; break; }
                rf_fit<GK>(&S, P, list, cnt, a.stage + 2 * b);
                fits++;
                bool fin = true;
#pragma unroll
                for (int i = 0; i < 9; i++) fin = fin && fabs(S.cand[i]) <= 1.7976931348623157e308;
                if (!fin) { status = MI_DEGENSAC_REFIT_BAD_FIT; break; }
                const int c2 = rf_pass<GK, false>(&S, S.cand, P, n, a.th, a.hk, list, cnt, &same, nullptr, nullptr);
                if (c2 < cnt) { status = MI_DEGENSAC_REFIT_WORSE; break; }
                __syncthreads();
                if (tid < 9) S.best[tid] = S.cand[tid];
                cnt = c2;
                if (same) { status = MI_DEGENSAC_REFIT_FIXED; break; }
            }
            if (n > 0) (void)rf_pass<GK, true>(&S, S.best, P, n, a.th, a.hk, nullptr, 0, nullptr, a.inlier + b, a.resid ? a.resid + b : nullptr);
        }
        __syncthreads();
        if (tid < 9) a.models_out[(size_t)p * 9 + tid] = S.best[tid];
        if (HOMOG && a.models_user && tid == 0) {
            double M[9], Hinv[9], H1[9];
#pragma unroll
            for (int i = 0; i < 9; i++) M[i] = S.best[i];
            bool good = rf_model_ok(M);
#pragma unroll
            for (int i = 0; i < 9; i++) Hinv[i] = M[3 * (i % 3) + i / 3];
#pragma unroll
            for (int i = 0; i < 9; i++) H1[i] = good ? Hinv[i] : (i % 4 == 0 ? 1.0 : 0.0);
            good = dg_inv3(H1) == 0 && good;
#pragma unroll
            for (int i = 0; i < 9; i++) good = good && fabs(H1[i]) <= 1.7976931348623157e308;
#pragma unroll
            for (int i = 0; i < 9; i++) a.models_user[(size_t)p * 9 + i] = good ? H1[i] : 0.0;
        }
        if (!HOMOG && a.models_user && tid < 9) a.models_user[(size_t)p * 9 + tid] = S.best[tid];
        if (a.info && tid == 0) { int32_t *o = a.info + 4 * (size_t)p; o[0] = n0; o[1] = cnt; o[2] = fits; o[3] = status; }
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_refit_tile(int which) { return which == 0 ? RF_STEP : which == 1 ? RF_GRID : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int rf_check(const void *pts, const void *off, const void *models, const void *models_out, const void *inlier, int K, int64_t cap,
                    const mi_degensac_guide_params *gp, int max_fits, mt_gate *g)
{
    if (K < 0) return mi_einval("n_entries < 0");
    if (cap < 0) return mi_einval("cap < 0");
    if (cap > 0x3fffffff) return mi_einval("too many rows in one list (cap > 0x3fffffff)");
    if (max_fits < 0) return mi_einval("max_fits < 0");
    if (!gp) return mi_einval("guide params are NULL");
    if (gp->struct_size != 0 && gp->struct_size < (int32_t)sizeof(mi_degensac_guide_params)) return mi_einval("guide params: struct_size too small");
    if (gp->homography != 0 && gp->homography != 1) return mi_einval("homography must be 0 or 1");
    const int rc = mt_guided_gate(gp->homography, gp->error_type, gp->px_th, g); if (rc) return rc;
    if (!off) return mi_einval("NULL argument: corr_offsets");
    if (K > 0 && (!models || !models_out)) return mi_einval("NULL argument: models and models_out");
    if (cap > 0 && (!pts || !inlier)) return mi_einval("NULL argument: pts and inlier");
    return 0;
}

extern "C" int mi_degensac_refit_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const double *d_models, int n_entries, int64_t cap,
                                           const mi_degensac_guide_params *gp, int max_fits, int device, void *stream, double *d_models_out,
                                           uint8_t *d_inlier, double *d_models_user, int32_t *d_info, double *d_resid)
{
    mt_gate g; int rc = rf_check(d_pts, d_corr_offsets, d_models, d_models_out, d_inlier, n_entries, cap, gp, max_fits, &g); if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (cap > 0) {                                                    /* positions that no entry owns keep 0 / NaN */
        MICHK(hipMemsetAsync(d_inlier, 0, (size_t)cap, s));
        if (d_resid) MICHK(hipMemsetAsync(d_resid, 0xff, (size_t)cap * 8, s));      /* all bits set: a NaN */
    }
    if (n_entries == 0) return 0;
    const size_t a_list = (size_t)cap * 64, a_all = a_list + (size_t)cap * 4 + 256;
    MiScratch scr; rc = scr.alloc(a_all, s); if (rc) return rc;
    char *blk = scr.p;
    rf_args a;
    memset(&a, 0, sizeof a);
    a.pts = (const dg_pt *)d_pts; a.off = d_corr_offsets; a.models = d_models; a.models_out = d_models_out; a.models_user = d_models_user;
    a.inlier = d_inlier; a.info = d_info; a.resid = d_resid; a.stage = (dg_pt *)blk; a.list = (int32_t *)(blk + a_list);
    a.K = n_entries; a.cap = cap; a.th = g.th; a.hk = g.hk; a.max_fits = max_fits;
    const dim3 grid((unsigned)std::min(n_entries, RF_GRID)), block(DG_T);
    switch (g.gk) {
    case RF_F_SAMPSON: hipLaunchKernelGGL((rf_refit_kernel<RF_F_SAMPSON>), grid, block, 0, s, a); break;
    case RF_F_SYM: hipLaunchKernelGGL((rf_refit_kernel<RF_F_SYM>), grid, block, 0, s, a); break;
    case RF_H_SAMPSON: hipLaunchKernelGGL((rf_refit_kernel<RF_H_SAMPSON>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((rf_refit_kernel<RF_H_SYM>), grid, block, 0, s, a); break;
    }
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_refit_lists(const double *pts, const int64_t *corr_offsets, const double *models, int n_entries, int64_t cap,
                                       const mi_degensac_guide_params *gp, int max_fits, int device, double *models_out, uint8_t *inlier,
                                       double *models_user, int32_t *info, double *resid)
{
    mt_gate g; int rc = rf_check(pts, corr_offsets, models, models_out, inlier, n_entries, cap, gp, max_fits, &g); if (rc) return rc;
    if (n_entries == 0 && cap == 0) return 0;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t K = (size_t)n_entries, C = (size_t)cap;
    MiStage st;
    const int i_pts = st.in(pts, C * 32), i_off = st.in(corr_offsets, (K + 1) * 8), i_mo = st.in(models, K * 72), o_out = st.out(models_out, K * 72),
              o_inl = st.out(inlier, C), o_us = st.out(models_user, K * 72), o_inf = st.out(info, K * 16), o_res = st.out(resid, C * 8);
    rc = st.upload(); if (rc) return rc;
    rc = mi_degensac_refit_lists_dev(st.dev<double>(i_pts), st.dev<int64_t>(i_off), st.dev<double>(i_mo), n_entries, cap, gp, max_fits, device, nullptr,
                                     st.dev<double>(o_out), st.dev<uint8_t>(o_inl), st.dev<double>(o_us), st.dev<int32_t>(o_inf), st.dev<double>(o_res));
    if (rc) return rc;
    return st.finish();
}
