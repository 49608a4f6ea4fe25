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
 * and slower than the dense matcher (one distance per lane instead of a 4 x 4 register block over LDS tiles).
 *
 * One path for two layouts, as in mi_matcher.hip: a "pair" is an entry of a list over image stores (mi_degensac_match_guided_*_pairs*,
 * rows from mt_pairs_layout: descriptors and keypoints stored once per image, one model per ENTRY, answers pair after pair in list
 * order) or of the ragged batch (mi_degensac_match_guided_*_batch*), which is the list whose entry p is (image p, image p) with its
 * answers at its queries' own rows (mt_identity_rows).  No row is gathered or copied for either. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_host.h"
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

/* grid = one workgroup per tile of MG_Q queries of one list entry.  toff [K + 1]: entry p owns tiles toff[p] .. toff[p+1] - 1; rows [K]: its
 * record (mi_match_batch.h).  swap = 0: the queries are rows q .. q + nq of dq / kq (side 1), the candidates rows t .. t + nt of dt / kt
 * (side 2), the answers go to the rows out .. out + nq of idx / dist; swap = 1 (the reverse search): dq / kq are side 2 and dt / kt side 1,
 * the queries are rows t .. t + nt, the candidates rows q .. q + nq, the answers go to the rows back .. back + nt.  In a ragged batch the
 * answers lie at the queries' own rows; in a pair list, where an image is stored once and queried by many entries, they do not.  The
 * model is that of the entry, models[9 p ..].  The record is wave-uniform (it follows blockIdx), so it costs scalar loads only.
 * Every branch around a barrier or a ballot is uniform: the chunk loop over the workgroup, query slots and list counts over the wave. */
template <int NORM, int GK>
__global__ __launch_bounds__(256) void mg_guided_kernel(const uint32_t *dq, const uint32_t *dt, int words, const double *kq, const double *kt, int kd,
                                                        const int32_t *toff, const mt_pair_rows *rows, int n_pairs, const double *models, int hk,
                                                        double th, double tb, int screen, int swap, int32_t *idx, float *dist)
{
    __shared__ double2 ts[MG_TC];
    __shared__ int lists[MG_W][MG_QPW][MG_LIST];
    const int b = (int)blockIdx.x;
    int lo = 0, hi = n_pairs - 1;                                    /* the last entry p with toff[p] <= b (an entry without queries owns no tile) */
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (toff[mid] <= b) lo = mid; else hi = mid - 1; }
    const int pair = lo;
    const mt_pair_rows r = rows[pair];
    const int q_b = swap ? r.t : r.q, n_q = swap ? r.nt : r.nq, t_b = swap ? r.q : r.t, n_t = swap ? r.nq : r.nt;
    const int q0 = q_b + (b - toff[pair]) * MG_Q, q_end = q_b + n_q;
    const int o_d = (swap ? r.back : r.out) - q_b;                   /* query row q answers at row q + o_d */
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double M[9], Hinv[9], H1[9];
    bool any = false;
#pragma unroll
    for (int i = 0; i < 9; i++) { M[i] = models[(size_t)pair * 9 + i]; any = any || M[i] != 0.0; }
    if (GK == MG_H_SYM) dg_hsym_prepare(M, Hinv, H1);
    const int t_e = any ? t_b + n_t : t_b;                           /* a zero model has no candidates */
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
            const size_t o = (size_t)(q + o_d);
            idx[2 * o] = m.i0; idx[2 * o + 1] = m.i1;
            dist[2 * o] = NORM != 1 ? sqrtf(m.d0) : m.d0; dist[2 * o + 1] = NORM != 1 ? sqrtf(m.d1) : m.d1;
        }
    }
}

/* FGINN inside the gate (include/mi_degensac.h mi_degensac_match_guided_fginn_*): the second distance of a guided query comes from the
 * nearest GATED train row whose keypoint lies at least r from the keypoint of the nearest gated row (the anchor, slot 0).  The gate takes
 * the look-alikes elsewhere in the image away and leaves a keypoint's own twin (a second orientation, a neighbouring scale) as its only
 * second neighbour; the twin lies inside the band too, so the plain guided rule drops exactly those queries.  A gated row t competes for
 * slot 1 iff t != i0 and dx dx + dy dy >= r r (dx = x2[t] - x2[i0], dy = y2[t] - y2[i0], fp64 in that order, a NaN is false): the rule of
 * mi_fginn.h word for word, applied after the gate.  The decision stays the guided one: a query whose only gated companions lie inside
 * the radius has dist1 = inf and is KEPT (nothing competes with it), where the unguided FGINN filter needs a second row.
 *
 * mg_guided_kernel runs unchanged; mf_mark_kernel (mi_fginn.h, through mt_batch_fginn_mark) lists per entry, in ascending query order,
 * the NEEDY queries (slot 1 exists and does not compete) as OUTPUT rows.  This kernel rescans only those, in the guided kernel's shape:
 * the grid is the forward search's tile table (the worst case, every query needy; no host synchronisation), tile k of an entry owns the
 * list positions MG_Q k .. of that entry and returns at once when they lie at or beyond the entry's needy count (uniform over the
 * workgroup, before any barrier).  A needy query has TWO rows: its output row o (the list's value; the anchor idx[o][0] is read and
 * slot 1 written there) and its query row in store 1, r.q + (o - r.out); only a ragged batch has them equal.  The anchor's x, y are
 * wave-uniform per query and the exclusion test is part of the pass predicate, so the candidate lists, their flushes at 64 with a carry
 * and the distances are those of the forward search; of the top-2 only slot 0 is merged and written, to slot 1 of the output row. */
template <int NORM, int GK>
__global__ __launch_bounds__(256) void mg_rescan_kernel(const uint32_t *dq, const uint32_t *dt, int words, const double *kq, const double *kt, int kd,
                                                        const int32_t *toff, const mt_pair_rows *rows, int n_pairs, const double *models, int hk,
                                                        double th, double tb, int screen, const int32_t *list, const int32_t *count, double rr,
                                                        int32_t *idx, float *dist)
{
    __shared__ double2 ts[MG_TC];
    __shared__ int lists[MG_W][MG_QPW][MG_LIST];
    const int b = (int)blockIdx.x;
    int lo = 0, hi = n_pairs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (toff[mid] <= b) lo = mid; else hi = mid - 1; }
    const int pair = lo;
    const mt_pair_rows r = rows[pair];
    const int k0 = (b - toff[pair]) * MG_Q, k_end = count[pair];     /* list positions of this tile, the entry's needy count (<= r.nq) */
    if (k0 >= k_end) return;                                         /* uniform over the workgroup */
    const int t_b = r.t, n_t = r.nt;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double M[9], Hinv[9], H1[9];
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = models[(size_t)pair * 9 + i];  /* a needy query has two gated rows: the model is not zero */
    if (GK == MG_H_SYM) dg_hsym_prepare(M, Hinv, H1);
    const int t_e = t_b + n_t;
    double qx[MG_QPW], qy[MG_QPW], ax[MG_QPW], ay[MG_QPW]; int cnt[MG_QPW], orow[MG_QPW], anc[MG_QPW]; mt_best best[MG_QPW];
#pragma unroll
    for (int j = 0; j < MG_QPW; j++) {
        const int k = k0 + wv + MG_W * j;
        const bool on = k < k_end;                                   /* wave-uniform */
        orow[j] = on ? list[r.out + k] : r.out;
        anc[j] = on ? idx[2 * (size_t)orow[j]] : -1;
        const size_t q = (size_t)(r.q + (orow[j] - r.out));
        qx[j] = on ? kq[q * kd] : 0.0; qy[j] = on ? kq[q * kd + 1] : 0.0;
        ax[j] = anc[j] >= 0 ? kt[(size_t)(t_b + anc[j]) * kd] : 0.0; ay[j] = anc[j] >= 0 ? kt[(size_t)(t_b + anc[j]) * kd + 1] : 0.0;
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
                if (k0 + wv + MG_W * j >= k_end) continue;                         /* wave-uniform */
                const double dx = p.x - ax[j], dy = p.y - ay[j];
                const bool pass = in && t - t_b != anc[j] && dx * dx + dy * dy >= rr
                                  && mg_gate<GK>(M, Hinv, H1, hk, th, tb, screen, qx[j], qy[j], p.x, p.y);
                const unsigned long long bal = __ballot(pass);
                int *lst = lists[wv][j];
                if (pass) lst[cnt[j] + __popcll(bal & ((1ull << lane) - 1ull))] = t - t_b;
                cnt[j] += __popcll(bal);
                if (cnt[j] >= 64) {                                                /* wave-uniform */
                    mg_flush<NORM>(dq + (size_t)(r.q + (orow[j] - r.out)) * words, dt, words, t_b, lst, 64, lane, best[j]);
                    if (lane < cnt[j] - 64) lst[lane] = lst[64 + lane];
                    cnt[j] -= 64;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MG_QPW; j++) {
        if (k0 + wv + MG_W * j >= k_end) continue;
        if (cnt[j] > 0) mg_flush<NORM>(dq + (size_t)(r.q + (orow[j] - r.out)) * words, dt, words, t_b, lists[wv][j], cnt[j], lane, best[j]);
        float d = best[j].d0; int i = best[j].i0;
        for (int k = 1; k < 64; k <<= 1) {                                         /* the minimum in (distance, index) order */
            const float d2 = __shfl_xor(d, k); const int i2 = __shfl_xor(i, k);
            if (i2 >= 0 && (i < 0 || d2 < d || (d2 == d && i2 < i))) { d = d2; i = i2; }
        }
        if (lane == 0) {
            const size_t o = (size_t)orow[j] * 2 + 1;
            idx[o] = i; dist[o] = NORM != 1 ? sqrtf(d) : d;
        }
    }
}

/* one workgroup per pair: every query's decision and the pair's number of guided matches */
__global__ __launch_bounds__(256) void mg_decide_kernel(const int32_t *idx, const float *dist, const int32_t *off1, const int32_t *off2, mt_rule rule,
                                                        const int32_t *back, const float *bdist, int32_t *match, int32_t *count)
{
    __shared__ int wsum[4];
    const int p = blockIdx.x, lo = off1[p], hi = off1[p + 1], b2 = off2[p];
    int c = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const bool ok = mt_decide<true>(rule, idx, dist, i, i - lo, back, bdist, b2);     /* one candidate: dist[1] = inf, the query passes */
        match[i] = ok ? idx[2 * i] : -1;
        c += ok ? 1 : 0;
    }
    for (int k = 32; k >= 1; k >>= 1) c += __shfl_xor(c, k);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0 && count) count[p] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
int mt_guided_gate(int homography, int error_type, double px_th, mt_gate *g)
{
    if (!(px_th >= 0)) return mi_einval("px_th must be >= 0 (not NaN)");
    if (!homography) {
        if (error_type != 0 && error_type != 1) return mi_einval("error_type must be 0 or 1 for the fundamental matrix");
        g->gk = error_type; g->hk = 0; g->th = px_th * px_th;
    } else {
        if (error_type < 0 || error_type > 4) return mi_einval("error_type must be 0..4 for the homography");
        g->gk = error_type == 0 ? MG_H_SAMPSON : MG_H_SYM; g->hk = error_type;
        g->th = (error_type == 2 || error_type == 4) ? px_th : px_th * px_th;
    }
    /* the screens' bound: 1 % above th (the symmetric H kinds screen d1: th, or th^2 for the square-root kinds 2 and 4) */
    const double t1 = (homography && (error_type == 2 || error_type == 4)) ? g->th * g->th : g->th;
    g->tb = t1 * 1.01; g->screen = g->th > 0 ? 1 : 0;
    return 0;
}

/* the forward / reverse search's tile table, one upload: the tile starts [K + 1], then (16-byte aligned, at *a_rows) the entries' records
 * as they are; returns the number of tiles */
static int64_t mg_tile_table(const mt_pair_rows *rows, int n_pairs, int swap, std::vector<char> &tab, size_t *a_rows)
{
    *a_rows = ((size_t)(n_pairs + 1) * 4 + 15) / 16 * 16;
    tab.resize(*a_rows + (size_t)n_pairs * sizeof(mt_pair_rows));
    int32_t *toff = (int32_t *)tab.data();
    int64_t tiles = 0;
    for (int p = 0; p <= n_pairs; p++) {
        toff[p] = (int32_t)tiles;
        if (p < n_pairs) tiles += ((swap ? rows[p].nt : rows[p].nq) + MG_Q - 1) / MG_Q;
    }
    memcpy(tab.data() + *a_rows, rows, (size_t)n_pairs * sizeof(mt_pair_rows));
    return tiles;
}

/* one launch per (norm, gate kind): KERNEL<N, G> with the arguments after it */
#define MG_DISPATCH(norm, gk, LAUNCH) switch (4 * mt_norm_index(norm) + (gk)) { \
    case 0: LAUNCH(0, MG_F_SAMPSON); break;  case 1: LAUNCH(0, MG_F_SYM); break;  case 2: LAUNCH(0, MG_H_SAMPSON); break;  case 3: LAUNCH(0, MG_H_SYM); break; \
    case 4: LAUNCH(1, MG_F_SAMPSON); break;  case 5: LAUNCH(1, MG_F_SYM); break;  case 6: LAUNCH(1, MG_H_SAMPSON); break;  case 7: LAUNCH(1, MG_H_SYM); break; \
    case 8: LAUNCH(2, MG_F_SAMPSON); break;  case 9: LAUNCH(2, MG_F_SYM); break;  case 10: LAUNCH(2, MG_H_SAMPSON); break; default: LAUNCH(2, MG_H_SYM); break; }

int mt_batch_guided_knn2(int norm, int words, const void *dq, const void *dt, const double *kq, const double *kt, int kd, const mt_pair_rows *rows,
                         int n_pairs, int n_rows, const double *d_models, const mt_gate &g, int swap, int device, hipStream_t s, int32_t *idx,
                         float *dist)
{
    if (n_pairs <= 0 || n_rows == 0) return 0;
    std::vector<char> tab; size_t a_rows;
    const int64_t tiles = mg_tile_table(rows, n_pairs, swap, tab, &a_rows);
    const size_t bytes = tab.size();
    char *d_tab = nullptr;
    MICHK(hipMallocAsync((void **)&d_tab, bytes, s));
    int rc = mt_batch_upload(device, s, tab.data(), bytes, d_tab);
    if (rc) { (void)hipFreeAsync(d_tab, s); return rc; }
    const dim3 grid((unsigned)tiles), block(256);
#define MG_LAUNCH(N, G) hipLaunchKernelGGL((mg_guided_kernel<N, G>), grid, block, 0, s, (const uint32_t *)dq, (const uint32_t *)dt, words, kq, kt, kd, \
        (const int32_t *)d_tab, (const mt_pair_rows *)(d_tab + a_rows), n_pairs, d_models, g.hk, g.th, g.tb, g.screen, swap, idx, dist)
    MG_DISPATCH(norm, g.gk, MG_LAUNCH)
#undef MG_LAUNCH
    const hipError_t le = hipGetLastError();
    (void)hipFreeAsync(d_tab, s);
    MICHK(le);
    return 0;
}

/* one stream-ordered block: the tile table | the needy lists (one int32 per output row) | the needy counts [K] */
int mt_batch_guided_fginn(int norm, int words, const void *dq, const void *dt, const double *kq, const double *kt, int kd, const mt_pair_rows *rows,
                          int n_pairs, int n_rows, const double *d_models, const mt_gate &g, double r, int device, hipStream_t s, int32_t *idx,
                          float *dist)
{
    if (n_pairs <= 0 || n_rows == 0) return 0;
    std::vector<char> tab; size_t a_rows;
    const int64_t tiles = mg_tile_table(rows, n_pairs, 0, tab, &a_rows);
    const size_t a_list = mi_up256(tab.size()), a_cnt = a_list + mi_up256((size_t)n_rows * 4), a_all = a_cnt + mi_up256((size_t)n_pairs * 4);
    MiScratch scr; int rc = scr.alloc(a_all, s); if (rc) return rc;
    char *blk = scr.p;
    rc = mt_batch_upload(device, s, tab.data(), tab.size(), blk); if (rc) return rc;
    const mt_pair_rows *d_rows = (const mt_pair_rows *)(blk + a_rows);
    int32_t *list = (int32_t *)(blk + a_list), *cnt = (int32_t *)(blk + a_cnt);
    const double rr = r * r;
    rc = mt_batch_fginn_mark(idx, d_rows, n_pairs, kt, kd, rr, s, list, cnt); if (rc) return rc;
    const dim3 grid((unsigned)tiles), block(256);
#define MG_LAUNCH(N, G) hipLaunchKernelGGL((mg_rescan_kernel<N, G>), grid, block, 0, s, (const uint32_t *)dq, (const uint32_t *)dt, words, kq, kt, kd, \
        (const int32_t *)blk, d_rows, n_pairs, d_models, g.hk, g.th, g.tb, g.screen, list, cnt, rr, idx, dist)
    MG_DISPATCH(norm, g.gk, MG_LAUNCH)
#undef MG_LAUNCH
    MICHK(hipGetLastError());
    return 0;
}

int mt_batch_guided_decide(const int32_t *d_idx, const float *d_dist, const int32_t *d_off1, const int32_t *d_off2, int n_pairs, const mt_rule &rule,
                           const int32_t *d_back, const float *d_bdist, hipStream_t s, int32_t *d_match, int32_t *d_count)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(mg_decide_kernel, dim3(n_pairs), dim3(256), 0, s, d_idx, d_dist, d_off1, d_off2, rule, d_back, d_bdist, d_match, d_count);
    MICHK(hipGetLastError());
    return 0;
}

/* ---- C-ABI ----------------------------------------------------------------------------------------------------------- */
/* norm, dim, keypoint width and the gate: what both layouts refuse before they look at offsets or a list */
static int mg_check_gate(int norm, int dim, int kp_dim, const mi_degensac_guide_params *gp, mt_gate *g)
{
    if (!mt_norm_known(norm) || dim <= 0) return mi_einval("bad norm or descriptor dim");
    if (const char *e = mt_norm_dim_error(norm, dim)) return mi_einval(e);
    if (kp_dim != 2 && kp_dim != 6) return mi_einval("keypoint rows must be [n,2] or [n,6]");
    if (!gp) return mi_einval("guide params are NULL");
    if (gp->struct_size != 0 && gp->struct_size < (int32_t)sizeof(mi_degensac_guide_params)) return mi_einval("guide params: struct_size too small");
    if (gp->homography != 0 && gp->homography != 1) return mi_einval("homography must be 0 or 1");
    return mt_guided_gate(gp->homography, gp->error_type, gp->px_th, g);
}

/* the ratio and the decision rule (mt_decide_rule); honour: the entry point reads second_nn, which NO_RATIO / BACK_RATIO exclude */
static int mg_check_ratio(const mi_degensac_match_params *mp, int honour, mt_rule *rule)
{
    if (!mp) return mi_einval("match params are NULL");
    if (const char *e = mt_decide_rule(mp, honour, rule)) return mi_einval(e);
    return 0;
}

/* the second-neighbour rule of a guided call.  honour = 0 (the plain entry points): second_nn / spatial_th are not read.  honour = 1 (the
 * guided_fginn entry points): mt_second_nn, so a struct_size that does not cover spatial_th, or second_nn = 0, is the plain call */
struct mg_second { int fginn; double r; };
static int mg_check_second(const mi_degensac_match_params *mp, int honour, mg_second *sn)
{
    sn->fginn = 0; sn->r = 0.0;
    if (!honour) return 0;
    if (const char *e = mt_second_nn(mp, &sn->fginn, &sn->r)) return mi_einval(e);
    return 0;
}
/* the radius of the guided_fginn_knn2 entry points */
static int mg_check_radius(double spatial_th)
{
    if (const char *e = mt_spatial_th_error(spatial_th)) return mi_einval(e);
    return 0;
}

/* the ragged batch */
static int mg_check(int norm, int dim, int kp_dim, const mi_degensac_guide_params *gp, const int64_t *o1, const int64_t *o2, int n_pairs, mt_gate *g)
{
    int rc = mg_check_gate(norm, dim, kp_dim, gp, g); if (rc) return rc;
    if (n_pairs < 0) return mi_einval("n_pairs < 0");
    if (n_pairs == 0) return 0;
    for (const int64_t *o : {o1, o2}) {
        if (!o || o[0] < 0) return mi_einval("offsets must be given and start at >= 0");
        for (int p = 0; p < n_pairs; p++) if (o[p + 1] < o[p]) return mi_einval("offsets must be non-decreasing");
        if (o[n_pairs] - o[0] > 0x3fffffff) return mi_einval("too many descriptor rows in one batch");
    }
    return 0;
}

/* the pair list: the gate, then the list (mt_pairs_layout: n_pairs < 0, offsets, image indices, the row limits) */
static int mg_check_pairs(int norm, int dim, int kp_dim, const mi_degensac_guide_params *gp, const int64_t *off1, int m1, const int64_t *off2, int m2,
                          const int32_t *pairs, int n_pairs, mt_gate *g, std::vector<mt_pair_rows> &rows, int64_t *n_out, int64_t *n_back)
{
    *n_out = *n_back = 0;
    int rc = mg_check_gate(norm, dim, kp_dim, gp, g); if (rc) return rc;
    if (n_pairs < 0) return mi_einval("n_pairs < 0");
    if (n_pairs == 0) return 0;
    rows.resize(n_pairs);
    return mt_pairs_layout(off1, m1, off2, m2, pairs, n_pairs, rows.data(), n_out, n_back);
}

static int mg_words(int norm, int dim) { return mt_row_words(norm, dim); }

/* the guided 2-NN of a ragged batch; fginn: then slot 1 by the FGINN rule at radius r */
static int mg_knn2_batch_dev(int fginn, double r, int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                             const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp1, const double *d_kp2, int kp_dim,
                             const double *d_models, const mi_degensac_guide_params *gp, int device, hipStream_t s, int32_t *d_idx, float *d_dist)
{
    mt_gate g; int rc = mg_check(norm, dim, kp_dim, gp, offsets1_host, offsets2_host, n_pairs, &g); if (rc) return rc;
    if (fginn) { rc = mg_check_radius(r); if (rc) return rc; }
    if (n_pairs == 0) return 0;
    const int64_t n1 = offsets1_host[n_pairs] - offsets1_host[0], n2 = offsets2_host[n_pairs] - offsets2_host[0];
    if (!d_models || (n1 > 0 && (!d_desc1 || !d_kp1 || !d_idx || !d_dist)) || (n2 > 0 && (!d_desc2 || !d_kp2))) return mi_einval("NULL argument");
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const int words = mg_words(norm, dim);
    std::vector<int64_t> o1, o2; std::vector<mt_pair_rows> rows;
    mt_ragged_rows(offsets1_host, offsets2_host, n_pairs, o1, o2, rows);
    const uint32_t *q1 = (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words, *q2 = (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words;
    const double *k1 = d_kp1 + (size_t)offsets1_host[0] * kp_dim, *k2 = d_kp2 + (size_t)offsets2_host[0] * kp_dim;
    int32_t *idx = d_idx + 2 * offsets1_host[0]; float *dist = d_dist + 2 * offsets1_host[0];
    rc = mt_batch_guided_knn2(norm, words, q1, q2, k1, k2, kp_dim, rows.data(), n_pairs, (int)n1, d_models, g, 0, device, s, idx, dist);
    if (rc || !fginn) return rc;
    return mt_batch_guided_fginn(norm, words, q1, q2, k1, k2, kp_dim, rows.data(), n_pairs, (int)n1, d_models, g, r, device, s, idx, dist);
}

extern "C" int mi_degensac_match_guided_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                       const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp1, const double *d_kp2,
                                                       int kp_dim, const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream,
                                                       int32_t *d_idx, float *d_dist)
{
    return mg_knn2_batch_dev(0, 0.0, norm, d_desc1, d_desc2, offsets1_host, offsets2_host, n_pairs, dim, d_kp1, d_kp2, kp_dim, d_models, gp, device,
                             (hipStream_t)stream, d_idx, d_dist);
}

extern "C" int mi_degensac_match_guided_fginn_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                             const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp1,
                                                             const double *d_kp2, int kp_dim, const double *d_models,
                                                             const mi_degensac_guide_params *gp, double spatial_th, int device, void *stream,
                                                             int32_t *d_idx, float *d_dist)
{
    return mg_knn2_batch_dev(1, spatial_th, norm, d_desc1, d_desc2, offsets1_host, offsets2_host, n_pairs, dim, d_kp1, d_kp2, kp_dim, d_models, gp,
                             device, (hipStream_t)stream, d_idx, d_dist);
}

/* The device path of both layouts, arguments checked and the device current: entry p's rows are rows[p], n_out output rows and n_back
 * rows of the reverse search in all; every pointer is already at its side's first row, idx / dist / match at the first output row. */
static int mg_rows_dev(const mi_degensac_match_params *mp, const mt_rule &rule, const uint32_t *q1, const uint32_t *q2, const double *kp1, const double *kp2, int kd,
                       const std::vector<mt_pair_rows> &rows, int64_t n_out, int64_t n_back, const double *d_models, const mt_gate &g,
                       const mg_second &sn, int device, hipStream_t s, int32_t *idx, float *dist, int32_t *match, int32_t *d_counts, int32_t *h_counts)
{
    const int K = (int)rows.size();
    const int words = mg_words(mp->norm, mp->dim);
    const bool mutual = mp->mutual != 0;
    /* the decision's tables: out [K + 1] (where the entry's idx / dist / match rows are) | back [K] (where its reverse-search rows start) */
    std::vector<int32_t> o32(2 * (size_t)(K + 1));
    for (int p = 0; p < K; p++) { o32[p] = rows[p].out; o32[K + 1 + p] = rows[p].back; }
    o32[K] = (int32_t)n_out; o32[2 * K + 1] = (int32_t)n_back;
    /* one stream-ordered block: tables | reverse idx | reverse dist | counts (when the caller gives none on the device) */
    const size_t a_bidx = mi_up256(o32.size() * 4), a_bdist = a_bidx + (mutual ? mi_up256((size_t)n_back * 8) : 0),
                 a_cnt = a_bdist + (mutual ? mi_up256((size_t)n_back * 8) : 0), a_all = a_cnt + mi_up256((size_t)K * 4);
    MiScratch scr; int rc = scr.alloc(a_all, s); if (rc) return rc;
    char *blk = scr.p;
    const int32_t *d_out = (const int32_t *)blk, *d_back = d_out + (K + 1);
    int32_t *bidx = mutual ? (int32_t *)(blk + a_bidx) : nullptr, *cnt = d_counts ? d_counts : (int32_t *)(blk + a_cnt);
    float *bdist = (float *)(blk + a_bdist);
    rc = mt_batch_upload(device, s, o32.data(), o32.size() * 4, blk); if (rc) return rc;
    rc = mt_batch_guided_knn2(mp->norm, words, q1, q2, kp1, kp2, kd, rows.data(), K, (int)n_out, d_models, g, 0, device, s, idx, dist); if (rc) return rc;
    /* FGINN inside the gate judges the forward search only: the reverse search and the mutual check stay the plain ones (slot 0) */
    if (sn.fginn) { rc = mt_batch_guided_fginn(mp->norm, words, q1, q2, kp1, kp2, kd, rows.data(), K, (int)n_out, d_models, g, sn.r, device, s, idx, dist);
        if (rc) return rc; }
    if (mutual) { rc = mt_batch_guided_knn2(mp->norm, words, q2, q1, kp2, kp1, kd, rows.data(), K, (int)n_back, d_models, g, 1, device, s, bidx, bdist);
        if (rc) return rc; }
    rc = mt_batch_guided_decide(idx, dist, d_out, d_back, K, rule, bidx, mutual ? bdist : nullptr, s, match, cnt); if (rc) return rc;
    if (h_counts) {                                                  /* the only synchronisation, and only when asked for */
        MICHK(hipMemcpyAsync(h_counts, cnt, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        MICHK(hipStreamSynchronize(s));
    }
    return 0;
}

static int mg_batch_dev(int honour, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *off1, const int64_t *off2,
                        const double *d_kp1, const double *d_kp2, int kd, int K, const double *d_models, const mi_degensac_guide_params *gp, int device,
                        hipStream_t s, int32_t *d_idx, float *d_dist, int32_t *d_match, int32_t *d_counts, int32_t *h_counts)
{
    mt_rule rule; int rc = mg_check_ratio(mp, honour, &rule); if (rc) return rc;
    mt_gate g; rc = mg_check(mp->norm, mp->dim, kd, gp, off1, off2, K, &g); if (rc) return rc;
    mg_second sn; rc = mg_check_second(mp, honour, &sn); if (rc) return rc;
    if (K == 0) return 0;
    const int64_t n1 = off1[K] - off1[0], n2 = off2[K] - off2[0];
    if (!d_models || (n1 > 0 && (!d_desc1 || !d_kp1 || !d_idx || !d_dist || !d_match)) || (n2 > 0 && (!d_desc2 || !d_kp2))) return mi_einval("NULL argument");
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const int words = mg_words(mp->norm, mp->dim);
    std::vector<int64_t> o1, o2; std::vector<mt_pair_rows> rows;
    mt_ragged_rows(off1, off2, K, o1, o2, rows);
    return mg_rows_dev(mp, rule, (const uint32_t *)d_desc1 + (size_t)off1[0] * words, (const uint32_t *)d_desc2 + (size_t)off2[0] * words,
                       d_kp1 + (size_t)off1[0] * kd, d_kp2 + (size_t)off2[0] * kd, kd, rows, n1, n2, d_models, g, sn, device, s, d_idx + 2 * off1[0],
                       d_dist + 2 * off1[0], d_match + off1[0], d_counts, h_counts);
}

extern "C" int mi_degensac_match_guided_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                  const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2, int kp_dim, int n_pairs,
                                                  const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx,
                                                  float *d_dist, int32_t *d_match, int32_t *d_counts, int32_t *h_counts)
{
    return mg_batch_dev(0, mp, d_desc1, d_desc2, offsets1_host, offsets2_host, d_kp1, d_kp2, kp_dim, n_pairs, d_models, gp, device, (hipStream_t)stream,
                        d_idx, d_dist, d_match, d_counts, h_counts);
}

extern "C" int mi_degensac_match_guided_fginn_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                                        const int64_t *offsets1_host, const int64_t *offsets2_host, const double *d_kp1,
                                                        const double *d_kp2, int kp_dim, int n_pairs, const double *d_models,
                                                        const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx, float *d_dist,
                                                        int32_t *d_match, int32_t *d_counts, int32_t *h_counts)
{
    return mg_batch_dev(1, mp, d_desc1, d_desc2, offsets1_host, offsets2_host, d_kp1, d_kp2, kp_dim, n_pairs, d_models, gp, device, (hipStream_t)stream,
                        d_idx, d_dist, d_match, d_counts, h_counts);
}

/* The host-pointer forms, arguments checked: side 1 (rows off1[0] .. off1[m1] of desc1 / kp1) goes to the device, side 2 too unless `same`
 * says both sides name the same arrays, then the models; the device path runs on the null stream and idx / dist / match (at the first
 * output row) come back. */
static int mg_rows_host(const mi_degensac_match_params *mp, const mt_rule &rule, const void *desc1, const void *desc2, const int64_t *off1, int m1, const int64_t *off2,
                        int m2, const double *kp1, const double *kp2, int kd, bool same, const std::vector<mt_pair_rows> &rows, int64_t n_out,
                        int64_t n_back, const double *models, const mt_gate &g, const mg_second &sn, int device, int32_t *idx, float *dist, int32_t *match,
                        int32_t *counts)
{
    const int K = (int)rows.size();
    MiDevGuard dg; int rc = dg.enter(device); if (rc) return rc;
    const int64_t n1 = off1[m1] - off1[0], n2 = off2[m2] - off2[0];
    const size_t row = mt_row_bytes(mp->norm, mp->dim);
    MiStage st;
    const int i_d1 = st.in((const char *)desc1 + off1[0] * row, n1 * row), i_k1 = st.in(kp1 + off1[0] * kd, (size_t)n1 * kd * 8),
              i_d2 = same ? i_d1 : st.in((const char *)desc2 + off2[0] * row, n2 * row), i_k2 = same ? i_k1 : st.in(kp2 + off2[0] * kd, (size_t)n2 * kd * 8),
              i_mo = st.in(models, (size_t)K * 72), o_ix = st.out(idx, (size_t)n_out * 8), o_ds = st.out(dist, (size_t)n_out * 8),
              o_ma = st.out(match, (size_t)n_out * 4);
    rc = st.upload(); if (rc) return rc;
    std::vector<int32_t> cnt(K);
    rc = mg_rows_dev(mp, rule, st.dev<uint32_t>(i_d1), st.dev<uint32_t>(i_d2), st.dev<double>(i_k1), st.dev<double>(i_k2), kd, rows, n_out, n_back,
                     st.dev<double>(i_mo), g, sn, device, nullptr, st.dev<int32_t>(o_ix), st.dev<float>(o_ds), st.dev<int32_t>(o_ma), nullptr, cnt.data());
    if (rc) return rc;
    rc = st.finish(); if (rc) return rc;
    if (counts) memcpy(counts, cnt.data(), (size_t)K * 4);
    return 0;
}

/* host pointers: stage, run the device path on the null stream, copy back.  The ragged batch never asks whether its two sides are the
 * same arrays: both are uploaded */
static int mg_batch_host(int honour, const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                         const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim, int n_pairs, const double *models,
                         const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist, int32_t *match, int32_t *counts)
{
    mt_rule rule; int rc = mg_check_ratio(mp, honour, &rule); if (rc) return rc;
    mt_gate g; rc = mg_check(mp->norm, mp->dim, kp_dim, gp, offsets1, offsets2, n_pairs, &g); if (rc) return rc;
    mg_second sn; rc = mg_check_second(mp, honour, &sn); if (rc) return rc;
    const int K = n_pairs;
    if (K == 0) return 0;
    if (!desc1 || !desc2 || !kp1 || !kp2 || !models || !idx || !dist || !match) return mi_einval("NULL argument");
    std::vector<int64_t> o1, o2; std::vector<mt_pair_rows> rows;
    mt_ragged_rows(offsets1, offsets2, K, o1, o2, rows);
    return mg_rows_host(mp, rule, desc1, desc2, offsets1, K, offsets2, K, kp1, kp2, kp_dim, false, rows, o1[K], o2[K], models, g, sn, device,
                        idx + 2 * offsets1[0], dist + 2 * offsets1[0], match + offsets1[0], counts);
}

extern "C" int mi_degensac_match_guided_batch(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                              const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim, int n_pairs, const double *models,
                                              const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist, int32_t *match, int32_t *counts)
{
    return mg_batch_host(0, mp, desc1, desc2, offsets1, offsets2, kp1, kp2, kp_dim, n_pairs, models, gp, device, idx, dist, match, counts);
}

extern "C" int mi_degensac_match_guided_fginn_batch(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                                    const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim, int n_pairs,
                                                    const double *models, const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist,
                                                    int32_t *match, int32_t *counts)
{
    return mg_batch_host(1, mp, desc1, desc2, offsets1, offsets2, kp1, kp2, kp_dim, n_pairs, models, gp, device, idx, dist, match, counts);
}

/* ---- guided matching over a pair list (include/mi_degensac.h mi_degensac_match_guided_*_pairs*) -------------------------------
 * The same path with descriptors and keypoints stored once per image: mt_pairs_layout fills the rows from the stores' offsets and the
 * (i, j) list, where the ragged batch takes the identity list over its own offsets; everything after the layout step is shared. */
static int mg_knn2_pairs_dev(int fginn, double r, int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                             const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim, const double *d_kp1,
                             const double *d_kp2, int kp_dim, const double *d_models, const mi_degensac_guide_params *gp, int device, hipStream_t s,
                             int32_t *d_idx, float *d_dist)
{
    mt_gate g; std::vector<mt_pair_rows> rows; int64_t n_out, n_back;
    int rc = mg_check_pairs(norm, dim, kp_dim, gp, offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, &g, rows, &n_out, &n_back);
    if (rc) return rc;
    if (fginn) { rc = mg_check_radius(r); if (rc) return rc; }
    if (n_pairs == 0) return 0;
    if (!d_models || (n_out > 0 && (!d_desc1 || !d_kp1 || !d_idx || !d_dist)) || (n_back > 0 && (!d_desc2 || !d_kp2))) return mi_einval("NULL argument");
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const int words = mg_words(norm, dim);
    const uint32_t *q1 = (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words, *q2 = (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words;
    const double *k1 = d_kp1 + (size_t)offsets1_host[0] * kp_dim, *k2 = d_kp2 + (size_t)offsets2_host[0] * kp_dim;
    rc = mt_batch_guided_knn2(norm, words, q1, q2, k1, k2, kp_dim, rows.data(), n_pairs, (int)n_out, d_models, g, 0, device, s, d_idx, d_dist);
    if (rc || !fginn) return rc;
    return mt_batch_guided_fginn(norm, words, q1, q2, k1, k2, kp_dim, rows.data(), n_pairs, (int)n_out, d_models, g, r, device, s, d_idx, d_dist);
}

extern "C" int mi_degensac_match_guided_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                                                       const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim,
                                                       const double *d_kp1, const double *d_kp2, int kp_dim, const double *d_models,
                                                       const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx, float *d_dist)
{
    return mg_knn2_pairs_dev(0, 0.0, norm, d_desc1, d_desc2, offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, dim, d_kp1, d_kp2,
                             kp_dim, d_models, gp, device, (hipStream_t)stream, d_idx, d_dist);
}

extern "C" int mi_degensac_match_guided_fginn_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                             int n_images1, const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host,
                                                             int n_pairs, int dim, const double *d_kp1, const double *d_kp2, int kp_dim,
                                                             const double *d_models, const mi_degensac_guide_params *gp, double spatial_th, int device,
                                                             void *stream, int32_t *d_idx, float *d_dist)
{
    return mg_knn2_pairs_dev(1, spatial_th, norm, d_desc1, d_desc2, offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, dim, d_kp1,
                             d_kp2, kp_dim, d_models, gp, device, (hipStream_t)stream, d_idx, d_dist);
}

static int mg_pairs_dev(int honour, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                        int n_images1, const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, const double *d_kp1,
                        const double *d_kp2, int kp_dim, const double *d_models, const mi_degensac_guide_params *gp, int device, hipStream_t s,
                        int32_t *d_idx, float *d_dist, int32_t *d_match, int32_t *d_counts, int32_t *h_counts)
{
    mt_rule rule; int rc = mg_check_ratio(mp, honour, &rule); if (rc) return rc;
    mt_gate g; std::vector<mt_pair_rows> rows; int64_t n_out, n_back;
    rc = mg_check_pairs(mp->norm, mp->dim, kp_dim, gp, offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, &g, rows, &n_out, &n_back);
    if (rc) return rc;
    mg_second sn; rc = mg_check_second(mp, honour, &sn); if (rc) return rc;
    if (n_pairs == 0) return 0;
    if (!d_models || (n_out > 0 && (!d_desc1 || !d_kp1 || !d_idx || !d_dist || !d_match)) || (n_back > 0 && (!d_desc2 || !d_kp2)))
        return mi_einval("NULL argument");
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const int words = mg_words(mp->norm, mp->dim);
    return mg_rows_dev(mp, rule, (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words, (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words,
                       d_kp1 + (size_t)offsets1_host[0] * kp_dim, d_kp2 + (size_t)offsets2_host[0] * kp_dim, kp_dim, rows, n_out, n_back, d_models, g, sn,
                       device, s, d_idx, d_dist, d_match, d_counts, h_counts);
}

/* each store goes to the device once: one copy when both sides name the same arrays */
static int mg_pairs_host(int honour, const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1, int n_images1,
                         const int64_t *offsets2, int n_images2, const int32_t *pairs, int n_pairs, const double *kp1, const double *kp2, int kp_dim,
                         const double *models, const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist, int32_t *match, int32_t *counts)
{
    mt_rule rule; int rc = mg_check_ratio(mp, honour, &rule); if (rc) return rc;
    mt_gate g; std::vector<mt_pair_rows> rows; int64_t n_out, n_back;
    rc = mg_check_pairs(mp->norm, mp->dim, kp_dim, gp, offsets1, n_images1, offsets2, n_images2, pairs, n_pairs, &g, rows, &n_out, &n_back);
    if (rc) return rc;
    mg_second sn; rc = mg_check_second(mp, honour, &sn); if (rc) return rc;
    if (n_pairs == 0) return 0;
    if (!desc1 || !desc2 || !kp1 || !kp2 || !models || !idx || !dist || !match) return mi_einval("NULL argument");
    const bool same = desc1 == desc2 && kp1 == kp2 && n_images1 == n_images2 && !memcmp(offsets1, offsets2, ((size_t)n_images1 + 1) * 8);
    return mg_rows_host(mp, rule, desc1, desc2, offsets1, n_images1, offsets2, n_images2, kp1, kp2, kp_dim, same, rows, n_out, n_back, models, g, sn, device,
                        idx, dist, match, counts);
}

#define MG_PAIRS_DEV_ARGS const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1, \
    const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, const double *d_kp1, const double *d_kp2, int kp_dim, \
    const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx, float *d_dist, int32_t *d_match, \
    int32_t *d_counts, int32_t *h_counts
#define MG_PAIRS_DEV_PASS mp, d_desc1, d_desc2, offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, d_kp1, d_kp2, kp_dim, d_models, gp, \
    device, (hipStream_t)stream, d_idx, d_dist, d_match, d_counts, h_counts
extern "C" int mi_degensac_match_guided_pairs_dev(MG_PAIRS_DEV_ARGS) { return mg_pairs_dev(0, MG_PAIRS_DEV_PASS); }
extern "C" int mi_degensac_match_guided_fginn_pairs_dev(MG_PAIRS_DEV_ARGS) { return mg_pairs_dev(1, MG_PAIRS_DEV_PASS); }

#define MG_PAIRS_HOST_ARGS const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1, int n_images1, \
    const int64_t *offsets2, int n_images2, const int32_t *pairs, int n_pairs, const double *kp1, const double *kp2, int kp_dim, const double *models, \
    const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist, int32_t *match, int32_t *counts
#define MG_PAIRS_HOST_PASS mp, desc1, desc2, offsets1, n_images1, offsets2, n_images2, pairs, n_pairs, kp1, kp2, kp_dim, models, gp, device, idx, dist, match, \
    counts
extern "C" int mi_degensac_match_guided_pairs(MG_PAIRS_HOST_ARGS) { return mg_pairs_host(0, MG_PAIRS_HOST_PASS); }
extern "C" int mi_degensac_match_guided_fginn_pairs(MG_PAIRS_HOST_ARGS) { return mg_pairs_host(1, MG_PAIRS_HOST_PASS); }
