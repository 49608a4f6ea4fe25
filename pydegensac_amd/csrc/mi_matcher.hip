/* libmi_degensac.so — tentative-correspondence stage in front of the estimators: brute-force 2-nearest-
 * neighbour search over descriptor matrices, the second-nearest-neighbour ratio test and the optional mutual check of
 * the reference's example pipeline (examples/simple-example.py:46-53: cv2.BFMatcher().knnMatch(descs1, descs2, k=2),
 * then `m.distance < 0.9 * n.distance`).  gfx950 only, no CPU path.
 *
 * Distances are formed the way the tests' oracle (oracle/matcher_np.py) forms them, so that ranks, ties and ratio
 * decisions are bit-reproducible: L2 = sqrt of the fp32 sum of squared differences accumulated over the descriptor
 * dimension in ascending order (no FMA contraction: compiled with -ffp-contract=off), Hamming = popcount over the
 * bytes; ties go to the lower train index.  For float rows that rules out the |a|^2 + |b|^2 - 2ab matrix-core form (different
 * roundings, cancellation near duplicates).  For uint8 rows under L2 (MI_DEGENSAC_NORM_L2_U8, dim <= 256) the same form is exact:
 * every term is an integer, the int8 matrix cores accumulate it in int32 in any order, and the result is < 2^24, hence bit for bit
 * the fp32 sum of the direct form on the same values; that tile body is mi_matcher_u8.h.  The direct form is 3 n1 n2 dim flop, a
 * few tens of microseconds for two images' worth of float descriptors, and is LDS-tiled: a workgroup owns 64 queries, streams the train set through
 * LDS 64 rows at a time (both tiles stored dimension-major, so a wave reads consecutive words / one broadcast word),
 * every thread keeps a 4 x 4 block of running sums in registers and its own running top-2 per query; the 16 threads
 * sharing a query merge their candidates at the end.  The train set is additionally split over blockIdx.y (see mt_knn2_kernel).
 * The batched form (mt_knn2_batch_kernel) runs the same tile body over every pair's query tiles in one launch and feeds the match-and-
 * verify path in mi_match_verify.hip (filter + rank, gather, scatter below).  It has one row layout, mt_pair_rows (mi_match_batch.h),
 * and two ways to fill it: a pair list over image stores (mi_degensac_match_*_pairs*: rows stored once per image, a list of (i, j);
 * mt_pairs_layout) and the ragged batch (mi_degensac_match_*_batch*), which is the list whose entry p is (image p, image p) with its
 * answers at its queries' own rows (mt_identity_rows). */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <vector>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_host.h"

#define MT_Q   64            /* queries per workgroup */
#define MT_T   64            /* train rows per LDS tile */
#define MT_DC  64            /* descriptor words per LDS chunk */

/* mt_best / mt_push (the running top-2 and its tie rule): mi_match_batch.h */
#include "mi_matcher_u8.h"

/* acc + the dot product of the four unsigned bytes of a and b */
__device__ __forceinline__ unsigned mt_udot4(uint32_t a, uint32_t b, unsigned acc) { return __builtin_amdgcn_udot4(a, b, acc, false); }

/* What the FGINN rescan (mi_fginn.h) adds to the tile body below.  mf_ctx: the entry's needy list (OUTPUT rows at the list
 * positions q0 .. q_end - 1), the plain 2-NN's idx (slot 0 is the anchor, at the output row), the train keypoints, r * r and qd = the
 * entry's first query row in q minus its first output row: a needy query's descriptor row is its output row + qd (0 only in a ragged
 * batch; of either sign in a pair list).  mf_lds: the tile's train keypoints next to the descriptor tile (16 bytes per row), every
 * query's anchor keypoint and output row, read once per workgroup. */
struct mf_ctx { const int32_t *list, *idx; const double *kt; int kd; double rr; int qd; };
struct mf_lds { double2 tk[MT_T], ak[MT_Q]; int ai[MT_Q], row[MT_Q]; };

/* One workgroup's tile: queries q0 .. q_end - 1 (at most 64) of q against train rows t_lo .. t_hi - 1 of t, candidates
 * indexed from t_base (0 for a single pair, the pair's first train row in a batch).  NORM: 0 = L2 over float words,
 * 1 = Hamming over 32-bit words of packed bytes; q, t: [n, words] row-major.  Returns true in the threads tid < 64 whose
 * query exists, with that query's merged top-2 (squared distances for L2) in m.
 * FGM != 0 (the FGINN rescan): q0 .. q_end - 1 are positions of fg->list, whose entries are the queries' output rows.  FGM 1 is the
 * ragged batch, where the output row is the descriptor row too (the instantiation of before the pair list, kept as it was); FGM 2 is
 * the pair list, descriptor row = output row + fg->qd.  A train row is pushed only when it competes with the query's anchor i0 = fg->idx[output row][0]: t != i0 and dx dx + dy dy >= rr in fp64 (false for a NaN).  NORM 2
 * (uint8 rows under L2, FGM != 0 only: the dense form is mu_knn2_tile) forms the exact integer S = |a|^2 + |b|^2 - 2 a.b with unsigned byte
 * dot products on the vector unit. */
template <int NORM, int FGM = 0>
__device__ __forceinline__ bool mt_knn2_tile(const uint32_t *q, int q0, int q_end, const uint32_t *t, int t_lo, int t_hi, int t_base, int words,
                                             uint32_t (&qs)[MT_DC][MT_Q + 1], uint32_t (&ts)[MT_DC][MT_T + 1], mt_best (&merge)[MT_Q][16], mt_best &m,
                                             const mf_ctx *fg = nullptr, mf_lds *fl = nullptr)
{
    constexpr bool FG = FGM != 0;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    mt_best best[4];
#pragma unroll
    for (int a = 0; a < 4; a++) { best[a].d0 = best[a].d1 = __builtin_inff(); best[a].i0 = best[a].i1 = -1; }
    double ax[4], ay[4]; int ai[4];
    if constexpr (FG) {
        if (tid < MT_Q) {
            const bool in = q0 + tid < q_end;
            const int row = in ? fg->list[q0 + tid] : 0, i0 = in ? fg->idx[2 * (size_t)row] : -1;
            const double *k = fg->kt + (size_t)(t_base + (i0 >= 0 ? i0 : 0)) * fg->kd;
            fl->row[tid] = row; fl->ai[tid] = i0;
            fl->ak[tid] = i0 >= 0 ? make_double2(k[0], k[1]) : make_double2(__builtin_nan(""), __builtin_nan(""));
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; a++) { const double2 k = fl->ak[4 * ty + a]; ax[a] = k.x; ay[a] = k.y; ai[a] = fl->ai[4 * ty + a]; }
    }
    for (int t0 = t_lo; t0 < t_hi; t0 += MT_T) {
        float acc[4][4]; unsigned hacc[4][4], hq[4], ht[4];
#pragma unroll
        for (int a = 0; a < 4; a++) {
            hq[a] = ht[a] = 0u;
#pragma unroll
            for (int b = 0; b < 4; b++) { acc[a][b] = 0.f; hacc[a][b] = 0u; }
        }
        for (int w0 = 0; w0 < words; w0 += MT_DC) {
            __syncthreads();
            /* stage both tiles dimension-major: thread r loads row (r / 4), a quarter of the chunk's words, coalesced per row */
            for (int e = tid; e < MT_Q * MT_DC; e += 256) {
                const int r = e / MT_DC, w = e - r * MT_DC;
                const bool okq = q0 + r < q_end && w0 + w < words, okt = t0 + r < t_hi && w0 + w < words;
                const int qr = FGM == 2 ? fl->row[r] + fg->qd : FG ? fl->row[r] : q0 + r;
                qs[w][r] = okq ? q[(size_t)qr * words + w0 + w] : 0u;
                ts[w][r] = okt ? t[(size_t)(t0 + r) * words + w0 + w] : 0u;
            }
            if constexpr (FG) {
                if (w0 == 0 && tid < MT_T) {
                    const double *k = fg->kt + (size_t)(t0 + tid < t_hi ? t0 + tid : t_lo) * fg->kd;
                    fl->tk[tid] = make_double2(k[0], k[1]);
                }
            }
            __syncthreads();
            const int wn = words - w0 < MT_DC ? words - w0 : MT_DC;
            for (int w = 0; w < wn; w++) {
                uint32_t qa[4], tb[4];
#pragma unroll
                for (int a = 0; a < 4; a++) qa[a] = qs[w][4 * ty + a];
#pragma unroll
                for (int b = 0; b < 4; b++) tb[b] = ts[w][tx + 16 * b];
                if constexpr (NORM == 2) {
#pragma unroll
                    for (int a = 0; a < 4; a++) { hq[a] = mt_udot4(qa[a], qa[a], hq[a]); ht[a] = mt_udot4(tb[a], tb[a], ht[a]); }
                }
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        if (NORM == 0) { const float df = __uint_as_float(qa[a]) - __uint_as_float(tb[b]); acc[a][b] = acc[a][b] + df * df; }
                        else if (NORM == 1) hacc[a][b] += (unsigned)__popc(qa[a] ^ tb[b]);
                        else hacc[a][b] = mt_udot4(qa[a], tb[b], hacc[a][b]);
                    }
            }
        }
        double2 tk[4];
        if constexpr (FG) {
#pragma unroll
            for (int b = 0; b < 4; b++) tk[b] = fl->tk[tx + 16 * b];
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int ti = t0 + tx + 16 * b;
                bool ok = ti < t_hi;
                if constexpr (FG) {
                    const double dx = tk[b].x - ax[a], dy = tk[b].y - ay[a];
                    ok = ok && ti - t_base != ai[a] && dx * dx + dy * dy >= fg->rr;
                }
                if (ok) mt_push(best[a], NORM == 0 ? acc[a][b] : NORM == 1 ? (float)hacc[a][b] : (float)(hq[a] + ht[b] - 2u * hacc[a][b]), ti - t_base);
            }
    }
    /* the 16 threads of a query row merge their candidates (lane order does not matter: mt_push orders by (d, i)) */
#pragma unroll
    for (int a = 0; a < 4; a++) merge[4 * ty + a][tx] = best[a];
    __syncthreads();
    if (tid >= MT_Q || q0 + tid >= q_end) return false;
    m = merge[tid][0];
    for (int k = 1; k < 16; k++) { const mt_best c = merge[tid][k]; if (c.i0 >= 0) mt_push(m, c.d0, c.i0); if (c.i1 >= 0) mt_push(m, c.d1, c.i1); }
    return true;
}

/* final answer of query row r from its merged top-2, or its partial of split `split` when the train set is split
 * (NORM 2, uint8 rows under L2, carries the exact integer S as a float and takes the root as L2 does) */
template <int NORM>
__device__ __forceinline__ void mt_store(const mt_best &m, int r, int n_rows, int split, int32_t *idx, float *dist, mt_best *part)
{
    if (part) { part[(size_t)split * n_rows + r] = m; return; }
    const size_t o = (size_t)r * 2;
    idx[o] = m.i0; idx[o + 1] = m.i1;
    dist[o] = NORM != 1 ? sqrtf(m.d0) : m.d0; dist[o + 1] = NORM != 1 ? sqrtf(m.d1) : m.d1;
}

/* the tile body of a norm: NORM 0 / 1 = mt_knn2_tile over LDS tiles, NORM 2 = mu_knn2_tile<NS> (mi_matcher_u8.h) */
template <int NORM, int NS>
__device__ __forceinline__ bool mt_tile(const uint32_t *q, int q0, int q_end, const uint32_t *t, int t_lo, int t_hi, int t_base, int words,
                                        mt_best (&merge)[MT_Q][16], mt_best &m)
{
    if constexpr (NORM == 2) {
        __shared__ int ntl[4 * 32];
        return mu_knn2_tile<NS>(q, q0, q_end, t, t_lo, t_hi, t_base, words, ntl, merge, m);
    } else {
        __shared__ uint32_t qs[MT_DC][MT_Q + 1], ts[MT_DC][MT_T + 1];
        return mt_knn2_tile<NORM>(q, q0, q_end, t, t_lo, t_hi, t_base, words, qs, ts, merge, m);
    }
}

/* Launch shape: grid = (ceil(n1 / 64), train splits).  Two images' worth of descriptors give only a few dozen query
 * tiles (1 500 queries = 24), so the train set is split over blockIdx.y until the grid covers the CUs about twice; a split
 * writes its top-2 per query (squared distances) to part[split][query] and mt_merge_kernel merges the splits with the same
 * (distance, index) order, so the result does not depend on the split count.  With one split the kernel writes the final
 * answer itself. */
template <int NORM, int NS = 0>
__global__ __launch_bounds__(256) void mt_knn2_kernel(const uint32_t *q, int n1, const uint32_t *t, int n2, int words,
    int t_chunk /* train rows per split, multiple of 64 */,
                                                      int32_t *idx /* [n1,2] */, float *dist /* [n1,2] */, mt_best *part /* [splits][n1] or null */)
{
    __shared__ mt_best merge[MT_Q][16];
    const int q0 = blockIdx.x * MT_Q;
    const int t_lo = (int)blockIdx.y * t_chunk, t_hi = t_lo + t_chunk < n2 ? t_lo + t_chunk : n2;
    mt_best m;
    if (mt_tile<NORM, NS>(q, q0, n1, t, t_lo, t_hi, 0, words, merge, m))
        mt_store<NORM>(m, q0 + threadIdx.x, n1, blockIdx.y, idx, dist, part);
}

/* The batched launch: one workgroup per 64-query tile of every pair, from a tile table built on the host (mt_batch_knn2).  A tile's
 * queries q0 .. q_end - 1 of the query rows meet the train rows t_b .. t_e - 1 of the train rows; the indices written are local to
 * the pair (from t_b), the answers go to the rows o0 .. of idx / dist (n_rows of them in all; the per-split partials are indexed by
 * output row too).  In a ragged batch o0 = q0; in a pair list, where descriptors are stored once per image, it is not.  Split y takes
 * the pair's train rows t_b + y t_chunk .. + t_chunk (possibly none: the partial then stays at (inf, -1)).  Tile bodies and the merge
 * are those of the dense kernel, so neither the split count nor the order of the tiles changes a result.
 * The record is read in two parts: the 16 bytes the tile body needs up front, o0 where it is used, after the body.  Measured: with
 * all five fields loaded up front the instruction stream is the same but for that load, the inner loop lies elsewhere and the fp32
 * kernel runs 1.2 % slower (profiles/matcher_one_path_ab.log). */
struct mt_ptile { int4 r /* q0, q_end, t_b, t_e */; int o0, pad[3]; };

template <int NORM, int NS = 0>
__global__ __launch_bounds__(256) void mt_knn2_batch_kernel(const uint32_t *q, const uint32_t *t, int words, const mt_ptile *tiles, int n_rows,
                                                            int t_chunk, int32_t *idx, float *dist, mt_best *part)
{
    __shared__ mt_best merge[MT_Q][16];
    const int4 tl = tiles[blockIdx.x].r;
    const int t_lo = tl.z + (int)blockIdx.y * t_chunk, t_hi = t_lo + t_chunk < tl.w ? t_lo + t_chunk : tl.w;
    mt_best m;
    if (mt_tile<NORM, NS>(q, tl.x, tl.y, t, t_lo, t_hi, tl.z, words, merge, m))
        mt_store<NORM>(m, tiles[blockIdx.x].o0 + threadIdx.x, n_rows, blockIdx.y, idx, dist, part);
}

/* merge the per-split top-2 of every query (any order gives the same result: mt_push orders by (distance, index)) */
__global__ void mt_merge_kernel(const mt_best *part, int splits, int n1, int l2, int32_t *idx, float *dist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    mt_best m = part[i];
    for (int s = 1; s < splits; s++) { const mt_best c = part[(size_t)s * n1 + i]; if (c.i0 >= 0) mt_push(m, c.d0, c.i0); if (c.i1 >= 0) mt_push(m, c.d1, c.i1);
        }
    idx[2 * i] = m.i0; idx[2 * i + 1] = m.i1;
    dist[2 * i] = l2 ? sqrtf(m.d0) : m.d0; dist[2 * i + 1] = l2 ? sqrtf(m.d1) : m.d1;
}

/* keep[i] = the decision rule (mt_decide, mi_match_batch.h).  With rule.flags = 0: the second-nearest-neighbour ratio test (strict, as
 * the example's `m.distance < ratio * n.distance`; a query with fewer than two train rows never passes) and, when back != 0, the
 * mutual check back[idx[i][0]][0] == i */
__global__ void mt_filter_kernel(const int32_t *idx, const float *dist, int n1, mt_rule rule, const int32_t *back, const float *bdist, uint8_t *keep)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    keep[i] = mt_decide<false>(rule, idx, dist, i, i, back, bdist, 0) ? 1 : 0;
}

/* utils.py:24-41 convert_cv2_kpts_to_xyA on the device: (x, y, size, angle in degrees) -> (x, y, s cos a, s sin a,
 * -s sin a, s cos a) in float64, the [n, 6] rows the estimators take for the LAF consistency checks */
__global__ void mt_kpts_to_xyA_kernel(const float *kp, int n, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = kp[4 * i], y = kp[4 * i + 1], s = kp[4 * i + 2], a = kp[4 * i + 3];
    const double r = a * 3.141592653589793 / 180.0, cs = cos(r), sn = sin(r);
    double *o = out + (size_t)i * 6;
    o[0] = x; o[1] = y; o[2] = s * cs; o[3] = s * sn; o[4] = -s * sn; o[5] = s * cs;
}

/* ---- the batched match-and-verify stages (mi_match_batch.h) ------------------------------------------------------------ */
/* One workgroup per pair sweeps its queries 256 at a time: keep[i] is mt_filter_kernel's decision, rank[i] its position
 * among the pair's kept queries in ascending query order (-1 when not kept), count[p] their number.  Positions come from
 * wave ballots and a four-entry prefix over the waves, so they do not depend on scheduling. */
__global__ __launch_bounds__(256) void mt_filter_rank_kernel(const int32_t *idx, const float *dist, const int32_t *off1, const int32_t *off2,
                                                             mt_rule rule, const int32_t *back, const float *bdist, uint8_t *keep, int32_t *rank,
                                                             int32_t *count)
{
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lo = off1[p], hi = off1[p + 1], b2 = off2[p];
    int base = 0;
    for (int i0 = lo; i0 < hi; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false;
        if (i < hi) ok = mt_decide<false>(rule, idx, dist, i, i - lo, back, bdist, b2);
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();
        int pre = base;
        for (int w = 0; w < wv; w++) pre += wsum[w];
        if (i < hi) { keep[i] = ok ? 1 : 0; rank[i] = ok ? pre + __popcll(bal & ((1ull << lane) - 1ull)) : -1; }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) count[p] = base;
}

/* one workgroup per eligible pair: its tentatives in query order become rows est_off[e] .. of the estimator's input.  keep / rank /
 * idx live at the pair's output rows out[p] .., its keypoints at the rows q1[p] .. of kp1 and (train rows, pair-local in idx)
 * t2[p] .. of kp2 */
__global__ __launch_bounds__(256) void mt_gather_kernel(const int32_t *pair_of_e, const int64_t *est_off, const int32_t *out, const int32_t *q1,
                                                        const int32_t *t2, const uint8_t *keep, const int32_t *rank, const int32_t *idx,
                                                        const double *kp1, const double *kp2, int kd, const uint32_t *seeds, double *pts1,
                                                        double *pts2, uint32_t *seeds_e)
{
    const int e = blockIdx.x, p = pair_of_e[e];
    const int lo = out[p], hi = out[p + 1];
    const int64_t o = est_off[e], b1 = (int64_t)q1[p] - lo, b2 = t2[p];
    if (threadIdx.x == 0) seeds_e[e] = seeds[p];
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        if (!keep[i]) continue;
        const int64_t r = o + rank[i], a = b1 + i, j = b2 + idx[2 * i];
        for (int c = 0; c < kd; c++) { pts1[r * kd + c] = kp1[a * kd + c]; pts2[r * kd + c] = kp2[j * kd + c]; }
    }
}

/* one workgroup per pair: model / stats from the eligible index (zeros for a short pair), match and inlier per query */
__global__ __launch_bounds__(256) void mt_scatter_kernel(const int32_t *e_of_p, const int64_t *est_off, const int32_t *off1, const uint8_t *keep,
                                                         const int32_t *rank, const int32_t *idx, const double *model_e, const int32_t *stats_e,
                                                         const uint8_t *mask_e, double *model, int32_t *stats, int32_t *match, uint8_t *inlier)
{
    const int p = blockIdx.x, tid = threadIdx.x, e = e_of_p[p];
    if (tid < 9) model[(int64_t)p * 9 + tid] = e >= 0 ? model_e[(int64_t)e * 9 + tid] : 0.0;
    if (stats && tid < MI_DEGENSAC_STATS_LEN)
        stats[(int64_t)p * MI_DEGENSAC_STATS_LEN + tid] = e >= 0 ? stats_e[(int64_t)e * MI_DEGENSAC_STATS_LEN + tid] : 0;
    const int64_t o = e >= 0 ? est_off[e] : 0;
    for (int i = off1[p] + tid; i < off1[p + 1]; i += 256) {
        const bool k = keep[i] != 0;
        match[i] = k ? idx[2 * i] : -1;
        inlier[i] = (k && e >= 0) ? mask_e[o + rank[i]] : 0;
    }
}

/* mt_scatter_kernel for two models on the same tentatives (F, then H): one workgroup per pair writes both models / stats rows from the
 * pair's eligible index of each half (ef / eh, each with its own est_off base; zeros where the index is -1), match and both inlier rows
 * per query, and summary[p] = (tentatives, nF, nH, nFH).  The counts come from wave ballots, summed per wave over the sweep, and a
 * four-entry LDS table per count that thread 0 adds up: no atomics, nothing depends on scheduling. */
__global__ __launch_bounds__(256) void mt_scatter_fh_kernel(const int32_t *e_of_p_f, const int64_t *est_off_f, const int32_t *e_of_p_h,
                                                            const int64_t *est_off_h, const int32_t *off1, const uint8_t *keep, const int32_t *rank,
                                                            const int32_t *idx, const double *model_ef, const int32_t *stats_ef,
                                                            const uint8_t *mask_ef, const double *model_eh, const int32_t *stats_eh,
                                                            const uint8_t *mask_eh, double *model_f, int32_t *stats_f, double *model_h,
                                                            int32_t *stats_h, int32_t *match, uint8_t *inlier_f, uint8_t *inlier_h, int32_t *summary)
{
    __shared__ int wsum[4][4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ef = e_of_p_f[p], eh = e_of_p_h[p];
    if (tid < 9) {
        model_f[(int64_t)p * 9 + tid] = ef >= 0 ? model_ef[(int64_t)ef * 9 + tid] : 0.0;
        model_h[(int64_t)p * 9 + tid] = eh >= 0 ? model_eh[(int64_t)eh * 9 + tid] : 0.0;
    }
    if (tid < MI_DEGENSAC_STATS_LEN) {
        if (stats_f) stats_f[(int64_t)p * MI_DEGENSAC_STATS_LEN + tid] = ef >= 0 ? stats_ef[(int64_t)ef * MI_DEGENSAC_STATS_LEN + tid] : 0;
        if (stats_h) stats_h[(int64_t)p * MI_DEGENSAC_STATS_LEN + tid] = eh >= 0 ? stats_eh[(int64_t)eh * MI_DEGENSAC_STATS_LEN + tid] : 0;
    }
    const int64_t of = ef >= 0 ? est_off_f[ef] : 0, oh = eh >= 0 ? est_off_h[eh] : 0;
    const int lo = off1[p], hi = off1[p + 1];
    int nt = 0, nf = 0, nh = 0, nfh = 0;                /* this wave's counts (the same in all its lanes) */
    for (int i0 = lo; i0 < hi; i0 += 256) {
        const int i = i0 + tid;
        bool k = false; uint8_t f = 0, h = 0;
        if (i < hi) {
            k = keep[i] != 0;
            if (k) { const int r = rank[i]; f = ef >= 0 ? mask_ef[of + r] : 0; h = eh >= 0 ? mask_eh[oh + r] : 0; }
            match[i] = k ? idx[2 * i] : -1;
            inlier_f[i] = f; inlier_h[i] = h;
        }
        nt += __popcll(__ballot(k)); nf += __popcll(__ballot(f != 0)); nh += __popcll(__ballot(h != 0)); nfh += __popcll(__ballot(f != 0 && h != 0));
    }
    if (lane == 0) { wsum[wv][0] = nt; wsum[wv][1] = nf; wsum[wv][2] = nh; wsum[wv][3] = nfh; }
    __syncthreads();
    if (tid == 0)
        for (int c = 0; c < 4; c++) summary[(int64_t)p * 4 + c] = wsum[0][c] + wsum[1][c] + wsum[2][c] + wsum[3][c];
}

static thread_local char mt_err[256] = "";
extern "C" const char *mi_degensac_match_last_error(void) { return mt_err; }
void mt_set_error(const char *msg) { snprintf(mt_err, sizeof mt_err, "%s", msg); }

/* norm and dim of a dense entry point (refused before the library looks for a device); uint8 rows are passed padded to whole
 * 32-bit words */
static int mt_check_norm(int norm, int dim)
{
    if (!mt_norm_known(norm) || dim <= 0) return mi_einval("bad argument");
    if (const char *e = mt_norm_dim_error(norm, dim)) return mi_einval(e);
    return 0;
}

/* one of the two dense kernels for a norm code; uint8 L2 rows take the instance with the fewest 32-byte k-steps covering the row */
#define MT_LAUNCH_NORM(KERNEL, norm, words, grid, block, s, ...) do { \
    if ((norm) == MI_DEGENSAC_NORM_L2)           hipLaunchKernelGGL((KERNEL<0>), grid, block, 0, s, __VA_ARGS__); \
    else if ((norm) == MI_DEGENSAC_NORM_HAMMING) hipLaunchKernelGGL((KERNEL<1>), grid, block, 0, s, __VA_ARGS__); \
    else if ((words) <= 16)                      hipLaunchKernelGGL((KERNEL<2, 2>), grid, block, 0, s, __VA_ARGS__); \
    else if ((words) <= 32)                      hipLaunchKernelGGL((KERNEL<2, 4>), grid, block, 0, s, __VA_ARGS__); \
    else                                         hipLaunchKernelGGL((KERNEL<2, 8>), grid, block, 0, s, __VA_ARGS__); } while (0)

extern "C" int mi_degensac_match_knn2_dev(int norm, const void *d_desc1, int n1, const void *d_desc2, int n2, int dim, int device,
                                          void *stream, int32_t *d_idx, float *d_dist)
{
    if (n1 < 0 || n2 < 0) return mi_einval("bad argument");
    int rc = mt_check_norm(norm, dim); if (rc) return rc;
    const int words = mt_row_words(norm, dim);
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    if (n1 == 0) return 0;
    /* train splits: enough workgroups to cover the device about twice, never less than one 64-row tile per split */
    const int qtiles = (n1 + MT_Q - 1) / MT_Q, ttiles = n2 > 0 ? (n2 + MT_T - 1) / MT_T : 1;
    int cus = 256; { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess) cus = pr.multiProcessorCount; else (void)hipGetLastError(); }
    int splits = (2 * cus + qtiles - 1) / qtiles; if (splits > ttiles) splits = ttiles; if (splits < 1) splits = 1; if (splits > 256) splits = 256;
    const int t_chunk = ((ttiles + splits - 1) / splits) * MT_T;
    splits = n2 > 0 ? (n2 + t_chunk - 1) / t_chunk : 1;
    mt_best *part = nullptr;
    if (splits > 1) MICHK(hipMallocAsync((void **)&part, (size_t)splits * n1 * sizeof(mt_best), (hipStream_t)stream));
    const dim3 grid(qtiles, splits), block(256);
    MT_LAUNCH_NORM(mt_knn2_kernel, norm, words, grid, block, (hipStream_t)stream, (const uint32_t *)d_desc1, n1, (const uint32_t *)d_desc2, n2, words,
        n2 > 0 ? t_chunk : MT_T, d_idx, d_dist, part);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess && part) {
        hipLaunchKernelGGL(mt_merge_kernel, dim3((n1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, splits, n1,
            norm != MI_DEGENSAC_NORM_HAMMING ? 1 : 0, d_idx, d_dist);
        le = hipGetLastError();
    }
    if (part) (void)hipFreeAsync(part, (hipStream_t)stream);
    MICHK(le);
    return 0;
}

extern "C" int mi_degensac_match_filter_dev(const int32_t *d_idx, const float *d_dist, int n1, float ratio, const int32_t *d_back_idx_or_null,
                                            int device, void *stream, uint8_t *d_keep)
{
    if (n1 < 0) return mi_einval("bad argument");
    MiDevGuard g; int rc = g.enter(device); if (rc) return rc;
    if (n1 == 0) return 0;
    hipLaunchKernelGGL(mt_filter_kernel, dim3((n1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_idx, d_dist, n1, mt_rule{ratio, 0, 0.f},
        d_back_idx_or_null, (const float *)nullptr, d_keep);
    MICHK(hipGetLastError());
    return 0;
}

/* the rule of a dense call: no keypoints here, so an FGINN request can only be refused */
static int mt_dense_rule(const mi_degensac_match_params *mp, int honour_second_nn, mt_rule *rule)
{
    if (!mp) return mi_einval("match params are NULL");
    if (const char *e = mt_decide_rule(mp, honour_second_nn, rule)) return mi_einval(e);
    return 0;
}

extern "C" int mi_degensac_match_decide_dev(const mi_degensac_match_params *mp, const int32_t *d_idx, const float *d_dist, int n1,
                                            const int32_t *d_back_idx, const float *d_back_dist, int device, void *stream, uint8_t *d_keep)
{
    mt_rule rule; int rc = mt_dense_rule(mp, 0, &rule); if (rc) return rc;
    if (n1 < 0) return mi_einval("bad argument");
    const bool mutual = mp->mutual != 0;
    if (n1 > 0 && (!d_idx || !d_dist || !d_keep)) return mi_einval("NULL argument");
    if (n1 > 0 && mutual && !d_back_idx) return mi_einval("mutual needs d_back_idx, the reverse search's idx");
    if (n1 > 0 && (rule.flags & MI_DEGENSAC_DECIDE_BACK_RATIO) && !d_back_dist) return mi_einval("BACK_RATIO needs d_back_dist, the reverse search's dist");
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    if (n1 == 0) return 0;
    hipLaunchKernelGGL(mt_filter_kernel, dim3((n1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_idx, d_dist, n1, rule,
        mutual ? d_back_idx : (const int32_t *)nullptr, mutual ? d_back_dist : (const float *)nullptr, d_keep);
    MICHK(hipGetLastError());
    return 0;
}

/* host pointers: stage, search both directions when the mutual check is asked for, decide, copy back; rule = null: the scalar call's
 * ratio test through mi_degensac_match_filter_dev, as it always ran */
static int mt_match_host(int norm, const void *desc1, int n1, const void *desc2, int n2, int dim, float ratio, int mutual, const mt_rule *rule,
                         int device, int32_t *idx, float *dist, uint8_t *keep);

extern "C" int mi_degensac_match(int norm, const void *desc1, int n1, const void *desc2, int n2, int dim, float ratio, int mutual, int device,
                                 int32_t *idx /* [n1,2] */, float *dist /* [n1,2] */, uint8_t *keep /* [n1] or NULL */)
{
    return mt_match_host(norm, desc1, n1, desc2, n2, dim, ratio, mutual, nullptr, device, idx, dist, keep);
}

extern "C" int mi_degensac_match_ex(const mi_degensac_match_params *mp, const void *desc1, int n1, const void *desc2, int n2, int device,
                                    int32_t *idx, float *dist, uint8_t *keep)
{
    mt_rule rule; int rc = mt_dense_rule(mp, 1, &rule); if (rc) return rc;
    int fginn; double r;
    if (const char *e = mt_second_nn(mp, &fginn, &r)) return mi_einval(e);
    if (fginn) return mi_einval("the FGINN rule (second_nn = 1) is not part of the dense call: it has no keypoints");
    return mt_match_host(mp->norm, desc1, n1, desc2, n2, mp->dim, mp->ratio, mp->mutual, &rule, device, idx, dist, keep);
}

static int mt_match_host(int norm, const void *desc1, int n1, const void *desc2, int n2, int dim, float ratio, int mutual, const mt_rule *rule,
                         int device, int32_t *idx, float *dist, uint8_t *keep)
{
    if (!desc1 || !desc2 || !idx || !dist || n1 < 0 || n2 < 0 || dim <= 0) return mi_einval("bad argument");
    int rc = mt_check_norm(norm, dim); if (rc) return rc;
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    if (n1 == 0) return 0;
    const size_t b1 = (size_t)n1 * mt_row_bytes(norm, dim), b2 = (size_t)n2 * mt_row_bytes(norm, dim);
    char *d1 = nullptr, *d2 = nullptr; int32_t *di = nullptr, *dbi = nullptr; float *dd = nullptr, *dbd = nullptr; uint8_t *dk = nullptr;
    struct Free { char *&a, *&b; int32_t *&c, *&d; float *&e, *&f; uint8_t *&g;
                  ~Free() { (void)hipFree(a); (void)hipFree(b); (void)hipFree(c); (void)hipFree(d); (void)hipFree(e); (void)hipFree(f); (void)hipFree(g);
                      } } fr{d1, d2, di, dbi, dd, dbd, dk};
    MICHK(hipMalloc((void **)&d1, b1 ? b1 : 4)); MICHK(hipMalloc((void **)&d2, b2 ? b2 : 4));
    MICHK(hipMalloc((void **)&di, (size_t)n1 * 8)); MICHK(hipMalloc((void **)&dd, (size_t)n1 * 8));
    MICHK(hipMemcpy(d1, desc1, b1, hipMemcpyHostToDevice)); MICHK(hipMemcpy(d2, desc2, b2, hipMemcpyHostToDevice));
    rc = mi_degensac_match_knn2_dev(norm, d1, n1, d2, n2, dim, device, nullptr, di, dd); if (rc) return rc;
    if (keep) {
        MICHK(hipMalloc((void **)&dk, (size_t)n1));
        if (mutual && n2 > 0) {
            MICHK(hipMalloc((void **)&dbi, (size_t)n2 * 8)); MICHK(hipMalloc((void **)&dbd, (size_t)n2 * 8));
            rc = mi_degensac_match_knn2_dev(norm, d2, n2, d1, n1, dim, device, nullptr, dbi, dbd); if (rc) return rc;
        }
        if (!rule) { rc = mi_degensac_match_filter_dev(di, dd, n1, ratio, dbi, device, nullptr, dk); if (rc) return rc; }
        else {
            hipLaunchKernelGGL(mt_filter_kernel, dim3((n1 + 255) / 256), dim3(256), 0, (hipStream_t) nullptr, di, dd, n1, *rule, dbi, dbd, dk);
            MICHK(hipGetLastError());
        }
    }
    MICHK(hipDeviceSynchronize());
    MICHK(hipMemcpy(idx, di, (size_t)n1 * 8, hipMemcpyDeviceToHost)); MICHK(hipMemcpy(dist, dd, (size_t)n1 * 8, hipMemcpyDeviceToHost));
    if (keep) MICHK(hipMemcpy(keep, dk, (size_t)n1, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mi_degensac_kpts_to_xyA_dev(const float *d_kpts, int n, int device, void *stream, double *d_out)
{
    if (n < 0) return mi_einval("bad argument");
    MiDevGuard g; int rc = g.enter(device); if (rc) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(mt_kpts_to_xyA_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_kpts, n, d_out);
    MICHK(hipGetLastError());
    return 0;
}
extern "C" int mi_degensac_kpts_to_xyA(const float *kpts, int n, int device, double *out)
{
    if (!kpts || !out || n < 0) return mi_einval("bad argument");
    MiDevGuard g; int rc = g.enter(device); if (rc) return rc;
    if (n == 0) return 0;
    float *dk = nullptr; double *dout = nullptr;
    struct Free { float *&a; double *&b; ~Free() { (void)hipFree(a); (void)hipFree(b); } } fr{dk, dout};
    MICHK(hipMalloc((void **)&dk, (size_t)n * 16)); MICHK(hipMalloc((void **)&dout, (size_t)n * 48));
    MICHK(hipMemcpy(dk, kpts, (size_t)n * 16, hipMemcpyHostToDevice));
    rc = mi_degensac_kpts_to_xyA_dev(dk, n, device, nullptr, dout); if (rc) return rc;
    MICHK(hipDeviceSynchronize());
    MICHK(hipMemcpy(out, dout, (size_t)n * 48, hipMemcpyDeviceToHost));
    return 0;
}

/* ---- batched matcher: host side ------------------------------------------------------------------------------------ */
static int mt_cus(int device)
{
    static int cache[64] = {0};
    if (device >= 0 && device < 64 && cache[device] > 0) return cache[device];
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    if (device >= 0 && device < 64) cache[device] = cus;
    return cus;
}

/* Pinned staging blocks of the uploads: a block is taken again only once the copy that read it has run (its event), so an
 * upload never waits for the stream; when all blocks of the device are busy a new one is made (at most 16, then the oldest
 * fitting one is waited for). */
struct MtPin { int device; char *h; size_t cap; hipEvent_t ev; };
static std::mutex mt_pin_mu;
static std::vector<MtPin> mt_pins;

int mt_batch_upload(int device, hipStream_t s, const void *h, size_t bytes, void *d)
{
    if (bytes == 0) return 0;
    std::lock_guard<std::mutex> lk(mt_pin_mu);
    MtPin *b = nullptr, *busy = nullptr; int mine = 0;
    for (auto &e : mt_pins) {
        if (e.device != device) continue;
        mine++;
        if (e.cap < bytes) continue;
        if (hipEventQuery(e.ev) == hipSuccess) { b = &e; break; }
        (void)hipGetLastError();
        if (!busy) busy = &e;
    }
    if (!b && busy && mine >= 16) { MICHK(hipEventSynchronize(busy->ev)); b = busy; }
    if (!b) {
        MtPin n{device, nullptr, bytes < ((size_t)1 << 16) ? ((size_t)1 << 16) : bytes + bytes / 4, nullptr};
        MICHK(hipHostMalloc((void **)&n.h, n.cap, hipHostMallocDefault));
        if (hipEventCreateWithFlags(&n.ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(n.h); MICHK(hipErrorOutOfMemory); }
        mt_pins.push_back(n); b = &mt_pins.back();
    }
    memcpy(b->h, h, bytes);
    MICHK(hipMemcpyAsync(d, b->h, bytes, hipMemcpyHostToDevice, s));
    MICHK(hipEventRecord(b->ev, s));
    return 0;
}

/* the train-split rule of the batched launches: (rows per split, splits) from the batch's query tiles and its largest train set */
static void mt_batch_split(int qtiles, int max_n2, int device, int *t_chunk, int *n_splits)
{
    const int ttiles = max_n2 > 0 ? (max_n2 + MT_T - 1) / MT_T : 1, cus = mt_cus(device);
    int splits = qtiles >= 2 * cus ? 1 : (2 * cus + qtiles - 1) / qtiles;
    if (splits > ttiles) splits = ttiles; if (splits < 1) splits = 1; if (splits > 256) splits = 256;
    *t_chunk = max_n2 > 0 ? ((ttiles + splits - 1) / splits) * MT_T : MT_T;
    *n_splits = max_n2 > 0 ? (max_n2 + *t_chunk - 1) / *t_chunk : 1;
}

/* One launch over the 64-query tiles of every pair (from the pair's first row on).  The train set is split over blockIdx.y only when
 * the batch's tiles do not cover the CUs about twice (as in mi_degensac_match_knn2_dev, with the largest pair's train set deciding
 * the chunk). */
int mt_batch_knn2(int norm, int words, const void *dq, const void *dt, const mt_pair_rows *rows, int n_pairs, int n_rows, int swap, int device,
                  hipStream_t s, int32_t *idx, float *dist)
{
    if (n_rows == 0) return 0;
    std::vector<mt_ptile> tiles;
    int max_n2 = 0;
    for (int p = 0; p < n_pairs; p++) {
        const mt_pair_rows &r = rows[p];
        const int qb = swap ? r.t : r.q, nq = swap ? r.nt : r.nq, tb = swap ? r.q : r.t, nt = swap ? r.nq : r.nt, ob = swap ? r.back : r.out;
        if (nt > max_n2) max_n2 = nt;
        for (int k = 0; k < nq; k += MT_Q) tiles.push_back(mt_ptile{make_int4(qb + k, qb + nq, tb, tb + nt), ob + k, {0, 0, 0}});
    }
    const int qtiles = (int)tiles.size();
    int t_chunk, splits; mt_batch_split(qtiles, max_n2, device, &t_chunk, &splits);
    const size_t b_tiles = ((size_t)qtiles * sizeof(mt_ptile) + 255) / 256 * 256, b_part = splits > 1 ? (size_t)splits * n_rows * sizeof(mt_best) : 0;
    char *buf = nullptr;
    MICHK(hipMallocAsync((void **)&buf, b_tiles + b_part, s));
    int rc = mt_batch_upload(device, s, tiles.data(), (size_t)qtiles * sizeof(mt_ptile), buf);
    if (rc) { (void)hipFreeAsync(buf, s); return rc; }
    mt_best *part = splits > 1 ? (mt_best *)(buf + b_tiles) : nullptr;
    const dim3 grid(qtiles, splits), block(256);
    MT_LAUNCH_NORM(mt_knn2_batch_kernel, norm, words, grid, block, s, (const uint32_t *)dq, (const uint32_t *)dt, words, (const mt_ptile *)buf, n_rows,
        t_chunk, idx, dist, part);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess && part) {
        hipLaunchKernelGGL(mt_merge_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, s, part, splits, n_rows, norm != MI_DEGENSAC_NORM_HAMMING ? 1 : 0, idx,
            dist);
        le = hipGetLastError();
    }
    (void)hipFreeAsync(buf, s);
    MICHK(le);
    return 0;
}

int mt_batch_filter_rank(const int32_t *d_idx, const float *d_dist, const int32_t *d_off1, const int32_t *d_off2, int n_pairs, const mt_rule &rule,
                         const int32_t *d_back, const float *d_bdist, hipStream_t s, uint8_t *d_keep, int32_t *d_rank, int32_t *d_count)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(mt_filter_rank_kernel, dim3(n_pairs), dim3(256), 0, s, d_idx, d_dist, d_off1, d_off2, rule, d_back, d_bdist, d_keep, d_rank,
        d_count);
    MICHK(hipGetLastError());
    return 0;
}

int mt_batch_gather(int n_eligible, const int32_t *d_pair_of_e, const int64_t *d_est_off, const int32_t *d_out, const int32_t *d_q1, const int32_t *d_t2,
                    const uint8_t *d_keep, const int32_t *d_rank, const int32_t *d_idx, const double *d_kp1, const double *d_kp2, int kp_dim,
                    const uint32_t *d_seeds, hipStream_t s, double *d_pts1, double *d_pts2, uint32_t *d_seeds_e)
{
    if (n_eligible <= 0) return 0;
    hipLaunchKernelGGL(mt_gather_kernel, dim3(n_eligible), dim3(256), 0, s, d_pair_of_e, d_est_off, d_out, d_q1, d_t2, d_keep, d_rank, d_idx, d_kp1,
        d_kp2, kp_dim, d_seeds, d_pts1, d_pts2, d_seeds_e);
    MICHK(hipGetLastError());
    return 0;
}

int mt_batch_scatter(int n_pairs, const int32_t *d_e_of_p, const int64_t *d_est_off, const int32_t *d_off1, const uint8_t *d_keep, const int32_t *d_rank,
                     const int32_t *d_idx, const double *d_model_e, const int32_t *d_stats_e, const uint8_t *d_mask_e, hipStream_t s, double *d_model,
                     int32_t *d_stats, int32_t *d_match, uint8_t *d_inlier)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(mt_scatter_kernel, dim3(n_pairs), dim3(256), 0, s, d_e_of_p, d_est_off, d_off1, d_keep, d_rank, d_idx, d_model_e, d_stats_e,
        d_mask_e, d_model, d_stats, d_match, d_inlier);
    MICHK(hipGetLastError());
    return 0;
}

int mt_batch_scatter_fh(int n_pairs, const mt_half &f, const mt_half &h, const int32_t *d_off1, const uint8_t *d_keep, const int32_t *d_rank,
                        const int32_t *d_idx, hipStream_t s, double *d_model_f, int32_t *d_stats_f, double *d_model_h, int32_t *d_stats_h,
                        int32_t *d_match, uint8_t *d_inlier_f, uint8_t *d_inlier_h, int32_t *d_summary)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(mt_scatter_fh_kernel, dim3(n_pairs), dim3(256), 0, s, f.e_of_p, f.est_off, h.e_of_p, h.est_off, d_off1, d_keep, d_rank, d_idx,
        f.model_e, f.stats_e, f.mask_e, h.model_e, h.stats_e, h.mask_e, d_model_f, d_stats_f, d_model_h, d_stats_h, d_match, d_inlier_f, d_inlier_h,
        d_summary);
    MICHK(hipGetLastError());
    return 0;
}

/* offsets of a ragged batch: non-decreasing, starting at >= 0, rows addressable with int32 */
static int mt_check_offsets(const int64_t *o, int n_pairs)
{
    if (!o || o[0] < 0) return 0;
    for (int p = 0; p < n_pairs; p++) if (o[p + 1] < o[p]) return 0;
    return o[n_pairs] - o[0] <= 0x3fffffff;
}

extern "C" int mi_degensac_match_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                const int64_t *offsets2_host, int n_pairs, int dim, int device, void *stream, int32_t *d_idx,
                                                float *d_dist)
{
    if (n_pairs < 0) return mi_einval("bad argument");
    int rc = mt_check_norm(norm, dim); if (rc) return rc;
    const int words = mt_row_words(norm, dim);
    if (n_pairs == 0) return 0;
    if (!mt_check_offsets(offsets1_host, n_pairs) || !mt_check_offsets(offsets2_host, n_pairs)) return mi_einval("offsets must be non-negative and non-decreasing");
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    std::vector<int64_t> o1, o2; std::vector<mt_pair_rows> rows;
    mt_ragged_rows(offsets1_host, offsets2_host, n_pairs, o1, o2, rows);
    return mt_batch_knn2(norm, words, (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words,
                         (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words, rows.data(), n_pairs, (int)o1[n_pairs], 0, device,
                         (hipStream_t)stream, d_idx + 2 * offsets1_host[0], d_dist + 2 * offsets1_host[0]);
}

/* ---- the pair list's row layout ------------------------------------------------------------------------------------------ */
int mt_pairs_layout(const int64_t *off1, int m1, const int64_t *off2, int m2, const int32_t *pairs, int n_pairs, mt_pair_rows *rows,
                    int64_t *n_out, int64_t *n_back)
{
    *n_out = *n_back = 0;
    if (n_pairs < 0 || m1 < 0 || m2 < 0) return mi_einval("n_pairs, n_images1 and n_images2 must be >= 0");
    if (n_pairs == 0) return 0;
    if (!pairs) return mi_einval("the pair list is NULL");
    if (!mt_check_offsets(off1, m1) || !mt_check_offsets(off2, m2))
        return mi_einval("store offsets must be non-negative and non-decreasing, with at most 0x3fffffff rows in a store");
    int64_t o = 0, b = 0;
    for (int p = 0; p < n_pairs; p++) {
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        if (i < 0 || i >= m1 || j < 0 || j >= m2) {
            snprintf(mt_err, sizeof mt_err, "pair %d = (%d, %d): image index outside its store (%d and %d images)", p, i, j, m1, m2); return MI_DEGENSAC_EINVAL; }
        const int64_t nq = off1[i + 1] - off1[i], nt = off2[j + 1] - off2[j];
        rows[p] = mt_pair_rows{(int32_t)o, (int32_t)(off1[i] - off1[0]), (int32_t)nq, (int32_t)(off2[j] - off2[0]), (int32_t)nt, (int32_t)b};
        o += nq; b += nt;
        if (o > 0x3fffffff || b > 0x3fffffff)
            return mi_einval("too many rows in one pair list: the output rows and the reverse-search rows are limited to 0x3fffffff each");
    }
    *n_out = o; *n_back = b;
    return 0;
}

extern "C" int mi_degensac_match_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                                                const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim,
                                                int device, void *stream, int32_t *d_idx, float *d_dist)
{
    if (n_pairs < 0) return mi_einval("n_pairs < 0");
    int rc = mt_check_norm(norm, dim); if (rc) return rc;
    const int words = mt_row_words(norm, dim);
    if (n_pairs == 0) return 0;
    std::vector<mt_pair_rows> rows(n_pairs);
    int64_t n_out, n_back;
    rc = mt_pairs_layout(offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, rows.data(), &n_out, &n_back); if (rc) return rc;
    if ((n_out > 0 && (!d_desc1 || !d_idx || !d_dist)) || (n_out > 0 && n_back > 0 && !d_desc2)) return mi_einval("NULL argument");
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    return mt_batch_knn2(norm, words, (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words,
                         (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words,
                         rows.data(), n_pairs, (int)n_out, 0, device, (hipStream_t)stream, d_idx, d_dist);
}

#include "mi_fginn.h"
#include "mi_quantize.h"
