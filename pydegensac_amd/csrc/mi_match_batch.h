/* Internal interface between the batched matcher stages (mi_matcher.hip) and the match-and-verify orchestration in
 * mi_match_verify.hip, which reaches the estimator through mi_estimator.h.  Not part of the C-ABI: hidden symbols of libmi_degensac.so.
 *
 * The batched stages have one row layout, mt_pair_rows, for the ragged batch and for a pair list over image stores.  Rows and row
 * offsets passed here are relative (offs[0] = 0) and every device pointer is already moved to its side's first row.
 * All functions enqueue on `s` and never synchronise; the device must be current.  Errors: a MI_DEGENSAC_E* code, message in
 * mi_degensac_match_last_error(). */
#ifndef MI_MATCH_BATCH_H
#define MI_MATCH_BATCH_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/mi_degensac.h"

#define MT_HIDDEN __attribute__((visibility("hidden")))

/* a running top-2 of (distance, train index) candidates, shared by the dense matcher and the guided stage (mi_guided.hip) */
struct mt_best { float d0, d1; int i0, i1; };     /* (d0, i0) <= (d1, i1) lexicographically */

/* candidate (d, i) into a running top-2; equal distances keep the lower index first */
__device__ __forceinline__ void mt_push(mt_best &b, float d, int i)
{
    const bool lt0 = d < b.d0 || (d == b.d0 && i < b.i0);
    const bool lt1 = d < b.d1 || (d == b.d1 && i < b.i1);
    if (lt0) { b.d1 = b.d0; b.i1 = b.i0; b.d0 = d; b.i0 = i; }
    else if (lt1) { b.d1 = d; b.i1 = i; }
}

/* ---- the norms (include/mi_degensac.h MI_DEGENSAC_NORM_*): one place for "is it a norm", the kernels' template index, the row size ---- */
static inline bool mt_norm_known(int norm) { return norm == MI_DEGENSAC_NORM_L2 || norm == MI_DEGENSAC_NORM_HAMMING || norm == MI_DEGENSAC_NORM_L2_U8; }
/* template index of the kernels: 0 = L2 over float words, 1 = Hamming, 2 = L2 over uint8 rows */
static inline int mt_norm_index(int norm) { return norm == MI_DEGENSAC_NORM_L2 ? 0 : norm == MI_DEGENSAC_NORM_HAMMING ? 1 : 2; }
/* what is wrong with dim (> 0) under a known norm, or null */
static inline const char *mt_norm_dim_error(int norm, int dim)
{
    if (norm == MI_DEGENSAC_NORM_HAMMING && dim % 4) return "Hamming descriptors must be padded to a multiple of 4 bytes";
    if (norm == MI_DEGENSAC_NORM_L2_U8 && dim % 4) return "uint8 L2 descriptors must be padded with zero bytes to a multiple of 4 bytes";
    if (norm == MI_DEGENSAC_NORM_L2_U8 && dim > MI_DEGENSAC_L2_U8_MAX_DIM)
        return "uint8 L2 descriptors are limited to dim <= 256 (the squared distance stays exact in fp32): use float32 rows beyond that";
    return nullptr;
}
/* 32-bit words / bytes of a descriptor row (float32 elements for L2, packed bytes else) */
static inline int mt_row_words(int norm, int dim) { return norm == MI_DEGENSAC_NORM_L2 ? dim : dim / 4; }
static inline size_t mt_row_bytes(int norm, int dim) { return (size_t)dim * (norm == MI_DEGENSAC_NORM_L2 ? 4 : 1); }

/* what is wrong with an FGINN radius, or null: finite and >= 0 */
static inline const char *mt_spatial_th_error(double r) { return r >= 0 && r <= 1.7976931348623157e308 ? nullptr : "spatial_th must be finite and >= 0"; }
/* the second-neighbour rule of a match_params: *fginn = the mode (0 plain, 1 FGINN at radius *r).  A caller with the layout before
 * spatial_th (struct_size 0, or one that does not cover the field) gets the plain rule whatever its last field holds.  Returns what
 * is wrong, or null. */
static inline const char *mt_second_nn(const mi_degensac_match_params *mp, int *fginn, double *r)
{
    *fginn = 0; *r = 0.0;
    if ((size_t)mp->struct_size < offsetof(mi_degensac_match_params, spatial_th) + sizeof(double)) return nullptr;
    if (mp->second_nn != 0 && mp->second_nn != 1) return "second_nn must be 0 (plain) or 1 (FGINN)";
    if (mp->second_nn == 0) return nullptr;
    *fginn = 1; *r = mp->spatial_th;
    return mt_spatial_th_error(mp->spatial_th);
}

/* ---- the decision rule (include/mi_degensac.h MI_DEGENSAC_DECIDE_*): parsed once on the host, evaluated once on the device ---- */
/* what the three decision kernels take by value */
struct mt_rule { float ratio; int32_t flags; float max_dist; };
/* the rule of a match_params.  A caller whose struct_size does not cover decide / max_dist gets flags = 0 whatever those bytes hold.
 * honour_second_nn: the entry point reads second_nn (an FGINN second neighbour goes with MAX_DIST only).  The ratio is checked here too
 * (not read under NO_RATIO).  Returns what is wrong, or null; needs no device. */
static inline const char *mt_decide_rule(const mi_degensac_match_params *mp, int honour_second_nn, mt_rule *r)
{
    r->ratio = mp->ratio; r->flags = 0; r->max_dist = 0.f;
    if (mp->struct_size > 0 && (size_t)mp->struct_size >= offsetof(mi_degensac_match_params, max_dist) + sizeof(float) && mp->decide != 0) {
        const int d = mp->decide;
        if (d & ~(MI_DEGENSAC_DECIDE_NO_RATIO | MI_DEGENSAC_DECIDE_BACK_RATIO | MI_DEGENSAC_DECIDE_MAX_DIST))
            return "decide: unknown bit (MI_DEGENSAC_DECIDE_NO_RATIO = 1, _BACK_RATIO = 2, _MAX_DIST = 4)";
        if ((d & MI_DEGENSAC_DECIDE_NO_RATIO) && (d & MI_DEGENSAC_DECIDE_BACK_RATIO))
            return "decide: NO_RATIO and BACK_RATIO exclude each other";
        if ((d & MI_DEGENSAC_DECIDE_BACK_RATIO) && !mp->mutual)
            return "decide: BACK_RATIO needs mutual != 0 (it reads the reverse search of the mutual check)";
        int fginn = 0; double rad;
        if (honour_second_nn) (void)mt_second_nn(mp, &fginn, &rad);
        if (fginn && (d & (MI_DEGENSAC_DECIDE_NO_RATIO | MI_DEGENSAC_DECIDE_BACK_RATIO)))
            return "decide: NO_RATIO and BACK_RATIO do not go with second_nn = 1 (FGINN defines a second neighbour for the forward test only)";
        if ((d & MI_DEGENSAC_DECIDE_MAX_DIST) && !(mp->max_dist >= 0.f && mp->max_dist <= 3.402823466e+38f))
            return "max_dist must be finite and >= 0";
        r->flags = d;
        if (d & MI_DEGENSAC_DECIDE_MAX_DIST) r->max_dist = mp->max_dist;
    }
    if (!(r->flags & MI_DEGENSAC_DECIDE_NO_RATIO) && !(mp->ratio > 0.f && mp->ratio <= 3.402823466e+38f)) return "ratio must be finite and > 0";
    return nullptr;
}

/* THE decision of query row i (local index qi in its pair) from the forward 2-NN idx / dist and, when back is set, the reverse one
 * back / bdist whose rows of this pair start at b2.  GUIDED: the guided form of both ratio tests, where a missing slot 1 (dist = inf)
 * passes because nothing competes.  With flags = 0 this is the ratio test and mutual check as they always were, load for load. */
template <bool GUIDED>
__device__ __forceinline__ bool mt_decide(const mt_rule &r, const int32_t *idx, const float *dist, int i, int qi, const int32_t *back,
                                          const float *bdist, int b2)
{
    const int j = idx[2 * i];
    bool ok = j >= 0;
    if (!(r.flags & MI_DEGENSAC_DECIDE_NO_RATIO)) {
        if (!GUIDED) ok = ok && idx[2 * i + 1] >= 0;
        ok = ok && dist[2 * i] < r.ratio * dist[2 * i + 1];
    }
    if ((r.flags & MI_DEGENSAC_DECIDE_MAX_DIST) && ok) ok = dist[2 * i] <= r.max_dist;
    if (ok && back) ok = back[2 * (b2 + j)] == qi;
    if ((r.flags & MI_DEGENSAC_DECIDE_BACK_RATIO) && ok) {
        const size_t o = 2 * (size_t)(b2 + j);
        ok = (GUIDED || back[o + 1] >= 0) && bdist[o] < r.ratio * bdist[o + 1];
    }
    return ok;
}

/* the message mi_degensac_match_last_error() returns for the calling thread */
MT_HIDDEN void mt_set_error(const char *msg);

/* host -> device copy of `bytes` through a pinned staging block: asynchronous, the host block may be reused at once */
MT_HIDDEN int mt_batch_upload(int device, hipStream_t s, const void *h, size_t bytes, void *d);
/* Where the rows of pair p are, relative to the first row of each side: its first output row (idx / dist / keep / rank / match /
 * inlier), its query rows on side 1 (q, nq), its train rows on side 2 (t, nt) and its first row in the back block of the mutual check's
 * reverse search.  The one layout of every batched stage below; mt_identity_rows and mt_pairs_layout fill it. */
struct mt_pair_rows { int32_t out, q, nq, t, nt, back; };
/* the ragged batch, from its relative offsets o1 / o2 [K + 1]: the list whose entry p is (image p of side 1, image p of side 2), with
 * the answers at the queries' own rows and the back block at the train rows */
static inline void mt_identity_rows(const int64_t *o1, const int64_t *o2, int n_pairs, mt_pair_rows *rows)
{
    for (int p = 0; p < n_pairs; p++)
        rows[p] = mt_pair_rows{(int32_t)o1[p], (int32_t)o1[p], (int32_t)(o1[p + 1] - o1[p]), (int32_t)o2[p], (int32_t)(o2[p + 1] - o2[p]), (int32_t)o2[p]};
}
/* the same from the offsets as a caller passes them (off[0] >= 0): o1 / o2 = the relative offsets, rows = the identity list over them */
static inline void mt_ragged_rows(const int64_t *off1, const int64_t *off2, int n_pairs, std::vector<int64_t> &o1, std::vector<int64_t> &o2,
                                  std::vector<mt_pair_rows> &rows)
{
    o1.resize(n_pairs + 1); o2.resize(n_pairs + 1); rows.resize(n_pairs);
    for (int p = 0; p <= n_pairs; p++) { o1[p] = off1[p] - off1[0]; o2[p] = off2[p] - off2[0]; }
    mt_identity_rows(o1.data(), o2.data(), n_pairs, rows.data());
}
/* a pair list over image stores (include/mi_degensac.h mi_degensac_match_*_pairs*): checks the stores' offsets ([m + 1] each) and the
 * (i, j) image indices, fills rows [K] and the row totals.  EINVAL (message set) for bad offsets, an image index outside its store, or
 * output / back rows beyond the batch path's row limit; needs no device */
MT_HIDDEN int mt_pairs_layout(const int64_t *off1, int m1, const int64_t *off2, int m2, const int32_t *pairs, int n_pairs, mt_pair_rows *rows,
                              int64_t *n_out, int64_t *n_back);
/* batched 2-NN, dq / dt at the first row of side 1 / 2.  swap = 0: rows q .. q + nq of dq against t .. t + nt of dt into the output
 * rows from `out`; swap = 1 (the reverse search): dq / dt are sides 2 / 1, rows t .. t + nt of dq against q .. q + nq of dt into the
 * rows from `back`.  idx / dist [n_rows, 2] with n_rows the total of the side written, indices local to the pair.  words = 32-bit
 * words per descriptor row. */
MT_HIDDEN int mt_batch_knn2(int norm, int words, const void *dq, const void *dt, const mt_pair_rows *rows, int n_pairs, int n_rows, int swap, int device,
                            hipStream_t s, int32_t *idx, float *dist);
/* FGINN (mi_fginn.h): after mt_batch_knn2 (swap = 0) over the same rows on s, slot 1 of idx / dist [n_rows, 2] becomes the nearest
 * train row whose keypoint (kt: [rows, kd] of side 2, at its first row) lies at least r from the keypoint of slot 0; no host
 * synchronisation */
MT_HIDDEN int mt_batch_fginn(int norm, int words, const void *dq, const void *dt, const double *kt, int kd, const mt_pair_rows *rows, int n_pairs,
                             int n_rows, double r, int device, hipStream_t s, int32_t *idx, float *dist);
/* the mark pass of FGINN alone, for any stage whose result lists have the matcher's layout: per entry (d_rows [K] on the device) the
 * queries whose slot 1 exists and does not compete with slot 0 at squared radius rr, as OUTPUT rows in ascending order to
 * list[out ..], their number to count[p]; no host synchronisation */
MT_HIDDEN int mt_batch_fginn_mark(const int32_t *idx, const mt_pair_rows *d_rows, int n_pairs, const double *kt, int kd, double rr, hipStream_t s,
                                  int32_t *list, int32_t *count);
/* the decision rule (mt_decide: ratio test, + mutual check when d_back is set, + what rule.flags adds; d_bdist, the reverse search's
 * distances next to d_back, is read only under BACK_RATIO) and the rank of every kept query among its pair's kept queries; one
 * workgroup per pair.  d_off1 / d_off2: [K + 1] relative int32 row offsets on the device.  d_off1 says where the pair's idx / dist /
 * keep / rank rows are (the `out` column and the total), d_off2[p] (the only entry read) where its rows of d_back start (the `back`
 * column). */
MT_HIDDEN int mt_batch_filter_rank(const int32_t *d_idx, const float *d_dist, const int32_t *d_off1, const int32_t *d_off2, int n_pairs,
                                   const mt_rule &rule, const int32_t *d_back, const float *d_bdist, hipStream_t s, uint8_t *d_keep, int32_t *d_rank,
                                   int32_t *d_count);
/* the estimator's input rows of the E eligible pairs: pts[est_off[e] + rank[i]] = kp rows of query i and of its nearest train row;
 * seeds_e[e] = seeds[pair_of_e[e]].  d_out [K + 1]: output-row offsets (where keep / rank / idx live), d_q1 / d_t2 [K]: the first
 * keypoint row of the pair's query image in kp1 and of its train image in kp2 */
MT_HIDDEN int mt_batch_gather(int n_eligible, const int32_t *d_pair_of_e, const int64_t *d_est_off, const int32_t *d_out, const int32_t *d_q1,
                              const int32_t *d_t2, const uint8_t *d_keep, const int32_t *d_rank, const int32_t *d_idx, const double *d_kp1,
                              const double *d_kp2, int kp_dim, const uint32_t *d_seeds, hipStream_t s, double *d_pts1, double *d_pts2,
                              uint32_t *d_seeds_e);
/* results back to pair order: model / stats of eligible index e_of_p[p] (zeros for short pairs, e_of_p[p] = -1), match[i] = the
 * pair-local train row of a tentative or -1, inlier[i] = tentative and inlier of the pair's model */
MT_HIDDEN int mt_batch_scatter(int n_pairs, const int32_t *d_e_of_p, const int64_t *d_est_off, const int32_t *d_off1, const uint8_t *d_keep,
                               const int32_t *d_rank, const int32_t *d_idx, const double *d_model_e, const int32_t *d_stats_e, const uint8_t *d_mask_e,
                               hipStream_t s, double *d_model, int32_t *d_stats /*nullable*/, int32_t *d_match, uint8_t *d_inlier);
/* one estimator's results over its eligible pairs, as mt_batch_scatter takes them: e_of_p [K] (-1 = short pair), est_off [E + 1], and
 * model [E*9] / stats [E*16] / mask [est_off[E]] in eligible order; all on the device */
struct mt_half { const int32_t *e_of_p; const int64_t *est_off; const double *model_e; const int32_t *stats_e; const uint8_t *mask_e; };
/* mt_batch_scatter for two estimators run on the same tentatives (f: fundamental matrix, h: homography; each half has its own eligible
 * list and row base) in one launch: both models / stats rows (d_stats_* nullable), one match, inlier_f / inlier_h per query, and
 * d_summary [K*4] = per pair (tentatives, rows with inlier_f, rows with inlier_h, rows with both), counted without atomics */
MT_HIDDEN int mt_batch_scatter_fh(int n_pairs, const mt_half &f, const mt_half &h, const int32_t *d_off1, const uint8_t *d_keep,
                                  const int32_t *d_rank, const int32_t *d_idx, hipStream_t s, double *d_model_f, int32_t *d_stats_f /*nullable*/,
                                  double *d_model_h, int32_t *d_stats_h /*nullable*/, int32_t *d_match, uint8_t *d_inlier_f, uint8_t *d_inlier_h,
                                  int32_t *d_summary);

/* ---- guided matching (mi_guided.hip) ---- */
/* the gate of a model kind: th from px_th / error_type as fill_params derives it; EINVAL (message set) for a bad error_type or a
 * px_th that is negative or NaN */
struct mt_gate { int gk, hk; double th, tb; int screen; };
MT_HIDDEN int mt_guided_gate(int homography, int error_type, double px_th, mt_gate *g);
/* guided 2-NN over the same rows as mt_batch_knn2 (dq / dt, kq / kt [rows, kd] at the first row of their side): every query row of
 * entry p against the candidate rows that pass the gate of ITS model d_models[9 p ..] (the model belongs to the list entry, not to an
 * image).  swap = 0: dq / kq are side 1, rows q .. q + nq against t .. t + nt of dt / kt, gate(query, candidate), into the output rows from
 * `out`; swap = 1 (the reverse search of the mutual check): dq / kq are side 2, rows t .. t + nt against q .. q + nq of dt / kt,
 * gate(candidate, query), into the rows from `back`.  idx / dist [n_rows, 2] with n_rows the total of the side written, indices local to
 * the entry's candidate image.  No row is gathered or copied. */
MT_HIDDEN int mt_batch_guided_knn2(int norm, int words, const void *dq, const void *dt, const double *kq, const double *kt, int kd,
                                   const mt_pair_rows *rows, int n_pairs, int n_rows, const double *d_models, const mt_gate &g, int swap, int device,
                                   hipStream_t s, int32_t *idx, float *dist);
/* FGINN inside the gate: after mt_batch_guided_knn2 (swap = 0) over the same rows, models and gate on s, slot 1 of idx / dist becomes the
 * nearest GATED train row whose keypoint lies at least r from the keypoint of slot 0 (-1 / inf when none does); no host synchronisation */
MT_HIDDEN int mt_batch_guided_fginn(int norm, int words, const void *dq, const void *dt, const double *kq, const double *kt, int kd,
                                    const mt_pair_rows *rows, int n_pairs, int n_rows, const double *d_models, const mt_gate &g, double r, int device,
                                    hipStream_t s, int32_t *idx, float *dist);
/* the decision: match[i] = idx[i][0] when it exists and dist[i][0] < ratio * dist[i][1] (and back[b2 + idx[i][0]][0] == i - lo when
 * d_back is set; the guided form of mt_decide under rule.flags, d_bdist as for mt_batch_filter_rank), else -1; count[p] (nullable) = guided matches of pair p.  d_off1 [K + 1]: the output-row offsets (the `out` column and
 * the total), d_off2[p] (the only entry read): where the pair's rows of d_back start (the `back` column), as for mt_batch_filter_rank */
MT_HIDDEN int mt_batch_guided_decide(const int32_t *d_idx, const float *d_dist, const int32_t *d_off1, const int32_t *d_off2, int n_pairs,
                                     const mt_rule &rule, const int32_t *d_back, const float *d_bdist, hipStream_t s, int32_t *d_match,
                                     int32_t *d_count);
#endif /* MI_MATCH_BATCH_H */
