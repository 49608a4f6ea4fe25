/* libmi_degensac.so — batched match-and-verify (include/mi_degensac.h mi_degensac_match_verify_*): host code only, no kernel.
 * Matching, the decision rule and ranks on the device (mi_matcher.hip through mi_match_batch.h) -> ONE read of the per-pair tentative
 * counts -> per model: gather of the eligible pairs' tentatives and the batched estimator (mi_estimator.h) -> scatter back to pair /
 * query order.  One path serves the ragged batch and the pair list over image stores (they differ in the layout step), one model or
 * two (F and H on the same tentatives), device pointers or host pointers.  Scratch: stream-ordered blocks, one for the matching half
 * and one per model.  Every message lands in mi_degensac_last_error(). */
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "mi_match_batch.h"
#include "mi_host.h"
#include "mi_estimator.h"

/* what the matcher stages and mi_host.h report through mt_set_error, as this stage's message */
static int match_rc(int rc) { if (rc) set_err("%s", mi_degensac_match_last_error()); return rc; }

/* One model asked of a call: where its [K, 9] models, per-query inlier flags and [K, 16] stats rows go (stats: optional). */
struct MvReq { int homography; const mi_degensac_params *prm; double *model; uint8_t *inlier; int32_t *stats; };
/* A call's one or two requests (two: the fundamental matrix, then the homography) and what they share: match per query, the [K, 4]
 * summary of the two-model calls, the tentative counts on the host (optional).  The _dev forms fill it with device pointers, the
 * host-pointer forms with host pointers; match / inlier are at the first output row once mv_first_row has been applied. */
struct MvCall { MvReq req[2]; int n; int32_t *match, *summary, *counts; };
/* the ragged batch's match / inlier arrays start at row 0 of side 1, its output rows at row r */
static void mv_first_row(MvCall &c, int64_t r)
{
    if (c.match) c.match += r;
    for (int i = 0; i < c.n; i++) if (c.req[i].inlier) c.req[i].inlier += r;
}

/* everything of a match-and-verify call but its row layout */
static int mv_check_params(int homography, const mi_degensac_match_params *mp, int kp_dim, int n_pairs)
{
    if (homography != 0 && homography != 1) { set_err("homography must be 0 or 1"); return MI_DEGENSAC_EINVAL; }
    if (!mp) { set_err("match params are NULL"); return MI_DEGENSAC_EINVAL; }
    if (!mt_norm_known(mp->norm) || mp->dim <= 0) { set_err("bad norm or descriptor dim"); return MI_DEGENSAC_EINVAL; }
    if (const char *e = mt_norm_dim_error(mp->norm, mp->dim)) { set_err("%s", e); return MI_DEGENSAC_EINVAL; }
    { mt_rule rule; if (const char *e = mt_decide_rule(mp, 1, &rule)) { set_err("%s", e); return MI_DEGENSAC_EINVAL; } }   /* the ratio too */
    if (kp_dim != 2 && kp_dim != 6) { set_err("keypoint rows must be [n,2] or [n,6]"); return MI_DEGENSAC_EINVAL; }
    { int fg; double r; if (const char *e = mt_second_nn(mp, &fg, &r)) { set_err("%s", e); return MI_DEGENSAC_EINVAL; } }
    if (n_pairs < 0) { set_err("n_pairs < 0"); return MI_DEGENSAC_EINVAL; }
    return 0;
}

static int mv_check(int homography, const mi_degensac_match_params *mp, const int64_t *off1, const int64_t *off2, int kp_dim, int n_pairs)
{
    int rc = mv_check_params(homography, mp, kp_dim, n_pairs); if (rc) return rc;
    if (n_pairs == 0) return 0;
    for (const int64_t *o : {off1, off2}) {
        if (!o || o[0] < 0) { set_err("offsets must be given and start at >= 0"); return MI_DEGENSAC_EINVAL; }
        for (int p = 0; p < n_pairs; p++) if (o[p + 1] < o[p]) { set_err("offsets must be non-decreasing"); return MI_DEGENSAC_EINVAL; }
        if (o[n_pairs] - o[0] > 0x3fffffff) { set_err("too many descriptor rows in one batch"); return MI_DEGENSAC_EINVAL; }
    }
    return 0;
}

/* the pair list's refusals and its rows (see the pair-list section below); with_fginn: the *_fginn_pairs* and the two-model entry
 * points, which honour second_nn / spatial_th where the plain ones refuse them */
static int mvp_check(int homography, const mi_degensac_match_params *mp, int kd, const int64_t *off1, int m1, const int64_t *off2, int m2,
                     const int32_t *pairs, int K, bool with_fginn, std::vector<mt_pair_rows> &rows, int64_t *n_out, int64_t *n_back)
{
    int rc = mv_check_params(homography, mp, kd, K); if (rc) return rc;
    int fginn; double r; (void)mt_second_nn(mp, &fginn, &r);
    if (fginn && !with_fginn) { set_err("the FGINN rule (second_nn = 1) is not part of the pair-list entry points: use mi_degensac_match_verify_batch*"
                                        " or, over a pair list, mi_degensac_match_verify_fginn_pairs*"); return MI_DEGENSAC_EINVAL; }
    *n_out = *n_back = 0;
    if (K == 0) return 0;
    rows.resize(K);
    return match_rc(mt_pairs_layout(off1, m1, off2, m2, pairs, K, rows.data(), n_out, n_back));
}

static int mv_check_prms(const MvCall &c, int kd)
{
    for (int i = 0; i < c.n; i++) if (int rc = est_check_params(c.req[i].prm, c.req[i].homography, kd)) return rc;
    return 0;
}
/* the only refusal of a device index here; one below 64 that is not there fails in DevGuard::enter, as EHIP */
static int mv_check_device(int device)
{
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    if (mi_degensac_device_count() == 0) { set_err("no HIP device: this library has no CPU path"); return MI_DEGENSAC_ENODEV; }
    return 0;
}
/* the _dev forms: the summary is required of a two-model call, row arrays only where there are rows */
static int mv_check_null(const void *d_desc1, const void *d_desc2, const double *d_kp1, const double *d_kp2, int64_t n_out, int64_t n_back,
                         const uint32_t *d_seeds, const MvCall &c)
{
    bool bad = !d_seeds || (c.n == 2 && !c.summary) || (n_out > 0 && (!d_desc1 || !d_kp1 || !c.match)) || (n_back > 0 && (!d_desc2 || !d_kp2));
    for (int i = 0; i < c.n; i++) bad = bad || !c.req[i].model || (n_out > 0 && !c.req[i].inlier);
    if (bad) { set_err("NULL argument"); return MI_DEGENSAC_EINVAL; }
    return 0;
}
/* the host-pointer forms: stats, summary and counts are optional */
static int mv_check_host_null(const void *desc1, const void *desc2, const double *kp1, const double *kp2, const uint32_t *seeds, const MvCall &c)
{
    bool bad = !desc1 || !desc2 || !kp1 || !kp2 || !seeds || !c.match;
    for (int i = 0; i < c.n; i++) bad = bad || !c.req[i].model || !c.req[i].inlier;
    if (bad) { set_err("NULL argument"); return MI_DEGENSAC_EINVAL; }
    return 0;
}

/* Where pair p's rows are, as int32 tables on the device (columns of mt_pair_rows).  out [K + 1]: its rows of idx / dist / keep / rank /
 * match / inlier; q1 / t2 [K]: the first keypoint row of its query image in kp1 and of its train image in kp2; back [K]: its first row
 * of the reverse search. */
struct MvRows { const int32_t *out, *q1, *t2, *back; };

/* what the matching half leaves on s (in block A) for the estimating half: nothing of it depends on the model */
struct MvMatched { MvRows R; const int32_t *cnt, *rank, *idx; const uint8_t *keep; const double *kp1, *kp2; };

/* The matching half of the device path, arguments checked and the device current: pair p's rows are rows[p], n_out output rows and
 * n_back rows of the reverse search in all; side 1 / 2 (descriptors and keypoints) start at row r1 / r2 of the arrays passed.  The FGINN
 * step (mp->second_nn) takes the same rows as the 2-NN in front of it.  Everything is enqueued on s into block A (a); m says where it
 * lies. */
static int mv_match(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const double *d_kp1, const double *d_kp2, int64_t r1,
                    int64_t r2, int kd, const std::vector<mt_pair_rows> &rows, int64_t n_out, int64_t n_back, int device, hipStream_t s, MiScratch &a,
                    MvMatched &m)
{
    const int K = (int)rows.size();
    int rc;
    const int words = mt_row_words(mp->norm, mp->dim);
    const bool mutual = mp->mutual != 0;
    /* every row pointer moves to its side's first row; the tables: out [K + 1] | q1 [K] | t2 [K] | back [K] */
    const uint32_t *q1 = (const uint32_t *)d_desc1 + (size_t)r1 * words, *q2 = (const uint32_t *)d_desc2 + (size_t)r2 * words;
    const double *kp1 = d_kp1 + (size_t)r1 * kd, *kp2 = d_kp2 + (size_t)r2 * kd;
    std::vector<int32_t> tab(4 * (size_t)K + 1);
    for (int p = 0; p < K; p++) { tab[p] = rows[p].out; tab[K + 1 + p] = rows[p].q; tab[2 * K + 1 + p] = rows[p].t; tab[3 * K + 1 + p] = rows[p].back; }
    tab[K] = (int32_t)n_out;

    /* block A: tables, forward (and backward) 2-NN, keep / rank / count */
    const size_t b_tab = mi_up256(tab.size() * 4), b_idx = mi_up256((size_t)n_out * 8), b_bidx = mutual ? mi_up256((size_t)n_back * 8) : 0,
                 b_keep = mi_up256((size_t)n_out), b_cnt = mi_up256((size_t)K * 4);
    const size_t a_idx = b_tab, a_dist = a_idx + b_idx, a_bidx = a_dist + b_idx, a_bdist = a_bidx + b_bidx, a_keep = a_bdist + b_bidx,
                 a_rank = a_keep + b_keep, a_cnt = a_rank + b_idx, a_all = a_cnt + b_cnt;
    if ((rc = match_rc(a.alloc(a_all, s)))) return rc;
    char *A = a.p;
    const int32_t *d_out = (const int32_t *)A;
    const MvRows R{d_out, d_out + (K + 1), d_out + (2 * K + 1), d_out + (3 * K + 1)};
    int32_t *idx = (int32_t *)(A + a_idx), *bidx = mutual ? (int32_t *)(A + a_bidx) : nullptr, *rank = (int32_t *)(A + a_rank), *cnt = (int32_t *)(A + a_cnt);
    float *dist = (float *)(A + a_dist), *bdist = (float *)(A + a_bdist);
    uint8_t *keep = (uint8_t *)(A + a_keep);
    m = MvMatched{R, cnt, rank, idx, keep, kp1, kp2};
    rc = match_rc(mt_batch_upload(device, s, tab.data(), tab.size() * 4, A)); if (rc) return rc;
    rc = match_rc(mt_batch_knn2(mp->norm, words, q1, q2, rows.data(), K, (int)n_out, 0, device, s, idx, dist)); if (rc) return rc;
    int fginn; double fginn_r; (void)mt_second_nn(mp, &fginn, &fginn_r);
    if (fginn) { rc = match_rc(mt_batch_fginn(mp->norm, words, q1, q2, kp2, kd, rows.data(), K, (int)n_out, fginn_r, device, s, idx, dist)); if (rc) return rc; }
    if (mutual) { rc = match_rc(mt_batch_knn2(mp->norm, words, q2, q1, rows.data(), K, (int)n_back, 1, device, s, bidx, bdist)); if (rc) return rc; }
    mt_rule rule; (void)mt_decide_rule(mp, 1, &rule);
    return match_rc(mt_batch_filter_rank(idx, dist, R.out, R.back, K, rule, bidx, mutual ? bdist : nullptr, s, keep, rank, cnt));
}

/* the second half of a match-and-verify call, after the filter has written keep / rank / cnt on s: (a) the read of the counts */
static int mv_counts(int K, const int32_t *cnt, hipStream_t s, std::vector<int32_t> &counts, int32_t *h_counts)
{
    /* the one synchronisation: the estimator's launch is sized and configured from the tentative counts on the host */
    counts.resize(K);
    HIPCHK(hipMemcpyAsync(counts.data(), cnt, (size_t)K * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_counts) memcpy(h_counts, counts.data(), (size_t)K * 4);
    return 0;
}

/* (b) one model on the counted tentatives: its eligible list, block B (into b), gather and estimator on s; `half` says where the results
 * lie for the scatter stage */
static int mv_half(int homography, int K, int kd, const mi_degensac_params *prm, const MvMatched &m, const std::vector<int32_t> &counts,
                   const uint32_t *d_seeds, int device, hipStream_t s, MiScratch &b, mt_half &half)
{
    int rc;
    const int min_pts = homography ? 4 : 8;
    std::vector<int64_t> est_off(1, 0); std::vector<int32_t> e_of_p(K, -1), pair_of_e;
    for (int p = 0; p < K; p++)
        if (counts[p] >= min_pts) { e_of_p[p] = (int32_t)pair_of_e.size(); pair_of_e.push_back(p); est_off.push_back(est_off.back() + counts[p]); }
    const int E = (int)pair_of_e.size(); const int64_t T = est_off.back();

    /* block B: est_off | e_of_p | pair_of_e (one upload), seeds, models, stats, the estimator's input rows and masks */
    const size_t c_eoff = 0, c_eop = (size_t)(E + 1) * 8, c_poe = c_eop + (size_t)K * 4, c_all = c_poe + (size_t)E * 4;
    std::vector<char> tab(c_all);
    memcpy(tab.data() + c_eoff, est_off.data(), (size_t)(E + 1) * 8); memcpy(tab.data() + c_eop, e_of_p.data(), (size_t)K * 4);
    if (E) memcpy(tab.data() + c_poe, pair_of_e.data(), (size_t)E * 4);
    const size_t g_seed = mi_up256(c_all), g_model = g_seed + mi_up256((size_t)E * 4), g_stats = g_model + mi_up256((size_t)E * 72),
                 g_p1 = g_stats + mi_up256((size_t)E * 64), g_p2 = g_p1 + mi_up256((size_t)T * kd * 8),
                 g_mask = g_p2 + mi_up256((size_t)T * kd * 8), g_all = g_mask + mi_up256((size_t)T);
    if ((rc = match_rc(b.alloc(g_all, s)))) return rc;
    char *B = b.p;
    const int64_t *d_eoff = (const int64_t *)(B + c_eoff); const int32_t *d_eop = (const int32_t *)(B + c_eop), *d_poe = (const int32_t *)(B + c_poe);
    uint32_t *seeds_e = (uint32_t *)(B + g_seed); double *model_e = (double *)(B + g_model), *pts1 = (double *)(B + g_p1), *pts2 = (double *)(B + g_p2);
    int32_t *stats_e = (int32_t *)(B + g_stats); uint8_t *mask_e = (uint8_t *)(B + g_mask);
    half = mt_half{d_eop, d_eoff, model_e, stats_e, mask_e};
    rc = match_rc(mt_batch_upload(device, s, tab.data(), c_all, B)); if (rc) return rc;
    if (E > 0) {
        rc = match_rc(mt_batch_gather(E, d_poe, d_eoff, m.R.out, m.R.q1, m.R.t2, m.keep, m.rank, m.idx, m.kp1, m.kp2, kd, d_seeds, s, pts1, pts2, seeds_e));
        if (rc) return rc;
        rc = est_launch_batch(homography, pts1, pts2, d_eoff, est_off.data(), E, kd, prm, seeds_e, device, s, model_e, mask_e, stats_e);
        if (rc) return rc;
    }
    return 0;
}

/* The device path of every form, arguments checked (c: device pointers, match / inlier at the first output row): the matching half,
 * the counts read ONCE, then each request's half one after the other on s (each persistent estimator fills the device) and one scatter:
 * the single-model kernel for one request, for two the kernel that writes both and the per-pair summary. */
static int match_verify_rows(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const double *d_kp1, const double *d_kp2,
                             int64_t r1, int64_t r2, int kd, const std::vector<mt_pair_rows> &rows, int64_t n_out, int64_t n_back, const MvCall &c,
                             const uint32_t *d_seeds, int device, hipStream_t s)
{
    const int K = (int)rows.size();
    DevGuard g; int rc = g.enter(device); if (rc) return rc;
    MiScratch b1, b0, a;          /* freed on s when the call returns, whichever way: block A, then the requests' block Bs */
    MiScratch *const b[2] = {&b0, &b1};
    MvMatched m; std::vector<int32_t> counts; mt_half h[2];
    if ((rc = mv_match(mp, d_desc1, d_desc2, d_kp1, d_kp2, r1, r2, kd, rows, n_out, n_back, device, s, a, m))) return rc;
    if ((rc = mv_counts(K, m.cnt, s, counts, c.counts))) return rc;
    for (int i = 0; i < c.n; i++)
        if ((rc = mv_half(c.req[i].homography, K, kd, c.req[i].prm, m, counts, d_seeds, device, s, *b[i], h[i]))) return rc;
    const MvReq &f = c.req[0], &q = c.req[1];
    if (c.n == 1)
        return match_rc(mt_batch_scatter(K, h[0].e_of_p, h[0].est_off, m.R.out, m.keep, m.rank, m.idx, h[0].model_e, h[0].stats_e, h[0].mask_e, s, f.model,
                                         f.stats, c.match, f.inlier));
    return match_rc(mt_batch_scatter_fh(K, h[0], h[1], m.R.out, m.keep, m.rank, m.idx, s, f.model, f.stats, q.model, q.stats, c.match, f.inlier, q.inlier,
                                        c.summary));
}

/* The host-pointer forms' re-run of the pairs discarded after a hand-over time-out (bit 10 of stats[15]): exactly their tentatives,
 * in the order the device gathered them (query order).  Pair p owns the rows out[p] .. out[p+1] of mt / in; the keypoints of its
 * query r are row b1[p] + r - out[p] of k1, those of train row t (pair-local) row b2[p] + t of k2. */
static int mv_rerun(int device, int homography, int kd, int K, const mi_degensac_params *prm, const uint32_t *seeds, const int64_t *out,
                    const int64_t *b1, const int64_t *b2, const double *k1, const double *k2, const int32_t *mt, double *model, uint8_t *in,
                    std::vector<int32_t> &st)
{
    std::vector<int> redo;
    for (int p = 0; p < K; p++) if (st[(size_t)p * 16 + 15] & 1024) redo.push_back(p);
    if (redo.empty()) return 0;
    std::vector<double> q1, q2; std::vector<int64_t> qo(1, 0); std::vector<uint32_t> qs;
    for (int p : redo) {
        for (int64_t i = out[p]; i < out[p + 1]; i++) if (mt[i] >= 0) {
            const int64_t a = b1[p] + (i - out[p]), b = b2[p] + mt[i];
            q1.insert(q1.end(), k1 + a * kd, k1 + (a + 1) * kd);
            q2.insert(q2.end(), k2 + b * kd, k2 + (b + 1) * kd);
        }
        qo.push_back((int64_t)q1.size() / kd); qs.push_back(seeds[p]);
    }
    const int R = (int)redo.size();
    std::vector<double> qm((size_t)R * 9); std::vector<uint8_t> qk((size_t)qo.back()); std::vector<int32_t> qst((size_t)R * 16);
    int rc = est_rerun(device, homography, q1.data(), q2.data(), qo.data(), R, kd, prm, qs.data(), qm.data(), qk.data(), qst.data());
    if (rc) return rc;
    for (int r = 0; r < R; r++) {
        const int p = redo[r]; int64_t k = qo[r];
        memcpy(model + (size_t)p * 9, qm.data() + (size_t)r * 9, 72);
        for (int64_t i = out[p]; i < out[p + 1]; i++) if (mt[i] >= 0) in[i] = qk[k++];
        memcpy(st.data() + (size_t)p * 16, qst.data() + (size_t)r * 16, 64); st[(size_t)p * 16 + 15] |= 2048;     /* bit 11: run again */
    }
    return 0;
}

/* The host-pointer forms (c: host pointers, match / inlier at the first output row): side 1 (rows off1[0] .. off1[m1] of desc1 / kp1)
 * goes to the device, side 2 too unless `same` says both sides name the same arrays, then the seeds; the device path runs on the calling
 * thread's stream and the results come back; then mv_rerun per request (the estimator's re-run, depth 1) for the pairs whose stats row
 * OF THAT MODEL carries bit 10, on exactly their gathered tentatives.  The summary of a pair run again is counted again from its masks. */
static int match_verify_host(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *off1, int m1, const int64_t *off2,
                             int m2, const double *kp1, const double *kp2, int kd, bool same, const std::vector<mt_pair_rows> &rows, int64_t n_out,
                             int64_t n_back, const MvCall &c, const uint32_t *seeds, int device)
{
    const int K = (int)rows.size();
    hipStream_t s; int rc = est_thread_stream(device, &s); if (rc) return rc;
    DevGuard g; rc = g.enter(device); if (rc) return rc;
    const int64_t n1 = off1[m1] - off1[0], n2 = off2[m2] - off2[0];
    const size_t row = mt_row_bytes(mp->norm, mp->dim);
    const double *h_k1 = kp1 + off1[0] * kd, *h_k2 = kp2 + off2[0] * kd;
    /* stats and summary always come back (the re-run reads and mends them); the caller's arrays are filled at the end */
    std::vector<int32_t> cnt(K), st[2], sum((size_t)K * 4);
    MiStage sg; MvCall d = c;
    const int i_d1 = sg.in((const char *)desc1 + off1[0] * row, n1 * row), i_k1 = sg.in(h_k1, (size_t)n1 * kd * 8);
    const int i_d2 = same ? i_d1 : sg.in((const char *)desc2 + off2[0] * row, n2 * row), i_k2 = same ? i_k1 : sg.in(h_k2, (size_t)n2 * kd * 8);
    const int i_sd = sg.in(seeds, (size_t)K * 4);
    int i_mo[2], i_in[2], i_st[2];
    for (int i = 0; i < c.n; i++) {
        st[i].resize((size_t)K * 16);
        i_mo[i] = sg.out(c.req[i].model, (size_t)K * 72); i_in[i] = sg.out(c.req[i].inlier, (size_t)n_out); i_st[i] = sg.out(st[i].data(), (size_t)K * 64);
    }
    const int i_ma = sg.out(c.match, (size_t)n_out * 4), i_su = c.n == 2 ? sg.out(sum.data(), (size_t)K * 16) : -1;
    if ((rc = match_rc(sg.upload()))) return rc;
    /* the single-model forms refuse the estimator's params only here, after the device and the upload, as they always did (the
     * two-model entry points have checked them already) */
    if ((rc = mv_check_prms(c, kd))) return rc;
    for (int i = 0; i < c.n; i++) { d.req[i].model = sg.dev<double>(i_mo[i]); d.req[i].inlier = sg.dev<uint8_t>(i_in[i]); d.req[i].stats = sg.dev<int32_t>(i_st[i]); }
    d.match = sg.dev<int32_t>(i_ma); d.summary = c.n == 2 ? sg.dev<int32_t>(i_su) : nullptr; d.counts = cnt.data();
    rc = match_verify_rows(mp, sg.dev<void>(i_d1), sg.dev<void>(i_d2), sg.dev<double>(i_k1), sg.dev<double>(i_k2), 0, 0, kd, rows, n_out, n_back, d,
                           sg.dev<uint32_t>(i_sd), device, s);
    if (rc) return rc;
    if ((rc = match_rc(sg.finish(s)))) return rc;
    std::vector<int64_t> out(K + 1), b1(K), b2(K);
    for (int p = 0; p < K; p++) { out[p] = rows[p].out; b1[p] = rows[p].q; b2[p] = rows[p].t; }
    out[K] = n_out;
    std::vector<uint8_t> redo(K, 0);
    for (int i = 0; i < c.n; i++) for (int p = 0; p < K; p++) redo[p] |= (st[i][(size_t)p * 16 + 15] & 1024) != 0;
    for (int i = 0; i < c.n; i++) {
        rc = mv_rerun(device, c.req[i].homography, kd, K, c.req[i].prm, seeds, out.data(), b1.data(), b2.data(), h_k1, h_k2, c.match, c.req[i].model,
                      c.req[i].inlier, st[i]);
        if (rc) return rc;
    }
    if (c.n == 2) for (int p = 0; p < K; p++) if (redo[p]) {
        const uint8_t *in_f = c.req[0].inlier, *in_h = c.req[1].inlier;
        int32_t nf = 0, nh = 0, nfh = 0;
        for (int64_t i = out[p]; i < out[p + 1]; i++) { nf += in_f[i] != 0; nh += in_h[i] != 0; nfh += in_f[i] && in_h[i]; }
        sum[(size_t)p * 4 + 1] = nf; sum[(size_t)p * 4 + 2] = nh; sum[(size_t)p * 4 + 3] = nfh;
    }
    for (int i = 0; i < c.n; i++) if (c.req[i].stats) memcpy(c.req[i].stats, st[i].data(), (size_t)K * 64);
    if (c.summary) memcpy(c.summary, sum.data(), (size_t)K * 16);
    if (c.counts) memcpy(c.counts, cnt.data(), (size_t)K * 4);
    return 0;
}

/* ---- the two layouts: each form's refusals in its own order, the layout step, the one run function ---------------------------
 * The ragged batch takes the identity list over its own offsets (mt_ragged_rows).  The pair list has descriptors and keypoints stored
 * once per image: mt_pairs_layout fills the rows from the stores' offsets and the (i, j) list.  Everything after the layout step is
 * shared.  Every refusal comes before a device is looked for, except in the single-model batch _dev form, which looks for the device
 * before the NULLs, and in the single-model host forms, which refuse the estimator's params after the upload. */
static int mv_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *off1, const int64_t *off2,
                        const double *d_kp1, const double *d_kp2, int kd, int K, MvCall c, const uint32_t *d_seeds, int device, void *stream)
{
    int rc = mv_check(c.req[0].homography, mp, off1, off2, kd, K);
    if (rc || K == 0) return rc;
    std::vector<int64_t> o1, o2; std::vector<mt_pair_rows> rows;
    mt_ragged_rows(off1, off2, K, o1, o2, rows);
    if ((rc = mv_check_prms(c, kd)) || (c.n == 1 && (rc = mv_check_device(device))) ||
        (rc = mv_check_null(d_desc1, d_desc2, d_kp1, d_kp2, o1[K], o2[K], d_seeds, c)) || (rc = mv_check_device(device))) return rc;
    mv_first_row(c, off1[0]);
    return match_verify_rows(mp, d_desc1, d_desc2, d_kp1, d_kp2, off1[0], off2[0], kd, rows, o1[K], o2[K], c, d_seeds, device, (hipStream_t)stream);
}

/* the ragged batch never asks whether its two sides are the same arrays: both are uploaded */
static int mv_batch_host(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *off1, const int64_t *off2,
                         const double *kp1, const double *kp2, int kd, int K, MvCall c, const uint32_t *seeds, int device)
{
    int rc = mv_check(c.req[0].homography, mp, off1, off2, kd, K);
    if (rc || K == 0) return rc;
    if ((c.n == 2 && (rc = mv_check_prms(c, kd))) || (rc = mv_check_host_null(desc1, desc2, kp1, kp2, seeds, c))) return rc;
    std::vector<int64_t> o1, o2; std::vector<mt_pair_rows> rows;
    mt_ragged_rows(off1, off2, K, o1, o2, rows);
    mv_first_row(c, off1[0]);
    return match_verify_host(mp, desc1, desc2, off1, K, off2, K, kp1, kp2, kd, false, rows, o1[K], o2[K], c, seeds, device);
}

static int mv_pairs_dev(bool with_fginn, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *off1, int m1,
                        const int64_t *off2, int m2, const double *d_kp1, const double *d_kp2, int kd, const int32_t *pairs, int K, const MvCall &c,
                        const uint32_t *d_seeds, int device, void *stream)
{
    std::vector<mt_pair_rows> rows; int64_t n_out, n_back;
    int rc = mvp_check(c.req[0].homography, mp, kd, off1, m1, off2, m2, pairs, K, with_fginn, rows, &n_out, &n_back);
    if (rc || K == 0) return rc;
    if ((rc = mv_check_prms(c, kd)) || (rc = mv_check_null(d_desc1, d_desc2, d_kp1, d_kp2, n_out, n_back, d_seeds, c)) ||
        (rc = mv_check_device(device))) return rc;
    return match_verify_rows(mp, d_desc1, d_desc2, d_kp1, d_kp2, off1[0], off2[0], kd, rows, n_out, n_back, c, d_seeds, device, (hipStream_t)stream);
}

/* each store goes to the device once: one copy when both sides name the same arrays */
static int mv_pairs_host(bool with_fginn, const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *off1, int m1,
                         const int64_t *off2, int m2, const double *kp1, const double *kp2, int kd, const int32_t *pairs, int K, const MvCall &c,
                         const uint32_t *seeds, int device)
{
    std::vector<mt_pair_rows> rows; int64_t n_out, n_back;
    int rc = mvp_check(c.req[0].homography, mp, kd, off1, m1, off2, m2, pairs, K, with_fginn, rows, &n_out, &n_back);
    if (rc || K == 0) return rc;
    if ((c.n == 2 && (rc = mv_check_prms(c, kd))) || (rc = mv_check_host_null(desc1, desc2, kp1, kp2, seeds, c))) return rc;
    const bool same = desc1 == desc2 && kp1 == kp2 && m1 == m2 && !memcmp(off1, off2, ((size_t)m1 + 1) * 8);
    return match_verify_host(mp, desc1, desc2, off1, m1, off2, m2, kp1, kp2, kd, same, rows, n_out, n_back, c, seeds, device);
}

/* ---- one model (include/mi_degensac.h mi_degensac_match_verify_batch*, _pairs*, _fginn_pairs*) ------------------------------- */
#define MV_ONE(model, match, inlier, stats, counts) MvCall{{{homography, prm, model, inlier, stats}, {}}, 1, match, nullptr, counts}
extern "C" int mi_degensac_match_verify_batch_dev(int homography, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
        const int64_t *offsets1_host, const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2, int kp_dim, int n_pairs,
        const mi_degensac_params *prm, const uint32_t *d_seeds, int device, void *stream, double *d_model, int32_t *d_match, uint8_t *d_inlier,
        int32_t *d_stats, int32_t *h_counts)
{
    return mv_batch_dev(mp, d_desc1, d_desc2, offsets1_host, offsets2_host, d_kp1, d_kp2, kp_dim, n_pairs, MV_ONE(d_model, d_match, d_inlier, d_stats, h_counts),
                        d_seeds, device, stream);
}
extern "C" int mi_degensac_match_verify_batch(int homography, const mi_degensac_match_params *mp, const void *desc1, const void *desc2,
        const int64_t *offsets1, const int64_t *offsets2, const double *kp1, const double *kp2, int kd, int K, const mi_degensac_params *prm,
        const uint32_t *seeds, int device, double *model, int32_t *match, uint8_t *inlier, int32_t *stats, int32_t *counts)
{
    return mv_batch_host(mp, desc1, desc2, offsets1, offsets2, kp1, kp2, kd, K, MV_ONE(model, match, inlier, stats, counts), seeds, device);
}

#define MVP_DEV_ARGS int homography, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, \
        int n_images1, const int64_t *offsets2_host, int n_images2, const double *d_kp1, const double *d_kp2, int kp_dim, const int32_t *pairs_host, \
        int n_pairs, const mi_degensac_params *prm, const uint32_t *d_seeds, int device, void *stream, double *d_model, int32_t *d_match, \
        uint8_t *d_inlier, int32_t *d_stats, int32_t *h_counts
#define MVP_DEV_PASS mp, d_desc1, d_desc2, offsets1_host, n_images1, offsets2_host, n_images2, d_kp1, d_kp2, kp_dim, pairs_host, n_pairs, \
        MV_ONE(d_model, d_match, d_inlier, d_stats, h_counts), d_seeds, device, stream
#define MVP_HOST_ARGS int homography, const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1, int n_images1, \
        const int64_t *offsets2, int n_images2, const double *kp1, const double *kp2, int kd, const int32_t *pairs, int K, \
        const mi_degensac_params *prm, const uint32_t *seeds, int device, double *model, int32_t *match, uint8_t *inlier, int32_t *stats, int32_t *counts
#define MVP_HOST_PASS mp, desc1, desc2, offsets1, n_images1, offsets2, n_images2, kp1, kp2, kd, pairs, K, MV_ONE(model, match, inlier, stats, counts), \
        seeds, device
extern "C" int mi_degensac_match_verify_pairs_dev(MVP_DEV_ARGS) { return mv_pairs_dev(false, MVP_DEV_PASS); }
extern "C" int mi_degensac_match_verify_pairs(MVP_HOST_ARGS) { return mv_pairs_host(false, MVP_HOST_PASS); }
/* the FGINN forms: the same calls without the refusal of second_nn = 1 (second_nn = 0 or the layout before spatial_th: the plain calls) */
extern "C" int mi_degensac_match_verify_fginn_pairs_dev(MVP_DEV_ARGS) { return mv_pairs_dev(true, MVP_DEV_PASS); }
extern "C" int mi_degensac_match_verify_fginn_pairs(MVP_HOST_ARGS) { return mv_pairs_host(true, MVP_HOST_PASS); }
#undef MVP_DEV_ARGS
#undef MVP_DEV_PASS
#undef MVP_HOST_ARGS
#undef MVP_HOST_PASS
#undef MV_ONE

/* ---- match once, verify F and H (include/mi_degensac.h mi_degensac_match_verify_fh_*) -----------------------------------------
 * The matching half once, then both estimators on its tentatives: F on the pairs with >= 8, H on those with >= 4.  The pair-list
 * forms honour second_nn as the *_fginn_pairs* calls do. */
#define MV_TWO(model_f, model_h, match, inlier_f, inlier_h, stats_f, stats_h, summary, counts) \
        MvCall{{{0, prm_f, model_f, inlier_f, stats_f}, {1, prm_h, model_h, inlier_h, stats_h}}, 2, match, summary, counts}
extern "C" int mi_degensac_match_verify_fh_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
        const int64_t *offsets1_host, const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2, int kp_dim, int n_pairs,
        const mi_degensac_params *prm_f, const mi_degensac_params *prm_h, const uint32_t *d_seeds, int device, void *stream, double *d_model_f,
        double *d_model_h, int32_t *d_match, uint8_t *d_inlier_f, uint8_t *d_inlier_h, int32_t *d_stats_f, int32_t *d_stats_h, int32_t *d_summary,
        int32_t *h_counts)
{
    return mv_batch_dev(mp, d_desc1, d_desc2, offsets1_host, offsets2_host, d_kp1, d_kp2, kp_dim, n_pairs,
                        MV_TWO(d_model_f, d_model_h, d_match, d_inlier_f, d_inlier_h, d_stats_f, d_stats_h, d_summary, h_counts), d_seeds, device, stream);
}
extern "C" int mi_degensac_match_verify_fh_pairs_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
        const int64_t *offsets1_host, int n_images1, const int64_t *offsets2_host, int n_images2, const double *d_kp1, const double *d_kp2, int kp_dim,
        const int32_t *pairs_host, int n_pairs, const mi_degensac_params *prm_f, const mi_degensac_params *prm_h, const uint32_t *d_seeds, int device,
        void *stream, double *d_model_f, double *d_model_h, int32_t *d_match, uint8_t *d_inlier_f, uint8_t *d_inlier_h, int32_t *d_stats_f,
        int32_t *d_stats_h, int32_t *d_summary, int32_t *h_counts)
{
    return mv_pairs_dev(true, mp, d_desc1, d_desc2, offsets1_host, n_images1, offsets2_host, n_images2, d_kp1, d_kp2, kp_dim, pairs_host, n_pairs,
                        MV_TWO(d_model_f, d_model_h, d_match, d_inlier_f, d_inlier_h, d_stats_f, d_stats_h, d_summary, h_counts), d_seeds, device, stream);
}
extern "C" int mi_degensac_match_verify_fh_batch(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
        const int64_t *offsets2, const double *kp1, const double *kp2, int kd, int K, const mi_degensac_params *prm_f, const mi_degensac_params *prm_h,
        const uint32_t *seeds, int device, double *model_f, double *model_h, int32_t *match, uint8_t *inlier_f, uint8_t *inlier_h, int32_t *stats_f,
        int32_t *stats_h, int32_t *summary, int32_t *counts)
{
    return mv_batch_host(mp, desc1, desc2, offsets1, offsets2, kp1, kp2, kd, K,
                         MV_TWO(model_f, model_h, match, inlier_f, inlier_h, stats_f, stats_h, summary, counts), seeds, device);
}
extern "C" int mi_degensac_match_verify_fh_pairs(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
        int n_images1, const int64_t *offsets2, int n_images2, const double *kp1, const double *kp2, int kd, const int32_t *pairs, int K,
        const mi_degensac_params *prm_f, const mi_degensac_params *prm_h, const uint32_t *seeds, int device, double *model_f, double *model_h,
        int32_t *match, uint8_t *inlier_f, uint8_t *inlier_h, int32_t *stats_f, int32_t *stats_h, int32_t *summary, int32_t *counts)
{
    return mv_pairs_host(true, mp, desc1, desc2, offsets1, n_images1, offsets2, n_images2, kp1, kp2, kd, pairs, K,
                         MV_TWO(model_f, model_h, match, inlier_f, inlier_h, stats_f, stats_h, summary, counts), seeds, device);
}
#undef MV_TWO
