/* libmi_degensac.so — verified matches as compact per-entry lists (include/mi_degensac.h mi_degensac_correspondences_*): a stable
 * stream compaction over the N output rows of a pair list (or of the ragged batch, the identity list), with the keypoint coordinates
 * and the estimator's own residual per surviving row.  gfx950 only, no CPU path.
 *
 * The rows already lie entry after entry, so one compaction in row order is the whole job.  Three passes, none of which waits for
 * another workgroup (no look-back, no flags, no atomics):
 *   count   a workgroup of 256 threads owns MX_ROWS = 1024 consecutive rows, 4 per thread (match as one 16-byte load, keep as one
 *           4-byte load where the row's address allows it, scalar loads else and in the tail); the selected rows are counted with
 *           wave ballots and popcounts plus four LDS words -> one int32 per workgroup;
 *   scan    one workgroup scans those counts exclusively, MX_SCAN = 256 per step with a running carry, writes d_total and the
 *           corr_offsets of the entries that start at row N (the trailing empty entries and element [K]);
 *   write   recomputes the flags, position = the workgroup's base + the ballot prefix, and writes rows / entry / pts / resid at
 *           positions < capacity; the thread that owns the first row of an entry writes that entry's corr_offsets (the selected rows
 *           before it, whether or not the row itself is selected) and those of the empty entries that start at the same row.
 * A row's entry is the last entry whose first output row is <= the row (binary search for a thread's first row, a forward walk for
 * its other three), which skips empty entries.  match is compared with the entry's train rows before it is used as an index. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_host.h"
#include "mi_dev_util.h"
#include "dg_geom.h"

#define MX_ROWS 1024              /* rows per workgroup: 256 threads x 4 consecutive rows */
#define MX_SCAN 256               /* workgroup counts per step of the scan */

enum { MX_NONE = -1, MX_F_SAMPSON = 0, MX_F_SYM = 1, MX_H_SAMPSON = 2, MX_H_SYM = 3 };      /* the gate kinds of mi_guided.hip */
enum { MX_VEC_ROWS = 1, MX_VEC_PTS = 2 };                                                    /* d_rows 8-byte / d_pts 16-byte aligned */

struct mx_args {
    const int32_t *out;           /* [K + 1] first output row per entry, out[K] = N */
    const mt_pair_rows *rec;      /* [K] */
    int K, N;
    const int32_t *match;         /* [N] */
    const uint8_t *keep;          /* [N] or null */
    /* the write pass only */
    const int32_t *base;          /* [workgroups] selected rows before the workgroup's first row */
    int64_t capacity;
    int64_t *corr_offsets;
    int32_t *rows, *entry;
    double *pts, *resid;
    const double *kp1, *kp2;      /* at the first row of each store */
    int kd;
    const double *models, *hprep; /* [K * 9]; [K * 18] = Hinv | H1 per entry (MX_H_SYM) */
    int hk;
    int32_t add1, add2;           /* MI_DEGENSAC_CORR_STORE_ROWS: the stores' first offsets, else 0 with store = 0 */
    int store, vec;
};

/* the four rows r0 .. r0 + 3 of one thread: bit j of the result = row r0 + j is selected; e[j] = its entry, m[j] = its match value
 * (both meaningful for rows < N only) */
__device__ __forceinline__ unsigned mx_flags(const mx_args &a, int r0, int (&e)[4], int (&m)[4])
{
    e[0] = e[1] = e[2] = e[3] = 0; m[0] = m[1] = m[2] = m[3] = -1;
    if (r0 >= a.N) return 0u;
    int lo = 0, hi = a.K - 1;                                        /* the last entry with out <= r0 */
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.out[mid] <= r0) lo = mid; else hi = mid - 1; }
    const bool full = r0 + 4 <= a.N;
    unsigned kb = 0xfu;
    if (full && (((uintptr_t)(a.match + r0)) & 15u) == 0) {
        const int4 v = *reinterpret_cast<const int4 *>(a.match + r0);
        m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) if (r0 + j < a.N) m[j] = a.match[r0 + j];
    }
    if (a.keep) {
        kb = 0u;
        if (full && (((uintptr_t)(a.keep + r0)) & 3u) == 0) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(a.keep + r0);
#pragma unroll
            for (int j = 0; j < 4; j++) kb |= ((v >> (8 * j)) & 255u) ? 1u << j : 0u;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) if (r0 + j < a.N && a.keep[r0 + j]) kb |= 1u << j;
        }
    }
    unsigned f = 0u;
    int ent = lo;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + j;
        if (r >= a.N) break;
        while (ent + 1 < a.K && a.out[ent + 1] <= r) ent++;
        e[j] = ent;
        if (m[j] >= 0 && m[j] < a.rec[ent].nt && ((kb >> j) & 1u)) f |= 1u << j;
    }
    return f;
}

__global__ __launch_bounds__(256) void mx_count_kernel(mx_args a, int32_t *cnt)
{
    int e[4], m[4];
    const unsigned f = mx_flags(a, (int)blockIdx.x * MX_ROWS + (int)threadIdx.x * 4, e, m);
    int before, total;
    mi_wave_prefix(f, threadIdx.x & 63, &before, &total);
    mi_block_count(total, cnt);
}

/* one workgroup: base[b] = the counts before workgroup b, *total, and corr_offsets of every entry that starts at row N */
__global__ __launch_bounds__(MX_SCAN) void mx_scan_kernel(const int32_t *cnt, int nb, int32_t *base, int64_t *total, const int32_t *out, int K, int N,
                                                          int64_t *corr_offsets)
{
    const int tid = threadIdx.x;
    const int64_t carry = mi_block_scan<MX_SCAN>(cnt, nb, base);
    if (tid == 0) *total = carry;
    for (int p = tid; p <= K; p += MX_SCAN) if (out[p] >= N) corr_offsets[p] = carry;
}

/* Hinv | H1 of every entry's model, as mg_guided_kernel prepares them */
__global__ __launch_bounds__(256) void mx_prepare_kernel(const double *models, int K, double *hprep)
{
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p >= K) return;
    double M[9], Hinv[9], H1[9];
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = models[(size_t)p * 9 + i];
    dg_hsym_prepare(M, Hinv, H1);
#pragma unroll
    for (int i = 0; i < 9; i++) { hprep[(size_t)p * 18 + i] = Hinv[i]; hprep[(size_t)p * 18 + 9 + i] = H1[i]; }
}

template <int GK>
__global__ __launch_bounds__(256) void mx_write_kernel(mx_args a)
{
    __shared__ int wsum[4];
    int e[4], m[4];
    const int r0 = (int)blockIdx.x * MX_ROWS + (int)threadIdx.x * 4;
    const unsigned f = mx_flags(a, r0, e, m);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int before, total;
    mi_wave_prefix(f, lane, &before, &total);
    if (lane == 0) wsum[wv] = total;
    __syncthreads();
    int64_t pos = (int64_t)a.base[blockIdx.x] + before;
#pragma unroll
    for (int w = 0; w < 4; w++) if (w < wv) pos += wsum[w];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + j;
        if (r >= a.N) break;
        const int ent = e[j];
        const int first = a.out[ent];
        if (r == first) {                                            /* the entry's offset, and that of the empty entries in front of it */
            a.corr_offsets[ent] = pos;
            for (int p = ent - 1; p >= 0 && a.out[p] == first; p--) a.corr_offsets[p] = pos;
        }
        if (!((f >> j) & 1u)) continue;
        const int64_t at = pos++;
        if (at >= a.capacity) continue;
        const mt_pair_rows rc = a.rec[ent];
        const int q = r - first;                                     /* 0 <= q < rc.nq, 0 <= m[j] < rc.nt */
        const int c0 = a.store ? a.add1 + rc.q + q : q, c1 = a.store ? a.add2 + rc.t + m[j] : m[j];
        if (a.vec & MX_VEC_ROWS) *reinterpret_cast<int2 *>(a.rows + 2 * at) = make_int2(c0, c1);
        else { a.rows[2 * at] = c0; a.rows[2 * at + 1] = c1; }
        if (a.entry) a.entry[at] = ent;
        if (!a.pts && GK == MX_NONE) continue;
        const double *k1 = a.kp1 + (size_t)(rc.q + q) * a.kd, *k2 = a.kp2 + (size_t)(rc.t + m[j]) * a.kd;
        const double x1 = k1[0], y1 = k1[1], x2 = k2[0], y2 = k2[1];
        if (a.pts) {
            if (a.vec & MX_VEC_PTS) {
                double2 *o = reinterpret_cast<double2 *>(a.pts + 4 * at);
                o[0] = make_double2(x1, y1); o[1] = make_double2(x2, y2);
            } else { double *o = a.pts + 4 * at; o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; }
        }
        if (GK != MX_NONE) {
            double res;
            if (GK == MX_H_SYM) {
                const double *hp = a.hprep + (size_t)ent * 18;
                double Hinv[9], H1[9];
#pragma unroll
                for (int i = 0; i < 9; i++) { Hinv[i] = hp[i]; H1[i] = hp[9 + i]; }
                res = dg_Hsym(Hinv, H1, x1, y1, x2, y2, a.hk, a.hk >= 3);
            } else {
                double M[9];
#pragma unroll
                for (int i = 0; i < 9; i++) M[i] = a.models[(size_t)ent * 9 + i];
                res = GK == MX_F_SAMPSON ? dg_FDs(M, x1, y1, x2, y2) : GK == MX_F_SYM ? dg_FDsSym(M, x1, y1, x2, y2) : dg_HDs(M, x1, y1, x2, y2);
            }
            a.resid[at] = res;
        }
    }
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_correspondences_tile(int which) { return which == 0 ? MX_ROWS : which == 1 ? MX_SCAN : -1; }

/* what the call is asked for, after the checks that need neither the list nor a device */
struct mx_what { int gk, hk; };

/* refusals 1 - 4 of include/mi_degensac.h, in that order */
static int mx_check_params(uint32_t flags, int kp_dim, bool want_pts, bool want_resid, const void *models, const mi_degensac_guide_params *gp,
                           int64_t capacity, int n_pairs, mx_what *w)
{
    w->gk = MX_NONE; w->hk = 0;
    if (flags & ~(uint32_t)MI_DEGENSAC_CORR_STORE_ROWS) return mi_einval("flags: unknown bit (MI_DEGENSAC_CORR_STORE_ROWS = 1)");
    if ((want_pts || want_resid) && kp_dim != 2 && kp_dim != 6) return mi_einval("keypoint rows must be [n,2] or [n,6]");
    if (want_resid) {
        if (!models) return mi_einval("resid needs models");
        if (!gp) return mi_einval("resid needs guide params (homography, error_type)");
        if (gp->struct_size != 0 && gp->struct_size < (int32_t)sizeof(mi_degensac_guide_params)) return mi_einval("guide params: struct_size too small");
        if (gp->homography != 0 && gp->homography != 1) return mi_einval("homography must be 0 or 1");
        mt_gate g;
        const int rc = mt_guided_gate(gp->homography, gp->error_type, 0.0, &g);      /* px_th is not read: the gate kind and its messages */
        if (rc) return rc;
        w->gk = g.gk; w->hk = g.hk;
    }
    if (capacity < 0) return mi_einval("capacity < 0");
    if (n_pairs < 0) return mi_einval("n_pairs < 0");
    return 0;
}

/* refusal 5 of the ragged batch: what the guided batch calls refuse */
static int mx_check_batch_offsets(const int64_t *o1, const int64_t *o2, int n_pairs)
{
    for (const int64_t *o : {o1, o2}) {
        if (!o || o[0] < 0) return mi_einval("offsets must be given and start at >= 0");
        for (int p = 0; p < n_pairs; p++) if (o[p + 1] < o[p]) return mi_einval("offsets must be non-decreasing");
        if (o[n_pairs] - o[0] > 0x3fffffff) return mi_einval("too many descriptor rows in one batch");
    }
    return 0;
}

/* refusal 6: the last row of each store as an int32 */
static int mx_check_store_rows(uint32_t flags, int64_t end1, int64_t end2)
{
    if ((flags & MI_DEGENSAC_CORR_STORE_ROWS) && (end1 > 0x7fffffff || end2 > 0x7fffffff))
        return mi_einval("MI_DEGENSAC_CORR_STORE_ROWS: the stores' rows do not fit int32 (offsets beyond 0x7fffffff)");
    return 0;
}

/* The device path of both layouts, arguments checked and the device current.  match / keep are at output row 0, kp1 / kp2 at the first
 * row of their store; add1 / add2 = the stores' first offsets. */
static int mx_rows_dev(const std::vector<mt_pair_rows> &rows, int64_t n_out, const int32_t *d_match, const uint8_t *d_keep, uint32_t flags, int64_t add1,
                       int64_t add2, const double *kp1, const double *kp2, int kd, const double *d_models, const mx_what &w, int64_t capacity, int device,
                       hipStream_t s, int64_t *d_corr_offsets, int64_t *d_total, int32_t *d_rows, int32_t *d_entry, double *d_pts, double *d_resid)
{
    const int K = (int)rows.size(), N = (int)n_out;
    const int nb = (N + MX_ROWS - 1) / MX_ROWS;
    std::vector<char> tab;
    const size_t a_rec = ((size_t)(K + 1) * 4 + 15) / 16 * 16;
    tab.resize(a_rec + (size_t)K * sizeof(mt_pair_rows));
    int32_t *out = (int32_t *)tab.data();
    for (int p = 0; p < K; p++) out[p] = rows[p].out;
    out[K] = N;
    memcpy(tab.data() + a_rec, rows.data(), (size_t)K * sizeof(mt_pair_rows));
    const bool hsym = w.gk == MX_H_SYM && N > 0;
    const size_t a_cnt = mi_up256(tab.size()), a_base = a_cnt + mi_up256((size_t)nb * 4), a_hp = a_base + mi_up256((size_t)nb * 4),
                 a_all = a_hp + (hsym ? mi_up256((size_t)K * 18 * 8) : 0);
    MiScratch scr; int rc = scr.alloc(a_all, s); if (rc) return rc;
    char *blk = scr.p;
    rc = mt_batch_upload(device, s, tab.data(), tab.size(), blk); if (rc) return rc;
    mx_args a;
    memset(&a, 0, sizeof a);
    a.out = (const int32_t *)blk; a.rec = (const mt_pair_rows *)(blk + a_rec); a.K = K; a.N = N;
    a.match = d_match; a.keep = d_keep;
    int32_t *cnt = (int32_t *)(blk + a_cnt), *base = (int32_t *)(blk + a_base);
    double *hprep = hsym ? (double *)(blk + a_hp) : nullptr;
    a.base = base; a.capacity = capacity; a.corr_offsets = d_corr_offsets; a.rows = d_rows; a.entry = d_entry; a.pts = d_pts; a.resid = d_resid;
    a.kp1 = kp1; a.kp2 = kp2; a.kd = kd; a.models = d_models; a.hprep = hprep; a.hk = w.hk;
    a.store = (flags & MI_DEGENSAC_CORR_STORE_ROWS) ? 1 : 0; a.add1 = a.store ? (int32_t)add1 : 0; a.add2 = a.store ? (int32_t)add2 : 0;
    a.vec = ((((uintptr_t)d_rows) & 7u) == 0 ? MX_VEC_ROWS : 0) | ((((uintptr_t)d_pts) & 15u) == 0 ? MX_VEC_PTS : 0);
    if (nb > 0) {
        hipLaunchKernelGGL(mx_count_kernel, dim3(nb), dim3(256), 0, s, a, cnt);
        MICHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mx_scan_kernel, dim3(1), dim3(MX_SCAN), 0, s, (const int32_t *)cnt, nb, base, d_total, a.out, K, N, d_corr_offsets);
    MICHK(hipGetLastError());
    if (nb > 0) {
        if (hsym) {
            hipLaunchKernelGGL(mx_prepare_kernel, dim3((K + 255) / 256), dim3(256), 0, s, d_models, K, hprep);
            MICHK(hipGetLastError());
        }
        const dim3 grid(nb), block(256);
        switch (w.gk) {
        case MX_F_SAMPSON: hipLaunchKernelGGL((mx_write_kernel<MX_F_SAMPSON>), grid, block, 0, s, a); break;
        case MX_F_SYM: hipLaunchKernelGGL((mx_write_kernel<MX_F_SYM>), grid, block, 0, s, a); break;
        case MX_H_SAMPSON: hipLaunchKernelGGL((mx_write_kernel<MX_H_SAMPSON>), grid, block, 0, s, a); break;
        case MX_H_SYM: hipLaunchKernelGGL((mx_write_kernel<MX_H_SYM>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((mx_write_kernel<MX_NONE>), grid, block, 0, s, a); break;
        }
        MICHK(hipGetLastError());
    }
    return 0;
}

/* refusal 7, then the device and the path above; off1_0 / off2_0 = the stores' first offsets (the rows the store pointers skip) */
static int mx_dev(const std::vector<mt_pair_rows> &rows, int n_pairs, int64_t n_out, int64_t off1_0, int64_t off2_0, const int32_t *d_match,
                  const uint8_t *d_keep, uint32_t flags, const double *d_kp1, const double *d_kp2, int kd, const double *d_models, const mx_what &w,
                  int64_t capacity, int device, hipStream_t s, int64_t *d_corr_offsets, int64_t *d_total, int32_t *d_rows, int32_t *d_entry, double *d_pts,
                  double *d_resid)
{
    if (!d_corr_offsets || !d_total) return mi_einval("NULL argument: d_corr_offsets and d_total are always written");
    if (n_pairs > 0 && n_out > 0 && (!d_match || (capacity > 0 && !d_rows) || ((d_pts || d_resid) && (!d_kp1 || !d_kp2))))
        return mi_einval("NULL argument");
    MiDevGuard dg; int rc = dg.enter(device); if (rc) return rc;
    if (n_pairs == 0) {                                              /* total = 0 and corr_offsets[0] = 0, asynchronously */
        MICHK(hipMemsetAsync(d_total, 0, 8, s));
        MICHK(hipMemsetAsync(d_corr_offsets, 0, 8, s));
        return 0;
    }
    const bool kp = d_pts || d_resid;
    return mx_rows_dev(rows, n_out, d_match, d_keep, flags, off1_0, off2_0, kp ? d_kp1 + (size_t)off1_0 * kd : nullptr,
                       kp ? d_kp2 + (size_t)off2_0 * kd : nullptr, kd, d_models, w, capacity, device, s, d_corr_offsets, d_total, d_rows, d_entry, d_pts,
                       d_resid);
}

extern "C" int mi_degensac_correspondences_pairs_dev(const int64_t *offsets1_host, int n_images1, const int64_t *offsets2_host, int n_images2,
                                                     const int32_t *pairs_host, int n_pairs, const int32_t *d_match, const uint8_t *d_keep, uint32_t flags,
                                                     const double *d_kp1, const double *d_kp2, int kp_dim, const double *d_models,
                                                     const mi_degensac_guide_params *gp, int64_t capacity, int device, void *stream,
                                                     int64_t *d_corr_offsets, int64_t *d_total, int32_t *d_rows, int32_t *d_entry, double *d_pts,
                                                     double *d_resid)
{
    mx_what w; int rc = mx_check_params(flags, kp_dim, d_pts != nullptr, d_resid != nullptr, d_models, gp, capacity, n_pairs, &w); if (rc) return rc;
    std::vector<mt_pair_rows> rows; int64_t n_out = 0, n_back = 0, o1 = 0, o2 = 0;
    if (n_pairs > 0) {
        rows.resize(n_pairs);
        rc = mt_pairs_layout(offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, rows.data(), &n_out, &n_back); if (rc) return rc;
        rc = mx_check_store_rows(flags, offsets1_host[n_images1], offsets2_host[n_images2]); if (rc) return rc;
        o1 = offsets1_host[0]; o2 = offsets2_host[0];
    }
    return mx_dev(rows, n_pairs, n_out, o1, o2, d_match, d_keep, flags, d_kp1, d_kp2, kp_dim, d_models, w, capacity, device, (hipStream_t)stream,
                  d_corr_offsets, d_total, d_rows, d_entry, d_pts, d_resid);
}

extern "C" int mi_degensac_correspondences_batch_dev(const int64_t *offsets1_host, const int64_t *offsets2_host, int n_pairs, const int32_t *d_match,
                                                     const uint8_t *d_keep, uint32_t flags, const double *d_kp1, const double *d_kp2, int kp_dim,
                                                     const double *d_models, const mi_degensac_guide_params *gp, int64_t capacity, int device,
                                                     void *stream, int64_t *d_corr_offsets, int64_t *d_total, int32_t *d_rows, int32_t *d_entry,
                                                     double *d_pts, double *d_resid)
{
    mx_what w; int rc = mx_check_params(flags, kp_dim, d_pts != nullptr, d_resid != nullptr, d_models, gp, capacity, n_pairs, &w); if (rc) return rc;
    std::vector<int64_t> r1, r2; std::vector<mt_pair_rows> rows; int64_t n_out = 0, o1 = 0, o2 = 0;
    if (n_pairs > 0) {
        rc = mx_check_batch_offsets(offsets1_host, offsets2_host, n_pairs); if (rc) return rc;
        rc = mx_check_store_rows(flags, offsets1_host[n_pairs], offsets2_host[n_pairs]); if (rc) return rc;
        mt_ragged_rows(offsets1_host, offsets2_host, n_pairs, r1, r2, rows);
        n_out = r1[n_pairs]; o1 = offsets1_host[0]; o2 = offsets2_host[0];
    }
    return mx_dev(rows, n_pairs, n_out, o1, o2, d_match ? d_match + o1 : nullptr, d_keep ? d_keep + o1 : nullptr, flags, d_kp1, d_kp2, kp_dim, d_models, w,
                  capacity, device, (hipStream_t)stream, d_corr_offsets, d_total, d_rows, d_entry, d_pts, d_resid);
}

/* The host-pointer forms, arguments checked: match / keep (at output row 0), the keypoint rows of each store (one copy when `same`) and
 * the models go to the device once, the device path runs on the null stream, and corr_offsets, total and the first min(total, capacity)
 * elements of the per-correspondence arrays come back.  No position beyond N exists, so the device arrays hold min(capacity, N). */
static int mx_host(const std::vector<mt_pair_rows> &rows, int64_t n_out, int64_t off1_0, int64_t n1, int64_t off2_0, int64_t n2, bool same,
                   const int32_t *match, const uint8_t *keep, uint32_t flags, const double *kp1, const double *kp2, int kd, const double *models,
                   const mx_what &w, int64_t capacity, int device, int64_t *corr_offsets, int64_t *total, int32_t *out_rows, int32_t *entry, double *pts,
                   double *resid)
{
    const int K = (int)rows.size();
    if (!corr_offsets || !total) return mi_einval("NULL argument: corr_offsets and total are always written");
    if (K == 0) { *total = 0; corr_offsets[0] = 0; return 0; }
    const bool kp = pts || resid;
    if (n_out > 0 && (!match || (capacity > 0 && !out_rows) || (kp && (!kp1 || !kp2)))) return mi_einval("NULL argument");
    MiDevGuard dg; int rc = dg.enter(device); if (rc) return rc;
    const int64_t cap = std::min(capacity, n_out);
    MiStage st;
    const int i_ma = st.in(match, (size_t)n_out * 4), i_ke = st.in(keep, (size_t)n_out), i_k1 = st.in(kp ? kp1 + off1_0 * kd : nullptr, (size_t)n1 * kd * 8),
              i_k2 = same ? i_k1 : st.in(kp ? kp2 + off2_0 * kd : nullptr, (size_t)n2 * kd * 8), i_mo = st.in(resid ? models : nullptr, (size_t)K * 72),
              o_co = st.out(corr_offsets, (size_t)(K + 1) * 8), o_to = st.out(total, 8), o_ro = st.late(out_rows, (size_t)cap * 8),
              o_en = st.late(entry, (size_t)cap * 4), o_pt = st.late(pts, (size_t)cap * 32), o_re = st.late(resid, (size_t)cap * 8);
    rc = st.upload(); if (rc) return rc;
    rc = mx_rows_dev(rows, n_out, st.dev<int32_t>(i_ma), st.dev<uint8_t>(i_ke), flags, off1_0, off2_0, st.dev<double>(i_k1), st.dev<double>(i_k2), kd,
                     st.dev<double>(i_mo), w, cap, device, nullptr, st.dev<int64_t>(o_co), st.dev<int64_t>(o_to), st.dev<int32_t>(o_ro),
                     st.dev<int32_t>(o_en), st.dev<double>(o_pt), st.dev<double>(o_re));
    if (rc) return rc;
    rc = st.finish(); if (rc) return rc;
    const size_t n = (size_t)std::min(*total, cap);
    rc = st.fetch(o_ro, n * 8); if (rc) return rc;
    rc = st.fetch(o_en, n * 4); if (rc) return rc;
    rc = st.fetch(o_pt, n * 32); if (rc) return rc;
    return st.fetch(o_re, n * 8);
}

extern "C" int mi_degensac_correspondences_pairs(const int64_t *offsets1, int n_images1, const int64_t *offsets2, int n_images2, const int32_t *pairs,
                                                 int n_pairs, const int32_t *match, const uint8_t *keep, uint32_t flags, const double *kp1,
                                                 const double *kp2, int kp_dim, const double *models, const mi_degensac_guide_params *gp,
                                                 int64_t capacity, int device, int64_t *corr_offsets, int64_t *total, int32_t *rows, int32_t *entry,
                                                 double *pts, double *resid)
{
    mx_what w; int rc = mx_check_params(flags, kp_dim, pts != nullptr, resid != nullptr, models, gp, capacity, n_pairs, &w); if (rc) return rc;
    std::vector<mt_pair_rows> rw; int64_t n_out = 0, n_back = 0, o1 = 0, o2 = 0, n1 = 0, n2 = 0; bool same = false;
    if (n_pairs > 0) {
        rw.resize(n_pairs);
        rc = mt_pairs_layout(offsets1, n_images1, offsets2, n_images2, pairs, n_pairs, rw.data(), &n_out, &n_back); if (rc) return rc;
        rc = mx_check_store_rows(flags, offsets1[n_images1], offsets2[n_images2]); if (rc) return rc;
        o1 = offsets1[0]; o2 = offsets2[0]; n1 = offsets1[n_images1] - o1; n2 = offsets2[n_images2] - o2;
        same = kp1 == kp2 && n_images1 == n_images2 && !memcmp(offsets1, offsets2, ((size_t)n_images1 + 1) * 8);
    }
    return mx_host(rw, n_out, o1, n1, o2, n2, same, match, keep, flags, kp1, kp2, kp_dim, models, w, capacity, device, corr_offsets, total, rows, entry,
                   pts, resid);
}

extern "C" int mi_degensac_correspondences_batch(const int64_t *offsets1, const int64_t *offsets2, int n_pairs, const int32_t *match, const uint8_t *keep,
                                                 uint32_t flags, const double *kp1, const double *kp2, int kp_dim, const double *models,
                                                 const mi_degensac_guide_params *gp, int64_t capacity, int device, int64_t *corr_offsets, int64_t *total,
                                                 int32_t *rows, int32_t *entry, double *pts, double *resid)
{
    mx_what w; int rc = mx_check_params(flags, kp_dim, pts != nullptr, resid != nullptr, models, gp, capacity, n_pairs, &w); if (rc) return rc;
    std::vector<int64_t> r1, r2; std::vector<mt_pair_rows> rw; int64_t n_out = 0, o1 = 0, o2 = 0, n2 = 0;
    if (n_pairs > 0) {
        rc = mx_check_batch_offsets(offsets1, offsets2, n_pairs); if (rc) return rc;
        rc = mx_check_store_rows(flags, offsets1[n_pairs], offsets2[n_pairs]); if (rc) return rc;
        mt_ragged_rows(offsets1, offsets2, n_pairs, r1, r2, rw);
        n_out = r1[n_pairs]; n2 = r2[n_pairs]; o1 = offsets1[0]; o2 = offsets2[0];
    }
    return mx_host(rw, n_out, o1, n_out, o2, n2, false, match ? match + o1 : nullptr, keep ? keep + o1 : nullptr, flags, kp1, kp2, kp_dim, models, w,
                   capacity, device, corr_offsets, total, rows, entry, pts, resid);
}
