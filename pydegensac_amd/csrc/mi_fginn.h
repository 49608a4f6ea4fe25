/* The first-geometrically-inconsistent-neighbour (FGINN) ratio test of the matcher stage (included at the end of mi_matcher.hip;
 * include/mi_degensac.h mi_degensac_match_fginn_knn2_batch_dev / _pairs_dev).  Detectors emit several keypoints for one image structure (two
 * orientations at one location, neighbouring scales a pixel apart) with nearly equal descriptors: the second neighbour of a correct
 * match is then its own twin and `d0 < ratio * d1` fails.  FGINN (Mishkin et al.) takes the second distance from the nearest train
 * row whose KEYPOINT lies at least spatial_th pixels from the nearest neighbour's keypoint.
 *
 * Semantics, per query of one pair (kp2 [n2, kd] float64, only x, y read; r = spatial_th, finite and >= 0):
 *   slot 0  (i0, d0) of the plain 2-NN, unchanged.
 *   a train row t competes for slot 1 iff t != i0 and dx dx + dy dy >= r r with dx = x2[t] - x2[i0], dy = y2[t] - y2[i0], in fp64
 *           in that order without contraction; a NaN makes the comparison false (a NaN anchor leaves no competitor; inf - inf is NaN, inf - finite
 *           squares to inf and competes).
 *   slot 1  the nearest competing row in the matcher's (distance, index) order, its distance from the dense matcher's accumulation;
 *           -1 / inf when nothing competes or i0 = -1.
 * r = 0 with finite keypoints gives the plain 2-NN bit for bit.
 *
 * The work follows the queries that need it.  The plain batched 2-NN runs unchanged.  Rows are found through the list's per-entry
 * records (mt_pair_rows: output rows, query rows in store 1, train rows in store 2; the ragged batch is the identity list).
 * mf_mark_kernel (one workgroup per entry) looks at every query's slot 1: when it competes, or is -1, the query is final; otherwise the
 * query is NEEDY and its OUTPUT row goes to the entry's needy list at a position given by wave ballots in ascending query order (no
 * atomic decides a position), and the entry's needy count is stored on the device.  mf_rescan_kernel runs mt_knn2_tile<NORM, FGM> over
 * tiles of up to 64 needy queries: the anchor read and slot 1 written at the output row, the descriptor row found from it (the same
 * number in a ragged batch, FGM 1; output row + the entry's query base - its output base in a pair list, FGM 2), the exclusion test
 * where a candidate is pushed, the dense tile's own accumulation.  Its grid is the list's full tile table (sized on the host for the
 * worst case, no synchronisation); a workgroup whose tile starts at or beyond the needy count returns at once.  Train splits follow
 * the batch rule; partials, indexed by list position, are merged by mf_merge_kernel in mt_push order.  uint8 rows under L2 take the
 * vector-unit form of the exact integer S (mt_knn2_tile NORM 2), not the matrix-core tile of mi_matcher_u8.h. */
#ifndef MI_FGINN_H
#define MI_FGINN_H

/* one workgroup per list entry: its needy queries, in ascending query order, to list[out ..] as OUTPUT rows; count[p] = their number.
 * rows[p] (mt_pair_rows) replaces the two offset tables of the ragged form: the entry's output rows out .. out + nq, the first row t of
 * its train image in kt */
__global__ __launch_bounds__(256) void mf_mark_kernel(const int32_t *idx, const mt_pair_rows *rows, const double *kt, int kd, double rr, int32_t *list,
                                                      int32_t *count)
{
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lo = rows[p].out, hi = lo + rows[p].nq, b2 = rows[p].t;
    int base = 0;
    for (int i0 = lo; i0 < hi; i0 += 256) {
        const int i = i0 + tid;
        bool needy = false;
        if (i < hi) {
            const int j = idx[2 * i], j2 = idx[2 * i + 1];
            if (j >= 0 && j2 >= 0) {
                const double *a = kt + (size_t)(b2 + j) * kd, *c = kt + (size_t)(b2 + j2) * kd;
                const double dx = c[0] - a[0], dy = c[1] - a[1];
                needy = !(dx * dx + dy * dy >= rr);
            }
        }
        const unsigned long long bal = __ballot(needy);
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();
        int pre = base;
        for (int w = 0; w < wv; w++) pre += wsum[w];
        if (needy) list[lo + pre + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) count[p] = base;
}

/* tiles[2 b] = (first output row of the entry = start of its needy list, first list position of the tile relative to it, first train
 * row of the entry, end of its train rows), tiles[2 b + 1] = (the entry, first row of its query image in q, -, -).  A needy query has
 * TWO rows: its output row (the list's value: the anchor is read and slot 1 written there) and its descriptor row, the entry's query
 * base + (output row - the entry's first output row); only a ragged batch has them equal.  FGM = 1 is the tile body of a ragged batch
 * (one row number, the instantiation from before the pair list: measured, the ragged uint8 call lay above its parent's range when it went
 * through the list's body), FGM = 2 the list's; the host picks FGM 1 when every entry has q == out.  Split y takes the entry's train rows from
 * t_begin + y t_chunk.  With one split the best competing row goes to slot 1 of the query's output row, else the partial goes to
 * part[split][list position]. */
template <int NORM, int FGM>
__global__ __launch_bounds__(256) void mf_rescan_kernel(const uint32_t *q, const uint32_t *t, int words, const int4 *tiles, const int32_t *list,
                                                        const int32_t *count, const double *kt, int kd, double rr, int n_rows, int t_chunk,
                                                        int32_t *idx, float *dist, mt_best *part)
{
    __shared__ mt_best merge[MT_Q][16];
    __shared__ uint32_t qs[MT_DC][MT_Q + 1], ts[MT_DC][MT_T + 1];
    __shared__ mf_lds fl;
    const int4 tl = tiles[2 * blockIdx.x], te = tiles[2 * blockIdx.x + 1];
    const int cnt = count[te.x];
    if (tl.y >= cnt) return;                                          /* uniform over the workgroup */
    const int q0 = tl.x + tl.y, q_end = tl.x + (tl.y + MT_Q < cnt ? tl.y + MT_Q : cnt);
    const int t_lo = tl.z + (int)blockIdx.y * t_chunk, t_hi = t_lo + t_chunk < tl.w ? t_lo + t_chunk : tl.w;
    const mf_ctx fg{list, idx, kt, kd, rr, te.y - tl.x};
    mt_best m;
    if (!mt_knn2_tile<NORM, FGM>(q, q0, q_end, t, t_lo, t_hi, tl.z, words, qs, ts, merge, m, &fg, &fl)) return;
    if (part) { part[(size_t)blockIdx.y * n_rows + q0 + threadIdx.x] = m; return; }
    const size_t o = (size_t)fl.row[threadIdx.x] * 2 + 1;
    idx[o] = m.i0; dist[o] = NORM != 1 ? sqrtf(m.d0) : m.d0;
}

/* one workgroup per list entry: the per-split partials of its needy queries, merged in mt_push order, to slot 1 of their output rows */
__global__ __launch_bounds__(256) void mf_merge_kernel(const mt_best *part, int splits, int n_rows, int l2, const mt_pair_rows *rows, const int32_t *list,
                                                       const int32_t *count, int32_t *idx, float *dist)
{
    const int p = blockIdx.x, lo = rows[p].out, cnt = count[p];
    for (int k = threadIdx.x; k < cnt; k += 256) {
        mt_best m = part[lo + k];
        for (int s = 1; s < splits; s++) { const mt_best c = part[(size_t)s * n_rows + lo + k]; if (c.i0 >= 0) mt_push(m, c.d0, c.i0);
            if (c.i1 >= 0) mt_push(m, c.d1, c.i1); }
        const size_t o = (size_t)list[lo + k] * 2 + 1;
        idx[o] = m.i0; dist[o] = l2 ? sqrtf(m.d0) : m.d0;
    }
}

/* mf_mark_kernel for another stage's result lists (the guided stage, mi_guided.hip, whose slot 1 is judged by the same rule) */
int mt_batch_fginn_mark(const int32_t *idx, const mt_pair_rows *d_rows, int n_pairs, const double *kt, int kd, double rr, hipStream_t s, int32_t *list,
                        int32_t *count)
{
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(mf_mark_kernel, dim3(n_pairs), dim3(256), 0, s, idx, d_rows, kt, kd, rr, list, count);
    MICHK(hipGetLastError());
    return 0;
}

/* slot 1 of idx / dist (the plain batched 2-NN of the same rows, already enqueued on s) becomes the FGINN second neighbour */
int mt_batch_fginn(int norm, int words, const void *dq, const void *dt, const double *kt, int kd, const mt_pair_rows *rows, int n_pairs, int n_rows,
                   double r, int device, hipStream_t s, int32_t *idx, float *dist)
{
    const int K = n_pairs;
    if (n_rows == 0) return 0;
    /* one upload: the entries' rows | two int4 per 64-query tile of every entry */
    const size_t b_rows = ((size_t)K * sizeof(mt_pair_rows) + 15) / 16 * 16;
    std::vector<int32_t> tab(b_rows / 4);
    memcpy(tab.data(), rows, (size_t)K * sizeof(mt_pair_rows));
    int max_n2 = 0;
    bool ident = true;                                                 /* a ragged batch: every entry's queries lie at its output rows */
    for (int p = 0; p < K; p++) {
        const mt_pair_rows &e = rows[p];
        if (e.nt > max_n2) max_n2 = e.nt;
        if (e.q != e.out) ident = false;
        for (int k0 = 0; k0 < e.nq; k0 += MT_Q) { const int32_t tl[8] = {e.out, k0, e.t, e.t + e.nt, p, e.q, 0, 0}; tab.insert(tab.end(), tl, tl + 8); }
    }
    const int qtiles = (int)((tab.size() * 4 - b_rows) / 32);
    int t_chunk, splits; mt_batch_split(qtiles, max_n2, device, &t_chunk, &splits);
    const size_t a_list = mi_up256(tab.size() * 4), a_cnt = a_list + mi_up256((size_t)n_rows * 4), a_part = a_cnt + mi_up256((size_t)K * 4),
                 a_all = a_part + (splits > 1 ? (size_t)splits * n_rows * sizeof(mt_best) : 0);
    MiScratch scr; int rc = scr.alloc(a_all, s); if (rc) return rc;
    char *buf = scr.p;
    rc = mt_batch_upload(device, s, tab.data(), tab.size() * 4, buf); if (rc) return rc;
    const mt_pair_rows *d_rows = (const mt_pair_rows *)buf;
    const int4 *d_tiles = (const int4 *)(buf + b_rows);
    int32_t *list = (int32_t *)(buf + a_list), *cnt = (int32_t *)(buf + a_cnt);
    mt_best *part = splits > 1 ? (mt_best *)(buf + a_part) : nullptr;
    const double rr = r * r;
    hipLaunchKernelGGL(mf_mark_kernel, dim3(K), dim3(256), 0, s, idx, d_rows, kt, kd, rr, list, cnt);
    MICHK(hipGetLastError());
    const dim3 grid(qtiles, splits), block(256);
#define MF_RESCAN(N) do { if (ident) MF_RESCAN_(N, 1); else MF_RESCAN_(N, 2); } while (0)
#define MF_RESCAN_(N, M) hipLaunchKernelGGL((mf_rescan_kernel<N, M>), grid, block, 0, s, (const uint32_t *)dq, (const uint32_t *)dt, words, d_tiles, list, \
        cnt, kt, kd, rr, n_rows, t_chunk, idx, dist, part)
    if (norm == MI_DEGENSAC_NORM_L2) MF_RESCAN(0); else if (norm == MI_DEGENSAC_NORM_HAMMING) MF_RESCAN(1); else MF_RESCAN(2);
#undef MF_RESCAN
#undef MF_RESCAN_
    MICHK(hipGetLastError());
    if (part) {
        hipLaunchKernelGGL(mf_merge_kernel, dim3(K), dim3(256), 0, s, part, splits, n_rows, norm != MI_DEGENSAC_NORM_HAMMING ? 1 : 0, d_rows, list, cnt, idx,
            dist);
        MICHK(hipGetLastError());
    }
    return 0;
}

/* the checks the two 2-NN + FGINN entry points share beyond their layouts */
static int mf_check(int norm, int dim, int n_pairs, int kp_dim, double spatial_th)
{
    if (n_pairs < 0) return mi_einval("bad argument");
    int rc = mt_check_norm(norm, dim); if (rc) return rc;
    if (kp_dim != 2 && kp_dim != 6) return mi_einval("keypoint rows must be [n,2] or [n,6]");
    if (const char *e = mt_spatial_th_error(spatial_th)) return mi_einval(e);
    return 0;
}

extern "C" int mi_degensac_match_fginn_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                      const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp2, int kp_dim,
                                                      double spatial_th, int device, void *stream, int32_t *d_idx, float *d_dist)
{
    int rc = mf_check(norm, dim, n_pairs, kp_dim, spatial_th); if (rc) return rc;
    const int words = mt_row_words(norm, dim);
    if (n_pairs == 0) return 0;
    if (!mt_check_offsets(offsets1_host, n_pairs) || !mt_check_offsets(offsets2_host, n_pairs)) return mi_einval("offsets must be non-negative and non-decreasing");
    const int64_t n1 = offsets1_host[n_pairs] - offsets1_host[0], n2 = offsets2_host[n_pairs] - offsets2_host[0];
    if ((n1 > 0 && (!d_desc1 || !d_idx || !d_dist)) || (n2 > 0 && (!d_desc2 || !d_kp2))) return mi_einval("NULL argument");
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    std::vector<int64_t> o1, o2; std::vector<mt_pair_rows> rows;
    mt_ragged_rows(offsets1_host, offsets2_host, n_pairs, o1, o2, rows);
    const uint32_t *q1 = (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words, *q2 = (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words;
    int32_t *idx = d_idx + 2 * offsets1_host[0]; float *dist = d_dist + 2 * offsets1_host[0];
    rc = mt_batch_knn2(norm, words, q1, q2, rows.data(), n_pairs, (int)n1, 0, device, (hipStream_t)stream, idx, dist); if (rc) return rc;
    return mt_batch_fginn(norm, words, q1, q2, d_kp2 + (size_t)offsets2_host[0] * kp_dim, kp_dim, rows.data(), n_pairs, (int)n1, spatial_th, device,
                          (hipStream_t)stream, idx, dist);
}

/* the same over a pair list: mt_pairs_layout fills the rows the ragged form takes from its own offsets, everything after that is shared */
extern "C" int mi_degensac_match_fginn_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                                                      const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim,
                                                      const double *d_kp2, int kp_dim, double spatial_th, int device, void *stream, int32_t *d_idx,
                                                      float *d_dist)
{
    int rc = mf_check(norm, dim, n_pairs, kp_dim, spatial_th); if (rc) return rc;
    const int words = mt_row_words(norm, dim);
    if (n_pairs == 0) return 0;
    std::vector<mt_pair_rows> rows(n_pairs);
    int64_t n_out, n_back;
    rc = mt_pairs_layout(offsets1_host, n_images1, offsets2_host, n_images2, pairs_host, n_pairs, rows.data(), &n_out, &n_back); if (rc) return rc;
    if ((n_out > 0 && (!d_desc1 || !d_idx || !d_dist)) || (n_out > 0 && n_back > 0 && (!d_desc2 || !d_kp2))) return mi_einval("NULL argument");
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    const uint32_t *q1 = (const uint32_t *)d_desc1 + (size_t)offsets1_host[0] * words, *q2 = (const uint32_t *)d_desc2 + (size_t)offsets2_host[0] * words;
    rc = mt_batch_knn2(norm, words, q1, q2, rows.data(), n_pairs, (int)n_out, 0, device, (hipStream_t)stream, d_idx, d_dist); if (rc) return rc;
    return mt_batch_fginn(norm, words, q1, q2, d_kp2 + (size_t)offsets2_host[0] * kp_dim, kp_dim, rows.data(), n_pairs, (int)n_out, spatial_th, device,
                          (hipStream_t)stream, d_idx, d_dist);
}
#endif /* MI_FGINN_H */
