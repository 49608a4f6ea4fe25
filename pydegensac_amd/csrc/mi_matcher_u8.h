/* Tile body of the dense matcher for MI_DEGENSAC_NORM_L2_U8 (included by mi_matcher.hip): exact squared L2 distances between
 * uint8 descriptor rows through the int8 matrix cores.
 *
 * For bytes every term of S = |a|^2 + |b|^2 - 2 a.b is an integer, so S is exact in int32 whatever the accumulation order, and for
 * dim <= 256 it is at most 256 * 255^2 = 16 646 400 < 2^24: exactly representable in fp32 and bit for bit the value the float32
 * path (mt_knn2_tile<0>) accumulates on the same values.  Ranks, ties and ratio decisions are therefore those of the float32 path.
 *
 * Layout.  The bytes are mapped to int8 by x ^ 0x80 = x - 128 on the packed words (a common offset leaves a - b unchanged); padding
 * past the row's end and missing rows are 0 AFTER the xor, so they add nothing to dots and norms.  v_mfma_i32_32x32x32_i8 computes
 * D[i][j] = sum_k A[i][k] B[k][j] with D's column j on the lane (j = lane & 31) and 16 rows in the lane's registers
 * (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  Train rows are the A side and queries the B side, so a query is a lane and its
 * train rows are that lane's accumulator registers: every lane keeps its own running top-2 for one query (per 32-query column block)
 * and no data crosses lanes until the end.  Lane l holds, of A and of B alike, the 16 bytes at 32 s + 16 (l >> 5) of row l & 31 in
 * k-step s; whichever k the hardware gives those 16 bytes, it gives the same to both operands (the two lane maps are mirror images),
 * and a permutation of k applied to both sides does not change the dot product.
 *
 * A workgroup owns 64 queries (two column blocks) whose fragments every wave keeps in registers for the whole tile (dim <= 256:
 * at most 8 k-steps), and streams the train rows 128 at a time, 32 per wave, straight from global memory into A fragments (a train
 * row is used by one wave only, so LDS would add a round trip and no reuse); the next 32 rows are in flight while the current ones
 * are multiplied.  Row norms come from the staged fragments (once per row: each lane squares its 16-byte pieces, the two lane halves
 * add up); the train norms reach the accumulator layout through a 32-entry LDS line per wave.
 *
 * Epilogue, per accumulator register: maximise v = 2 dot - nt (nq is constant on the lane), packed with the register number as
 * key = 16 v + (15 - reg), so that one integer max / min pair per element tracks the tile's top-2 and equal distances keep the
 * lower train row.  No intermediate overflows at dim = 256: |dot| <= 256 * 128^2 = 2^22, nt, nq <= 2^22, |v| <= 2^23 + 2^22,
 * |key| < 2^28; a missing train row carries MU_SKIP = -2^30 instead of -16 nt and a zero dot.  The two winners of a 32-row step
 * are unpacked to (S = nq - v, row) and go through mt_push like every other candidate; the 8 lanes sharing a query (2 halves x 4
 * waves) merge through the `merge` array as in mt_knn2_tile. */
#ifndef MI_MATCHER_U8_H
#define MI_MATCHER_U8_H

typedef int mu_i4 __attribute__((ext_vector_type(4)));
typedef int mu_i16 __attribute__((ext_vector_type(16)));

#define MU_SKIP (-(1 << 30))

/* 16 bytes of a row from word w on, as int8 (x - 128); zero past the row's end and for a missing row (row == null).  vec: rows are
 * whole 16-byte pieces at 16-byte aligned addresses */
__device__ __forceinline__ mu_i4 mu_load(const uint32_t *row, int w, int words, bool vec)
{
    mu_i4 v = {0, 0, 0, 0};
    if (!row) return v;
    if (vec) {
        if (w < words) { const uint4 u = *(const uint4 *)(row + w);
            v[0] = (int)(u.x ^ 0x80808080u); v[1] = (int)(u.y ^ 0x80808080u); v[2] = (int)(u.z ^ 0x80808080u); v[3] = (int)(u.w ^ 0x80808080u); }
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) if (w + c < words) v[c] = (int)(row[w + c] ^ 0x80808080u);
    }
    return v;
}

/* sum of the squares of 16 int8 values (<= 16 * 128^2) */
__device__ __forceinline__ int mu_sq(mu_i4 v)
{
    int s = 0;
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int b = 0; b < 4; b++) { const int x = (int)(int8_t)((uint32_t)v[c] >> (8 * b)); s += x * x; }
    return s;
}

/* mt_knn2_tile for uint8 rows under L2; NS = k-steps of 32 bytes (words <= 8 NS).  ntl: 4 x 32 ints of LDS. */
template <int NS>
__device__ __forceinline__ bool mu_knn2_tile(const uint32_t *q, int q0, int q_end, const uint32_t *t, int t_lo, int t_hi, int t_base, int words,
                                             int *ntl, mt_best (&merge)[MT_Q][16], mt_best &m)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    const bool vec = words % 4 == 0 && ((((uintptr_t)q) | ((uintptr_t)t)) & 15) == 0;
    mu_i4 bq[2][NS]; int nq[2]; mt_best best[2];
#pragma unroll
    for (int cb = 0; cb < 2; cb++) {
        const int qi = q0 + 32 * cb + r;
        const uint32_t *row = qi < q_end ? q + (size_t)qi * words : nullptr;
        int s = 0;
#pragma unroll
        for (int k = 0; k < NS; k++) { bq[cb][k] = mu_load(row, 8 * k + 4 * h, words, vec); s += mu_sq(bq[cb][k]); }
        nq[cb] = s + __shfl_xor(s, 32);
        best[cb].d0 = best[cb].d1 = __builtin_inff(); best[cb].i0 = best[cb].i1 = -1;
    }
    int *nt_w = ntl + 32 * wv;
    mu_i4 a[NS];
    {
        const int ti = t_lo + 32 * wv + r;
        const uint32_t *row = ti < t_hi ? t + (size_t)ti * words : nullptr;
#pragma unroll
        for (int k = 0; k < NS; k++) a[k] = mu_load(row, 8 * k + 4 * h, words, vec);
    }
    for (int t0 = t_lo + 32 * wv; t0 < t_hi; t0 += 128) {                /* wave-uniform */
        mu_i4 an[NS];                                                   /* the wave's next 32 rows, in flight during this step */
        {
            const int ti = t0 + 128 + r;
            const uint32_t *row = ti < t_hi ? t + (size_t)ti * words : nullptr;
#pragma unroll
            for (int k = 0; k < NS; k++) an[k] = mu_load(row, 8 * k + 4 * h, words, vec);
        }
        int s = 0;
#pragma unroll
        for (int k = 0; k < NS; k++) s += mu_sq(a[k]);
        s += __shfl_xor(s, 32);
        if (h == 0) nt_w[r] = t0 + r < t_hi ? -16 * s : MU_SKIP;
        mu_i16 acc0, acc1;
#pragma unroll
        for (int e = 0; e < 16; e++) { acc0[e] = 0; acc1[e] = 0; }
#pragma unroll
        for (int k = 0; k < NS; k++) {
            acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[k], bq[0][k], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[k], bq[1][k], acc1, 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          /* the other lanes' norms are written before they are read */
        __builtin_amdgcn_wave_barrier();
        int k0a = INT32_MIN, k1a = INT32_MIN, k0b = INT32_MIN, k1b = INT32_MIN;      /* top-2 keys of the step, k0 > k1 */
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int c = nt_w[(e & 3) + 8 * (e >> 2) + 4 * h] + (15 - e);
            const int ka = acc0[e] * 32 + c, kb = acc1[e] * 32 + c;
            k1a = max(k1a, min(k0a, ka)); k0a = max(k0a, ka);
            k1b = max(k1b, min(k0b, kb)); k0b = max(k0b, kb);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          /* ... and read before the next step overwrites them */
        __builtin_amdgcn_wave_barrier();
        const int keys[2][2] = {{k0a, k1a}, {k0b, k1b}};
#pragma unroll
        for (int cb = 0; cb < 2; cb++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int key = keys[cb][j];
                if (key > MU_SKIP / 2) {
                    const int e = 15 - (key & 15), v = key >> 4;         /* v = 2 dot - nt; S = nq + nt - 2 dot */
                    mt_push(best[cb], (float)(nq[cb] - v), t0 + (e & 3) + 8 * (e >> 2) + 4 * h - t_base);
                }
            }
#pragma unroll
        for (int k = 0; k < NS; k++) a[k] = an[k];
    }
    /* the 8 lanes of a query (2 halves x 4 waves) merge their candidates (any order: mt_push orders by (d, i)) */
#pragma unroll
    for (int cb = 0; cb < 2; cb++) merge[32 * cb + r][2 * wv + h] = best[cb];
    __syncthreads();
    if (tid >= MT_Q || q0 + tid >= q_end) return false;
    m = merge[tid][0];
    for (int k = 1; k < 8; k++) { const mt_best c = merge[tid][k]; if (c.i0 >= 0) mt_push(m, c.d0, c.i0); if (c.i1 >= 0) mt_push(m, c.d1, c.i1); }
    return true;
}
#endif /* MI_MATCHER_U8_H */
