/* Device helpers the stage kernels share: the finite / NaN / infinity spellings of the list stages and the count-and-scan pieces of the two
 * stream compactions (mi_correspond.hip, mi_tracks.hip).  All __forceinline__. */
#ifndef MI_DEV_UTIL_H
#define MI_DEV_UTIL_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define MI_DBL_MAX 1.7976931348623157e308
__device__ __forceinline__ bool mi_finite(double x) { return fabs(x) <= MI_DBL_MAX; }
__device__ __forceinline__ double mi_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double mi_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

/* four flags per thread (bit j of f = this thread's j-th consecutive position): the set flags of the wave's lower lanes, and of the whole wave */
__device__ __forceinline__ void mi_wave_prefix(unsigned f, int lane, int *before, int *total)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    int b = 0, t = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned long long bal = __ballot((f >> j) & 1u);
        b += __popcll(bal & below); t += __popcll(bal);
    }
    *before = b; *total = t;
}

/* the tail of a count kernel of 256 threads: the four wave totals through four LDS words of its own into cnt[blockIdx.x] */
__device__ __forceinline__ void mi_block_count(int total, int32_t *cnt)
{
    __shared__ int wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

/* one workgroup of W threads: base[b] = cnt[0] + .. + cnt[b - 1] for b < nb, W counts per step with a running carry through W / 64 LDS
 * words of its own.  Returns the sum of all counts, in every thread. */
template <int W>
__device__ __forceinline__ int64_t mi_block_scan(const int32_t *cnt, int nb, int32_t *base)
{
    __shared__ int wsum[W / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t carry = 0;
    for (int s = 0; s < nb; s += W) {                                 /* uniform over the workgroup */
        const int i = s + tid;
        const int c = i < nb ? cnt[i] : 0;
        int v = c;
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v += t; }
        if (lane == 63) wsum[wv] = v;
        __syncthreads();
        int wbase = 0, all = 0;
#pragma unroll
        for (int w = 0; w < W / 64; w++) { if (w < wv) wbase += wsum[w]; all += wsum[w]; }
        if (i < nb) base[i] = (int32_t)(carry + wbase + v - c);
        carry += all;
        __syncthreads();
    }
    return carry;
}
#endif /* MI_DEV_UTIL_H */
