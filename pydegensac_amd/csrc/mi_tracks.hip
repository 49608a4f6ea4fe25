/* libmi_degensac.so — tracks: the connected components of exported matches over one image store (include/mi_degensac.h
 * mi_degensac_tracks_*).  The input is the edge list the correspondence export writes with MI_DEGENSAC_CORR_STORE_ROWS (rows [M, 2] of
 * store rows and its device total); node k is store row offsets[0] + k.  gfx950 only, no CPU path.
 *
 * Passes, each its own launch on the caller's stream (the launch boundaries are the only ordering between them):
 *   init      parent[k] = k, multi[k] = 0;
 *   link      one thread per edge (grid-stride over min(total, M), read on the device): both ends are chased to a root, the larger root
 *             is hooked under the smaller with atomicCAS(&parent[hi], hi, lo), and a failed CAS continues from the value it returned
 *             (the ECL-CC / Afforest link).  parent[x] <= x holds throughout and a word changes at most once, from x to a smaller node
 *             of the same component (no path shortening: a shortening store could put back a larger ancestor and would break the
 *             monotone argument below for a chase that the tracks of a collection keep short anyway).  The smallest node of a component
 *             can never be hooked, so it ends as the root of the whole component whatever the schedule;
 *   compress  label[k] = the root of k, a read-only chase; multi[label[k]] = 1 where label[k] != k (a same-value byte store);
 *   keys      key[k] = label[k] if k is in a track (label[k] != k or multi[k]) else R, value[k] = k;
 *   sort      rocprim::radix_sort_pairs over bits(R) key bits: stable, so the values come out track after track in ascending label order and
 *             ascending inside a track, the nodes without a track behind them;
 *   count / scan / write   the pattern of mi_correspond.hip over the sorted keys: a position whose key is < R and differs from its
 *             predecessor's starts a track; TK_ROWS = 1024 positions per workgroup counted with wave ballots, one workgroup scans the
 *             counts (TK_SCAN per step) and writes n_tracks and n_obs (the lower bound of R in the sorted keys); the write pass gives
 *             track[node], obs, obs_image (a binary search in the device copy of the offsets), track_offsets and every tail fill;
 *   images    track_images: one position per thread, an observation counts when it starts a track or its image differs from its
 *             predecessor's; the counts of the wave's lanes of one track are summed with two ballots and added by the track's first lane
 *             in the wave with one integer atomicAdd on the zeroed array (integer sums do not depend on their order).
 *
 * Why nothing here can hang.  No loop's exit depends on a store by another workgroup: there are no flags, no tickets and no pass that is
 * launched again until nothing changes.  A chase follows strictly decreasing values (it stops at the first p >= x, which under the
 * invariant is p == x), so it ends after at most x steps whatever it reads; it reads parent with relaxed agent-scope loads, and even a
 * stale value would be x itself, which the CAS then refuses.  The CAS retry: a CAS on parent[hi] fails only because another thread hooked
 * hi, and it returns that smaller value; the next round starts from it and from lo, both below hi, so max(x, y) falls strictly with
 * every retry of one edge: at most hi retries without any help from others, and over all threads every failure stands for a parent word
 * that strictly decreased, so the sum of all parent values bounds the retries of the whole launch.
 * Edge ends outside [offsets[0], offsets[n_images]) are compared before they are used as an index and the edge is dropped. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"
#include "mi_host.h"
#include "mi_dev_util.h"

#define TK_ROWS 1024              /* sorted positions per workgroup: 256 threads x 4 consecutive positions */
#define TK_SCAN 256               /* workgroup counts per step of the scan */
#define TK_LINK_BLOCKS 2048       /* cap on the link grid (256 threads each, grid-stride beyond) */

__global__ __launch_bounds__(256) void tk_init_kernel(int32_t *parent, uint8_t *multi, int R)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < R) { parent[k] = (int32_t)k; multi[k] = 0; }
}

__device__ __forceinline__ int tk_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

/* the root above x as far as this thread can see; strictly decreasing, so at most x steps */
__device__ __forceinline__ int tk_chase(const int32_t *parent, int x)
{
    for (;;) { const int p = tk_load(parent + x); if (p >= x) return x; x = p; }
}

__global__ __launch_bounds__(256) void tk_link_kernel(const int32_t *rows, int64_t M, const int64_t *total, int vec, int64_t first, int R, int32_t *parent)
{
    int64_t n = M;
    if (total) { const int64_t t = *total; n = t < 0 ? 0 : t < M ? t : M; }
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        int a, b;
        if (vec) { const int2 v = reinterpret_cast<const int2 *>(rows)[e]; a = v.x; b = v.y; }
        else { a = rows[2 * e]; b = rows[2 * e + 1]; }
        const int64_t da = (int64_t)a - first, db = (int64_t)b - first;
        if (da < 0 || da >= R || db < 0 || db >= R || da == db) continue;
        int x = (int)da, y = (int)db;
        for (;;) {
            x = tk_chase(parent, x); y = tk_chase(parent, y);
            if (x == y) break;
            const int hi = x > y ? x : y, lo = x > y ? y : x;
            const int old = atomicCAS(parent + hi, hi, lo);
            if (old >= hi) break;                                    /* == hi: hooked (a value above hi never stands there) */
            x = old; y = lo;                                         /* both < hi */
        }
    }
}

__global__ __launch_bounds__(256) void tk_compress_kernel(const int32_t *parent, int R, int32_t *label, uint8_t *multi)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= R) return;
    int x = (int)k;
    for (;;) { const int p = parent[x]; if (p >= x) break; x = p; }
    label[k] = x;
    if (x != (int)k) multi[x] = 1;
}

__global__ __launch_bounds__(256) void tk_keys_kernel(const int32_t *label, const uint8_t *multi, int R, uint32_t *key, int32_t *val)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= R) return;
    const int l = label[k];
    key[k] = (l != (int)k || multi[k]) ? (uint32_t)l : (uint32_t)R;
    val[k] = (int32_t)k;
}

/* the four sorted positions i0 .. i0 + 3 of one thread: k[j] = their keys (R beyond the end), bit j of the result = position i0 + j
 * starts a track */
__device__ __forceinline__ unsigned tk_starts(const uint32_t *key, int64_t i0, int R, uint32_t (&k)[4])
{
    uint32_t prev = (uint32_t)R;
    if (i0 > 0 && i0 <= R) prev = key[i0 - 1];
    unsigned f = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        k[j] = i0 + j < R ? key[i0 + j] : (uint32_t)R;
        if (k[j] < (uint32_t)R && (i0 + j == 0 || k[j] != prev)) f |= 1u << j;
        prev = k[j];
    }
    return f;
}

__global__ __launch_bounds__(256) void tk_count_kernel(const uint32_t *key, int R, int32_t *cnt)
{
    uint32_t k[4];
    const unsigned f = tk_starts(key, (int64_t)blockIdx.x * TK_ROWS + (int64_t)threadIdx.x * 4, R, k);
    int before, total;
    mi_wave_prefix(f, threadIdx.x & 63, &before, &total);
    mi_block_count(total, cnt);
}

/* one workgroup: base[b] = the track starts before workgroup b, *n_tracks, and *n_obs = the sorted keys below R */
__global__ __launch_bounds__(TK_SCAN) void tk_scan_kernel(const int32_t *cnt, int nb, int32_t *base, const uint32_t *key, int R, int64_t *n_tracks,
                                                          int64_t *n_obs)
{
    const int64_t carry = mi_block_scan<TK_SCAN>(cnt, nb, base);
    if (threadIdx.x == 0) {
        *n_tracks = carry;
        int64_t lo = 0, hi = R;                                       /* the first position whose key is R */
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] < (uint32_t)R) lo = mid + 1; else hi = mid; }
        *n_obs = lo;
    }
}

/* the image of node k: the last i < n_images with rel[i] <= k (rel = the offsets minus offsets[0]), which skips empty images */
__device__ __forceinline__ int tk_image(const int32_t *rel, int n_images, int k)
{
    int lo = 0, hi = n_images - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (rel[mid] <= k) lo = mid; else hi = mid - 1; }
    return lo;
}

struct tk_out {
    int32_t *track; int64_t *track_offsets; int32_t *obs, *obs_image, *track_images;
    const int64_t *n_tracks, *n_obs;
};

__global__ __launch_bounds__(256) void tk_write_kernel(const uint32_t *key, const int32_t *val, const int32_t *base, int R, int32_t first,
                                                       const int32_t *rel, int n_images, tk_out o)
{
    __shared__ int wsum[4];
    uint32_t k[4];
    const int64_t i0 = (int64_t)blockIdx.x * TK_ROWS + (int64_t)threadIdx.x * 4;
    const unsigned f = tk_starts(key, i0, R, k);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int before, total;
    mi_wave_prefix(f, lane, &before, &total);
    if (lane == 0) wsum[wv] = total;
    __syncthreads();
    int t = base[blockIdx.x] + before;                                /* the track starts before this thread's first position */
#pragma unroll
    for (int w = 0; w < 4; w++) if (w < wv) t += wsum[w];
    const int64_t nt = *o.n_tracks, no = *o.n_obs, half = R / 2;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t i = i0 + j;
        if (i >= R) break;
        if ((f >> j) & 1u) o.track_offsets[t++] = i;                 /* from here on t - 1 is this position's track */
        const int node = val[i];                                     /* 0 <= node < R: the sort permutes 0 .. R - 1 */
        const bool in = k[j] < (uint32_t)R;
        o.track[node] = in ? t - 1 : -1;
        if (o.obs) o.obs[i] = in ? first + node : -1;
        if (o.obs_image) o.obs_image[i] = in ? tk_image(rel, n_images, node) : -1;
        /* the tails: positions 0 .. R/2 cover track_offsets [R/2 + 1] and track_images [R/2] */
        if (i <= half && i >= nt) o.track_offsets[i] = no;
        if (o.track_images && i < half) o.track_images[i] = i < nt ? 0 : -1;
    }
}

/* track_images[t] += the observations of t in this wave that start the track or lie in another image than their predecessor */
__global__ __launch_bounds__(256) void tk_images_kernel(const uint32_t *key, const int32_t *val, int R, const int32_t *rel, int n_images,
                                                        const int64_t *n_obs, const int32_t *track, int32_t *track_images)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < *n_obs;
    const int node = in ? val[i] : 0;
    const uint32_t k = in ? key[i] : (uint32_t)R;
    const int img = in ? tk_image(rel, n_images, node) : -1;
    uint32_t pk = (uint32_t)__shfl_up((int)k, 1);
    int pimg = __shfl_up(img, 1);
    if (lane == 0 && in && i > 0) { pk = key[i - 1]; pimg = tk_image(rel, n_images, val[i - 1]); }
    const bool start = in && (i == 0 || k != pk);
    const bool flag = in && (start || img != pimg);
    const bool head = in && (start || lane == 0);
    const unsigned long long S = __ballot(head), F = __ballot(flag);
    if (!head) return;
    const unsigned long long above = lane == 63 ? 0ull : (S >> (lane + 1)) << (lane + 1);
    const int end = above ? __ffsll((long long)above) - 1 : 64;     /* the next head in the wave */
    const unsigned long long upto = end == 64 ? ~0ull : (1ull << end) - 1ull;
    const int c = __popcll(F & upto & ~((1ull << lane) - 1ull));
    if (c) atomicAdd(track_images + track[node], c);
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
extern "C" int mi_degensac_tracks_tile(int which) { return which == 0 ? TK_ROWS : which == 1 ? TK_SCAN : -1; }

/* the refusals of include/mi_degensac.h, in that order; needs no device */
static int tk_check(const int64_t *offsets, int n_images, const int32_t *rows, int64_t n_edges, const void *track, const void *n_tracks,
                    const void *n_obs, const void *track_offsets, const void *obs, const void *obs_image, const void *track_images)
{
    if (n_images < 0) return mi_einval("n_images < 0");
    if (!offsets) return mi_einval("NULL argument: offsets");
    if (offsets[0] < 0) return mi_einval("offsets must be non-decreasing and start at >= 0");
    for (int i = 0; i < n_images; i++) if (offsets[i + 1] < offsets[i]) return mi_einval("offsets must be non-decreasing and start at >= 0");
    if (offsets[n_images] > 0x7fffffff) return mi_einval("the store's rows do not fit int32 (offsets beyond 0x7fffffff)");
    if (n_edges < 0 || n_edges > 0x3fffffff) return mi_einval("n_edges must lie in 0 .. 0x3fffffff");
    if (!rows && n_edges > 0) return mi_einval("NULL argument: rows of a list that is not empty");
    if (!track || !n_tracks || !n_obs || !track_offsets) return mi_einval("NULL argument: track, n_tracks, n_obs and track_offsets are always written");
    if ((obs_image || track_images) && !obs) return mi_einval("obs_image and track_images need obs");
    if (((uintptr_t)rows) & 3u) return mi_einval("rows must be 4-byte aligned");
    return 0;
}

/* the device path, arguments checked and the device current */
static int tk_run(const int64_t *offsets, int n_images, const int32_t *d_rows, int64_t n_edges, const int64_t *d_total, int device, hipStream_t s,
                  int32_t *d_label, int32_t *d_track, int64_t *d_n_tracks, int64_t *d_n_obs, int64_t *d_track_offsets, int32_t *d_obs,
                  int32_t *d_obs_image, int32_t *d_track_images)
{
    const int64_t first = offsets[0];
    const int R = (int)(offsets[n_images] - first);
    if (R == 0) {                                                    /* no node: zero tracks, track_offsets [1] = 0 */
        MICHK(hipMemsetAsync(d_n_tracks, 0, 8, s));
        MICHK(hipMemsetAsync(d_n_obs, 0, 8, s));
        MICHK(hipMemsetAsync(d_track_offsets, 0, 8, s));
        return 0;
    }
    const int nb = (int)(((int64_t)R + TK_ROWS - 1) / TK_ROWS), g256 = (int)(((int64_t)R + 255) / 256);
    unsigned bits = 1;
    while (((uint32_t)R >> bits) != 0) bits++;                       /* the keys are <= R */
    size_t sort_bytes = 0;
    MICHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (unsigned)R,
                                    0u, bits, s));
    std::vector<int32_t> rel((size_t)n_images + 1);
    for (int i = 0; i <= n_images; i++) rel[i] = (int32_t)(offsets[i] - first);
    const size_t w = mi_up256((size_t)R * 4);
    const size_t a_par = mi_up256(rel.size() * 4), a_lab = a_par + w, a_mul = a_lab + (d_label ? 0 : w), a_k0 = a_mul + mi_up256((size_t)R), a_k1 = a_k0 + w,
                 a_v0 = a_k1 + w, a_v1 = a_v0 + w, a_cnt = a_v1 + w, a_base = a_cnt + mi_up256((size_t)nb * 4), a_sort = a_base + mi_up256((size_t)nb * 4),
                 a_all = a_sort + mi_up256(sort_bytes);
    MiScratch scr; int rc = scr.alloc(a_all, s); if (rc) return rc;
    char *blk = scr.p;
    rc = mt_batch_upload(device, s, rel.data(), rel.size() * 4, blk); if (rc) return rc;
    const int32_t *d_rel = (const int32_t *)blk;
    int32_t *parent = (int32_t *)(blk + a_par), *label = d_label ? d_label : (int32_t *)(blk + a_lab);
    uint8_t *multi = (uint8_t *)(blk + a_mul);
    uint32_t *k0 = (uint32_t *)(blk + a_k0), *k1 = (uint32_t *)(blk + a_k1);
    int32_t *v0 = (int32_t *)(blk + a_v0), *v1 = (int32_t *)(blk + a_v1), *cnt = (int32_t *)(blk + a_cnt), *base = (int32_t *)(blk + a_base);

    hipLaunchKernelGGL(tk_init_kernel, dim3(g256), dim3(256), 0, s, parent, multi, R);
    MICHK(hipGetLastError());
    if (n_edges > 0) {
        const int lb = (int)std::min<int64_t>((n_edges + 255) / 256, TK_LINK_BLOCKS);
        hipLaunchKernelGGL(tk_link_kernel, dim3(lb), dim3(256), 0, s, d_rows, n_edges, d_total, (((uintptr_t)d_rows) & 7u) == 0 ? 1 : 0, first, R, parent);
        MICHK(hipGetLastError());
    }
    hipLaunchKernelGGL(tk_compress_kernel, dim3(g256), dim3(256), 0, s, (const int32_t *)parent, R, label, multi);
    MICHK(hipGetLastError());
    hipLaunchKernelGGL(tk_keys_kernel, dim3(g256), dim3(256), 0, s, (const int32_t *)label, (const uint8_t *)multi, R, k0, v0);
    MICHK(hipGetLastError());
    MICHK(rocprim::radix_sort_pairs((void *)(blk + a_sort), sort_bytes, k0, k1, v0, v1, (unsigned)R, 0u, bits, s));
    hipLaunchKernelGGL(tk_count_kernel, dim3(nb), dim3(256), 0, s, (const uint32_t *)k1, R, cnt);
    MICHK(hipGetLastError());
    hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(TK_SCAN), 0, s, (const int32_t *)cnt, nb, base, (const uint32_t *)k1, R, d_n_tracks, d_n_obs);
    MICHK(hipGetLastError());
    tk_out o{d_track, d_track_offsets, d_obs, d_obs_image, d_track_images, d_n_tracks, d_n_obs};
    hipLaunchKernelGGL(tk_write_kernel, dim3(nb), dim3(256), 0, s, (const uint32_t *)k1, (const int32_t *)v1, (const int32_t *)base, R, (int32_t)first,
                       d_rel, n_images, o);
    MICHK(hipGetLastError());
    if (d_track_images) {
        hipLaunchKernelGGL(tk_images_kernel, dim3(g256), dim3(256), 0, s, (const uint32_t *)k1, (const int32_t *)v1, R, d_rel, n_images,
                           (const int64_t *)d_n_obs, (const int32_t *)d_track, d_track_images);
        MICHK(hipGetLastError());
    }
    return 0;
}

extern "C" int mi_degensac_tracks_dev(const int64_t *offsets_host, int n_images, const int32_t *d_rows, int64_t n_edges, const int64_t *d_total, int device,
                                      void *stream, int32_t *d_label, int32_t *d_track, int64_t *d_n_tracks, int64_t *d_n_obs, int64_t *d_track_offsets,
                                      int32_t *d_obs, int32_t *d_obs_image, int32_t *d_track_images)
{
    int rc = tk_check(offsets_host, n_images, d_rows, n_edges, d_track, d_n_tracks, d_n_obs, d_track_offsets, d_obs, d_obs_image, d_track_images);
    if (rc) return rc;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    return tk_run(offsets_host, n_images, d_rows, n_edges, d_total, device, (hipStream_t)stream, d_label, d_track, d_n_tracks, d_n_obs, d_track_offsets,
                  d_obs, d_obs_image, d_track_images);
}

extern "C" int mi_degensac_tracks(const int64_t *offsets, int n_images, const int32_t *rows, int64_t n_edges, int64_t total, int device, int32_t *label,
                                  int32_t *track, int64_t *n_tracks, int64_t *n_obs, int64_t *track_offsets, int32_t *obs, int32_t *obs_image,
                                  int32_t *track_images)
{
    int rc = tk_check(offsets, n_images, rows, n_edges, track, n_tracks, n_obs, track_offsets, obs, obs_image, track_images); if (rc) return rc;
    MiDevGuard dg; rc = dg.enter(device); if (rc) return rc;
    const size_t R = (size_t)(offsets[n_images] - offsets[0]), half = R / 2;
    MiStage st;
    const int i_rows = st.in(rows, (size_t)n_edges * 8), i_tot = st.in(total >= 0 ? &total : nullptr, 8), o_nt = st.out(n_tracks, 8), o_no = st.out(n_obs, 8),
              o_to = st.out(track_offsets, (half + 1) * 8), o_lab = st.out(label, R * 4), o_trk = st.out(track, R * 4), o_obs = st.out(obs, R * 4),
              o_oi = st.out(obs_image, R * 4), o_ti = st.out(track_images, half * 4);
    rc = st.upload(); if (rc) return rc;
    rc = tk_run(offsets, n_images, st.dev<int32_t>(i_rows), n_edges, st.dev<int64_t>(i_tot), device, nullptr, st.dev<int32_t>(o_lab), st.dev<int32_t>(o_trk),
                st.dev<int64_t>(o_nt), st.dev<int64_t>(o_no), st.dev<int64_t>(o_to), st.dev<int32_t>(o_obs), st.dev<int32_t>(o_oi), st.dev<int32_t>(o_ti));
    if (rc) return rc;
    return st.finish();
}
