/* Float descriptors -> the uint8 rows of MI_DEGENSAC_NORM_L2_U8 (include/mi_degensac.h, mi_degensac_desc_quantize*), included at the end
 * of mi_matcher.hip (compiled with -ffp-contract=off; host plumbing: mi_host.h).
 *
 * One row is held by LPR = 64, 32 or 16 lanes of a wave (the smallest that covers its words: 4 columns per lane), so a wave holds
 * 1, 2 or 4 rows and a 256-thread workgroup 4, 8 or 16.  Lane i of a row owns columns 4 i .. 4 i + 3: one float4 load when
 * dim % 4 == 0 and the base is 16-byte aligned, scalar loads otherwise; columns past dim read as 0.  The row sum is the fp64 sum of
 * the header's rule: the lane's own columns in ascending order, then s += s[lane ^ m] for m = 32, 16, 8, 4, 2, 1.  Lanes past the row
 * hold +0.0 and every term is >= 0, so the steps whose partner lies past the row change nothing: running only the steps m < LPR
 * inside the row's LPR lanes gives the same bits as the 64-lane butterfly the header states.  Every lane then forms its four bytes
 * and writes them as one 32-bit word: a row's output, pad bytes included, is one contiguous store.  No LDS, no atomics, no scratch. */
#pragma once
#include <stddef.h>

#define MQ_MAX_GRID 2048       /* workgroups: 8 per CU on 256 CUs; more rows are reached by the grid-stride loop */

struct mq_args { const float *in; uint8_t *out; int32_t *clipped; int64_t n; int dim, normalize, vec4; double scale, offset; };

static int mq_lanes_per_row(int dim) { const int words = (dim + 3) >> 2; return words <= 16 ? 16 : words <= 32 ? 32 : 64; }

template <int LPR>
__global__ __launch_bounds__(256) void mq_quantize_kernel(const mq_args a)
{
    constexpr int RPW = 64 / LPR, RPB = 4 * RPW;               /* rows per wave, per workgroup */
    const int lane = threadIdx.x & 63, sub = lane & (LPR - 1), grp = lane / LPR, wave = threadIdx.x >> 6;
    const int c0 = 4 * sub, words = (a.dim + 3) >> 2;
    const int64_t out_dim = 4 * (int64_t)words;
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < a.n; base += (int64_t)gridDim.x * RPB) {      /* uniform over the workgroup */
        const int64_t row = base + wave * RPW + grp;
        const bool live = row < a.n;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (live && c0 < a.dim) {
            const float *p = a.in + row * a.dim + c0;
            if (a.vec4) { const float4 v = *(const float4 *)p; x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
            else
                for (int j = 0; j < 4; j++) if (c0 + j < a.dim) x[j] = p[j];
        }
        bool bad = false;
        double s = 0.0;
        for (int j = 0; j < 4; j++) {                          /* a column past dim adds +0.0: the same bits as leaving it out */
            bad |= (__float_as_uint(x[j]) & 0x7f800000u) == 0x7f800000u;
            const double xd = (double)x[j];
            s += a.normalize == 1 ? xd * xd : fabs(xd);
        }
        for (int m = LPR / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        const unsigned long long bm = __ballot(bad);
        const bool dead = ((LPR == 64 ? bm : (bm >> (grp * LPR)) & ((1ull << (LPR & 63)) - 1)) != 0) || (a.normalize != 0 && s == 0.0);
        const double r = a.normalize == 1 ? sqrt(s) : s;
        uint32_t w = 0; int nclip = 0;
        for (int j = 0; j < 4; j++) {
            if (c0 + j >= a.dim) break;
            const double xd = (double)x[j];
            const double y = a.normalize == 0 ? xd : a.normalize == 1 ? xd / r : copysign(sqrt(fabs(xd) / r), xd);
            double v = rint(a.scale * y) + a.offset;
            const bool cl = v < 0.0 || v > 255.0;
            v = v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v;
            if (dead) v = a.offset;                            /* before the cast: a NaN never reaches it */
            w |= (uint32_t)(int)v << (8 * j);
            nclip += cl && !dead;
        }
        if (a.clipped) {                                       /* uniform */
            for (int m = LPR / 2; m >= 1; m >>= 1) nclip += __shfl_xor(nclip, m, 64);
            if (live && sub == 0) a.clipped[row] = dead ? -1 : nclip;
        }
        if (live && sub < words) ((uint32_t *)(a.out + row * out_dim))[sub] = w;
    }
}

/* rows one pass of the largest grid covers at this width (the grid-stride loop takes a second step beyond it); 0 for a bad dim */
extern "C" int64_t mi_degensac_desc_quantize_pass_rows(int dim)
{
    if (dim < 1 || dim > MI_DEGENSAC_L2_U8_MAX_DIM) return 0;
    return (int64_t)MQ_MAX_GRID * 4 * (64 / mq_lanes_per_row(dim));
}

#define MQ_REFUSE(msg) return mi_einval(msg)

/* every refusal of the two entry points, before a device is looked for; *empty = the call has nothing to do */
static int mq_check(const mi_degensac_quant_params *qp, const void *in, int64_t n, int dim, const void *out, bool *empty)
{
    *empty = false;
    if (dim < 1 || dim > MI_DEGENSAC_L2_U8_MAX_DIM) MQ_REFUSE("dim should be 1 .. 256 (MI_DEGENSAC_L2_U8_MAX_DIM)");
    if (n < 0) MQ_REFUSE("n < 0");
    if (qp) {
        if (qp->struct_size < (int)(offsetof(mi_degensac_quant_params, offset) + sizeof qp->offset))
            MQ_REFUSE("quant params: struct_size does not cover offset (set it to sizeof(mi_degensac_quant_params))");
        if (qp->normalize < 0 || qp->normalize > 2) MQ_REFUSE("quant params: normalize should be 0 (none), 1 (L2) or 2 (L1-root)");
        if (!(qp->scale > 0.0) || qp->scale > 1.7976931348623157e308) MQ_REFUSE("quant params: scale should be finite and > 0");
        if (qp->offset < 0 || qp->offset > 255) MQ_REFUSE("quant params: offset should be 0 .. 255");
    }
    if (n == 0) { *empty = true; return 0; }
    if (!qp) MQ_REFUSE("quant params are NULL");
    if (!in || !out) MQ_REFUSE("NULL argument");
    return 0;
}

extern "C" int mi_degensac_desc_quantize_dev(const mi_degensac_quant_params *qp, const float *d_desc, int64_t n, int dim, int device, void *stream,
                                             uint8_t *d_out, int32_t *d_clipped_or_null)
{
    bool empty; int rc = mq_check(qp, d_desc, n, dim, d_out, &empty); if (rc || empty) return rc;
    if (((uintptr_t)d_desc & 3) || ((uintptr_t)d_out & 3) || ((uintptr_t)d_clipped_or_null & 3))
        MQ_REFUSE("d_desc, d_out and d_clipped should be 4-byte aligned (the output rows are written as 32-bit words)");
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    const int lpr = mq_lanes_per_row(dim), rpb = 4 * (64 / lpr);
    const int64_t blocks = (n + rpb - 1) / rpb;
    const dim3 grid((unsigned)(blocks < MQ_MAX_GRID ? blocks : MQ_MAX_GRID)), block(256);
    const mq_args a{d_desc, d_out, d_clipped_or_null, n, dim, qp->normalize, (dim % 4 == 0 && ((uintptr_t)d_desc & 15) == 0) ? 1 : 0, qp->scale,
                    (double)qp->offset};
    if (lpr == 16)      hipLaunchKernelGGL(mq_quantize_kernel<16>, grid, block, 0, (hipStream_t)stream, a);
    else if (lpr == 32) hipLaunchKernelGGL(mq_quantize_kernel<32>, grid, block, 0, (hipStream_t)stream, a);
    else                hipLaunchKernelGGL(mq_quantize_kernel<64>, grid, block, 0, (hipStream_t)stream, a);
    MICHK(hipGetLastError());
    return 0;
}

extern "C" int mi_degensac_desc_quantize(const mi_degensac_quant_params *qp, const float *desc, int64_t n, int dim, int device, uint8_t *out,
                                         int32_t *clipped_or_null)
{
    bool empty; int rc = mq_check(qp, desc, n, dim, out, &empty); if (rc || empty) return rc;
    MiDevGuard g; rc = g.enter(device); if (rc) return rc;
    const size_t out_dim = (size_t)((dim + 3) & ~3), bi = (size_t)n * dim * sizeof(float), bo = (size_t)n * out_dim, bc = (size_t)n * sizeof(int32_t);
    float *di = nullptr; uint8_t *dout = nullptr; int32_t *dc = nullptr;
    struct Free { float *&a; uint8_t *&b; int32_t *&c; ~Free() { (void)hipFree(a); (void)hipFree(b); (void)hipFree(c); } } fr{di, dout, dc};
    MICHK(hipMalloc((void **)&di, bi)); MICHK(hipMalloc((void **)&dout, bo));
    if (clipped_or_null) MICHK(hipMalloc((void **)&dc, bc));
    MICHK(hipMemcpy(di, desc, bi, hipMemcpyHostToDevice));
    rc = mi_degensac_desc_quantize_dev(qp, di, n, dim, device, nullptr, dout, dc); if (rc) return rc;
    MICHK(hipDeviceSynchronize());
    MICHK(hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost));
    if (clipped_or_null) MICHK(hipMemcpy(clipped_or_null, dc, bc, hipMemcpyDeviceToHost));
    return 0;
}
