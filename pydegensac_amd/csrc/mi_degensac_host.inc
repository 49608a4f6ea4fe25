/* Host side of the C-ABI (include/mi_degensac.h): per-device state, contexts, the per-(device, stream)
 * scratch cache and the batch launch.  Included by mi_degensac.hip after the device headers. */
#include <math.h>
#include "mi_estimator.h"

static thread_local char g_err[512] = "";
void est_set_error(const char *fmt, const char *a, const char *b) { snprintf(g_err, sizeof g_err, fmt, a, b); }

extern "C" const char *mi_degensac_last_error(void) { return g_err; }
extern "C" const char *mi_degensac_version(void) { return "mi_degensac 0.2 (gfx950)"; }
extern "C" const char *mi_degensac_kernel_name(int homography) { return homography ? "dg_find_homography_kernel" : "dg_find_fundamental_kernel"; }
extern "C" int mi_degensac_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }

/* ---- per-device state: RNG tables uploaded once, device limits, the LDS exchange-order self-check ---- */
struct DevState { bool init = false; int max_lds = 0, cus = 0, pool_par_ok = 0;
                  int static_lds[3][2] = {{0, 0}, {0, 0}, {0, 0}};   /* [variant: 0 = 512 threads, 1 = 256, 2 = 128][F, H] */ };
static const int g_variant_threads[3] = {512, 256, 128};
typedef hipError_t (*dg_resident_fn)(int, int, size_t, int *);
typedef hipError_t (*dg_launch_fn)(int, int, int, size_t, hipStream_t, const dg_args &);
static const dg_resident_fn g_variant_resident[3] = {dg_variant_512_resident, dg_variant_256_resident, dg_variant_128_resident};
static const dg_launch_fn   g_variant_launch[3]   = {dg_variant_512_launch, dg_variant_256_launch, dg_variant_128_launch};
static DevState g_dev[64];
static std::mutex g_mu;                      /* guards g_dev[] initialisation (taken once per call, released before any launch) */
static std::mutex g_dev_mu[64];              /* per device: its scratch cache and the enqueue of a launch that uses it */
/* environment overrides of the automatic choices, read ONCE (development aid; the per-call knob is params.tuning) */
static uint32_t g_env_tuning = 0;

/* T[j][p] = ring word p after srandom's 310 discarded steps when the initial ring is the unit vector e_j (dg_srand_wave) */
static void rng_state_table(unsigned T[31][32])
{
    for (int j = 0; j < 31; j++) {
        unsigned r[31]; for (int i = 0; i < 31; i++) r[i] = (i == j);
        int f = 3, b = 0;
        for (int t = 0; t < 310; t++) { r[f] += r[b]; if (++f >= 31) f = 0; if (++b >= 31) b = 0; }
        for (int p = 0; p < 31; p++) T[j][p] = r[p];
        T[j][31] = 0;
    }
}
static void rng_tables(unsigned C[8][32], unsigned G[32])
{
    /* C[k][j] = raw (pre-shift) k-th output after srandom's 310 discards when the initial state is
     * the unit vector e_j: the additive-feedback recurrence is linear over Z/2^32. */
    for (int j = 0; j < 31; j++) {
        unsigned r[31]; for (int i = 0; i < 31; i++) r[i] = (i == j);
        int f = 3, b = 0;
        for (int t = 0; t < 310 + 8; t++) {
            r[f] += r[b];
            if (t >= 310) C[t - 310][j] = r[f];
            if (++f >= 31) f = 0; if (++b >= 31) b = 0;
        }
    }
    for (int k = 0; k < 8; k++) C[k][31] = 0;
    unsigned long long g = 1;
    for (int j = 0; j < 32; j++) { G[j] = (unsigned)g; g = (g * 16807ull) % 2147483647ull; }
}

/* Self-check behind the parallel pool-swap stage (dg_sample_pool_par): when several lanes of ONE LDS atomic exchange
 * hit the same address, the stage needs them served in ascending lane order (each lane must get its predecessor's
 * value).  The ISA manual does not promise that, so the device is probed once at initialisation — many-to-one patterns
 * with 1..64 lanes per address — and any violation switches every launch to the sequential stage. */
__global__ void dg_exchange_order_kernel(int reps, long long *out)
{
    __shared__ int tab[64];
    const int lane = threadIdx.x; long long bad = 0, tot = 0;
    for (int rep = 0; rep < reps; rep++) {
        for (int K = 1; K <= 64; K = (K < 8 ? K + 1 : K * 2)) {
            tab[lane] = 0;
            DG_WSYNC();
            const int addr = (lane * 7 + rep) % K;
            const int old = __hip_atomic_exchange(&tab[addr], lane + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            int expect = 0;                       /* the nearest lower lane with the same address, else the initial 0 */
            for (int l2 = 0; l2 < lane; l2++) if ((l2 * 7 + rep) % K == addr) expect = l2 + 1;
            bad += (old != expect); tot++;
            DG_WSYNC();
        }
    }
    for (int o = 32; o >= 1; o >>= 1) { bad += __shfl_xor(bad, o, 64); tot += __shfl_xor(tot, o, 64); }
    if (lane == 0) { out[0] = bad; out[1] = tot; }
}

static int exchange_order_probe(int reps, long long out[2])
{
    long long *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, 16));
    hipLaunchKernelGGL(dg_exchange_order_kernel, dim3(1), dim3(64), 0, 0, reps, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d, 16, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(e);
    return 0;
}

/* needs the device current (DevGuard) */
static int dev_init(int device)
{
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); set_err("no HIP device: this library has no CPU path");
        return MI_DEGENSAC_ENODEV; }
    if (device >= ndev) { set_err("device index out of range"); return MI_DEGENSAC_ENODEV; }
    std::lock_guard<std::mutex> lk(g_mu);
    DevState &d = g_dev[device];
    if (!d.init) {
        hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_err("device is %s, this build targets gfx950 only", prop.gcnArchName); return MI_DEGENSAC_ENODEV;
            }
        unsigned C[8][32], G[32], Ct[32][8]; rng_tables(C, G);
        static unsigned T[31][32]; rng_state_table(T);
        for (int j = 0; j < 32; j++) for (int k = 0; k < 8; k++) Ct[j][k] = C[k][j];
        d.max_lds = (int)prop.sharedMemPerBlock; d.cus = prop.multiProcessorCount;
        HIPCHK(dg_variant_512_init(C, Ct, G, T, d.max_lds, d.static_lds[0]));
        HIPCHK(dg_variant_256_init(C, Ct, G, T, d.max_lds, d.static_lds[1]));
        HIPCHK(dg_variant_128_init(C, Ct, G, T, d.max_lds, d.static_lds[2]));
        long long pr[2] = {1, 0};
        int rc = exchange_order_probe(64, pr); if (rc) return rc;
        d.pool_par_ok = (pr[0] == 0 && pr[1] > 0) ? 1 : 0;
        static bool env_read = false;
        if (!env_read) {
            env_read = true;
            if (const char *e = getenv("MI_DEGENSAC_TUNING")) g_env_tuning = (uint32_t)strtoul(e, nullptr, 0);
        }
        d.init = true;
    }
    return 0;
}

extern "C" int mi_degensac_pool_stage_parallel(int device)
{
    DevGuard g; int rc = g.enter(device); if (rc) return rc;
    rc = dev_init(device); if (rc) return rc;
    return g_dev[device].pool_par_ok;
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
#define DG_HDR_BYTES 1024        /* scratch header: ticket, spare counter, 2 x 2 queue counters, one 128-byte line each */

static dg_ws_layout make_layout(int n_max, bool pts_in_ws, int nw, int coop_k, size_t park_bytes, bool hrep)
{
    dg_ws_layout w; memset(&w, 0, sizeof w);
    size_t o = 0;
    w.n_max = n_max;
    w.off_lists = o;  o += align_up((size_t)10 * n_max * sizeof(int), 256);
    w.off_flags = o;  o += align_up((size_t)5 * n_max, 256);
    w.off_ht = o;     o += align_up((size_t)(80 + 4 * DG_HT_CAP) * sizeof(int), 256);
    /* + the seeds of the chunk that is being chained */
    w.off_models = o; o += coop_k > 0 ? 2 * DG_MTAB_BYTES + align_up(DG_PRE_BYTES + (size_t)2 * DG_CHUNK * sizeof(unsigned), 256) : DG_MTAB_BYTES;
    w.off_stage = o;  o += align_up((size_t)2 * n_max * sizeof(dg_pt), 256);   /* the staged points + 32 B per point of the long-list fit */
    /* per-wave lists + stage of the one-repetition-per-wave sections; in the cooperative mode also the 4 x DG_RAN_REP lists of
     * a local optimisation's repetitions (stage 4, one claiming workgroup each: two lists + the staging of its sliced passes) */
    {
        size_t wave_b = (size_t)nw * n_max * (sizeof(int) + sizeof(dg_pt));
        if (coop_k > 0 && wave_b < (size_t)4 * DG_RAN_REP * n_max * sizeof(int)) wave_b = (size_t)4 * DG_RAN_REP * n_max * sizeof(int);
        w.off_wave = o;   o += align_up(wave_b, 256);
    }
    w.off_res = o;    o += align_up((size_t)3 * DG_CHUNK * 12 + (size_t)DG_CHUNK * 20, 256);
    w.off_pts = o;    if (pts_in_ws) o += align_up((size_t)n_max * sizeof(dg_pt), 256);
    w.off_pool = o;   if (pts_in_ws) o += align_up((size_t)n_max * sizeof(int), 256);
    w.off_mslot = o;  if (coop_k > 0) o += align_up((size_t)3 * DG_CHUNK * (2 * sizeof(unsigned short) + sizeof(unsigned)), 256);
    w.off_hjbuf = o;  if (coop_k > 0) o += align_up((size_t)(coop_k + 1) * n_max * sizeof(double), 256);
    w.off_job = o;    if (coop_k > 0) o += align_up(sizeof(dg_coop_job), 256) + align_up(DG_COOP_MAX_SLICES * sizeof(dg_coop_rec), 256) +
                                         align_up((size_t)n_max * (2 * sizeof(int) + sizeof(double)), 256) + align_up(DG_LOJOB_BYTES, 256);
    w.off_hrep = o;   w.hrep = hrep ? 1 : 0;
    if (hrep) o += DG_HREP_HDR_BYTES +
                   (size_t)nw * align_up((size_t)n_max * (2 * sizeof(int) + sizeof(double) + 2 * sizeof(dg_pt)), 256);
    w.off_park = o;   o += align_up(park_bytes, 256);
    w.stride = align_up(o, 4096);
    return w;
}

/* ---- scratch cache: one buffer per (device, stream) ------------------------------------------------
 * Launches on one stream execute in order, so they can share a buffer; launches on different streams get different
 * buffers.  Growing never synchronises: the old buffer is retired with an event recorded on its stream and freed by a
 * later call once that event has completed. */
struct Scratch { int device; hipStream_t stream; char *p; size_t bytes; int small_runs; };
struct Retired { int device; char *p; hipEvent_t ev; };
static std::vector<Scratch> g_scratch_dev[64];   /* per device, guarded by g_dev_mu[device] */
static std::vector<Retired> g_retired_dev[64];

static void reap_retired_locked(int device, bool wait)
{
    std::vector<Retired> &g_retired = g_retired_dev[device];
    for (size_t i = 0; i < g_retired.size();) {
        Retired &r = g_retired[i];
        if (r.device == device && (wait ? hipEventSynchronize(r.ev) == hipSuccess : hipEventQuery(r.ev) == hipSuccess)) {
            (void)hipFree(r.p); (void)hipEventDestroy(r.ev);
            g_retired[i] = g_retired.back(); g_retired.pop_back();
        } else { (void)hipGetLastError(); i++; }
    }
}

/* g_dev_mu[device] must be held by the caller until the kernel that uses the buffer has been enqueued (another thread
 * growing the same stream's buffer retires the old one with an event that must come after that kernel).  Launches on
 * different devices do not serialise on each other. */
/* bytes this (device, stream) already holds in its cached scratch (they come back when the buffer is re-allocated) */
static size_t cached_scratch_locked(int device, hipStream_t stream)
{
    for (auto &e : g_scratch_dev[device]) if (e.device == device && e.stream == stream) return e.bytes;
    return 0;
}
static int get_scratch_locked(int device, hipStream_t stream, size_t bytes, char **out)
{
    std::vector<Scratch> &g_scratch = g_scratch_dev[device];
    std::vector<Retired> &g_retired = g_retired_dev[device];
    reap_retired_locked(device, false);
    Scratch *s = nullptr;
    for (auto &e : g_scratch) if (e.device == device && e.stream == stream) { s = &e; break; }
    if (!s) { g_scratch.push_back(Scratch{device, stream, nullptr, 0, 0}); s = &g_scratch.back(); }
    /* grow when too small; give an oversized buffer back (more than 1 GiB and more than four times what the launches need: one
     * huge batch must not pin gigabytes on every stream that ever saw it) — but only after EIGHT launches in a row that were that
     * much smaller: a stream that alternates a large batch with small calls keeps its buffer instead of freeing and
     * re-allocating gigabytes on every switch */
    const bool oversized = s->bytes > ((size_t)1 << 30) && s->bytes / 4 > bytes;
    s->small_runs = oversized ? s->small_runs + 1 : 0;
    if (s->bytes < bytes || (oversized && s->small_runs >= 8)) {
        s->small_runs = 0;
        if (s->p) {
            Retired r; r.device = device; r.p = s->p;
            HIPCHK(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
            HIPCHK(hipEventRecord(r.ev, stream));
            g_retired.push_back(r);
            s->p = nullptr; s->bytes = 0;
        }
        const size_t want = bytes + bytes / 8;
        if (hipMalloc((void **)&s->p, want) != hipSuccess) { (void)hipGetLastError(); s->p = nullptr; set_err("scratch allocation failed");
            return MI_DEGENSAC_ENOMEM; }
        s->bytes = want;
    }
    *out = s->p;
    return 0;
}

extern "C" int mi_degensac_release_scratch(int device, void *stream_or_null)
{
    DevGuard g; int rc = g.enter(device); if (rc) return rc;
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    std::lock_guard<std::mutex> lk(g_dev_mu[device]);
    std::vector<Scratch> &g_scratch = g_scratch_dev[device];
    for (size_t i = 0; i < g_scratch.size();) {
        Scratch &e = g_scratch[i];
        if (e.device == device && (!stream_or_null || e.stream == (hipStream_t)stream_or_null)) {
            if (e.p) { (void)hipStreamSynchronize(e.stream); (void)hipFree(e.p); (void)hipGetLastError(); }
            g_scratch[i] = g_scratch.back(); g_scratch.pop_back();
        } else i++;
    }
    reap_retired_locked(device, true);
    return 0;
}

static int fill_params(const mi_degensac_params *p, int homography, int dim, dg_params *o)
{
    if (!p) { set_err("params is NULL"); return MI_DEGENSAC_EINVAL; }
    memset(o, 0, sizeof *o);
    const double coef = 3.0 * (p->symmetric_error_check ? 1 : 0);
    if (!homography) {
        /* bindings.cpp:297-318 */
        if (p->error_type != 0 && p->error_type != 1) { set_err("error_type must be 0 or 1 for the fundamental matrix"); return MI_DEGENSAC_EINVAL; }
        o->th = p->px_th * p->px_th; o->sym_th = p->px_th * p->px_th * coef;
    } else {
        /* bindings.cpp:64-107 */
        switch (p->error_type) {
        case 0: o->th = p->px_th * p->px_th; o->sym_th = p->px_th * coef; break;
        case 1: o->th = p->px_th * p->px_th; o->sym_th = 0; break;
        case 2: o->th = p->px_th;            o->sym_th = 0; break;
        case 3: o->th = p->px_th * p->px_th; o->sym_th = p->px_th * coef; break;
        case 4: o->th = p->px_th;            o->sym_th = p->px_th * coef; break;
        default: set_err("error_type must be 0..4 for the homography"); return MI_DEGENSAC_EINVAL;
        }
    }
    o->laf_coef = (p->laf_consistensy_coef > 0 && dim == 6) ? p->laf_consistensy_coef : 0.0;
    o->conf = p->conf; o->max_iters = p->max_iters; o->error_type = p->error_type;
    o->degen = p->enable_degeneracy_check ? 1 : 0;
    o->final_laf_filter = (p->flags & MI_DEGENSAC_FLAG_FINAL_LAF_FILTER) ? 1 : 0;
    if (p->flags & MI_DEGENSAC_FLAG_LEGACY_F) {
        /* exp_ransacF / exp_ransacFcustom (exp_ranF.c:242, :811): no LAF arguments.  Their symmetric check works on all points
         * with its own constant CHECK_COEF * th = 16 th (exp_ranF.c:19, :837) and, in the final mask, on the model the driver
         * computed last (:1196-1203) */
        if (homography) { set_err("MI_DEGENSAC_FLAG_LEGACY_F applies to the fundamental matrix only"); return MI_DEGENSAC_EINVAL; }
        if (o->laf_coef > 0) { set_err("MI_DEGENSAC_FLAG_LEGACY_F takes no LAF check"); return MI_DEGENSAC_EINVAL; }
        if (p->symmetric_error_check) o->sym_th = 16.0 * o->th;
        o->legacy = 1;
    }
    return 0;
}
int est_check_params(const mi_degensac_params *prm, int homography, int dim) { dg_params chk; return fill_params(prm, homography, dim, &chk); }

#ifdef MI_DEGENSAC_DEV
static int *g_trace_dev = nullptr; static int g_trace_cap = 0;
static long long *g_phase_dev = nullptr;
#endif

/* stream mode switch: -1 = automatic (on), 0 = off, odd > 0 = on with test bits (value >> 1: bit 0 = the owner re-scores every
 * chunk it takes from the ring, bit 1 = ask for a producer whether or not unstarted pairs remain); environment
 * MI_DEGENSAC_STREAM at load time, mi_degensac_set_stream_mode at run time (tests, A/B measurements) */
static std::atomic<int> g_stream_mode{[] { const char *e = getenv("MI_DEGENSAC_STREAM"); return e ? atoi(e) : -1; }()};
extern "C" int mi_degensac_set_stream_mode(int mode) { return g_stream_mode.exchange(mode); }
/* homography helpers (dg_hjob_cb): 1 = on (default), 0 = off; environment MI_DEGENSAC_HJOB, mi_degensac_set_hjob_mode (tests, A/B) */
static std::atomic<int> g_hjob_mode{[] { const char *e = getenv("MI_DEGENSAC_HJOB"); return e ? atoi(e) : 1; }()};
extern "C" int mi_degensac_set_hjob_mode(int mode) { return g_hjob_mode.exchange(mode); }
/* -1 = automatic */
static const int g_stream_min_sam = [] { const char *e = getenv("MI_DEGENSAC_STREAM_MIN_SAM"); const int v = e ? atoi(e) : -1; return v >= 0 ? v : -1; }();
/* 0 = automatic */
static std::atomic<int> g_stream_depth{[] { const char *e = getenv("MI_DEGENSAC_STREAM_DEPTH"); const int v = e ? atoi(e) : 0;
    return v >= 2 && v <= 1024 ? v : 0; }()};

/* the error word of the calling thread's last launch that used the stream mode (null: none): the host-pointer entry points read
 * it back with the results and fail loudly when a wait inside the kernel timed out (the asynchronous _dev entry points cannot) */
/* development knobs (A/B experiments, tools/gpu_ab5.py): exported by the development build only; the product library runs the defaults */
static std::atomic<int> g_lo_width{-1};        /* repetitions per round of the fundamental-matrix local optimisation (-1 = environment / automatic) */
static std::atomic<int> g_dev_knob{0};
/* fan mode workers per owner: -1 = environment / automatic, 0 = off; development build: mi_degensac_dev_set_fan */
static std::atomic<int> g_fan_k{-1};
static std::atomic<int> g_per_cu_cap{0};       /* cap on the resident workgroups per CU (0 = none); development build: mi_degensac_dev_set_per_cu */
#ifdef MI_DEGENSAC_DEV
extern "C" int mi_degensac_dev_set_per_cu(int v) { return g_per_cu_cap.exchange(v); }
extern "C" int mi_degensac_dev_set_fan(int k) { return g_fan_k.exchange(k); }
extern "C" int mi_degensac_dev_set_lo_width(int w) { return g_lo_width.exchange(w); }
extern "C" int mi_degensac_dev_set_knob(int v) { return g_dev_knob.exchange(v); }
#endif
static std::atomic<long long> g_wait_ticks{400000000ll};
/* test hook: limit of the stream mode's data waits in 100 MHz ticks (default 4 s; 0 = every data wait fails at once: fault injection;
 * < 0 restores the default); returns the previous value */
extern "C" long long mi_degensac_set_wait_ticks(long long ticks) { return g_wait_ticks.exchange(ticks >= 0 ? ticks : 400000000ll); }

static int launch_batch_impl(int homography, const double *d_p1, const double *d_p2, const int64_t *d_off, const int64_t *h_off,
                             int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
                             hipStream_t stream, double *d_model, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag,
                             int *d_err_copy);

/* ---- batched device entry point (asynchronous on `stream`; the device must be current) -------------
 * (Round 6 built a "mixed-width" form of this launch — a 256-thread and a 128-thread kernel side by side on two streams, sharing the
 * ticket counter, with the narrow launch's long pairs handed to the wide one through a cross queue — measured it slower (154-168 ms
 * against 131 ms on C2 x 4096: profiles/r6_ab_mixed_width.log, DESIGN.md 3) and took it out again; commit d779705 has it.) */
int est_launch_batch(int homography, const double *d_p1, const double *d_p2, const int64_t *d_off, const int64_t *h_off,
                     int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
                     hipStream_t stream, double *d_model, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag, int *d_err_copy)
{
    if (n_pairs <= 0) return 0;
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    std::lock_guard<std::mutex> lk(g_dev_mu[device]);
    return launch_batch_impl(homography, d_p1, d_p2, d_off, h_off, n_pairs, dim, prm, d_seeds, device, stream, d_model, d_mask, d_stats, diag, d_err_copy);
}

static int launch_batch_impl(int homography, const double *d_p1, const double *d_p2, const int64_t *d_off, const int64_t *h_off,
                        int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
                             hipStream_t stream, double *d_model, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag,
                             int *d_err_copy)
{
    /* (g_dev_mu[device] is held by the caller) */
    if (n_pairs <= 0) return 0;
    if (dim != 2 && dim != 6) { set_err("points must be [n,2] or [n,6]"); return MI_DEGENSAC_EINVAL; }
    if (!h_off) { set_err("offsets_host is NULL"); return MI_DEGENSAC_EINVAL; }
    if (!d_p1 || !d_p2 || !d_off || !d_seeds || !d_model || !d_mask) {
        set_err("NULL argument (pts1, pts2, offsets, seeds, the model and the mask are required)"); return MI_DEGENSAC_EINVAL; }
    int rc = dev_init(device); if (rc) return rc;
    dg_args A; memset(&A, 0, sizeof A);
    rc = fill_params(prm, homography, dim, &A.prm); if (rc) return rc;
    int n_max = 0, n_min = 1 << 30;
    for (int p = 0; p < n_pairs; p++) {
        long long n = h_off[p+1] - h_off[p];
        if (n > 0x7fffffff / 64) { set_err("too many correspondences in one pair"); return MI_DEGENSAC_EINVAL; }
        if (n > n_max) n_max = (int)n; if (n < n_min) n_min = (int)n;
    }
    const int min_pts = homography ? 4 : 8;                      /* bindings.cpp:35,270 */
    if (n_min < min_pts) { set_err(homography ? "need n >= 4 correspondences" : "need n >= 8 correspondences"); return MI_DEGENSAC_EINVAL; }
    /* Variant and placement.  Latency: 512-thread workgroups, one pair per CU, point set + sampler pool in LDS when
     * they fit (36 B per correspondence next to the static LDS).  Throughput: once the batch holds several pairs per CU,
     * 256-thread workgroups with only the pool in LDS leave room for two resident pairs per CU, which hides the serial
     * small-solver chains of one pair behind the other (DESIGN.md 5).  params.tuning overrides. */
    const DevState &ds = g_dev[device];
    uint32_t tune = prm->tuning;
    if (!tune && g_env_tuning) {
        /* the environment word is process-wide and meets both kinds of call: fields that do not apply to this one are dropped
         * (only a word that arrives in params.tuning is checked strictly) */
        tune = g_env_tuning;
        if (homography) tune &= ~(MI_DEGENSAC_TUNE_F_SERIAL_REPS | MI_DEGENSAC_TUNE_COOP_ALL_PASSES | (7u << 29));
        else            tune &= ~MI_DEGENSAC_TUNE_H_SERIAL_LO;
    }
    /* every tuning field has its own bits (include/mi_degensac.h); a field that does not apply to this call is an error */
    if (homography && (tune & MI_DEGENSAC_TUNE_F_SERIAL_REPS)) { set_err("MI_DEGENSAC_TUNE_F_SERIAL_REPS applies to the fundamental matrix only");
        return MI_DEGENSAC_EINVAL; }
    if (!homography && (tune & MI_DEGENSAC_TUNE_H_SERIAL_LO)) { set_err("MI_DEGENSAC_TUNE_H_SERIAL_LO applies to the homography only");
        return MI_DEGENSAC_EINVAL; }
    if (homography && (tune & MI_DEGENSAC_TUNE_COOP_ALL_PASSES)) { set_err("MI_DEGENSAC_TUNE_COOP_ALL_PASSES applies to the fundamental matrix only");
        return MI_DEGENSAC_EINVAL; }
    if (homography && (tune >> 29)) { set_err("MI_DEGENSAC_TUNE_LONG_SHIFT applies to the fundamental matrix only"); return MI_DEGENSAC_EINVAL; }
    const size_t dyn_all = (size_t)n_max * (sizeof(dg_pt) + sizeof(int)), dyn_pool = (size_t)n_max * sizeof(int);
    int variant = 0, mode;
    /* the throughput variant needs its pool in LDS next to the other resident workgroup of the CU: 256 threads x 2 per CU
     * from MORE THAN 2 pairs per CU on (measured crossover: up to two pairs per CU the 512-thread kernel with its producers wins, C2 x 512
     * 44.3 against 47.1 ms; past that it has no producers and two generations of pairs, C2 x 640 / 767: 61.7 / 62.0 against 48.3 / 49.7 ms;
     * profiles/r6_ab_f_variants_midsize.log).  The 128-thread variant (3-4 pairs per CU) is only taken
     * on request: its steady state is ~5 % better but its slowest pairs take 1.6 x longer, which a batch of a few
     * thousand pairs does not amortise. */
    if (n_pairs > 2 * ds.cus && ds.static_lds[1][homography] + dyn_pool + 512 <= (size_t)ds.max_lds / 2) variant = 1;
    /* homography: a pair's time is its local optimisation, whose ten repetitions run one per wave (dg_inHranic_waves); a
     * batch that fills the device runs best on the smallest workgroups, which leave no wave idle in a partly filled round
     * of repetitions (C3 x 1024: 27.2 ms at 128 threads x 4 per CU, 30.7 ms at 512 x 1, 35.2 ms at 256 x 2) */
    /* round 6: between one and three pairs per CU the whole batch is resident at two or four workgroups per CU, and one generation of
     * pairs on four or two waves each ends before two generations on eight (C3 x 384 / 512 / 640: 12.6 / 13.9 / 14.8 ms at 512 threads,
     * 10.7 / 12.2 / 13.1 at 256 x 2 per CU, 11.6 / 12.3 / 13.0 at 128 x 4; profiles/r6_ab_homography_variants.log) */
    if (homography && n_pairs > 2 * ds.cus && ds.static_lds[2][1] + 512 <= (size_t)ds.max_lds / 4) variant = 2;
    else if (homography && n_pairs > ds.cus && ds.static_lds[1][1] + 512 <= (size_t)ds.max_lds / 2) variant = 1;
    if ((tune & 3u) == 1u) variant = 0; else if ((tune & 3u) == 2u) variant = 1; else if ((tune & 3u) == 3u) variant = 2;
    const size_t room = (size_t)(ds.max_lds - ds.static_lds[variant][homography] - 256);
    if (variant >= 1)           mode = dyn_pool <= room ? DG_MODE_POOL_LDS : DG_MODE_HBM;
    else if (dyn_all <= room)   mode = DG_MODE_LDS;
    else                        mode = dyn_pool <= room ? DG_MODE_POOL_LDS : DG_MODE_HBM;
    if (homography && variant >= 1 && mode == DG_MODE_POOL_LDS) {
        /* ... and residency counts for more than the sampler pool's placement: with the pool in the workspace more
         * workgroups fit a CU (C3 x 1024: 27.2 ms with 4 per CU against 35.3 ms with 3) */
        const long long fit_pool = (long long)((size_t)ds.max_lds / (ds.static_lds[variant][1] + dyn_pool + 256));
        long long fit_hbm = (long long)((size_t)ds.max_lds / (ds.static_lds[variant][1] + 256)); if (fit_hbm > 8) fit_hbm = 8;
        if (fit_pool * ds.cus < n_pairs && fit_hbm > fit_pool) mode = DG_MODE_HBM;
    }
    switch ((tune >> 2) & 3u) {
    case 1: mode = DG_MODE_HBM; break;
    case 2: if (dyn_all <= room) mode = DG_MODE_LDS; break;
    case 3: if (dyn_pool <= room) mode = DG_MODE_POOL_LDS; break;
    default: break;
    }
    const size_t dyn = mode == DG_MODE_LDS ? dyn_all : (mode == DG_MODE_POOL_LDS ? dyn_pool : 0);
    /* persistent grid: as many workgroups as the device keeps resident, never more than there are pairs */
    int per_cu = 0;
    hipError_t oe = g_variant_resident[variant](homography, mode, dyn, &per_cu);
    if (oe != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
    {   /* the occupancy query is advisory; LDS is the resource that binds these kernels */
        const int by_lds = (int)((size_t)ds.max_lds / (ds.static_lds[variant][homography] + dyn + 256));
        if (by_lds >= 1 && per_cu > by_lds) per_cu = by_lds;
        if (per_cu > 8) per_cu = 8;
        /* development aid (A/B of residency, tools/): MI_DEGENSAC_PER_CU=<k> caps the resident workgroups per CU; read once */
        static const int env_per_cu = [] { const char *e = getenv("MI_DEGENSAC_PER_CU"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 0; }();
        const int cap_pc = g_per_cu_cap.load() > 0 ? g_per_cu_cap.load() : env_per_cu;
        if (cap_pc > 0 && per_cu > cap_pc) per_cu = cap_pc;
    }
    /* Cooperative large-n mode (fundamental matrix, everything in the HBM workspace): when the batch leaves most of the
     * device idle and one scoring pass is long, every owner gets helper workgroups that score groups of its chunk's
     * models (dg_f_helper).  All workgroups of the grid must be resident (helpers spin on their owner), so the grid
     * never exceeds what the device admits.  tuning bits 8-15: 0 = automatic, 255 = off, else the helper count. */
    const long long capacity = (long long)per_cu * ds.cus;
    int coop_k = 0;
    if (!homography && mode == DG_MODE_HBM) {
        const unsigned th_ = (tune >> 8) & 255u;
        /* automatic: 23 helpers (three workgroups per XCD: C5 takes 98 ms against 104 with 15 and 107 with 31 — more
         * claimers shorten a stage's units, and lengthen its hand-off), 15 when the batch leaves room for no more */
        if (th_ == 0) { if (n_max >= 8192 && (long long)n_pairs * 24 <= capacity) coop_k = 23;
            else if (n_max >= 8192 && (long long)n_pairs * 16 <= capacity) coop_k = 15; }
        else if (th_ != 255u) coop_k = (int)th_;
        while (coop_k > 0 && (long long)(coop_k + 1) > capacity) coop_k--;
    }
    long long owners = coop_k > 0 ? capacity / (coop_k + 1) : capacity; if (owners > n_pairs) owners = n_pairs;
    {   /* tuning bits 24-28: cap on the resident workgroups (tests of the queueing paths on small batches) */
        const unsigned gc = (tune >> 24) & 31u;
        if (gc > 0 && coop_k == 0 && owners > (long long)gc) owners = gc;
    }
    long long grid = owners * (coop_k + 1);
    /* Stream mode (dg_stream_cb): a pair with many samples left hands the outcome-independent part of its main loop to a
     * workgroup that has run out of pairs.  Fundamental matrix, pool (and maybe points) in LDS, no helpers, no diagnostics.
     * A batch smaller than the device gets one extra workgroup per pair as a producer from the start. */
    /* per call: params.flags wins over the process-wide default (mi_degensac_set_stream_mode / MI_DEGENSAC_STREAM) */
    int stream_mode = g_stream_mode.load();
    if (prm->flags & MI_DEGENSAC_FLAG_NO_STREAM) stream_mode = 0;
    else if (prm->flags & MI_DEGENSAC_FLAG_STREAM_ON) stream_mode = 1 | (int)(((prm->flags >> 8) & 3u) << 1);
    else if (prm->flags & MI_DEGENSAC_FLAG_STREAM_AUTO) stream_mode = -1;
    const int hjob_mode = (prm->flags & MI_DEGENSAC_FLAG_NO_HJOB) ? 0 : (prm->flags & MI_DEGENSAC_FLAG_HJOB_ON) ? 1 : g_hjob_mode.load();
    /* automatic: batches of at most two pairs per resident workgroup.  There the launch ends with its slowest pair while most
     * of the device idles (C2 x 512: 63.4 -> 59.1 ms; one pair per call: 11.3 -> 10.5 ms median).  A batch many times the device
     * ends with a handful of event-bound pairs that a producer cannot help, and pays for the idle workgroups' polling and the
     * producers next to owners on the same CU (C2 x 4096: 144.0 -> 148.7 ms): off. */
    bool stream_on = !homography && coop_k == 0 && mode != DG_MODE_HBM && !(diag && (diag->d_resids || diag->d_hist)) && stream_mode != 0 &&
                     prm->max_iters >= 8192 && ((tune >> 24) & 31u) == 0 && (stream_mode > 0 || (long long)n_pairs <= 2 * capacity);
    bool stream_early = false;         /* a spare workgroup per pair from the start: pairs ask for their producer with their first chunk */
    if (stream_on && grid < capacity) { long long extra = capacity - grid; if (extra > n_pairs) extra = n_pairs; stream_early = extra >= n_pairs; grid += extra;
        owners = grid; }
    /* Homography: workgroups that have run out of pairs take repetitions of the local optimisations that still run (dg_hjob_cb);
     * the points must be in the owner's workspace for that (not in its LDS).  A batch smaller than the device gets up to two
     * extra workgroups per pair as helpers from the start. */
    const bool hjob_on = homography && mode != DG_MODE_LDS && !(diag && diag->d_resids) && !(tune & MI_DEGENSAC_TUNE_H_SERIAL_LO) && hjob_mode != 0 &&
                         ((tune >> 24) & 31u) == 0;
    if (hjob_on && grid < capacity) { long long extra = capacity - grid; if (extra > 2 * (long long)n_pairs) extra = 2 * (long long)n_pairs; grid += extra;
        owners = grid; }
    /* Fan mode (dg_f_fan.h): one large pair per owner on a mostly idle device, cooperative helpers on.  Per owner fan_k extra workgroups: one
     * draws the pair's sample stream into the ring, the others solve and score its chunks (stream-mode ring entries, 32 by default: C5 takes
     * 30.1 ms with 16, 30.7 with 64); the owner commits, the helpers keep the local optimisations.
     * Needs every pair on its own owner (workers serve one pair) and room for at least eight workers per owner; off with the stream mode
     * (MI_DEGENSAC_FLAG_NO_STREAM / mi_degensac_set_stream_mode(0)) and with per-pair diagnostics. */
    int fan_k = 0;
    if (!homography && variant == 0 && coop_k > 0 && mode == DG_MODE_HBM && stream_mode != 0 && owners >= n_pairs && !(diag && (diag->d_resids || diag->d_hist))
        &&
        ((tune >> 24) & 31u) == 0 && !(prm->flags & MI_DEGENSAC_FLAG_LEGACY_F)) {
        /* -1 = automatic, 0 = off, else the worker count */
        static const int env_fan = [] { const char *e = getenv("MI_DEGENSAC_FAN"); return e ? atoi(e) : -1; }();
        long long k = (capacity - grid) / owners;
        const long long want = g_fan_k.load() >= 0 ? g_fan_k.load() : (env_fan >= 0 ? env_fan : 32);
        if (k > want) k = want;
        if (k >= 8) fan_k = (int)k;
    }
    if (fan_k > 0) grid += owners * fan_k;
    /* Setting pairs aside (dg_args::park_sam; fundamental matrix): only when pairs queue behind the resident grid.
     * Threshold: tuning bits 16-23 in units of 256 samples, 255 = off, 0 = automatic = 1024 samples (the discovery round:
     * at 40 % inliers four pairs in five have drawn their first all-inlier sample by then and had their sample budget cut
     * by a local optimisation; the others, and the pairs whose model comes from the DEGENSAC branch and which keep the full
     * budget, go to the "many samples left" queue, which is served first).  Spare workspaces: one per pair that can still
     * be queued, bounded by 24 GB of scratch; a pair that finds no spare simply keeps running. */
    int park_sam = 0; long long spares = 0; size_t park_bytes = 0;
    if (stream_on) park_bytes = align_up((size_t)ds.static_lds[variant][0], 256) + align_up(dyn, 256);      /* the image a producer starts from */
    if (!homography && coop_k == 0 && !(diag && (diag->d_resids || diag->d_hist)) && (long long)n_pairs > owners) {
        const unsigned pt = (tune >> 16) & 255u;
        if (pt == 0) park_sam = 1024;
        else if (pt != 255u) park_sam = (int)pt * 256;
        if (park_sam > 0) {
            spares = (long long)n_pairs - owners;
            park_bytes = align_up((size_t)ds.static_lds[variant][0], 256) + align_up(dyn, 256);   /* static LDS of the kernel >= its dg_f_shared */
        }
    }
    A.wl = make_layout(n_max, mode != DG_MODE_LDS, g_variant_threads[variant] / 64, coop_k, park_bytes, homography != 0);
    if (spares > 0) {
        /* spare workspaces are an optimisation (spares = 0 only turns setting pairs aside off), so they take at most half of
         * what the device can still give this stream, and never more than 24 GB */
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)4 << 30; }
        size_t budget = (free_b + cached_scratch_locked(device, stream)) / 2;
        if (budget > ((size_t)24 << 30)) budget = (size_t)24 << 30;
        const long long room_ws = (long long)(budget / (A.wl.stride + A.wl.stride / 8)) - owners;
        if (spares > room_ws) spares = room_ws > 0 ? room_ws : 0;
    }
    const size_t hdr_coop = DG_HDR_BYTES + align_up((size_t)owners * sizeof(dg_coop_cb), 256);
    /* dg_hjob_cb has the same size */
    const size_t hdr_cb = hdr_coop + ((stream_on || hjob_on || fan_k > 0) ? align_up((size_t)owners * sizeof(dg_stream_cb), 256) : 0);
    /* ring depth: a pair's events tend to come first (the DEGENSAC completions of a degenerate pair take tens of milliseconds in
     * its first thousand samples) and its long stretch of uneventful samples afterwards, so the producer must be able to run the
     * whole budget ahead: one entry per chunk of the budget, at most 512, within a quarter of the free memory and 8 GB */
    const size_t ent_bytes = align_up(sizeof(dg_stream_ent), 256);      /* this translation unit has the largest chunk and workgroup size */
    int stream_depth = g_stream_depth.load();
    if (stream_depth <= 0) { stream_depth = prm->max_iters / 256 + 2; if (stream_depth > 512) stream_depth = 512; if (stream_depth < 8) stream_depth = 8; }
    if (stream_on || fan_k > 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)4 << 30; }
        size_t budget = (free_b + cached_scratch_locked(device, stream)) / 4; if (budget > ((size_t)8 << 30)) budget = (size_t)8 << 30;
        const size_t fit = budget / ((size_t)owners * ent_bytes);
        if (fit < (size_t)stream_depth) stream_depth = (int)fit;
        if (stream_depth < 8) { stream_on = false; if (fan_k > 0) { grid -= owners * fan_k; fan_k = 0; } }
    }
    const size_t fan_ws = fan_k > 0 ? (size_t)owners * fan_k : 0;                     /* one workspace per worker, behind the owners' and the spares */
    size_t hdr, ring_bytes; char *ws;
    for (;;) {
        hdr = hdr_cb + align_up((size_t)2 * spares * sizeof(long long), 256);
        /* fan mode: + one flag line per entry */
        ring_bytes = (stream_on || fan_k > 0) ? (size_t)owners * stream_depth * (ent_bytes + (fan_k > 0 ? 128 : 0)) : 0;
        rc = get_scratch_locked(device, stream, hdr + A.wl.stride * (size_t)(owners + spares + fan_ws) + ring_bytes, &ws);
        if (rc != MI_DEGENSAC_ENOMEM || (spares == 0 && !stream_on)) break;
        if (spares > 0) spares /= 2;                   /* allocation failed: fewer spare workspaces, down to none ... */
        else stream_on = false;                        /* ... then no producer rings */
    }
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(ws, 0, (coop_k > 0 || stream_on || hjob_on) ? hdr_cb : DG_HDR_BYTES, stream));
    if (fan_k > 0) HIPCHK(hipMemsetAsync(ws + hdr + A.wl.stride * (size_t)(owners + spares + fan_ws) + (size_t)owners * stream_depth * ent_bytes, 0,
        (size_t)owners * stream_depth * 128, stream));
    if (spares > 0) HIPCHK(hipMemsetAsync(ws + hdr_cb, 0xff, (size_t)2 * spares * sizeof(long long), stream));
    /* header: ticket at +0, the spare counter and the two queues' counters on their own 128-byte lines from +128, control
     * blocks from +DG_HDR_BYTES */
    A.ticket = (int *)ws; A.park_ctl = (int *)(ws + 128); A.park_q = (long long *)(ws + hdr_cb); A.park_cap = (int)spares;
    A.park_sam = spares > 0 ? park_sam : 0; A.n_res = (int)owners; A.n_ws = (int)(owners + spares); A.dyn_bytes = (int)dyn;
    {   /* "many samples left": tuning bits 29-31 = log2 of the factor on park_sam (0 = automatic = 8 x park_sam) */
        const unsigned lg = (tune >> 29) & 7u;
        A.park_long = park_sam << (lg ? lg : 3);
    }
    A.coop = (dg_coop_cb *)(ws + DG_HDR_BYTES);          /* 256-byte aligned: hipMalloc returns at least that */
    A.done_pairs = (int *)(ws + 768); A.err_flag = (int *)(ws + 896);
    A.stream_on = stream_on ? 1 : 0; A.scb = (dg_stream_cb *)(ws + hdr_coop); A.stream_depth = stream_depth; A.stream_ent_bytes = ent_bytes;
    A.ring = ws + hdr + A.wl.stride * (size_t)(owners + spares + fan_ws);
    A.fan_k = fan_k; A.fan_ws0 = (int)(owners + spares); A.fan_flags = fan_k > 0 ? (int *)(A.ring + (size_t)owners * stream_depth * ent_bytes) : nullptr;
    A.hjob = hjob_on ? (dg_hjob_cb *)(ws + hdr_coop) : nullptr;
    /* a pair asks with the first chunk it starts after the launch has run out of unstarted pairs (at once when the launch has a spare
     * workgroup for every pair anyway): a pair's events (local optimisations, DEGENSAC completions: milliseconds each) fall into its
     * first samples, and a producer that starts with them has the uneventful rest of the budget ready when the owner gets there
     * (64 pairs: 48.8 -> 34.2 ms; C2 x 512: 59.2 -> 52.1 ms against asking after 1024 samples) */
    (void)stream_early;
    /* a request that nobody can take yet costs one image; the workgroups that look for requests are the ones without pairs */
    A.stream_early = stream_on ? 1 : 0;
    A.stream_min_sam = g_stream_min_sam >= 0 ? g_stream_min_sam : 0; A.stream_min_left = 4096;
    A.stream_test = stream_mode > 0 ? (stream_mode >> 1) : 0;
    { const long long wt = g_wait_ticks.load(); A.wait_ticks = wt > 2000000000ll ? 2000000000 : (int)wt; }
    A.coop_k = coop_k; A.ws = ws + hdr; A.order = nullptr;
    A.coop_pass_min = (coop_k > 0 && (tune & MI_DEGENSAC_TUNE_COOP_ALL_PASSES)) ? 0 : 8192;      /* distribute every full pass (tests) */
    A.pts1 = d_p1; A.pts2 = d_p2; A.offsets = (const long long *)d_off; A.seeds = d_seeds;
    A.lo_serial = (homography && (tune & MI_DEGENSAC_TUNE_H_SERIAL_LO)) ? 1 : 0;      /* local optimisation repetitions one after the other */
    A.innerh_serial = (!homography && (tune & MI_DEGENSAC_TUNE_F_SERIAL_REPS)) ? 1 : 0;
    A.dev_knob = g_dev_knob.load();
    A.lo_width = g_lo_width.load() >= 0 ? g_lo_width.load() : 0;
    A.pool_seq = (!ds.pool_par_ok || (tune & MI_DEGENSAC_TUNE_SEQ_POOL)) ? 1 : 0;
    A.variant_threads = g_variant_threads[variant]; A.mode = mode;
#ifdef MI_DEGENSAC_DEV
    A.trace = g_trace_dev; A.trace_cap = g_trace_cap; A.phase_out = g_phase_dev;
#endif
    if (diag && diag->d_resids && diag->resid_runs > 0) { A.resids_out = diag->d_resids; A.resid_runs = diag->resid_runs; }
    if (diag && diag->d_hist && !homography) A.hist_out = diag->d_hist;
    /* d_screen was added to the struct after its first version: only a caller that states a size covering it is read there */
    if (diag && (size_t)diag->struct_size >= offsetof(mi_degensac_diag, d_screen) + sizeof(int32_t *) && diag->d_screen &&
        !homography) A.screen_out = diag->d_screen;
    A.model_out = d_model; A.mask_out = d_mask; A.stats_out = d_stats; A.dim = dim; A.n_pairs = n_pairs; A.pts_in_lds = mode == DG_MODE_LDS;
    HIPCHK(g_variant_launch[variant](homography, mode, (int)grid, dyn, stream, A));
    /* still under g_dev_mu: another thread that regrows this stream's scratch retires the buffer behind an event recorded after this copy */
    if (d_err_copy) HIPCHK(hipMemcpyAsync(d_err_copy, A.err_flag, sizeof(int), hipMemcpyDeviceToDevice, stream));
    return 0;
}

static int batch_dev(int homography, const double *d_pts1, const double *d_pts2, const int64_t *d_offsets, const int64_t *offsets_host,
                     int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device, void *stream,
                     double *d_M, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag = nullptr)
{
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    if (mi_degensac_device_count() == 0) { set_err("no HIP device: this library has no CPU path"); return MI_DEGENSAC_ENODEV; }
    DevGuard g; int rc = g.enter(device); if (rc) return rc;
    return est_launch_batch(homography, d_pts1, d_pts2, d_offsets, offsets_host, n_pairs, dim, prm, d_seeds, device, (hipStream_t)stream, d_M, d_mask, d_stats,
        diag);
}
extern "C" int mi_degensac_find_fundamental_batch_dev(const double *d_pts1, const double *d_pts2, const int64_t *d_offsets,
        const int64_t *offsets_host, int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
        void *stream, double *d_F, uint8_t *d_mask, int32_t *d_stats)
{ return batch_dev(0, d_pts1, d_pts2, d_offsets, offsets_host, n_pairs, dim, prm, d_seeds, device, stream, d_F, d_mask, d_stats); }
extern "C" int mi_degensac_find_homography_batch_dev(const double *d_pts1, const double *d_pts2, const int64_t *d_offsets,
        const int64_t *offsets_host, int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
        void *stream, double *d_H, uint8_t *d_mask, int32_t *d_stats)
{ return batch_dev(1, d_pts1, d_pts2, d_offsets, offsets_host, n_pairs, dim, prm, d_seeds, device, stream, d_H, d_mask, d_stats); }

extern "C" int mi_degensac_find_fundamental_batch_dev_ex(const double *d_pts1, const double *d_pts2, const int64_t *d_offsets,
        const int64_t *offsets_host, int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
        void *stream, double *d_F, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag)
{ return batch_dev(0, d_pts1, d_pts2, d_offsets, offsets_host, n_pairs, dim, prm, d_seeds, device, stream, d_F, d_mask, d_stats, diag); }
extern "C" int mi_degensac_find_homography_batch_dev_ex(const double *d_pts1, const double *d_pts2, const int64_t *d_offsets,
        const int64_t *offsets_host, int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
        void *stream, double *d_H, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag)
{ return batch_dev(1, d_pts1, d_pts2, d_offsets, offsets_host, n_pairs, dim, prm, d_seeds, device, stream, d_H, d_mask, d_stats, diag); }

/* ---- contexts: one stream, pinned host staging and device I/O buffers that persist across calls ------ */
struct mi_degensac_ctx {
    int device = 0; hipStream_t stream = nullptr;
    char *h_pin = nullptr; size_t h_cap = 0;       /* pinned host staging (inputs and outputs of one call) */
    char *d_io = nullptr;  size_t d_cap = 0;       /* device mirror */
    int stream_mode = -2, hjob_mode = -2;          /* scheduling defaults of this context (-2 = the process-wide ones): mi_degensac_ctx_set_scheduling */
};

static int ctx_reserve(mi_degensac_ctx *c, size_t bytes)
{
    if (c->h_cap < bytes) {
        if (c->h_pin) { HIPCHK(hipStreamSynchronize(c->stream)); (void)hipHostFree(c->h_pin); c->h_pin = nullptr; c->h_cap = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipHostMalloc((void **)&c->h_pin, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); set_err("pinned host allocation failed");
            return MI_DEGENSAC_ENOMEM; }
        c->h_cap = want;
    }
    if (c->d_cap < bytes) {
        if (c->d_io) { HIPCHK(hipStreamSynchronize(c->stream)); (void)hipFree(c->d_io); c->d_io = nullptr; c->d_cap = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipMalloc((void **)&c->d_io, want) != hipSuccess) { (void)hipGetLastError(); set_err("device allocation failed"); return MI_DEGENSAC_ENOMEM; }
        c->d_cap = want;
    }
    return 0;
}

extern "C" int mi_degensac_ctx_create(int device, mi_degensac_ctx **out)
{
    if (!out) { set_err("NULL argument"); return MI_DEGENSAC_EINVAL; }
    *out = nullptr;
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    if (mi_degensac_device_count() == 0) { set_err("no HIP device: this library has no CPU path"); return MI_DEGENSAC_ENODEV; }
    if (device >= mi_degensac_device_count()) { set_err("device index out of range"); return MI_DEGENSAC_ENODEV; }
    DevGuard g; int rc = g.enter(device); if (rc) return rc;
    rc = dev_init(device); if (rc) return rc;
    mi_degensac_ctx *c = new (std::nothrow) mi_degensac_ctx; if (!c) { set_err("out of memory"); return MI_DEGENSAC_ENOMEM; }
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; set_err("hipStreamCreate failed: %s", hipGetErrorString(e)); (void)hipGetLastError(); return MI_DEGENSAC_EHIP; }
    *out = c;
    return 0;
}

extern "C" void mi_degensac_ctx_destroy(mi_degensac_ctx *c)
{
    if (!c) return;
    DevGuard g; if (g.enter(c->device)) { delete c; return; }
    (void)hipStreamSynchronize(c->stream);
    (void)mi_degensac_release_scratch(c->device, c->stream);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    if (c->d_io) (void)hipFree(c->d_io);
    (void)hipStreamDestroy(c->stream);
    (void)hipGetLastError();
    delete c;
}
extern "C" void *mi_degensac_ctx_stream(mi_degensac_ctx *c) { return c ? (void *)c->stream : nullptr; }
extern "C" int mi_degensac_ctx_set_scheduling(mi_degensac_ctx *c, int stream_mode, int hjob_mode)
{
    if (!c) { set_err("context is NULL"); return MI_DEGENSAC_EINVAL; }
    if (stream_mode < -2 || hjob_mode < -2 || hjob_mode > 1) { set_err("bad scheduling mode"); return MI_DEGENSAC_EINVAL; }
    c->stream_mode = stream_mode; c->hjob_mode = hjob_mode;
    return 0;
}

/* Where the time of one host-pointer call goes (include/mi_degensac.h: mi_degensac_set_call_timing / _last_call_timing): host clocks
 * around the phases of ctx_batch, HIP events around the copies and the kernel on the context's stream.  Off by default (four events per call). */
static std::atomic<int> g_call_timing{0};
static thread_local double g_last_timing[MI_DEGENSAC_TIMING_LEN] = {0};
extern "C" int mi_degensac_set_call_timing(int on) { return g_call_timing.exchange(on ? 1 : 0); }
extern "C" int mi_degensac_last_call_timing(double *out)
{
    if (!out) { set_err("NULL argument"); return MI_DEGENSAC_EINVAL; }
    for (int i = 0; i < MI_DEGENSAC_TIMING_LEN; i++) out[i] = g_last_timing[i];
    return 0;
}
static double host_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* the parameters of a re-run after a hand-over time-out: no producer workgroups, no homography helpers and no helper workgroups
 * of the cooperative mode (results do not depend on them) */
static mi_degensac_params rerun_params(const mi_degensac_params *prm, int homography)
{
    mi_degensac_params p2s = *prm; p2s.flags = (p2s.flags & ~MI_DEGENSAC_FLAG_STREAM_ON) | MI_DEGENSAC_FLAG_NO_STREAM | MI_DEGENSAC_FLAG_NO_HJOB;
    if (!homography) p2s.tuning = (p2s.tuning & ~(255u << 8)) | MI_DEGENSAC_TUNE_HELPERS(255);
    return p2s;
}

/* host pointers -> one packed pinned block -> one H2D copy -> kernel -> one D2H copy, all on the context's stream */
static int ctx_batch(mi_degensac_ctx *c, int homography, const double *p1, const double *p2, const int64_t *off, int n_pairs, int dim,
                     const mi_degensac_params *prm, const uint32_t *seeds, double *model, uint8_t *mask, int32_t *stats, int depth = 0)
{
    if (!c) { set_err("context is NULL"); return MI_DEGENSAC_EINVAL; }
    if (!p1 || !p2 || !off || !model || !mask || !seeds) { set_err("NULL argument"); return MI_DEGENSAC_EINVAL; }
    if (n_pairs <= 0) return 0;
    if (dim != 2 && dim != 6) { set_err("points must be [n,2] or [n,6]"); return MI_DEGENSAC_EINVAL; }
    for (int p = 0; p < n_pairs; p++) if (off[p+1] < off[p]) { set_err("offsets must be non-decreasing"); return MI_DEGENSAC_EINVAL; }
    DevGuard g; int rc = g.enter(c->device); if (rc) return rc;
    const size_t total = (size_t)(off[n_pairs] - off[0]);
    const size_t b_pts = align_up(total * dim * sizeof(double), 256), b_off = align_up((size_t)(n_pairs + 1) * 8, 256),
                 b_seed = align_up((size_t)n_pairs * 4, 256), b_model = align_up((size_t)n_pairs * 72, 256),
                 b_mask = align_up(total, 256), b_stats = align_up((size_t)n_pairs * 64, 256);
    const size_t o_p1 = 0, o_p2 = b_pts, o_off = 2 * b_pts, o_seed = o_off + b_off, in_bytes = o_seed + b_seed;
    const size_t o_model = in_bytes, o_mask = o_model + b_model, o_stats = o_mask + b_mask, o_err = o_stats + b_stats, all_bytes = o_err + 256;
    /* the context's own scheduling defaults become per-call flags where the caller's flags are silent */
    mi_degensac_params prm_ctx;
    if (prm && (c->stream_mode != -2 || c->hjob_mode != -2)) {
        prm_ctx = *prm;
        if (c->stream_mode != -2 && !(prm_ctx.flags & (MI_DEGENSAC_FLAG_NO_STREAM | MI_DEGENSAC_FLAG_STREAM_ON | MI_DEGENSAC_FLAG_STREAM_AUTO)))
            prm_ctx.flags |= c->stream_mode == 0 ? MI_DEGENSAC_FLAG_NO_STREAM : c->stream_mode < 0 ? MI_DEGENSAC_FLAG_STREAM_AUTO
                                                 : (MI_DEGENSAC_FLAG_STREAM_ON | MI_DEGENSAC_FLAG_STREAM_TEST(c->stream_mode >> 1));
        if (c->hjob_mode != -2 && !(prm_ctx.flags & (MI_DEGENSAC_FLAG_NO_HJOB | MI_DEGENSAC_FLAG_HJOB_ON)))
            prm_ctx.flags |= c->hjob_mode == 0 ? MI_DEGENSAC_FLAG_NO_HJOB : MI_DEGENSAC_FLAG_HJOB_ON;
        prm = &prm_ctx;
    }
    const bool timing = depth == 0 && g_call_timing.load() != 0;
    const double t0 = timing ? host_ms() : 0.0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvFree { hipEvent_t *e; ~EvFree() { for (int i = 0; i < 4; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evfree{ev};
    if (timing) for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&ev[i]));
    rc = ctx_reserve(c, all_bytes); if (rc) return rc;
    memcpy(c->h_pin + o_p1, p1 + (size_t)off[0] * dim, total * dim * sizeof(double));
    memcpy(c->h_pin + o_p2, p2 + (size_t)off[0] * dim, total * dim * sizeof(double));
    int64_t *ho = (int64_t *)(c->h_pin + o_off);
    for (int p = 0; p <= n_pairs; p++) ho[p] = off[p] - off[0];
    memcpy(c->h_pin + o_seed, seeds, (size_t)n_pairs * 4);
    const double t1 = timing ? host_ms() : 0.0;
    if (timing) HIPCHK(hipEventRecord(ev[0], c->stream));
    HIPCHK(hipMemcpyAsync(c->d_io, c->h_pin, in_bytes, hipMemcpyHostToDevice, c->stream));
    if (timing) HIPCHK(hipEventRecord(ev[1], c->stream));
    rc = est_launch_batch(homography, (const double *)(c->d_io + o_p1), (const double *)(c->d_io + o_p2), (const int64_t *)(c->d_io + o_off), ho,
                      n_pairs, dim, prm, (const uint32_t *)(c->d_io + o_seed), c->device, c->stream,
                      (double *)(c->d_io + o_model), (uint8_t *)(c->d_io + o_mask), (int32_t *)(c->d_io + o_stats), nullptr, (int *)(c->d_io + o_err));
    if (rc) return rc;
    if (timing) HIPCHK(hipEventRecord(ev[2], c->stream));
    HIPCHK(hipMemcpyAsync(c->h_pin + o_model, c->d_io + o_model, all_bytes - o_model, hipMemcpyDeviceToHost, c->stream));
    if (timing) HIPCHK(hipEventRecord(ev[3], c->stream));
    const double t2 = timing ? host_ms() : 0.0;
    HIPCHK(hipStreamSynchronize(c->stream));
    const double t3 = timing ? host_ms() : 0.0;
    struct TimingDone {      /* filled when the call returns, whichever way */
        bool on; double t0, t1, t2, t3; hipEvent_t *ev;
        ~TimingDone() {
            if (!on) return;
            float h2d = 0.f, ker = 0.f, d2h = 0.f;
            (void)hipEventElapsedTime(&h2d, ev[0], ev[1]); (void)hipEventElapsedTime(&ker, ev[1], ev[2]); (void)hipEventElapsedTime(&d2h, ev[2], ev[3]);
            (void)hipGetLastError();
            const double t4 = host_ms();
            g_last_timing[0] = t4 - t0;        /* the whole call                                                     */
            g_last_timing[1] = t1 - t0;        /* packing the inputs into the pinned block (host memcpy)            */
            g_last_timing[2] = t2 - t1;        /* enqueueing: H2D copy, scratch set-up + memsets, the launch, D2H copy */
            g_last_timing[3] = t3 - t2;        /* waiting for the stream                                             */
            g_last_timing[4] = t4 - t3;        /* unpacking the results (host memcpy)                                */
            g_last_timing[5] = h2d;            /* device time line: H2D copy                                         */
            g_last_timing[6] = ker;            /* ... header memsets + the kernel + the copy of its error word       */
            g_last_timing[7] = d2h;            /* ... D2H copy                                                       */
        }
    } tdone{timing, t0, t1, t2, t3, ev};
    const int kerr = *(const int *)(c->h_pin + o_err);
    const int32_t *hst = (const int32_t *)(c->h_pin + o_stats);
    if (kerr) {
        /* A hand-over wait inside the kernel timed out (a time-sliced or debugger-attached GPU can do that): the pairs that ended
         * after it discarded their results and carry bit 10 in stats[15].  Run exactly those again, one launch, without producer
         * or helper workgroups — the result of a pair does not depend on how it was scheduled. */
        if (depth >= 1) { char code[16]; snprintf(code, sizeof code, "%d", kerr);
            set_err("a hand-over between workgroups inside the kernel failed (code %s) and the retry without helpers failed too", code);
                return MI_DEGENSAC_EHIP; }
        std::vector<int> redo;
        for (int p = 0; p < n_pairs; p++) if (hst[(size_t)p * 16 + 15] & 1024) redo.push_back(p);
        memcpy(model, c->h_pin + o_model, (size_t)n_pairs * 72);
        memcpy(mask, c->h_pin + o_mask, total);
        if (stats) memcpy(stats, c->h_pin + o_stats, (size_t)n_pairs * 64);
        if (redo.empty()) return 0;
        const mi_degensac_params p2s = rerun_params(prm, homography);
        std::vector<double> q1, q2, qm(redo.size() * 9); std::vector<int64_t> qo(redo.size() + 1, 0); std::vector<uint32_t> qs(redo.size());
        std::vector<int32_t> qst(redo.size() * 16);
        for (size_t i = 0; i < redo.size(); i++) { const int p = redo[i]; qo[i + 1] = qo[i] + (off[p + 1] - off[p]); qs[i] = seeds[p]; }
        q1.resize((size_t)qo.back() * dim); q2.resize((size_t)qo.back() * dim); std::vector<uint8_t> qk((size_t)qo.back());
        for (size_t i = 0; i < redo.size(); i++) {
            const int p = redo[i]; const size_t cnt = (size_t)(off[p + 1] - off[p]) * dim;
            memcpy(q1.data() + (size_t)qo[i] * dim, p1 + (size_t)off[p] * dim, cnt * sizeof(double));
            memcpy(q2.data() + (size_t)qo[i] * dim, p2 + (size_t)off[p] * dim, cnt * sizeof(double));
        }
        rc = ctx_batch(c, homography, q1.data(), q2.data(), qo.data(), (int)redo.size(), dim, &p2s, qs.data(), qm.data(), qk.data(), qst.data(), depth + 1);
        if (rc) return rc;
        for (size_t i = 0; i < redo.size(); i++) {
            const int p = redo[i];
            memcpy(model + (size_t)p * 9, qm.data() + i * 9, 72);
            memcpy(mask + (size_t)(off[p] - off[0]), qk.data() + (size_t)qo[i], (size_t)(off[p + 1] - off[p]));
            /* bit 11: the pair ran again after a hand-over time-out */
            if (stats) { memcpy(stats + (size_t)p * 16, qst.data() + i * 16, 64); stats[(size_t)p * 16 + 15] |= 2048; }
        }
        return 0;
    }
    memcpy(model, c->h_pin + o_model, (size_t)n_pairs * 72);
    memcpy(mask, c->h_pin + o_mask, total);
    if (stats) memcpy(stats, c->h_pin + o_stats, (size_t)n_pairs * 64);
    return 0;
}

extern "C" int mi_degensac_ctx_find_fundamental_batch(mi_degensac_ctx *c, const double *pts1, const double *pts2, const int64_t *offsets,
        int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *seeds, double *F, uint8_t *mask, int32_t *stats)
{ return ctx_batch(c, 0, pts1, pts2, offsets, n_pairs, dim, prm, seeds, F, mask, stats); }
extern "C" int mi_degensac_ctx_find_homography_batch(mi_degensac_ctx *c, const double *pts1, const double *pts2, const int64_t *offsets,
        int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *seeds, double *H, uint8_t *mask, int32_t *stats)
{ return ctx_batch(c, 1, pts1, pts2, offsets, n_pairs, dim, prm, seeds, H, mask, stats); }

/* The calling thread's own contexts (one per device).  A thread that exits hands its contexts back to a process-wide
 * idle list for the next new thread instead of destroying them: no HIP call is ever made from a thread-exit or
 * process-exit destructor (the runtime may already be gone there). */
static std::mutex g_idle_mu;
static std::vector<mi_degensac_ctx *> g_idle_ctx;
struct ThreadCtxs {
    mi_degensac_ctx *c[64] = {nullptr};
    ~ThreadCtxs() { std::lock_guard<std::mutex> lk(g_idle_mu); for (auto *p : c) if (p) g_idle_ctx.push_back(p); }
};
static int thread_ctx(int device, mi_degensac_ctx **out)
{
    static thread_local ThreadCtxs t;
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    if (!t.c[device]) {
        {
            std::lock_guard<std::mutex> lk(g_idle_mu);
            for (size_t i = 0; i < g_idle_ctx.size(); i++)
                if (g_idle_ctx[i]->device == device) { t.c[device] = g_idle_ctx[i]; g_idle_ctx[i] = g_idle_ctx.back(); g_idle_ctx.pop_back(); break; }
        }
        if (!t.c[device]) { int rc = mi_degensac_ctx_create(device, &t.c[device]); if (rc) return rc; }
    }
    *out = t.c[device];
    return 0;
}
int est_thread_stream(int device, hipStream_t *stream)
{
    mi_degensac_ctx *c; int rc = thread_ctx(device, &c); if (rc) return rc;
    *stream = c->stream;
    return 0;
}
int est_rerun(int device, int homography, const double *p1, const double *p2, const int64_t *off, int n_pairs, int dim, const mi_degensac_params *prm,
              const uint32_t *seeds, double *model, uint8_t *mask, int32_t *stats)
{
    mi_degensac_ctx *c; int rc = thread_ctx(device, &c); if (rc) return rc;
    const mi_degensac_params p2s = rerun_params(prm, homography);
    return ctx_batch(c, homography, p1, p2, off, n_pairs, dim, &p2s, seeds, model, mask, stats, 1);
}

extern "C" int mi_degensac_find_fundamental_batch(const double *pts1, const double *pts2, const int64_t *offsets, int n_pairs, int dim,
        const mi_degensac_params *prm, const uint32_t *seeds, int device, double *F, uint8_t *mask, int32_t *stats)
{ mi_degensac_ctx *c; int rc = thread_ctx(device, &c); if (rc) return rc; return ctx_batch(c, 0, pts1, pts2, offsets, n_pairs, dim, prm, seeds, F, mask, stats);
    }
extern "C" int mi_degensac_find_homography_batch(const double *pts1, const double *pts2, const int64_t *offsets, int n_pairs, int dim,
        const mi_degensac_params *prm, const uint32_t *seeds, int device, double *H, uint8_t *mask, int32_t *stats)
{ mi_degensac_ctx *c; int rc = thread_ctx(device, &c); if (rc) return rc; return ctx_batch(c, 1, pts1, pts2, offsets, n_pairs, dim, prm, seeds, H, mask, stats);
    }

/* ---- one batch over several devices from ONE process (SURVEY 8e: "no collective at all in single-process multi-device mode
 * (host gathers D2H)"): device k gets the k-th contiguous block of pairs (the first n_pairs % n_devices blocks hold one pair
 * more, as pydegensac_amd.parallel.shard_range), one host thread per block stages, launches and copies back through that
 * thread's own context of its device.  Seeds travel with their pairs, so the results do not depend on the device list; a
 * device may be listed more than once (two concurrent launches on it). */
static int batch_multi(int homography, const double *p1, const double *p2, const int64_t *off, int n_pairs, int dim, const mi_degensac_params *prm,
                       const uint32_t *seeds, const int *devices, int n_devices, double *model, uint8_t *mask, int32_t *stats)
{
    if (!devices || n_devices <= 0) { set_err("need at least one device"); return MI_DEGENSAC_EINVAL; }
    if (!p1 || !p2 || !off || !model || !mask || !seeds || !prm) { set_err("NULL argument"); return MI_DEGENSAC_EINVAL; }
    if (n_pairs <= 0) return 0;
    for (int p = 0; p < n_pairs; p++) if (off[p+1] < off[p]) { set_err("offsets must be non-decreasing"); return MI_DEGENSAC_EINVAL; }
    const int ndev = mi_degensac_device_count();
    if (ndev == 0) { set_err("no HIP device: this library has no CPU path"); return MI_DEGENSAC_ENODEV; }
    for (int k = 0; k < n_devices; k++) {
        if (devices[k] < 0 || devices[k] >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
        if (devices[k] >= ndev) { set_err("device index out of range"); return MI_DEGENSAC_ENODEV; }
    }
    auto run = [&](int k, int lo, int hi) -> int {
        return (homography ? mi_degensac_find_homography_batch : mi_degensac_find_fundamental_batch)(
            p1, p2, off + lo, hi - lo, dim, prm, seeds + lo, devices[k], model + (size_t)lo * 9, mask + (size_t)(off[lo] - off[0]),
            stats ? stats + (size_t)lo * 16 : nullptr);
    };
    if (n_devices == 1) return run(0, 0, n_pairs);
    std::vector<int> rcs((size_t)n_devices, 0); std::vector<std::string> errs((size_t)n_devices);
    std::vector<std::thread> th;
    const int base = n_pairs / n_devices, rem = n_pairs % n_devices;
    for (int k = 0; k < n_devices; k++) {
        const int lo = k * base + (k < rem ? k : rem), hi = lo + base + (k < rem ? 1 : 0);
        if (hi <= lo) continue;
        th.emplace_back([&, k, lo, hi] { rcs[(size_t)k] = run(k, lo, hi); if (rcs[(size_t)k]) errs[(size_t)k] = g_err; });
    }
    for (auto &t : th) t.join();
    for (int k = 0; k < n_devices; k++) if (rcs[(size_t)k]) { set_err("%s", errs[(size_t)k].c_str()); return rcs[(size_t)k]; }
    return 0;
}
extern "C" int mi_degensac_find_fundamental_batch_multi(const double *pts1, const double *pts2, const int64_t *offsets, int n_pairs, int dim,
        const mi_degensac_params *prm, const uint32_t *seeds, const int *devices, int n_devices, double *F, uint8_t *mask, int32_t *stats)
{ return batch_multi(0, pts1, pts2, offsets, n_pairs, dim, prm, seeds, devices, n_devices, F, mask, stats); }
extern "C" int mi_degensac_find_homography_batch_multi(const double *pts1, const double *pts2, const int64_t *offsets, int n_pairs, int dim,
        const mi_degensac_params *prm, const uint32_t *seeds, const int *devices, int n_devices, double *H, uint8_t *mask, int32_t *stats)
{ return batch_multi(1, pts1, pts2, offsets, n_pairs, dim, prm, seeds, devices, n_devices, H, mask, stats); }

/* ---- ransacH2el (ranH2el.h:35): one persistent workgroup per CU pulls pairs from the ticket; everything lives in the
 * HBM workspace (dg_kernel_h2el.h).  Asynchronous on `stream`. */
static int launch_h2el(const double *d_u10, const int64_t *d_off, const int64_t *h_off, int n_pairs, const mi_degensac_h2el_params *prm,
                       const uint32_t *d_seeds, int device, hipStream_t stream, double *d_H, uint8_t *d_mask, int32_t *d_stats)
{
    if (n_pairs <= 0) return 0;
    if (!prm) { set_err("params is NULL"); return MI_DEGENSAC_EINVAL; }
    if (!h_off) { set_err("offsets_host is NULL"); return MI_DEGENSAC_EINVAL; }
    if (prm->inl_limit < 0 || (prm->inl_limit > 0 && prm->inl_limit < 4)) { set_err("inl_limit must be 0 (none) or >= 4"); return MI_DEGENSAC_EINVAL; }
    if (!(prm->th > 0)) { set_err("th must be > 0"); return MI_DEGENSAC_EINVAL; }
    if (!(prm->conf > 0 && prm->conf < 1)) { set_err("conf must be in (0, 1)"); return MI_DEGENSAC_EINVAL; }
    if (prm->max_iters <= 0) { set_err("max_iters must be > 0"); return MI_DEGENSAC_EINVAL; }
    /* the kernel writes the model and the mask of every pair (the reference's ransacH2el accepts inl == NULL; here the mask is required) */
    if (!d_u10 || !d_off || !d_seeds || !d_H || !d_mask) { set_err("NULL argument (u10, offsets, seeds, H and mask are required)"); return MI_DEGENSAC_EINVAL; }
    int rc = dev_init(device); if (rc) return rc;
    int n_max = 0, n_min = 1 << 30;
    for (int p = 0; p < n_pairs; p++) {
        const long long n = h_off[p+1] - h_off[p];
        if (n > 0x7fffffff / 64) { set_err("too many correspondences in one pair"); return MI_DEGENSAC_EINVAL; }
        if (n > n_max) n_max = (int)n; if (n < n_min) n_min = (int)n;
    }
    if (n_min < 2) { set_err("need n >= 2 correspondences"); return MI_DEGENSAC_EINVAL; }
    const DevState &ds = g_dev[device];
    dg_args A; memset(&A, 0, sizeof A);
    A.prm.th = prm->th; A.prm.conf = prm->conf; A.prm.max_iters = prm->max_iters;
    A.prm.h2_do_lo = prm->do_lo ? 1 : 0; A.prm.h2_inl_limit = prm->inl_limit;
    const long long grid = n_pairs < ds.cus ? n_pairs : ds.cus;
    A.wl = make_layout(n_max, true, 512 / 64, 0, 0, false);
    std::lock_guard<std::mutex> lk(g_dev_mu[device]);
    char *ws; rc = get_scratch_locked(device, stream, DG_HDR_BYTES + A.wl.stride * (size_t)grid, &ws); if (rc) return rc;
    HIPCHK(hipMemsetAsync(ws, 0, DG_HDR_BYTES, stream));
    A.ticket = (int *)ws; A.park_ctl = (int *)(ws + 128); A.n_res = (int)grid; A.n_ws = (int)grid;
    A.ws = ws + DG_HDR_BYTES;
    A.pts1 = d_u10; A.pts2 = d_u10; A.offsets = (const long long *)d_off; A.seeds = d_seeds;
    A.variant_threads = 512; A.mode = DG_MODE_HBM; A.dim = 10; A.n_pairs = n_pairs;
    A.model_out = d_H; A.mask_out = d_mask; A.stats_out = d_stats;
    hipLaunchKernelGGL(dg_ransac_h2el_kernel, dim3((unsigned)grid), dim3(512), 0, stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int mi_degensac_ransac_h2el_batch_dev(const double *d_u10, const int64_t *d_offsets, const int64_t *offsets_host, int n_pairs,
        const mi_degensac_h2el_params *prm, const uint32_t *d_seeds, int device, void *stream, double *d_H, uint8_t *d_mask, int32_t *d_stats)
{
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    if (mi_degensac_device_count() == 0) { set_err("no HIP device: this library has no CPU path"); return MI_DEGENSAC_ENODEV; }
    DevGuard g; int rc = g.enter(device); if (rc) return rc;
    return launch_h2el(d_u10, d_offsets, offsets_host, n_pairs, prm, d_seeds, device, (hipStream_t)stream, d_H, d_mask, d_stats);
}
/* host pointers: staged through the calling thread's context like the other host-pointer entry points */
extern "C" int mi_degensac_ransac_h2el_batch(const double *u10, const int64_t *off, int n_pairs, const mi_degensac_h2el_params *prm,
        const uint32_t *seeds, int device, double *H, uint8_t *mask, int32_t *stats)
{
    mi_degensac_ctx *c; int rc = thread_ctx(device, &c); if (rc) return rc;
    if (!u10 || !off || !H || !mask || !seeds) { set_err("NULL argument"); return MI_DEGENSAC_EINVAL; }
    if (n_pairs <= 0) return 0;
    for (int p = 0; p < n_pairs; p++) if (off[p+1] < off[p]) { set_err("offsets must be non-decreasing"); return MI_DEGENSAC_EINVAL; }
    DevGuard g; rc = g.enter(c->device); if (rc) return rc;
    const size_t total = (size_t)(off[n_pairs] - off[0]);
    const size_t b_pts = align_up(total * 10 * sizeof(double), 256), b_off = align_up((size_t)(n_pairs + 1) * 8, 256),
                 b_seed = align_up((size_t)n_pairs * 4, 256), b_model = align_up((size_t)n_pairs * 72, 256),
                 b_mask = align_up(total, 256), b_stats = align_up((size_t)n_pairs * 64, 256);
    const size_t o_off = b_pts, o_seed = o_off + b_off, in_bytes = o_seed + b_seed;
    const size_t o_model = in_bytes, o_mask = o_model + b_model, o_stats = o_mask + b_mask, all_bytes = o_stats + b_stats;
    rc = ctx_reserve(c, all_bytes); if (rc) return rc;
    memcpy(c->h_pin, u10 + (size_t)off[0] * 10, total * 10 * sizeof(double));
    int64_t *ho = (int64_t *)(c->h_pin + o_off);
    for (int p = 0; p <= n_pairs; p++) ho[p] = off[p] - off[0];
    memcpy(c->h_pin + o_seed, seeds, (size_t)n_pairs * 4);
    HIPCHK(hipMemcpyAsync(c->d_io, c->h_pin, in_bytes, hipMemcpyHostToDevice, c->stream));
    rc = launch_h2el((const double *)c->d_io, (const int64_t *)(c->d_io + o_off), ho, n_pairs, prm, (const uint32_t *)(c->d_io + o_seed),
                     c->device, c->stream, (double *)(c->d_io + o_model), (uint8_t *)(c->d_io + o_mask), (int32_t *)(c->d_io + o_stats));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->h_pin + o_model, c->d_io + o_model, all_bytes - o_model, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(H, c->h_pin + o_model, (size_t)n_pairs * 72);
    memcpy(mask, c->h_pin + o_mask, total);
    if (stats) memcpy(stats, c->h_pin + o_stats, (size_t)n_pairs * 64);
    return 0;
}

extern "C" int mi_degensac_find_fundamental(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *F, uint8_t *mask, int32_t *stats)
{ int64_t off[2] = {0, n}; return mi_degensac_find_fundamental_batch(pts1, pts2, off, 1, dim, prm, &seed, device, F, mask, stats); }
extern "C" int mi_degensac_find_homography(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *H, uint8_t *mask, int32_t *stats)
{ int64_t off[2] = {0, n}; return mi_degensac_find_homography_batch(pts1, pts2, off, 1, dim, prm, &seed, device, H, mask, stats); }

/* one pair, host pointers, with the per-LO residual dump copied back (diagnostics: plain device buffers per call) */
static int pair_resids(int homography, const double *p1, const double *p2, int n, int dim, const mi_degensac_params *prm, uint32_t seed,
                       int device, double *model, uint8_t *mask, int32_t *stats, double *resids, int resid_runs, int32_t *hist = nullptr)
{
    if (!p1 || !p2 || !model || !mask || (!resids && !hist) || (resids && resid_runs <= 0) || n <= 0) { set_err("bad argument"); return MI_DEGENSAC_EINVAL; }
    if (!resids) resid_runs = 0;
    if (device < 0 || device >= 64) { set_err("bad device index"); return MI_DEGENSAC_EINVAL; }
    if (mi_degensac_device_count() == 0) { set_err("no HIP device: this library has no CPU path"); return MI_DEGENSAC_ENODEV; }
    DevGuard g; int rc = g.enter(device); if (rc) return rc;
    const size_t nr = (size_t)n * resid_runs * 62;
    double *d1 = nullptr, *d2 = nullptr, *dm = nullptr, *dr = nullptr; int64_t *doff = nullptr; uint32_t *ds = nullptr; uint8_t *dk = nullptr;
        int32_t *dst = nullptr, *dh = nullptr;
    struct Free { void **p[9]; ~Free() { for (auto q : p) (void)hipFree(*q);
        } } fr{{(void **)&d1, (void **)&d2, (void **)&dm, (void **)&dr, (void **)&doff, (void **)&ds, (void **)&dk, (void **)&dst, (void **)&dh}};
    HIPCHK(hipMalloc((void **)&d1, (size_t)n * dim * 8)); HIPCHK(hipMalloc((void **)&d2, (size_t)n * dim * 8)); HIPCHK(hipMalloc((void **)&dm, 72));
    HIPCHK(hipMalloc((void **)&dr, nr ? nr * 8 : 8)); HIPCHK(hipMalloc((void **)&doff, 16)); HIPCHK(hipMalloc((void **)&dh, ((size_t)n + 3) * 4));
        HIPCHK(hipMalloc((void **)&ds, 4));
    HIPCHK(hipMalloc((void **)&dk, (size_t)n)); HIPCHK(hipMalloc((void **)&dst, 64));
    const int64_t off[2] = {0, n};
    HIPCHK(hipMemcpy(d1, p1, (size_t)n * dim * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d2, p2, (size_t)n * dim * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(doff, off, 16, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(ds, &seed, 4, hipMemcpyHostToDevice));
    if (nr) HIPCHK(hipMemset(dr, 0xff, nr * 8));               /* runs that never happen read as NaN */
    HIPCHK(hipMemset(dh, 0, ((size_t)n + 3) * 4));
    mi_degensac_diag dg; dg.d_resids = nr ? dr : nullptr; dg.resid_runs = resid_runs; dg.struct_size = (int32_t)sizeof dg; dg.d_hist = hist ? dh : nullptr;
        dg.d_screen = nullptr;
    rc = est_launch_batch(homography, d1, d2, doff, off, 1, dim, prm, ds, device, nullptr, dm, dk, dst, &dg); if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(model, dm, 72, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(mask, dk, (size_t)n, hipMemcpyDeviceToHost));
    if (stats) HIPCHK(hipMemcpy(stats, dst, 64, hipMemcpyDeviceToHost));
    if (nr) HIPCHK(hipMemcpy(resids, dr, nr * 8, hipMemcpyDeviceToHost));
    if (hist) HIPCHK(hipMemcpy(hist, dh, ((size_t)n + 3) * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int mi_degensac_find_fundamental_resids(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *F, uint8_t *mask, int32_t *stats, double *resids, int resid_runs)
{ return pair_resids(0, pts1, pts2, n, dim, prm, seed, device, F, mask, stats, resids, resid_runs); }
extern "C" int mi_degensac_find_homography_resids(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *H, uint8_t *mask, int32_t *stats, double *resids, int resid_runs)
{ return pair_resids(1, pts1, pts2, n, dim, prm, seed, device, H, mask, stats, resids, resid_runs); }
extern "C" int mi_degensac_find_fundamental_hist(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *F, uint8_t *mask, int32_t *stats, int32_t *hist)
{ return pair_resids(0, pts1, pts2, n, dim, prm, seed, device, F, mask, stats, nullptr, 0, hist); }
