/* mi_degensac — C-ABI of the MI355X-native LO-RANSAC / DEGENSAC estimator (libmi_degensac.so).
 *
 * Drop-in boundary for the reference's pybind11 FFI (src/pydegensac/bindings.cpp):
 *   findFundamentalMatrix_  bindings.cpp:253-467  -> mi_degensac_find_fundamental[_batch|_batch_dev]
 *   findHomography_         bindings.cpp:19-251   -> mi_degensac_find_homography[_batch|_batch_dev]
 * which in turn replace the two C drivers those bindings call:
 *   exp_ransacFcustomLAF    degensac/exp_ranF.h:72-74 (exp_ranF.c:1244-1767)
 *   exp_ransacHcustomLAF    degensac/exp_ranH.h:27-33 (exp_ranH.c:470-930)
 *
 * Plain pointers and sizes only; no exceptions cross the boundary; every entry point returns 0 or a
 * negative MI_DEGENSAC_E* code.  Host-pointer entry points stage through device memory themselves;
 * the *_dev entry points take device pointers (HBM-resident inputs/outputs) and a hipStream_t.
 * The whole estimation (sampling, minimal solver, scoring, DEGENSAC test, local optimisation,
 * adaptive termination, final mask) runs in one persistent HIP kernel; workgroups pull image pairs
 * from a device-wide ticket.
 * There is NO CPU fallback: without a usable gfx950 device every call fails with MI_DEGENSAC_ENODEV.
 *
 * Threading (SURVEY 8b "thread-safe handle/context"; the reference is not re-entrant: global
 * HASH_TABLE hash.h:32 + libc RNG).  Every entry point may be called from any number of host
 * threads at once:
 *   - a `mi_degensac_ctx` owns one HIP stream, pinned host staging and its device buffers; calls on
 *     ONE context are serialised by the caller, different contexts are independent;
 *   - the entry points without a context argument use a context private to the calling thread;
 *   - the *_dev entry points are asynchronous on the caller's stream; the per-launch scratch is
 *     private to (device, stream), so launches on different streams never share memory, and the
 *     thread's current HIP device is left as it was found;
 *   - enqueueing is serialised per DEVICE only (launches for different devices never wait for each other);
 *   - launches may overlap on one device, also with other processes' work: no workgroup of these kernels ever waits for
 *     a workgroup that may not have been dispatched.  (Cross-workgroup work — the cooperative mode for one very large
 *     pair, pairs that are set aside and resumed — is handed over through queues and claim counters: whoever is
 *     running takes the next unit, and a wait is only ever for a unit that a RUNNING workgroup has claimed.)
 */
#ifndef MI_DEGENSAC_H
#define MI_DEGENSAC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_DEGENSAC_OK        0
#define MI_DEGENSAC_EINVAL   -1   /* bad shape / argument (bindings.cpp:32-47, :267-282 -> ValueError) */
#define MI_DEGENSAC_ENODEV   -2   /* no HIP device / wrong architecture */
#define MI_DEGENSAC_EHIP     -3   /* HIP runtime error (see mi_degensac_last_error) */
#define MI_DEGENSAC_ENOMEM   -4

/* error_type values: utils.py:15-22, bindings.cpp:10-17 */
#define MI_DEGENSAC_F_SAMPSON        0
#define MI_DEGENSAC_F_SYMM_EPIPOLAR  1
#define MI_DEGENSAC_H_SAMPSON        0
#define MI_DEGENSAC_H_SYMM_SQ_MAX    1
#define MI_DEGENSAC_H_SYMM_MAX       2
#define MI_DEGENSAC_H_SYMM_SQ_SUM    3
#define MI_DEGENSAC_H_SYMM_SUM       4

/* flags */
#define MI_DEGENSAC_FLAG_FINAL_LAF_FILTER 1u  /* apply the F driver's final LAF filter, which the reference
                                                 guards with an uninitialised variable (exp_ranF.c:1254,1725) */

#define MI_DEGENSAC_FLAG_LEGACY_F 2u          /* fundamental matrix: behave like the reference's older drivers exp_ransacF (exp_ranF.c:242)
                                                 and exp_ransacFcustom (:811) instead of exp_ransacFcustomLAF: the sample budget
                                                 follows EVERY new best model, also one found by the main loop or the DEGENSAC
                                                 branch between two local optimisations (:1085-1090 sits outside the LO block
                                                 there).  No LAF check.  symmetric_error_check = 1 gives exp_ransacFcustom's own
                                                 symmetric check: over ALL points, against CHECK_COEF * th = 16 px_th^2, and in
                                                 the final mask against the model the driver computed LAST, not the best one
                                                 (exp_ranF.c:943-953, :1196-1203); error_type 0 without it = exp_ransacF */

/* per-call scheduling switches (results never depend on them).  They win over the process-wide defaults below
 * (mi_degensac_set_stream_mode / mi_degensac_set_hjob_mode and their environment variables): */
#define MI_DEGENSAC_FLAG_NO_STREAM   4u       /* fundamental matrix: no producer workgroups for this call (stream mode off)           */
#define MI_DEGENSAC_FLAG_STREAM_ON   8u       /* fundamental matrix: stream mode on whatever the batch size                            */
#define MI_DEGENSAC_FLAG_STREAM_TEST(b) (((uint32_t)(b) & 3u) << 8)   /* with STREAM_ON: bit 0 = the owner scores every chunk it takes from
                                                 the producer again, bit 1 = pairs ask for a producer even while unstarted pairs remain */
#define MI_DEGENSAC_FLAG_STREAM_AUTO 64u      /* fundamental matrix: the library's automatic choice for this call, whatever the process-wide default says \
 */
#define MI_DEGENSAC_FLAG_HJOB_ON     128u     /* homography: helper workgroups on for this call, whatever the process-wide default says \
 */
#define MI_DEGENSAC_FLAG_NO_HJOB     16u      /* homography: no helper workgroups for the local optimisations of this call             */

/* tuning word (0 = let the library decide; results never depend on it, only speed does):
 *   bits 0-1  kernel variant    1 = latency (512-thread workgroups)   2 = throughput (256-thread, 2 pairs per CU)
 *                               3 = high throughput (128-thread, up to 4 pairs per CU)
 *   bits 2-3  placement         1 = points + sampler pool in HBM      2 = both in LDS      3 = pool in LDS
 *             (a placement that does not fit the device's LDS is ignored)
 *   bit  4    sampler           1 = always use the sequential pool-swap stage
 *   bit  5    homography only: run the ten repetitions of every local optimisation one after the other on the whole
 *             workgroup instead of one repetition per wave (tests; the residual dump of
 *             mi_degensac_find_homography_resids always does).  EINVAL on a fundamental-matrix call
 *   bit  6    fundamental matrix with helper workgroups only (bits 8-15 or automatic): distribute EVERY pass over the whole
 *             point set over the claiming workgroups, not only those over >= 8192 points (tests).  EINVAL on a homography call
 *   bit  7    fundamental matrix only: run the repetitions of the local optimisation (exp_inFranicustom) and of innerH (the
 *             plane homography's local optimisation inside the DEGENSAC branch) one after the other on the whole workgroup
 *             instead of one repetition per wave from speculated generator states (tests).  EINVAL on a homography call
 *   bits 8-15 helper workgroups per pair of the cooperative large-n mode (fundamental matrix, placement HBM):
 *             0 = automatic (23 helpers when n >= 8192 and the batch leaves the device mostly idle, 15 with less room), 255 = off
 *   bits 16-23 setting pairs aside (fundamental matrix, batches larger than the resident grid): a pair still running
 *             after this many samples (units of 256) while unstarted pairs remain is written back to its workspace and
 *             queued; free workgroups take unstarted pairs first, then the queued pairs with many samples left, then
 *             the rest.  The first samples of every pair become a short discovery round after which the pairs with the
 *             most work left restart first, so the batch ends at about (sum of pair times) / (resident workgroups)
 *             instead of one long pair after the last pair was started.  0 = automatic (1024 samples), 255 = off
 *   bits 24-28 cap on the number of resident workgroups (0 = none, 1..31; for tests of the queueing paths on small batches)
 *   bits 29-31 with bits 16-23: a pair set aside with at least (threshold << this) samples left counts as "long" and is
 *             resumed before the others; 0 = automatic (threshold x 8).  EINVAL on a homography call
 * Every field has its own bits; a field that does not apply to the call (see above) is rejected with MI_DEGENSAC_EINVAL
 * rather than silently reinterpreted. */
#define MI_DEGENSAC_TUNE_VARIANT(v)   ((uint32_t)(v) & 3u)
#define MI_DEGENSAC_TUNE_PLACEMENT(p) (((uint32_t)(p) & 3u) << 2)
#define MI_DEGENSAC_TUNE_SEQ_POOL     (1u << 4)
#define MI_DEGENSAC_TUNE_H_SERIAL_LO  (1u << 5)
#define MI_DEGENSAC_TUNE_COOP_ALL_PASSES (1u << 6)
#define MI_DEGENSAC_TUNE_F_SERIAL_REPS (1u << 7)
#define MI_DEGENSAC_TUNE_HELPERS(h)   (((uint32_t)(h) & 255u) << 8)
#define MI_DEGENSAC_TUNE_SET_ASIDE(t)  (((uint32_t)(t) & 255u) << 16)
#define MI_DEGENSAC_TUNE_GRID_CAP(g)   (((uint32_t)(g) & 31u) << 24)
#define MI_DEGENSAC_TUNE_LONG_SHIFT(l) (((uint32_t)(l) & 7u) << 29)

typedef struct mi_degensac_params {
    double   px_th;                    /* pixel threshold (utils.py:76,113)                         */
    double   conf;                     /* confidence for adaptive termination                       */
    int32_t  max_iters;                /* hard cap on minimal samples                               */
    int32_t  error_type;               /* MI_DEGENSAC_F_* / MI_DEGENSAC_H_*                          */
    int32_t  symmetric_error_check;    /* bool                                                      */
    int32_t  enable_degeneracy_check;  /* bool, fundamental only (utils.py:119)                     */
    double   laf_consistensy_coef;     /* <=0: off; needs dim == 6                                  */
    uint32_t flags;
    uint32_t tuning;                   /* MI_DEGENSAC_TUNE_*; 0 = automatic                          */
} mi_degensac_params;

/* per-pair int32 statistics block (the reference computes most of these and drops them:
 * bindings.cpp:242-243, exp_ranF.c:1758-1759, exp_ranH.c:922-927) */
#define MI_DEGENSAC_STATS_LEN 16
enum {
    MI_ST_SAMPLES = 0,      /* minimal samples drawn (data_out[0])                                  */
    MI_ST_LO_RUNS = 1,      /* local optimisations run (data_out[1])                                */
    MI_ST_REJECTED = 2,     /* H: samples rejected before scoring (data_out[2]); F: candidates turned down by the LAF
                               consistency check (S.Ilafs < maxS.Ilafs, exp_ranF.c:1410, :1553, :1681)                 */
    MI_ST_I = 3,            /* inlier count of the returned model (driver return value)             */
    MI_ST_MODELS = 4,       /* models scored against all N points through the metric pointers       */
    MI_ST_DEGEN = 5,        /* F: DEGENSAC plane-and-parallax completions                           */
    MI_ST_IH = 6,           /* F: largest H-inlier count seen (exp_ranF.c *Ih)                      */
    MI_ST_BEST_SAMPLE = 7,  /* sample number at which the returned model was committed              */
    MI_ST_FULL_PASSES = 8, MI_ST_EX_PASSES = 9, MI_ST_H_PASSES = 10, MI_ST_AUX_PASSES = 11,
    MI_ST_TICKS_BEST = 12,  /* 100 MHz device wall-clock ticks from the pair's start to that commit; the time a pair waits
                               while it is set aside (batches) is not counted: ticks = time it was being worked on */
    MI_ST_TICKS_TOTAL = 13, /* ... to the pair's end                                                */
    MI_ST_THREADS = 14,     /* workgroup size of the kernel variant that ran (512 / 256 / 128)      */
    MI_ST_PLACEMENT = 15    /* bits 0-7: 0 = points + pool in HBM, 1 = both in LDS, 2 = pool in LDS; bit 8: the pair was set aside once;
                               bit 9: its chunks came from a producer workgroup (stream mode); bit 10: a hand-over wait of the launch
                               timed out before this pair ended and its results were DISCARDED (zero model, all-zero mask, I = 0) —
                               the asynchronous *_dev entry points report the failure this way, the host-pointer entry points run
                               such pairs again without producers / helpers and set bit 11 on the pairs they re-ran */
};

/* Stream mode (fundamental matrix): a pair hands the outcome-independent part of its main loop (sample stream, 7-point
 * solves, screening / scoring) to a workgroup that has run out of pairs; results never depend on it.  Every pair of a launch that
 * uses the mode (automatic: batches of at most two pairs per resident workgroup) posts its request with its first chunk; idle
 * workgroups take the request with the most samples left, the oldest first.  MI_DEGENSAC_STREAM_MIN_SAM=<n> (environment, read
 * once) makes pairs ask only after n samples; MI_DEGENSAC_STREAM_DEPTH=<chunks> bounds the ring.
 * mode: -1 = automatic (default), 0 = off, values > 0 = on with test bits in (mode >> 1): bit 0 = the owner scores every chunk
 * it takes from the producer again, bit 1 = pairs ask for a producer even while unstarted pairs remain.  This is the process-wide
 * DEFAULT (returns the previous one; environment: MI_DEGENSAC_STREAM); a call chooses for itself with MI_DEGENSAC_FLAG_NO_STREAM /
 * MI_DEGENSAC_FLAG_STREAM_ON in params.flags. */
int mi_degensac_set_stream_mode(int mode);      /* any mode > 0 turns the mode on; its test bits are (mode >> 1).  Default of the calls that
                                                   set none of MI_DEGENSAC_FLAG_NO_STREAM / _STREAM_ON / _STREAM_AUTO and run on a context
                                                   without its own setting (mi_degensac_ctx_set_scheduling): process-wide, kept for the
                                                   entry points that take no context */
/* Homography: workgroups that have run out of pairs take whole repetitions of the local optimisations of the pairs that still
 * run (results never depend on it).  1 = on (default), 0 = off.  Process-wide DEFAULT (returns the previous one; environment:
 * MI_DEGENSAC_HJOB); a call switches them off for itself with MI_DEGENSAC_FLAG_NO_HJOB in params.flags. */
int mi_degensac_set_hjob_mode(int mode);        /* default of the calls that do not set MI_DEGENSAC_FLAG_NO_HJOB */
/* Hand-overs between workgroups (stream mode, homography helpers, the cooperative large-n mode) never wait for a workgroup that
 * may not have been dispatched.  Every wait for a RUNNING workgroup — the stream mode's data waits, the owner's wait for the
 * repetitions its homography helpers claimed, the cooperative mode's waits for claimed units — gives up after the same limit, 4 s of
 * device wall clock (dg_wait_count / dg_stream_wait).  The launch then raises its error word, every pair that ends afterwards
 * discards its results (MI_ST_PLACEMENT bit 10: zero model, all-zero mask, I = 0), and the host-pointer entry points run those pairs
 * again in a second launch without producers / helpers (bit 11) instead of failing the call.  The asynchronous *_dev entry points
 * cannot do that: their ONLY report of a discarded pair is bit 10 of its stats block, so a caller that wants to tell "discarded" from
 * "no model found" must pass d_stats (with d_stats = NULL both read as a zero model).  (One wait is not a hand-over and has no limit:
 * an idle helper workgroup of the cooperative mode sleeping until its owner publishes the next stage or retires the slot.)
 * Test hook: the limit in 100 MHz ticks (0 = fault injection: every such wait fails at once; < 0 restores the default); returns the
 * previous limit. */
long long mi_degensac_set_wait_ticks(long long ticks);
/* Memory: the library caches one scratch buffer per (device, stream): one workspace per resident workgroup (about 0.65 MB at
 * n = 2000) plus, for fundamental-matrix batches larger than the resident grid, one spare workspace per queued pair (within half
 * of the free memory, at most 24 GB) and, in stream mode, one ring of at most 512 chunk entries of 13.5 KB per resident workgroup
 * (within a quarter of the free memory, at most 8 GB; about 2.7 GB at the default max_iters on a whole device).  A buffer more
 * than four times larger than eight launches in a row needed is given back; mi_degensac_release_scratch frees it at once. */

/* ---- contexts ---------------------------------------------------------------------------------- */
typedef struct mi_degensac_ctx mi_degensac_ctx;
int  mi_degensac_ctx_create(int device, mi_degensac_ctx **out);
void mi_degensac_ctx_destroy(mi_degensac_ctx *ctx);
/* the context's stream (hipStream_t), e.g. to order other work after a call */
void *mi_degensac_ctx_stream(mi_degensac_ctx *ctx);
/* Scheduling defaults of ONE context (results never depend on them): every call on `ctx` whose params.flags say nothing about the stream
 * mode / the homography helpers takes these instead of the process-wide defaults of mi_degensac_set_stream_mode / _set_hjob_mode (which
 * remain for the entry points without a context).  stream_mode: -2 = inherit the process-wide default (initial), -1 = automatic,
 * 0 = off, > 0 = on with test bits in (mode >> 1).  hjob_mode: -2 = inherit (initial), 0 = off, 1 = on.  Returns 0 or MI_DEGENSAC_EINVAL. */
int mi_degensac_ctx_set_scheduling(mi_degensac_ctx *ctx, int stream_mode, int hjob_mode);

/* ---- host-pointer entry points (mirror the pybind signatures) -------------------------------- */
/* pts1, pts2: [n, dim] row-major float64, dim in {2, 6}; F/H: 9 doubles row-major as the reference's C
 * driver returns them (H is the internal image2->image1 column-wise form; the Python layer applies
 * inv(H.T), utils.py:108); mask: n bytes (0/1); stats: MI_DEGENSAC_STATS_LEN int32 or NULL. */
int mi_degensac_find_fundamental(const double *pts1, const double *pts2, int n, int dim,
                                 const mi_degensac_params *prm, uint32_t seed, int device,
                                 double *F, uint8_t *mask, int32_t *stats);
int mi_degensac_find_homography(const double *pts1, const double *pts2, int n, int dim,
                                const mi_degensac_params *prm, uint32_t seed, int device,
                                double *H, uint8_t *mask, int32_t *stats);

/* ---- batches of independent pairs (ragged): pair p owns rows offsets[p] .. offsets[p+1] ------- */
int mi_degensac_find_fundamental_batch(const double *pts1, const double *pts2, const int64_t *offsets,
                                       int n_pairs, int dim, const mi_degensac_params *prm,
                                       const uint32_t *seeds, int device,
                                       double *F /*[n_pairs*9]*/, uint8_t *mask /*[offsets[n_pairs]]*/,
                                       int32_t *stats /*[n_pairs*16] or NULL*/);
int mi_degensac_find_homography_batch(const double *pts1, const double *pts2, const int64_t *offsets,
                                      int n_pairs, int dim, const mi_degensac_params *prm,
                                      const uint32_t *seeds, int device,
                                      double *H, uint8_t *mask, int32_t *stats);
/* ONE batch over several devices from one process (no collective: the host gathers): device devices[k] gets the k-th contiguous
 * block of pairs (blocks as even as possible, the first n_pairs % n_devices hold one pair more), one host thread per block;
 * seeds travel with their pairs, so results do not depend on the device list.  A device may be listed more than once. */
int mi_degensac_find_fundamental_batch_multi(const double *pts1, const double *pts2, const int64_t *offsets, int n_pairs, int dim,
                                             const mi_degensac_params *prm, const uint32_t *seeds, const int *devices, int n_devices,
                                             double *F, uint8_t *mask, int32_t *stats);
int mi_degensac_find_homography_batch_multi(const double *pts1, const double *pts2, const int64_t *offsets, int n_pairs, int dim,
                                            const mi_degensac_params *prm, const uint32_t *seeds, const int *devices, int n_devices,
                                            double *H, uint8_t *mask, int32_t *stats);
/* the same on an explicit context (its device, its stream, its staging buffers); blocking */
int mi_degensac_ctx_find_fundamental_batch(mi_degensac_ctx *ctx, const double *pts1, const double *pts2,
                                           const int64_t *offsets, int n_pairs, int dim,
                                           const mi_degensac_params *prm, const uint32_t *seeds,
                                           double *F, uint8_t *mask, int32_t *stats);
int mi_degensac_ctx_find_homography_batch(mi_degensac_ctx *ctx, const double *pts1, const double *pts2,
                                          const int64_t *offsets, int n_pairs, int dim,
                                          const mi_degensac_params *prm, const uint32_t *seeds,
                                          double *H, uint8_t *mask, int32_t *stats);

/* ---- device-pointer entry points: everything except `offsets_host` and `prm` lives in HBM ----- */
/* `stream` is a hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing; never
 * synchronises the device.
 * d_offsets holds ABSOLUTE row numbers into d_pts1, d_pts2 and d_mask, so with d_offsets[0] > 0 the three pointers stay the bases of the
 * whole store, pair p reads rows d_offsets[p] .. d_offsets[p+1] and writes those mask bytes, while d_F / d_H, d_stats and d_seeds are
 * indexed by p from 0.  Nothing is written outside the owned mask ranges and the n_pairs model and stats blocks.  A pair without a
 * model leaves a zero model and an all-zero mask whatever the buffers held before the call.  d_stats may be NULL; every other pointer
 * is required (a NULL one is MI_DEGENSAC_EINVAL when n_pairs > 0; n_pairs <= 0 returns 0 and touches nothing).  offsets_host must hold
 * the same n_pairs + 1 values as d_offsets (the launch and its workspace are sized from it). */
int mi_degensac_find_fundamental_batch_dev(const double *d_pts1, const double *d_pts2,
                                           const int64_t *d_offsets, const int64_t *offsets_host,
                                           int n_pairs, int dim, const mi_degensac_params *prm,
                                           const uint32_t *d_seeds, int device, void *stream,
                                           double *d_F, uint8_t *d_mask, int32_t *d_stats);
int mi_degensac_find_homography_batch_dev(const double *d_pts1, const double *d_pts2,
                                          const int64_t *d_offsets, const int64_t *offsets_host,
                                          int n_pairs, int dim, const mi_degensac_params *prm,
                                          const uint32_t *d_seeds, int device, void *stream,
                                          double *d_H, uint8_t *d_mask, int32_t *d_stats);
/* ---- RANSAC on ellipse-to-ellipse correspondences: the reference's ransacH2el (degensac/ranH2el.h:35, ranH2el.c:19-206;
 * no binding in the reference's Python layer — this is its C signature with the allocation-free device conventions of
 * the entry points above).  u10: [total, 10] doubles, per correspondence x1 y1 a1 b1 c1 | x2 y2 a2 b2 c2 with the local
 * affine frame [a 0; b c] of each image; a sample is TWO correspondences (14 x 15 system of Chum & Matas, ICPR 2012).
 * H (9 doubles per pair, column-wise like the reference's internal H) maps image 2 to image 1; mask[j] = HDs residual of
 * the returned model <= th (ranH2el.c:189-198).  stats as for the other drivers ([0] samples, [1] LO runs, [3] I).
 * Device entry: d_offsets holds ABSOLUTE row numbers into d_u10 and d_mask, so with d_offsets[0] > 0 both pointers stay the bases of the
 * whole store, pair p reads rows d_offsets[p] .. d_offsets[p+1] and writes those mask bytes and nothing outside them, while d_H, d_stats
 * (may be NULL) and d_seeds are indexed by p from 0; offsets_host must hold the same n_pairs + 1 values as d_offsets (the workspace is
 * sized from it). */
typedef struct mi_degensac_h2el_params {
    double   th;          /* threshold on the squared transfer error HDs returns (the reference's `th`)       */
    double   conf;        /* confidence of the sample-count rule (nsamples with sample size 2)                  */
    int32_t  max_iters;   /* max_sam                                                                            */
    int32_t  do_lo;       /* bool: local optimisation (inHraniEl)                                               */
    int32_t  inl_limit;   /* inlLimit: correspondences per least-squares fit inside the LO; 0 = all (>= 4 else)  */
    int32_t  reserved;
} mi_degensac_h2el_params;
int mi_degensac_ransac_h2el_batch(const double *u10, const int64_t *offsets, int n_pairs,
                                  const mi_degensac_h2el_params *prm, const uint32_t *seeds, int device,
                                  double *H, uint8_t *mask, int32_t *stats);
int mi_degensac_ransac_h2el_batch_dev(const double *d_u10, const int64_t *d_offsets, const int64_t *offsets_host, int n_pairs,
                                      const mi_degensac_h2el_params *prm, const uint32_t *d_seeds, int device, void *stream,
                                      double *d_H, uint8_t *d_mask, int32_t *d_stats);

/* release the scratch cached for (device, stream) pairs whose work has completed (all of them when
 * `stream_or_null` is NULL, else only that stream's); call before destroying a stream */
int mi_degensac_release_scratch(int device, void *stream_or_null);

/* ---- structured diagnostics ----------------------------------------------------------------
 * The reference's drivers fill a residual dump per local-optimisation run and the binding throws it away
 * (`double *resids`, exp_ranF.c:1503-1511 / :776-779 / :670-672 / :729-730, exp_ranH.c:679-698 / :445-446 / :344 /
 * :400; freed at bindings.cpp:242-243, :458-459).  Per LO run RESIDS_M = 62 rows of n residuals (rtools.h:15):
 *   row 0      the so-far-the-best sample's model (errs[4])        row 1      the least-squares model before the LO
 *   row 2+6i   repetition i: the model of its random subset        rows 3+6i .. 6+6i  its inner iterations (LO metric)
 *   row 7+6i   its final full-metric pass
 * resids[(pair_offset * resid_runs + run * n) * 62 + row * n + j]; rows the reference never writes for a run (early
 * exits: it leaves them uninitialised) are NaN here, rows it memsets keep its byte pattern (0 for F, 0xFF for H); the
 * after-loop LO of the F driver leaves row 0 NaN.  LO runs beyond resid_runs are not recorded. */
#define MI_DEGENSAC_RESIDS_M 62
typedef struct mi_degensac_diag {
    double  *d_resids;        /* device buffer of total_points * resid_runs * 62 doubles, or NULL              */
    int32_t  resid_runs;      /* LO runs per pair the buffer has room for                                     */
    int32_t  struct_size;     /* sizeof(mi_degensac_diag) of the caller's header.  0 (what callers built against the first layout
                                 pass in this field, then called `reserved`) = the layout that ends at d_hist: d_screen is NOT read.
                                 Fields added later are only read when struct_size covers them.                                */
    int32_t *d_hist;          /* fundamental matrix only: the drivers' `data_out` (exp_ranF.c:1495, :1758-1759; allocated and freed at
                                 bindings.cpp:412, :459): per pair n + 3 ints at d_hist[offsets[pair] + 3 * pair]: [0] samples drawn,
                                 [1] LO runs, [2 + I] number of samples whose best model had I inliers.  Device buffer of
                                 total_points + 3 * n_pairs ints, or NULL.  Every model is scored exactly when this is set (the
                                 screening passes are skipped): results are unchanged, the call is slower.               */
    int32_t *d_screen;        /* fundamental matrix only: per pair 4 ints at d_screen[4 * pair]: the models of the main loop's scoring phase
                                 (every chunk the pair's own workgroup scored, including samples speculated past the final budget) by the
                                 arithmetic they got: [0] entered the level-1 screen (single precision, two points per instruction),
                                 [1] entered the level-2 screen (double precision, the point's own denominator), [2] scored with the exact
                                 metric in the reference's operation order, [3] all of them.  MI_ST_MODELS counts every one of [3] (minus
                                 the speculated tail) as a reference-equivalent "model scored" although only [2] ran the exact arithmetic
                                 over all points.  Device buffer of 4 * n_pairs ints, or NULL; costs nothing measurable.            */
} mi_degensac_diag;
int mi_degensac_find_fundamental_batch_dev_ex(const double *d_pts1, const double *d_pts2, const int64_t *d_offsets,
        const int64_t *offsets_host, int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
        void *stream, double *d_F, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag /*nullable*/);
int mi_degensac_find_homography_batch_dev_ex(const double *d_pts1, const double *d_pts2, const int64_t *d_offsets,
        const int64_t *offsets_host, int n_pairs, int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device,
        void *stream, double *d_H, uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag /*nullable*/);
/* one pair, host pointers: resids[resid_runs * 62 * n] */
int mi_degensac_find_fundamental_resids(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *F, uint8_t *mask, int32_t *stats /*nullable*/, double *resids, int resid_runs);
int mi_degensac_find_homography_resids(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *H, uint8_t *mask, int32_t *stats /*nullable*/, double *resids, int resid_runs);
/* one pair, host pointers: hist[n + 3] (see mi_degensac_diag.d_hist) */
int mi_degensac_find_fundamental_hist(const double *pts1, const double *pts2, int n, int dim, const mi_degensac_params *prm,
        uint32_t seed, int device, double *F, uint8_t *mask, int32_t *stats /*nullable*/, int32_t *hist);

/* ---- tentative correspondences: the stage in front of the estimators -------------------
 * Replaces the matcher calls of the reference's example, examples/simple-example.py:46-53
 * (cv2.BFMatcher().knnMatch(descs1, descs2, k=2) followed by `m.distance < 0.9 * n.distance`):
 * brute-force 2-nearest-neighbour search of every row of desc1 among the rows of desc2, the
 * second-nearest-neighbour ratio test and an optional mutual-nearest-neighbour check.
 *   norm L2:      float32 descriptors [n, dim]; distance = sqrt(sum_k (a_k - b_k)^2), fp32, summed in ascending k
 *   norm HAMMING: uint8 descriptors [n, dim] with dim % 4 == 0 (pad with zero bytes); distance = differing bits
 *   norm L2_U8:   uint8 descriptors [n, dim] with dim % 4 == 0 (pad with zero bytes on both sides: they add nothing) and
 *                 dim <= MI_DEGENSAC_L2_U8_MAX_DIM (SIFT / RootSIFT x 512, quantised HardNet / SOSNet / SuperPoint);
 *                 S = sum_k (a_k - b_k)^2 as an exact integer (int8 matrix cores in the dense matcher), distance = sqrtf((float)S),
 *                 ranking by (S, lower index).  S <= 256 * 255^2 < 2^24, so S is exact in fp32 too and idx / dist are bit for bit
 *                 those of norm L2 on the same rows cast to float32.  No non-finite cases.  Wider rows: cast to float32, norm L2.
 * idx[i] = the two nearest train rows of query i (ties: lower index first; -1 when desc2 has fewer rows),
 * dist[i] their distances, keep[i] = dist[i][0] < ratio * dist[i][1] (and, with mutual, the nearest neighbour of
 * desc2[idx[i][0]] in desc1 is i). */
#define MI_DEGENSAC_NORM_L2       0
#define MI_DEGENSAC_NORM_HAMMING  1
#define MI_DEGENSAC_NORM_L2_U8    4     /* (2 and 3 are not norms: MI_DEGENSAC_EINVAL) */
#define MI_DEGENSAC_L2_U8_MAX_DIM 256
int mi_degensac_match(int norm, const void *desc1, int n1, const void *desc2, int n2, int dim, float ratio, int mutual,
                      int device, int32_t *idx /*[n1,2]*/, float *dist /*[n1,2]*/, uint8_t *keep /*[n1], nullable*/);
/* Non-finite distances (L2 only; a Hamming distance is always finite): a train row whose distance to the query is NaN or +inf —
 * NaN or +-inf in either descriptor row, or finite rows whose fp32 sum of squares overflows — is NOT a neighbour.  It takes no
 * slot of idx; a query left with fewer than two finite distances gets idx = -1 / dist = inf in the free slots, exactly as with
 * fewer than two train rows, and such a slot never passes the ratio test or the mutual check.  The same rule holds in
 * mi_degensac_match_knn2_batch_dev and, for the rows that pass the gate, in the guided entry points; oracle/matcher_np.py
 * (top2) states it for the tests. */
/* device pointers, asynchronous on `stream` */
int mi_degensac_match_knn2_dev(int norm, const void *d_desc1, int n1, const void *d_desc2, int n2, int dim, int device,
                               void *stream, int32_t *d_idx, float *d_dist);
int mi_degensac_match_filter_dev(const int32_t *d_idx, const float *d_dist, int n1, float ratio,
                                 const int32_t *d_back_idx_or_null /*[n2,2]: knn2 of desc2 in desc1*/, int device, void *stream,
                                 uint8_t *d_keep);
/* utils.py:24-41 convert_cv2_kpts_to_xyA on the device: kpts [n,4] float32 = (pt.x, pt.y, size, angle in degrees) ->
 * out [n,6] float64 = (x, y, s cos a, s sin a, -s sin a, s cos a), the LAF rows of the estimators' [n,6] input */
int mi_degensac_kpts_to_xyA(const float *kpts, int n, int device, double *out);
int mi_degensac_kpts_to_xyA_dev(const float *d_kpts, int n, int device, void *stream, double *d_out);
const char *mi_degensac_match_last_error(void);

/* ---- float descriptors -> the uint8 rows of MI_DEGENSAC_NORM_L2_U8, on the device ---------------------------------------
 * Every extractor emits float32 descriptors; norm L2_U8 takes bytes.  This is the conversion, with its rounding, clamping, padding
 * and its zero / NaN rows fixed here.  in: float32 [n, dim], 1 <= dim <= MI_DEGENSAC_L2_U8_MAX_DIM, rows dim floats apart;
 * out: uint8 [n, out_dim] with out_dim = (dim + 3) & ~3, the width the L2_U8 entry points take.
 * The arithmetic is fp64 throughout, one IEEE operation per step and no FMA contraction.  Per row, x_k = (double)in[k]:
 *   normalize 0 (none):     y_k = x_k
 *   normalize 1 (L2):       s = sum_k x_k^2,  y_k = x_k / sqrt(s)                      (a division, not a reciprocal multiply)
 *   normalize 2 (L1-root):  s = sum_k |x_k|,  y_k = copysign(sqrt(|x_k| / s), x_k)     (RootSIFT)
 *   v_k = rint(scale * y_k) + offset   (round half to even, no + 0.5),   q_k = v_k clamped to 0 .. 255
 * Summation order of s: think of 64 lanes, lane i owning columns 4 i .. 4 i + 3.  Each lane adds the terms of its own columns below
 * dim in ascending order, starting from +0.0 (a lane without columns holds +0.0); then, for m = 32, 16, 8, 4, 2, 1 in this order,
 * every lane i replaces its value by (its value) + (the value lane i ^ m held before the step).  All lanes end with the same s.
 * Pad columns dim .. out_dim - 1 are written as 0 (zero bytes on both sides add nothing to the distance).
 * clipped [n] int32 (optional): the number of columns of the row whose v_k lay outside 0 .. 255.
 * Dead rows: a row with a non-finite x_k, or with normalize != 0 and s == 0, gets `offset` in every column below dim and
 * clipped = -1: a constant descriptor.  No NaN is ever cast to an integer.
 * Distances: an L2_U8 distance between two quantised rows is about `scale` times the float distance of the normalised rows (each
 * byte is within 1/2 of scale * y_k, clamping apart; a common offset cancels in every difference), so a max_dist stated in float
 * units is multiplied by scale.
 * Errors, with a message in mi_degensac_match_last_error() and before a device is looked for: MI_DEGENSAC_EINVAL for dim < 1 or
 * dim > 256, n < 0, NULL qp / input / output when n > 0, normalize outside 0 .. 2, a scale that is not finite or <= 0, an offset
 * outside 0 .. 255, a struct_size that does not cover offset, and (_dev) a device pointer that is not 4-byte aligned (a row's output
 * is written as 32-bit words).  n == 0 succeeds and touches nothing.  The _dev form is asynchronous on `stream`, allocates nothing
 * and never synchronises; it reads 16 bytes per lane when dim % 4 == 0 and d_desc is 16-byte aligned, single floats otherwise. */
#define MI_DEGENSAC_QUANT_NONE   0
#define MI_DEGENSAC_QUANT_L2     1
#define MI_DEGENSAC_QUANT_L1ROOT 2
typedef struct {
    int    struct_size;    /* sizeof(mi_degensac_quant_params) of the caller's header; has to cover offset */
    int    normalize;      /* MI_DEGENSAC_QUANT_* */
    double scale;          /* finite and > 0: 512 for SIFT / RootSIFT, 256 with offset 128 for signed unit-norm descriptors */
    int    offset;         /* 0 .. 255 */
} mi_degensac_quant_params;
int mi_degensac_desc_quantize_dev(const mi_degensac_quant_params *qp, const float *d_desc, int64_t n, int dim, int device,
                                  void *stream, uint8_t *d_out /*[n, out_dim]*/, int32_t *d_clipped_or_null /*[n]*/);
int mi_degensac_desc_quantize(const mi_degensac_quant_params *qp, const float *desc, int64_t n, int dim, int device,
                              uint8_t *out /*[n, out_dim]*/, int32_t *clipped_or_null /*[n]*/);
/* the rows one pass of the largest grid of mi_degensac_desc_quantize_dev covers at this width (more rows are reached by its
 * grid-stride loop; tests size a case just beyond it); 0 for a dim outside 1 .. 256 */
int64_t mi_degensac_desc_quantize_pass_rows(int dim);

/* ---- batched match-and-verify: many image pairs from descriptors to F / H -------------------------------------------
 * A ragged batch of K image pairs: pair p owns the rows offsets1_host[p] .. offsets1_host[p+1] of desc1 / kp1 (its queries) and
 * offsets2_host[p] .. offsets2_host[p+1] of desc2 / kp2 (its train set); offsets are host arrays of K + 1 non-decreasing values.
 *
 * The batched 2-NN: for every query the two nearest train rows OF ITS OWN PAIR, in one launch over all pairs (64-query tiles;
 * the train set is split over more workgroups only when the batch is too small to fill the device).  d_idx / d_dist:
 * [offsets1_host[K], 2]; indices are local to the pair (0 .. n2_p - 1).  Per pair bit-identical to mi_degensac_match_knn2_dev
 * on that pair (-1 / inf when the pair has fewer than two train rows).  Asynchronous on `stream`. */
int mi_degensac_match_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                     const int64_t *offsets2_host, int n_pairs, int dim, int device, void *stream,
                                     int32_t *d_idx, float *d_dist);
/* The batched 2-NN with the first-geometrically-inconsistent-neighbour rule (FGINN, Mishkin et al.) for slot 1.  Detectors emit
 * several keypoints for one image structure (two orientations, neighbouring scales) with nearly equal descriptors; the second
 * neighbour of a correct match is then its twin and the ratio test fails.  d_kp2: [offsets2_host[K], kp_dim] float64 keypoints of
 * the train rows, kp_dim 2 or 6 (only x, y are read).  Per query of a pair, with r = spatial_th:
 *   slot 0 = (i0, d0) of mi_degensac_match_knn2_batch_dev, unchanged (non-finite rule and tie order included);
 *   a train row t competes for slot 1 iff t != i0 and dx dx + dy dy >= r r, dx = x2[t] - x2[i0], dy = y2[t] - y2[i0], in fp64 in
 *            that order without contraction; a NaN makes the comparison false, so a NaN anchor keypoint leaves no competitor (infinite
 *            coordinates follow the same arithmetic: inf - inf is NaN, inf - finite squares to inf and competes);
 *   slot 1 = the nearest competing row in the matcher's (distance, index) order, its distance bits those of the dense matcher;
 *            -1 / inf when nothing competes or i0 = -1.
 * r = 0 with finite keypoints is mi_degensac_match_knn2_batch_dev bit for bit.  The ratio test on the result is unchanged
 * (i1 >= 0 && d0 < ratio d1: a query whose every other train row lies inside the radius is not kept); so is the mutual check (the
 * plain reverse nearest neighbour).  Cost: the plain 2-NN, a pass over its output, and a rescan of the queries whose plain second
 * neighbour lies inside the radius.  Asynchronous on `stream`, no host synchronisation.  Errors: as
 * mi_degensac_match_knn2_batch_dev, and MI_DEGENSAC_EINVAL for kp_dim not 2 / 6 or a spatial_th that is negative or not finite
 * (before a device is looked for); n_pairs == 0 returns 0. */
int mi_degensac_match_fginn_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                           const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp2, int kp_dim,
                                           double spatial_th, int device, void *stream, int32_t *d_idx, float *d_dist);
typedef struct mi_degensac_match_params {
    int32_t norm;          /* MI_DEGENSAC_NORM_L2 (float32 rows) / _HAMMING (uint8 rows, dim % 4 == 0) / _L2_U8 (uint8 rows,
                              dim % 4 == 0, dim <= 256)                                                                 */
    int32_t dim;           /* descriptor length (elements)                                                              */
    float   ratio;         /* tentative when dist[0] < ratio * dist[1]; finite and > 0                                   */
    int32_t mutual;        /* bool: also require that the query is the nearest neighbour of its nearest train row         */
    int32_t struct_size;   /* sizeof(mi_degensac_match_params) of the caller's header (0 = this layout); fields added later
                              are only read when struct_size covers them                                                  */
    int32_t second_nn;     /* where dist[1] of the ratio test comes from: 0 = the second nearest train row, 1 = FGINN, the nearest
                              train row whose keypoint lies at least spatial_th from the nearest neighbour's (see
                              mi_degensac_match_fginn_knn2_batch_dev).  Read only together with spatial_th                   */
    double  spatial_th;    /* FGINN radius in pixels, finite and >= 0.  Added after the first layout: a caller whose struct_size
                              is 0 or does not cover it gets second_nn = 0 whatever that field holds                        */
    int32_t decide;        /* the decision rule, MI_DEGENSAC_DECIDE_* bit flags (below); 0 = the ratio test above.  Read, with
                              max_dist, only when struct_size covers both (40): a caller whose struct_size is 0, 24 or 32 gets
                              the rule above whatever these bytes hold                                                      */
    float   max_dist;      /* with MI_DEGENSAC_DECIDE_MAX_DIST: the largest dist[0] of a tentative, finite and >= 0; not read
                              without that bit                                                                              */
} mi_degensac_match_params;
/* The decision rule: which queries of a 2-NN result become tentatives.  Every entry point that reads mp->ratio reads it from the same
 * struct (no twins); the data is what the searches already leave on the device: idx / dist of the forward 2-NN and, with mutual, bidx /
 * bdist of the reverse one (16 bytes per train row).  With j = idx[i][0], query i is a tentative when ALL of these hold:
 *   slot 0 exists                 j >= 0
 *   the forward ratio test        idx[i][1] >= 0 && dist[i][0] < ratio * dist[i][1]   (fp32 product, strict), unless NO_RATIO.  In the
 *                                 guided entry points a missing slot 1 has dist = inf and passes: nothing competes
 *   the mutual check              bidx[j][0] == i, when mp->mutual != 0
 *   the reverse ratio test        bidx[j][1] >= 0 && bdist[j][0] < ratio * bdist[j][1]  (the same fp32 product and strict <, at the
 *                                 train row's own reverse search), with BACK_RATIO.  Guided form as above: a missing slot 1 passes
 *   the distance threshold        dist[i][0] <= max_dist  (fp32, NOT strict, in the unit of the returned dist: the square-rooted L2
 *                                 distance, or Hamming bits), with MAX_DIST
 * NO_RATIO: no ratio test at all; a second train row is not needed, so a pair with exactly one train row can match, and mp->ratio is
 *   not read.  NO_RATIO alone is nearest-neighbour matching, with mutual it is mutual-nearest-neighbour matching.
 * BACK_RATIO needs mutual != 0 (the reverse search is the mutual check's); with it the ratio test holds in both directions.
 * Refused with MI_DEGENSAC_EINVAL and a message, before a device is looked for: a bit other than these three; NO_RATIO | BACK_RATIO;
 * BACK_RATIO without mutual; NO_RATIO or BACK_RATIO together with an honoured second_nn = 1 (FGINN defines a second neighbour for the
 * forward test only; MAX_DIST with FGINN is allowed); with MAX_DIST a max_dist that is negative or not finite.  A zero-initialised
 * struct of this size is the rule of decide = 0, and with decide = 0 every output of every call is bit for bit what it was. */
#define MI_DEGENSAC_DECIDE_NO_RATIO   1
#define MI_DEGENSAC_DECIDE_BACK_RATIO 2
#define MI_DEGENSAC_DECIDE_MAX_DIST   4
/* The dense calls under a rule (mi_degensac_match / mi_degensac_match_filter_dev take scalars and stay as they are).
 * mi_degensac_match_decide_dev: d_keep[i] = the decision above on a 2-NN result on the device; mp->norm / dim / second_nn are not read
 * (the rule judges whatever slot 1 holds, so MAX_DIST on an FGINN result is fine).  The mutual check runs when mp->mutual != 0 and
 * then needs d_back_idx ([n2, 2]: the 2-NN of desc2 in desc1), BACK_RATIO needs d_back_dist too: a NULL one is MI_DEGENSAC_EINVAL;
 * without mutual both are ignored and may be NULL.  Asynchronous on `stream`.
 * mi_degensac_match_ex: mi_degensac_match with the rule of mp (norm, dim, ratio, mutual, decide, max_dist; second_nn must be 0: there
 * are no keypoints here); the reverse search runs when mp->mutual != 0 and keep is asked for. */
int mi_degensac_match_decide_dev(const mi_degensac_match_params *mp, const int32_t *d_idx, const float *d_dist, int n1,
                                 const int32_t *d_back_idx /*nullable*/, const float *d_back_dist /*nullable*/, int device, void *stream,
                                 uint8_t *d_keep);
int mi_degensac_match_ex(const mi_degensac_match_params *mp, const void *desc1, int n1, const void *desc2, int n2, int device,
                         int32_t *idx /*[n1,2]*/, float *dist /*[n1,2]*/, uint8_t *keep /*[n1], nullable*/);
/* Match and verify: per pair the 2-NN search, the ratio test (+ mutual check) of mi_degensac_match, then the estimator of
 * mi_degensac_find_fundamental_batch_dev (homography = 0) or _homography_batch_dev (homography = 1) on the pair's tentatives in
 * query order — exactly the rows mi_degensac_match + the per-pair gather would hand it.  kp1 / kp2: [rows, kp_dim] float64,
 * kp_dim 2 or 6 (LAF rows).  A pair with fewer than 8 (F) / 4 (H) tentatives is SHORT: it is not estimated, gets a zero model
 * and a zero stats row, and does not make the call fail.  d_seeds[K]: seed of pair p (results of a pair do not depend on the other
 * pairs of the batch).  Outputs per pair: d_model [K*9] (the driver's form, as the batch entry points), d_stats [K*16] or NULL;
 * per query row of desc1: d_match = train row local to the pair or -1 when the row is not a tentative, d_inlier = 1 when it is a
 * tentative and an inlier of the pair's model.  h_counts (host, [K], nullable): tentatives per pair.
 * mp->second_nn = 1 (with struct_size covering spatial_th) switches the ratio test to FGINN at mp->spatial_th on this call's d_kp2;
 * the plain guided entry points ignore both fields (mi_degensac_match_guided_fginn_* below are the guided calls that read them).
 * Synchronisation: the matching is enqueued on `stream`, then the call reads the K tentative counts back (ONE device-to-host copy
 * followed by a wait for `stream`: the only synchronisation; the estimator's launch is sized from them on the host), enqueues the
 * gather, the estimator and the scatter and returns.  Discarded pairs (hand-over time-out) carry bit 10 of stats[15] as with the
 * other *_dev entry points.  Errors: MI_DEGENSAC_EINVAL for a bad norm / dim / kp_dim, uint8 rows with dim % 4 != 0
 * (or dim > 256 under L2_U8), decreasing offsets,
 * a ratio that is not finite and > 0, a second_nn other than 0 / 1 or a spatial_th that is negative or not finite (when struct_size
 * covers them), bad params; n_pairs == 0 returns 0. */
int mi_degensac_match_verify_batch_dev(int homography, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                       const int64_t *offsets1_host, const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2,
                                       int kp_dim, int n_pairs, const mi_degensac_params *prm, const uint32_t *d_seeds, int device, void *stream,
                                       double *d_model, int32_t *d_match, uint8_t *d_inlier, int32_t *d_stats, int32_t *h_counts /*nullable*/);
/* the same on host pointers (blocking; seeds[K] on the host).  Like the other host-pointer entry points, pairs discarded after a
 * hand-over time-out are run again without producer / helper workgroups (bit 11 of stats[15]). */
int mi_degensac_match_verify_batch(int homography, const mi_degensac_match_params *mp, const void *desc1, const void *desc2,
                                   const int64_t *offsets1, const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim,
                                   int n_pairs, const mi_degensac_params *prm, const uint32_t *seeds, int device,
                                   double *model, int32_t *match, uint8_t *inlier, int32_t *stats /*nullable*/, int32_t *counts /*nullable*/);

/* ---- the pair-list form: image stores + a list of (i, j) image indices ------------------------------------------------------
 * An image collection matched against itself, or queries against a database: every image takes part in many pairs, so its rows are
 * stored ONCE.  Store 1 holds n_images1 images, image i owning the rows offsets1_host[i] .. offsets1_host[i+1] of desc1 / kp1; store
 * 2 likewise with offsets2_host [n_images2 + 1] (offsets: non-negative, non-decreasing, a non-zero first offset allowed; the two
 * stores may be the same memory).  pairs_host: [2 * n_pairs] int32 on the host, entry p = (i, j): the queries are image i of store
 * 1, the train set image j of store 2.  Any list is allowed: self pairs, repeated pairs, (i, j) next to (j, i), unused and empty
 * images, any order.  Per-query results are laid out pair after pair in list order from row 0: pair p owns the output rows
 * out[p] .. out[p+1], out[p+1] - out[p] = the rows of image pairs[p][0]; train indices are local to image j.
 * Every output is bit for bit what the batched entry point of the same name (knn2_batch_dev / verify_batch_dev / verify_batch)
 * returns when pair p's rows are copied out of the stores and the seeds are the same; no descriptor row is copied on the device.
 * The forward search runs once per list entry, and with mutual the reverse search too (image j's rows against image i, into a block
 * of sum_p rows(image pairs[p][1]) rows): nothing is shared between (i, j) and (j, i).
 * Errors, before a device is looked for: MI_DEGENSAC_EINVAL for an image index outside its store, n_pairs < 0, bad offsets, and
 * output or reverse-search rows beyond 0x3fffffff (the row limit of the batched entry points); n_pairs == 0 returns 0 and touches
 * nothing.  mi_degensac_match_knn2_pairs_dev: asynchronous on `stream`, no host synchronisation; d_idx / d_dist [out[K], 2]. */
int mi_degensac_match_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                                     const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim,
                                     int device, void *stream, int32_t *d_idx, float *d_dist);
/* mi_degensac_match_verify_batch_dev on a pair list: d_kp1 / d_kp2 are the stores' keypoint rows, d_seeds [K] one seed per list
 * entry, d_model [K*9], d_stats [K*16] or NULL, d_match / d_inlier [out[K]] in output-row order, h_counts [K] (host, nullable).  One
 * synchronisation, as there: the read of the K tentative counts.  The FGINN rule is not part of this call: a match_params
 * that asks for it (second_nn = 1 with struct_size covering it) is MI_DEGENSAC_EINVAL; mi_degensac_match_verify_fginn_pairs[_dev]
 * below runs it. */
int mi_degensac_match_verify_pairs_dev(int homography, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                       const int64_t *offsets1_host, int n_images1, const int64_t *offsets2_host, int n_images2,
                                       const double *d_kp1, const double *d_kp2, int kp_dim, const int32_t *pairs_host, int n_pairs,
                                       const mi_degensac_params *prm, const uint32_t *d_seeds, int device, void *stream, double *d_model,
                                       int32_t *d_match, uint8_t *d_inlier, int32_t *d_stats, int32_t *h_counts /*nullable*/);
/* the same on host pointers (blocking; seeds[K] on the host): each store is uploaded once (one upload when both sides name the same
 * arrays).  Pairs discarded after a hand-over time-out are run again as in mi_degensac_match_verify_batch, their tentatives'
 * keypoints picked out of the stores through the pair's image rows (bit 11 of stats[15]). */
int mi_degensac_match_verify_pairs(int homography, const mi_degensac_match_params *mp, const void *desc1, const void *desc2,
                                   const int64_t *offsets1, int n_images1, const int64_t *offsets2, int n_images2, const double *kp1,
                                   const double *kp2, int kp_dim, const int32_t *pairs, int n_pairs, const mi_degensac_params *prm,
                                   const uint32_t *seeds, int device, double *model, int32_t *match, uint8_t *inlier,
                                   int32_t *stats /*nullable*/, int32_t *counts /*nullable*/);

/* FGINN over a pair list.  The plain pair-list calls above keep refusing it; these are the calls that run it.
 * mi_degensac_match_fginn_knn2_pairs_dev = mi_degensac_match_knn2_pairs_dev followed by the FGINN rule of
 * mi_degensac_match_fginn_knn2_batch_dev for slot 1: d_kp2 is the keypoint store of side 2, one [kp_dim] float64 row per row of
 * desc2 (kp_dim 2 or 6, only x, y are read; indexed like desc2, so a non-zero first offset skips keypoint rows too).  Entry p's
 * anchors and competitors are the keypoints of image pairs[p][1]; d_idx / d_dist [out[K], 2] in list order, train indices local to
 * image j; bit for bit mi_degensac_match_fginn_knn2_batch_dev on the entries' copied rows.  A needy query is rescanned through its
 * image's rows in the store: no descriptor or keypoint row is copied.  Asynchronous on `stream`, no host synchronisation.  Errors,
 * before a device is looked for: those of mi_degensac_match_knn2_pairs_dev, and MI_DEGENSAC_EINVAL for kp_dim not 2 / 6 or a
 * spatial_th that is negative or not finite; n_pairs == 0 returns 0. */
int mi_degensac_match_fginn_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                                           const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim,
                                           const double *d_kp2, int kp_dim, double spatial_th, int device, void *stream, int32_t *d_idx,
                                           float *d_dist);
/* mi_degensac_match_verify_pairs_dev / _pairs that honour mp->second_nn / mp->spatial_th (FGINN at that radius on the keypoints of
 * store 2) instead of refusing them; everything else, the one synchronisation included, is that call.  With second_nn = 0, or a
 * struct_size that does not cover spatial_th, they ARE the plain pair-list calls.  Per entry bit for bit
 * mi_degensac_match_verify_batch[_dev] with the same match_params on the entry's copied rows and the same seeds. */
int mi_degensac_match_verify_fginn_pairs_dev(int homography, const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                             const int64_t *offsets1_host, int n_images1, const int64_t *offsets2_host, int n_images2,
                                             const double *d_kp1, const double *d_kp2, int kp_dim, const int32_t *pairs_host, int n_pairs,
                                             const mi_degensac_params *prm, const uint32_t *d_seeds, int device, void *stream, double *d_model,
                                             int32_t *d_match, uint8_t *d_inlier, int32_t *d_stats, int32_t *h_counts /*nullable*/);
int mi_degensac_match_verify_fginn_pairs(int homography, const mi_degensac_match_params *mp, const void *desc1, const void *desc2,
                                         const int64_t *offsets1, int n_images1, const int64_t *offsets2, int n_images2, const double *kp1,
                                         const double *kp2, int kp_dim, const int32_t *pairs, int n_pairs, const mi_degensac_params *prm,
                                         const uint32_t *seeds, int device, double *model, int32_t *match, uint8_t *inlier,
                                         int32_t *stats /*nullable*/, int32_t *counts /*nullable*/);

/* ---- match once, verify F and H: both models on the same tentatives ---------------------------------------------------------
 * A pipeline that classifies its pairs (general scene: keep F; planar or panoramic: H explains what F explains; rejected) needs both
 * models on the SAME tentatives, the two inlier sets and their overlap.  These calls run the matching half of
 * mi_degensac_match_verify_batch_dev ONCE (2-NN, FGINN step, reverse search, ratio test, ranks), read the K tentative counts back ONCE
 * (the only synchronisation), then run the fundamental-matrix estimator with prm_f and the homography estimator with prm_h one after
 * the other on `stream`, and one scatter stage writes everything.  Arguments as mi_degensac_match_verify_batch_dev without
 * `homography`; d_seeds[p] seeds BOTH estimators of pair p.
 * Per pair, d_model_f / d_inlier_f / d_stats_f are bit for bit those of mi_degensac_match_verify_batch_dev with homography = 0 and
 * prm_f, d_model_h / d_inlier_h / d_stats_h those of the call with homography = 1 and prm_h, d_match and h_counts those of either, on
 * the same inputs, seeds and mp.  So a pair with 4 .. 7 tentatives has an H and a zero F; below 4 both are zero.
 * Outputs: d_model_f / d_model_h [K*9] in the driver's form, d_stats_f / d_stats_h [K*16] or NULL, d_match / d_inlier_f / d_inlier_h one
 * entry per query row, d_summary [K*4] int32 (not nullable): per pair (tentatives, nF, nH, nFH) = its tentatives, its rows with
 * inlier_f = 1, with inlier_h = 1, and with both; h_counts (host, [K], nullable).  Discarded pairs carry bit 10 of stats[15] in the
 * stats row of the model that was discarded.
 * Errors, all before a device is looked for: those of mi_degensac_match_verify_batch_dev, with prm_f checked as a fundamental-matrix
 * and prm_h as a homography parameter block; n_pairs == 0 returns 0. */
int mi_degensac_match_verify_fh_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                          const int64_t *offsets1_host, const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2,
                                          int kp_dim, int n_pairs, const mi_degensac_params *prm_f, const mi_degensac_params *prm_h,
                                          const uint32_t *d_seeds, int device, void *stream, double *d_model_f, double *d_model_h,
                                          int32_t *d_match, uint8_t *d_inlier_f, uint8_t *d_inlier_h, int32_t *d_stats_f /*nullable*/,
                                          int32_t *d_stats_h /*nullable*/, int32_t *d_summary, int32_t *h_counts /*nullable*/);
/* the same on host pointers (blocking; seeds[K] on the host; summary nullable): one upload, the device path, and per model the re-run of
 * the pairs whose stats row of THAT model carries bit 10 (bit 11 afterwards, as in mi_degensac_match_verify_batch); the summary of such
 * a pair is counted again from its masks. */
int mi_degensac_match_verify_fh_batch(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                      const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim, int n_pairs,
                                      const mi_degensac_params *prm_f, const mi_degensac_params *prm_h, const uint32_t *seeds, int device,
                                      double *model_f, double *model_h, int32_t *match, uint8_t *inlier_f, uint8_t *inlier_h,
                                      int32_t *stats_f /*nullable*/, int32_t *stats_h /*nullable*/, int32_t *summary /*nullable*/,
                                      int32_t *counts /*nullable*/);
/* mi_degensac_match_verify_fh_batch_dev on a pair list over image stores (arguments and layout as mi_degensac_match_verify_pairs_dev).
 * mp->second_nn / mp->spatial_th are honoured as by mi_degensac_match_verify_fginn_pairs_dev: there is no separate FGINN twin.  Per
 * entry and model bit for bit mi_degensac_match_verify_fginn_pairs_dev with that model's homography flag and parameter block. */
int mi_degensac_match_verify_fh_pairs_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                          const int64_t *offsets1_host, int n_images1, const int64_t *offsets2_host, int n_images2,
                                          const double *d_kp1, const double *d_kp2, int kp_dim, const int32_t *pairs_host, int n_pairs,
                                          const mi_degensac_params *prm_f, const mi_degensac_params *prm_h, const uint32_t *d_seeds, int device,
                                          void *stream, double *d_model_f, double *d_model_h, int32_t *d_match, uint8_t *d_inlier_f,
                                          uint8_t *d_inlier_h, int32_t *d_stats_f /*nullable*/, int32_t *d_stats_h /*nullable*/,
                                          int32_t *d_summary, int32_t *h_counts /*nullable*/);
/* the same on host pointers (blocking): each store is uploaded once, re-runs per model as in mi_degensac_match_verify_fh_batch */
int mi_degensac_match_verify_fh_pairs(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                      int n_images1, const int64_t *offsets2, int n_images2, const double *kp1, const double *kp2, int kp_dim,
                                      const int32_t *pairs, int n_pairs, const mi_degensac_params *prm_f, const mi_degensac_params *prm_h,
                                      const uint32_t *seeds, int device, double *model_f, double *model_h, int32_t *match, uint8_t *inlier_f,
                                      uint8_t *inlier_h, int32_t *stats_f /*nullable*/, int32_t *stats_h /*nullable*/,
                                      int32_t *summary /*nullable*/, int32_t *counts /*nullable*/);

/* ---- guided matching: the batched 2-NN restricted to each pair's model inlier band (mi_guided.hip) ------------------------
 * Same ragged batch as mi_degensac_match_knn2_batch_dev (host offsets of K + 1 values, pair-local indices), plus keypoints
 * kp1 / kp2 [rows, kp_dim] float64 (kp_dim 2 or 6; only x, y are read) and one model per pair, d_models [K*9] in the driver's form
 * (what mi_degensac_match_verify_batch_dev and the *_batch_dev entry points write).  For pair p with model M_p:
 *   gate(q, t) = r(M_p; x1_q, y1_q, x2_t, y2_t) <= th with the estimator's own residual and threshold for (homography, error_type,
 *                px_th) — F: 0 Sampson, 1 symmetric epipolar, th = px_th^2; H: 0 Sampson, 1..4 the symmetric transfer errors, th =
 *                px_th^2 (0, 1, 3) or px_th (2, 4) — in fp64 with the reference's operation order; `<=` as the reference's inlier
 *                rule, a NaN residual fails, a model of nine zeros passes nothing.  The symmetric check and the LAF check of the
 *                estimators are not part of the gate.
 *   guided 2-NN = the two nearest train rows of the pair that pass the gate (the matcher's distances and (distance, index) order;
 *                -1 / inf where fewer than two pass).
 *   decision: a query gets match = idx[q][0] when at least one row passes and dist[q][0] < ratio * dist[q][1].  With exactly one
 *                candidate dist[q][1] = inf and the query passes — unlike the unguided filter, which needs two train rows.  mutual:
 *                the reverse guided 2-NN (the pair's train rows as queries against its query rows, the same gate(q, t)) must return q.
 * Cost follows the rows that pass the gate (a screen without division first, the exact residual for the survivors, distances only
 * for the candidates); a gate that passes everything is correct and slower than mi_degensac_match_knn2_batch_dev.
 * Errors: MI_DEGENSAC_EINVAL for a bad norm / dim / kp_dim / error_type / offsets / ratio, a px_th that is negative or NaN, bad
 * params; n_pairs == 0 returns 0. */
typedef struct mi_degensac_guide_params {
    int32_t homography;    /* 0 = fundamental matrix, 1 = homography                                                     */
    int32_t error_type;    /* MI_DEGENSAC_F_* / MI_DEGENSAC_H_*                                                          */
    double  px_th;         /* pixel threshold, >= 0; th derived as the estimators derive it                              */
    int32_t struct_size;   /* sizeof(mi_degensac_guide_params) of the caller's header (0 = this layout)                  */
    int32_t reserved;
} mi_degensac_guide_params;
/* the guided 2-NN alone: d_idx / d_dist [offsets1_host[K], 2]; asynchronous on `stream`, no host synchronisation */
int mi_degensac_match_guided_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                            const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp1, const double *d_kp2,
                                            int kp_dim, const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream,
                                            int32_t *d_idx, float *d_dist);
/* the guided 2-NN + the decision (mp: norm, dim, ratio, mutual): d_idx / d_dist as above, d_match [rows] = pair-local train row or -1,
 * d_counts [K] (nullable) guided matches per pair on the device.  Asynchronous; it synchronises (once) only when h_counts is given. */
int mi_degensac_match_guided_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                       const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2, int kp_dim, int n_pairs,
                                       const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx,
                                       float *d_dist, int32_t *d_match, int32_t *d_counts /*nullable*/, int32_t *h_counts /*nullable*/);
/* the same on host pointers (blocking) */
int mi_degensac_match_guided_batch(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                   const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim, int n_pairs, const double *models,
                                   const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist, int32_t *match,
                                   int32_t *counts /*nullable*/);

/* ---- guided matching over a pair list: image stores + (i, j) image indices + one model per list entry ------------------------
 * The guided entry points above on the layout of the pair-list form (stores, offsets [n_images + 1], pairs_host [2 * n_pairs]; see "the
 * pair-list form").  Entry p = (i, j) with model M_p = d_models[9 p ..] (driver form): the queries are the rows of image i of store 1,
 * the candidates the rows of image j of store 2 that pass gate(q, t) under M_p; its answers are the output rows out[p] .. out[p+1] (list
 * order from row 0, out[p+1] - out[p] = the rows of image i), indices local to image j.  The model and the zero-model rule belong to
 * the list entry, not to an image: the same (i, j) twice with two models gives two results.  With mp->mutual the reverse guided search
 * (image j's rows against image i's under the same gate(q, t)) runs per entry into a block of 16 bytes per back row (sum_p rows(image
 * pairs[p][1]) rows), which the call allocates stream-ordered and frees.  No descriptor or keypoint row is gathered or copied on the
 * device.  Every output is bit for bit what the batched entry point of the same name (guided_knn2_batch_dev / guided_batch_dev /
 * guided_batch) returns when entry p's rows are copied out of the stores and the models are the same.  mp->second_nn is ignored, as
 * there (mi_degensac_match_guided_fginn_pairs* reads it).
 * Errors, before a device is looked for: MI_DEGENSAC_EINVAL for a bad norm / dim / kp_dim / guide params / ratio, then n_pairs < 0,
 * then (n_pairs > 0) bad offsets, an image index outside its store, output or back rows beyond 0x3fffffff, NULL pointers.
 * n_pairs == 0 with good params returns 0 and looks at nothing else. */
/* the guided 2-NN alone: d_idx / d_dist [out[K], 2]; asynchronous on `stream`, no host synchronisation */
int mi_degensac_match_guided_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                                            const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim,
                                            const double *d_kp1, const double *d_kp2, int kp_dim, const double *d_models /* [K*9] */,
                                            const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx, float *d_dist);
/* the guided 2-NN + the decision: d_match [out[K]] = train row local to image j or -1, d_counts [K] (nullable) guided matches per entry
 * on the device.  Asynchronous; it synchronises (once) only when h_counts [K] (host) is given. */
int mi_degensac_match_guided_pairs_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                       int n_images1, const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs,
                                       const double *d_kp1, const double *d_kp2, int kp_dim, const double *d_models,
                                       const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx, float *d_dist,
                                       int32_t *d_match, int32_t *d_counts /*nullable*/, int32_t *h_counts /*nullable*/);
/* the same on host pointers (blocking): each store is uploaded once (one upload when both sides name the same arrays) */
int mi_degensac_match_guided_pairs(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                   int n_images1, const int64_t *offsets2, int n_images2, const int32_t *pairs, int n_pairs, const double *kp1,
                                   const double *kp2, int kp_dim, const double *models, const mi_degensac_guide_params *gp, int device,
                                   int32_t *idx, float *dist, int32_t *match, int32_t *counts /*nullable*/);

/* ---- guided matching with the FGINN second neighbour INSIDE the gate (mi_guided.hip) --------------------------------------------
 * The two remedies for tentatives the ratio test drops, composed.  The gate takes the look-alikes elsewhere in the image away and leaves
 * a keypoint's own twin (a second orientation, a neighbouring scale a pixel away) as its only second neighbour: the twin lies inside the
 * band too, d1 ~ d0, and the plain guided decision drops exactly the multi-orientation, multi-scale keypoints.  Here, per list entry p
 * with model M_p, the train keypoints kp2 of the entry and r = spatial_th (finite, >= 0):
 *   gate(q, t)  exactly as above (the same residual, `<=`, a NaN fails, a zero model passes nothing);
 *   slot 0      (i0, d0) = the nearest gated train row, unchanged from the plain guided 2-NN;
 *   a train row t competes for slot 1 iff gate(q, t) passes and t != i0 and dx dx + dy dy >= r r, dx = x2[t] - x2[i0], dy = y2[t] -
 *               y2[i0], in fp64 in that order without contraction; a NaN makes the comparison false (the rule of
 *               mi_degensac_match_fginn_knn2_batch_dev word for word, applied after the gate and anchored at the GATED nearest row);
 *   slot 1      the nearest competing row in the matcher's (distance, index) order, distances formed as the guided 2-NN forms them;
 *               -1 / inf when nothing competes or i0 = -1;
 *   decision    the guided one, unchanged: match = i0 when i0 >= 0 && dist0 < ratio * dist1.  A query whose only gated companions lie
 *               inside the radius has dist1 = inf and is KEPT: nothing competes with it.  This is the guided rule, not the unguided
 *               FGINN rule (which needs a second row), and it is the case these calls exist for;
 *   mutual      the reverse guided search and the mutual check stay the plain ones (slot 0 only).
 * r = 0 with finite keypoints is the plain guided 2-NN and decision bit for bit.
 * Cost: the plain guided pass (the same kernels, unchanged), one pass over its output that lists per entry the NEEDY queries (slot 1
 * exists and does not compete), and a rescan of those only, in the guided kernel's shape with the exclusion test in the gate's place in
 * the pass predicate.  A needy query has two rows, its output row and its query row in store 1 (equal only in a ragged batch); both are
 * found through the entry's record and no descriptor or keypoint row is copied.  The rescan's grid is sized on the host for the worst
 * case: no host synchronisation.  Memory: 4 bytes per output row and per entry next to the plain call's, stream-ordered and freed.
 *
 * mi_degensac_match_guided_fginn_knn2_batch_dev / _pairs_dev: mi_degensac_match_guided_knn2_batch_dev / _pairs_dev with spatial_th after
 * the guide params; asynchronous on `stream`, no host synchronisation.
 * mi_degensac_match_guided_fginn_batch_dev / _batch / _pairs_dev / _pairs: the signatures of the plain guided calls; they honour
 * mp->second_nn / mp->spatial_th when mp->struct_size covers spatial_th.  With second_nn = 0, or a struct_size that does not cover it
 * (0 included), they ARE the plain guided calls.
 * Errors, before a device is looked for: those of the plain guided call of the same layout in its order (params, gate, n_pairs < 0, then
 * for n_pairs > 0 the offsets and the list), then MI_DEGENSAC_EINVAL for a spatial_th that is negative or not finite or a second_nn
 * other than 0 / 1, then (n_pairs > 0) NULL pointers.  n_pairs == 0 with good params returns 0. */
int mi_degensac_match_guided_fginn_knn2_batch_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host,
                                                  const int64_t *offsets2_host, int n_pairs, int dim, const double *d_kp1, const double *d_kp2,
                                                  int kp_dim, const double *d_models, const mi_degensac_guide_params *gp, double spatial_th,
                                                  int device, void *stream, int32_t *d_idx, float *d_dist);
int mi_degensac_match_guided_fginn_knn2_pairs_dev(int norm, const void *d_desc1, const void *d_desc2, const int64_t *offsets1_host, int n_images1,
                                                  const int64_t *offsets2_host, int n_images2, const int32_t *pairs_host, int n_pairs, int dim,
                                                  const double *d_kp1, const double *d_kp2, int kp_dim, const double *d_models /* [K*9] */,
                                                  const mi_degensac_guide_params *gp, double spatial_th, int device, void *stream, int32_t *d_idx,
                                                  float *d_dist);
int mi_degensac_match_guided_fginn_batch_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                             const int64_t *offsets1_host, const int64_t *offsets2_host, const double *d_kp1, const double *d_kp2,
                                             int kp_dim, int n_pairs, const double *d_models, const mi_degensac_guide_params *gp, int device,
                                             void *stream, int32_t *d_idx, float *d_dist, int32_t *d_match, int32_t *d_counts /*nullable*/,
                                             int32_t *h_counts /*nullable*/);
int mi_degensac_match_guided_fginn_batch(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                         const int64_t *offsets2, const double *kp1, const double *kp2, int kp_dim, int n_pairs,
                                         const double *models, const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist,
                                         int32_t *match, int32_t *counts /*nullable*/);
int mi_degensac_match_guided_fginn_pairs_dev(const mi_degensac_match_params *mp, const void *d_desc1, const void *d_desc2,
                                             const int64_t *offsets1_host, int n_images1, const int64_t *offsets2_host, int n_images2,
                                             const int32_t *pairs_host, int n_pairs, const double *d_kp1, const double *d_kp2, int kp_dim,
                                             const double *d_models, const mi_degensac_guide_params *gp, int device, void *stream, int32_t *d_idx,
                                             float *d_dist, int32_t *d_match, int32_t *d_counts /*nullable*/, int32_t *h_counts /*nullable*/);
int mi_degensac_match_guided_fginn_pairs(const mi_degensac_match_params *mp, const void *desc1, const void *desc2, const int64_t *offsets1,
                                         int n_images1, const int64_t *offsets2, int n_images2, const int32_t *pairs, int n_pairs,
                                         const double *kp1, const double *kp2, int kp_dim, const double *models,
                                         const mi_degensac_guide_params *gp, int device, int32_t *idx, float *dist, int32_t *match,
                                         int32_t *counts /*nullable*/);

/* ---- verified matches as compact per-entry lists with coordinates and residuals (mi_correspond.hip) ---------------------------
 * Every call above answers per query row: match [N] (train row local to image j, or -1) and a per-row mask.  What follows the library
 * (a two-view database, triangulation, track building) wants, per list entry, the (row in image i, row in image j) that survived, the
 * four coordinates and the residual under the entry's model.  These calls make that list on the device, without a host synchronisation.
 * Inputs, all device arrays on one device:
 *   the layout    of the pair-list form (offsets1_host [n_images1 + 1], offsets2_host [n_images2 + 1], pairs_host [2 * n_pairs]): entry
 *                 p = (i, j) owns the N = out[K] output rows out[p] .. out[p+1] in list order, out[p+1] - out[p] = rows(image i).  The
 *                 batch form is the identity list: entry p = (image p, image p) of offsets1_host / offsets2_host [K + 1].
 *   d_match [N]   int32, d_keep [N] uint8 or NULL: at output row 0 in the pair-list form; in the batch form indexed like the batch's
 *                 other per-query arrays (row offsets1_host[0] is entry 0's first row).
 * Selection: row r of entry p = (i, j), query q = r - out[p], is selected iff 0 <= d_match[r] < rows(image j) and (d_keep == NULL or
 * d_keep[r] != 0).  A match value outside that range means "not selected": it is no error and is never used as an index.
 * Outputs: the selected rows in row order (list order, query order inside an entry) at positions 0, 1, ...; with total = their number
 * and capacity = the length of the per-correspondence arrays, the correspondence at position pos < capacity is written, the others are
 * dropped, and no element at a position >= min(total, capacity) is written.  d_total and d_corr_offsets are exact whatever capacity
 * is, so an overflow shows as total > capacity.
 *   d_corr_offsets [K + 1] int64   the selected rows that lie before out[p]; [K] = total; an empty entry repeats its successor's value
 *   d_total [1] int64
 *   d_rows [capacity, 2] int32     (q, d_match[r]), local to images i and j; with MI_DEGENSAC_CORR_STORE_ROWS in flags
 *                                  (offsets1_host[i] + q, offsets2_host[j] + d_match[r]), the rows of the stores
 *   d_entry [capacity] int32       p (nullable)
 *   d_pts [capacity, 4] float64    x1, y1 of row offsets1_host[i] + q of d_kp1 and x2, y2 of row offsets2_host[j] + d_match[r] of d_kp2
 *                                  ([rows, kp_dim] float64, kp_dim 2 or 6, only x, y are read; nullable)
 *   d_resid [capacity] float64     r(M_p; x1, y1, x2, y2), M_p = d_models[9 p ..] in the driver's form, the estimator's own residual
 *                                  for gp->homography / gp->error_type (F: 0 dg_FDs, 1 dg_FDsSym; H: 0 dg_HDs, 1..4 dg_Hsym on
 *                                  dg_hsym_prepare(M_p)) exactly as the gate of the guided calls forms it: fp64 without contraction,
 *                                  no screen, a zero or non-finite model gives whatever the function gives; gp->px_th is not read
 *                                  (nullable; needs d_models and gp)
 * Asynchronous on `stream`, no host synchronisation; temporaries (8 bytes per 1024 rows, 28 bytes per entry, 144 more per entry for
 * the symmetric H errors) are allocated and freed stream-ordered.  Deterministic: no atomics, the same bits on every call.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * a flag bit other than MI_DEGENSAC_CORR_STORE_ROWS; kp_dim not 2 / 6 when d_pts or d_resid is given; d_resid without d_models or
 * without gp, a gp whose struct_size does not cover the fields, homography other than 0 / 1, an error_type of the other model kind;
 * capacity < 0; n_pairs < 0; then for n_pairs > 0 what the layout refuses (offsets, image indices, more than 0x3fffffff rows); under
 * MI_DEGENSAC_CORR_STORE_ROWS store offsets beyond 0x7fffffff; NULL d_corr_offsets or d_total, and for N > 0 NULL d_match, NULL d_rows
 * with capacity > 0, NULL d_kp1 / d_kp2 with d_pts or d_resid.  n_pairs == 0 with good parameters writes d_total = 0 and
 * d_corr_offsets[0] = 0 (asynchronously) and looks at nothing else; N == 0 with K > 0 writes K + 1 zeros. */
#define MI_DEGENSAC_CORR_STORE_ROWS 1u
int mi_degensac_correspondences_pairs_dev(const int64_t *offsets1_host, int n_images1, const int64_t *offsets2_host, int n_images2,
                                          const int32_t *pairs_host, int n_pairs, const int32_t *d_match, const uint8_t *d_keep /*nullable*/,
                                          uint32_t flags, const double *d_kp1, const double *d_kp2,
                                          int kp_dim /* all three unused when d_pts and d_resid are NULL */, const double *d_models /*nullable*/,
                                          const mi_degensac_guide_params *gp /*nullable*/, int64_t capacity, int device, void *stream,
                                          int64_t *d_corr_offsets, int64_t *d_total, int32_t *d_rows, int32_t *d_entry /*nullable*/,
                                          double *d_pts /*nullable*/, double *d_resid /*nullable*/);
int mi_degensac_correspondences_batch_dev(const int64_t *offsets1_host, const int64_t *offsets2_host, int n_pairs, const int32_t *d_match,
                                          const uint8_t *d_keep /*nullable*/, uint32_t flags, const double *d_kp1, const double *d_kp2, int kp_dim,
                                          const double *d_models /*nullable*/, const mi_degensac_guide_params *gp /*nullable*/, int64_t capacity,
                                          int device, void *stream, int64_t *d_corr_offsets, int64_t *d_total, int32_t *d_rows,
                                          int32_t *d_entry /*nullable*/, double *d_pts /*nullable*/, double *d_resid /*nullable*/);
/* the same on host pointers (blocking): match / keep, the keypoint rows of each store (one upload when both sides name the same arrays)
 * and the models go to the device once; corr_offsets [K + 1], total [1] and the first min(total, capacity) elements of rows / entry /
 * pts / resid come back, capacity = what the caller allocated.  n_pairs == 0 writes total = 0 and corr_offsets[0] = 0 without a device. */
int mi_degensac_correspondences_pairs(const int64_t *offsets1, int n_images1, const int64_t *offsets2, int n_images2, const int32_t *pairs,
                                      int n_pairs, const int32_t *match, const uint8_t *keep /*nullable*/, uint32_t flags, const double *kp1,
                                      const double *kp2, int kp_dim, const double *models /*nullable*/,
                                      const mi_degensac_guide_params *gp /*nullable*/, int64_t capacity, int device, int64_t *corr_offsets,
                                      int64_t *total, int32_t *rows, int32_t *entry /*nullable*/, double *pts /*nullable*/,
                                      double *resid /*nullable*/);
int mi_degensac_correspondences_batch(const int64_t *offsets1, const int64_t *offsets2, int n_pairs, const int32_t *match,
                                      const uint8_t *keep /*nullable*/, uint32_t flags, const double *kp1, const double *kp2, int kp_dim,
                                      const double *models /*nullable*/, const mi_degensac_guide_params *gp /*nullable*/, int64_t capacity,
                                      int device, int64_t *corr_offsets, int64_t *total, int32_t *rows, int32_t *entry /*nullable*/,
                                      double *pts /*nullable*/, double *resid /*nullable*/);
/* the tile constants of the compaction: which = 0 rows per workgroup, 1 workgroup counts per scan step (-1 for any other value) */
int mi_degensac_correspondences_tile(int which);

/* ---- tracks: the connected components of exported matches over one image store (mi_tracks.hip) ---------------------------------
 * A track is a set of keypoints across the images of a collection that are transitively matched.  The input is exactly what the
 * correspondence export writes for a collection matched against itself with MI_DEGENSAC_CORR_STORE_ROWS: d_rows [n_edges, 2] int32 of
 * store rows and its device total.  Both columns index ONE store, described by offsets_host [n_images + 1] (the two-store form of a
 * pair list has no tracks): R = offsets_host[n_images] - offsets_host[0] nodes, node k = store row offsets_host[0] + k.
 * Edges: only the first min(*d_total, n_edges) count (d_total NULL: all n_edges; a negative total: none).  An edge with either end
 * outside [offsets_host[0], offsets_host[n_images]) is ignored and never used as an index, which covers the export's -1 fill; self
 * edges and repeated edges are legal and change nothing.
 * Outputs, all device arrays, each a pure function of the input (the same bits on every call, whatever the scheduling):
 *   d_label [R] int32                 the smallest node of k's connected component; an isolated node has itself (nullable)
 *   d_track [R] int32                 a track is a component of at least two nodes, numbered 0, 1, ... in ascending order of their
 *                                     label: the node's track, or -1
 *   d_n_tracks [1], d_n_obs [1] int64 the tracks and their members in all
 *   d_track_offsets [R/2 + 1] int64   track t owns d_obs[d_track_offsets[t] .. d_track_offsets[t + 1]); the elements after [n_tracks]
 *                                     equal n_obs, so every prefix is a valid table
 *   d_obs [R] int32                   the store rows of all track members, track after track, ascending inside a track; -1 at
 *                                     positions >= n_obs (nullable)
 *   d_obs_image [R] int32             their image: the last i with offsets_host[i] <= row, which skips empty images; -1 at positions
 *                                     >= n_obs (nullable; needs d_obs)
 *   d_track_images [R/2] int32        the distinct images of the track; -1 at positions >= n_tracks.  A track is consistent (at most
 *                                     one keypoint per image) iff d_track_images[t] == d_track_offsets[t + 1] - d_track_offsets[t]
 *                                     (nullable; needs d_obs)
 * R == 0 writes n_tracks = n_obs = 0 and track_offsets[0] = 0; n_edges == 0 gives label[k] = k, track = -1 and zero tracks.
 * Asynchronous on `stream`, no host synchronisation; temporaries (up to 25 bytes per node, 4 per image, 8 per 1024 nodes and the sort's
 * own) are allocated and freed stream-ordered.  The components come from a lock-free link (hook the larger root under the smaller by
 * compare-and-swap) whose result does not depend on the schedule: the smallest node of a component always ends as its root; the
 * grouping is a stable radix sort, the track numbers a scan, and track_images integer sums.  No pass waits for another workgroup.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_images < 0; NULL offsets_host; decreasing or negative offsets, or offsets beyond 0x7fffffff; n_edges < 0 or > 0x3fffffff; NULL d_rows
 * with n_edges > 0; NULL d_track, d_n_tracks, d_n_obs or d_track_offsets; d_obs_image or d_track_images without d_obs; a d_rows that is
 * not 4-byte aligned (an 8-byte-aligned d_rows is read as int2). */
int mi_degensac_tracks_dev(const int64_t *offsets_host, int n_images, const int32_t *d_rows, int64_t n_edges, const int64_t *d_total /*nullable*/,
                           int device, void *stream, int32_t *d_label /*nullable*/, int32_t *d_track, int64_t *d_n_tracks, int64_t *d_n_obs,
                           int64_t *d_track_offsets, int32_t *d_obs /*nullable*/, int32_t *d_obs_image /*nullable*/,
                           int32_t *d_track_images /*nullable*/);
/* the same on host pointers (blocking): the edges go to the device once and every array comes back whole, fills included; total is
 * passed by value, < 0 = all n_edges */
int mi_degensac_tracks(const int64_t *offsets, int n_images, const int32_t *rows, int64_t n_edges, int64_t total, int device,
                       int32_t *label /*nullable*/, int32_t *track, int64_t *n_tracks, int64_t *n_obs, int64_t *track_offsets,
                       int32_t *obs /*nullable*/, int32_t *obs_image /*nullable*/, int32_t *track_images /*nullable*/);
/* the tile constants of the boundary passes: which = 0 sorted positions per workgroup, 1 workgroup counts per scan step (-1 else) */
int mi_degensac_tracks_tile(int which);

/* ---- refit F / H on exported correspondence lists (mi_refit.hip) ---------------------------------------------------------------
 * The guided stage brings back matches the estimator never saw, and matches may come from elsewhere altogether (a learned matcher, a
 * previous frame's model).  This call judges such a list against a model and refits the model on what it keeps, per list entry, on the
 * device and without a host synchronisation: the row ranges are read from device memory, so the host never learns a length.
 * Inputs per entry p (all device arrays on one device, as mi_degensac_correspondences_* write them):
 *   its rows     d_pts[o[p] .. o[p + 1]) of d_pts [cap, 4] float64 = x1, y1, x2, y2, with o = d_corr_offsets [K + 1] int64
 *   M0[p]        d_models[9 p ..], the start model in the driver's form
 *   th           from gp->px_th and gp->error_type exactly as the guided gate derives it (F: px_th^2; H: px_th^2 for 0, 1, 3 and px_th
 *                for 2, 4); resid(M; row) is the estimator's own function of that error type, the one the guided gate and the export's
 *                d_resid use (F: 0 dg_FDs, 1 dg_FDsSym; H: 0 dg_HDs, 1..4 dg_Hsym on dg_hsym_prepare(M)), fp64 without contraction.
 *   members(M)   the rows with resid(M; row) <= th, in row order.  A NaN residual is not a member; a model of nine zeros, or with an entry
 *                that is not finite, has no members.
 * The rule:
 *   best = M0; I = members(best); n0 = |I|
 *   repeat at most max_fits times (0 is allowed):
 *       if |I| < 8 (F) / 4 (H): stop, MI_DEGENSAC_REFIT_SHORT
 *       M = u2f / u2h on the rows of I in list order: the reference's non-minimal solver, in the variant the drivers use for that length
 *           (F: <= 16 rows the small solver — 8 rows the 9 x 8 null vector —, beyond the sequential normalised least squares; H: 4 rows
 *           the DLT null vector, 5 .. 12 the small normalised DLT, beyond the sequential one)
 *       if M has an entry that is not finite: stop, MI_DEGENSAC_REFIT_BAD_FIT
 *       I' = members(M)
 *       if |I'| < |I|: stop, MI_DEGENSAC_REFIT_WORSE (best and I stay)
 *       best = M; same = (I' == I); I = I'
 *       if same: stop, MI_DEGENSAC_REFIT_FIXED
 *   all max_fits rounds used: MI_DEGENSAC_REFIT_MAX_FITS
 * The estimators' symmetric check and LAF check are not part of it, as in the guided gate: the call judges a list against a model, it
 * does not choose correspondences.  An entry whose range does not lie wholly inside [0, cap) — a truncated export (total > capacity),
 * or a decreasing pair of offsets — keeps M0, flags no member and has status MI_DEGENSAC_REFIT_TRUNCATED; d_corr_offsets is device
 * data and is not validated on the host.  An empty entry keeps M0 (SHORT, or MAX_FITS with max_fits == 0).  Ranges must not overlap.
 * Outputs:
 *   d_models_out [K, 9]    best, driver form
 *   d_inlier [cap] uint8   1 for the members of best; a position no entry owns keeps 0
 *   d_models_user [K, 9]   (nullable) H: the user-facing inv(H_c^T) of best, nine zeros where best is zero, singular or not finite; F: best
 *   d_info [K, 4] int32    (nullable) n0, |I| at the end, fits run, status
 *   d_resid [cap]          (nullable) resid(best; row); a position no entry owns keeps NaN
 * One workgroup per entry, no atomics, every sum in list order: the same bits on every call.  Asynchronous on `stream`; temporaries
 * (68 bytes per row of cap: the fits' staging array and the member lists) are allocated and freed stream-ordered.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_entries < 0; cap < 0 or > 0x3fffffff; max_fits < 0; NULL gp, a gp whose struct_size does not cover the fields, homography other than
 * 0 / 1, an error_type of the other model kind, a px_th that is negative or NaN; NULL d_corr_offsets; for n_entries > 0 NULL d_models or
 * d_models_out; for cap > 0 NULL d_pts or d_inlier.  n_entries == 0 and cap == 0 succeed (with n_entries == 0 the fills are all that
 * is written). */
enum { MI_DEGENSAC_REFIT_FIXED = 0, MI_DEGENSAC_REFIT_MAX_FITS = 1, MI_DEGENSAC_REFIT_SHORT = 2, MI_DEGENSAC_REFIT_BAD_FIT = 3,
       MI_DEGENSAC_REFIT_WORSE = 4, MI_DEGENSAC_REFIT_TRUNCATED = 5 };
int mi_degensac_refit_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const double *d_models, int n_entries, int64_t cap,
                                const mi_degensac_guide_params *gp, int max_fits, int device, void *stream, double *d_models_out,
                                uint8_t *d_inlier, double *d_models_user /*nullable*/, int32_t *d_info /*nullable*/,
                                double *d_resid /*nullable*/);
/* the same on host pointers (blocking): pts, corr_offsets and models go to the device once, every output comes back whole */
int mi_degensac_refit_lists(const double *pts, const int64_t *corr_offsets, const double *models, int n_entries, int64_t cap,
                            const mi_degensac_guide_params *gp, int max_fits, int device, double *models_out, uint8_t *inlier,
                            double *models_user /*nullable*/, int32_t *info /*nullable*/, double *resid /*nullable*/);
/* the tile constants: which = 0 rows per workgroup and step of a scoring pass, 1 the cap on the grid (-1 for any other value) */
int mi_degensac_refit_tile(int which);

/* ---- relative pose and triangulation on exported correspondence lists --------------------------------------------------------------
 * What a structure-from-motion front end stores per pair besides F: the relative pose (R, t) under known intrinsics, which of the
 * exported matches triangulate in front of both cameras, and how much parallax they have.  Per list entry, on the device and without a
 * host synchronisation: the row ranges are read from device memory, so the host never learns a length.
 * Inputs per entry p (all device arrays on one device):
 *   its rows     d_pts[o[p] .. o[p + 1]) of d_pts [cap, 4] float64 = x1, y1, x2, y2, with o = d_corr_offsets [K + 1] int64
 *   d_keep       (nullable) [cap] uint8: only rows with keep != 0 are USED; the refit's d_inlier goes in as it is.  NULL: every row.
 *   F[p]         d_F[9 p ..], row-major, x2^T F x1 = 0 as everywhere in this library (any scale)
 *   cameras      two pinhole cameras (fx, fy, cx, cy): rows i1, i2 of d_cams [n_cams, 4] float64 with (i1, i2) = d_cam_idx[2 p], [2 p + 1]
 *                (int32 [K, 2]); d_cam_idx NULL: i1 = 2 p, i2 = 2 p + 1.  Camera 1 belongs to x1, y1.
 * Every step below is ONE IEEE float64 operation per written operator, no contraction; a sum of three terms is (first + second) + third.
 * Per entry (statuses in their order of precedence):
 *   range        not 0 <= o[p] <= o[p + 1] <= cap (a truncated export, a decreasing pair): MI_DEGENSAC_POSE_TRUNCATED
 *   cameras      i1 or i2 outside [0, n_cams), or an fx / fy that is zero or not finite: MI_DEGENSAC_POSE_BAD_CAMERA
 *   E = K2^T F K1  G = F K1: G[i][0] = F[i][0] fx1, G[i][1] = F[i][1] fy1, G[i][2] = (F[i][0] cx1 + F[i][1] cy1) + F[i][2];
 *                then E[0][j] = fx2 G[0][j], E[1][j] = fy2 G[1][j], E[2][j] = (cx2 G[0][j] + cy2 G[1][j]) + G[2][j]
 *                m = the largest |E[i][j]|; an entry that is not finite, or m == 0: MI_DEGENSAC_POSE_BAD_MODEL.  A = E / m.
 *   V, sigma     the singular value decomposition of A by one-sided Jacobi rotations: V = I, B = A (b_i = column i of A), then six sweeps
 *                over the column pairs (i j) = (0 1) (0 2) (1 2), a dot product being (first + second) + third:
 *                al = b_i . b_i, be = b_j . b_j, ga = b_i . b_j; if ga != 0: z = (be - al) / (2 ga), t = sign(z) / (|z| + sqrt(1 + z z))
 *                (sign(0) = 1), c = 1 / sqrt(1 + t t), s = c t; (b_i, b_j) <- (c b_i - s b_j, s b_i + c b_j), (v_i, v_j) likewise.
 *                V stays orthogonal to rounding for every A and B = A V throughout; four sweeps converge to 1e-15 on general, rank-2 and
 *                (near-)essential matrices, six are run.  (The reference's 3 x 3 routine of the DEGENSAC branch, dg_svd3_right, is not
 *                used here: the pose needs all of V orthogonal and the singular values, which it does not return on every input.)
 *                sigma_i = sqrt(b_i . b_i); sorted by sigma descending with ties keeping the lower column in front: v1, v2, v3, b1, b2 and
 *                sigma1 >= sigma2 >= sigma3.  sigma2 not > 0: BAD_MODEL.
 *   U            u_i = b_i / sigma_i for i = 1, 2;
 *                u3 = u1 x u2 (each component a difference of two products, (1 2 - 2 1), (2 0 - 0 2), (0 1 - 1 0));
 *                t = u3 / sqrt((u3[0]^2 + u3[1]^2) + u3[2]^2)
 *   R            U W V^T and U W^T V^T with W = [0 -1 0; 1 0 0; 0 0 1] and t as the third column of U:
 *                Ra[r][c] = (u2[r] v1[c] - u1[r] v2[c]) + t[r] v3[c],  Rb[r][c] = (u1[r] v2[c] - u2[r] v1[c]) + t[r] v3[c];
 *                each is negated when its determinant (R00 (R11 R22 - R12 R21) - R01 (R10 R22 - R12 R20)) + R02 (R10 R21 - R11 R20) is < 0
 *   candidates   in this order 0: (Ra, t), 1: (Ra, -t), 2: (Rb, t), 3: (Rb, -t); the meaning is X2 = R X1 + t, |t| = 1.
 *                A candidate with a number that is not finite: BAD_MODEL.
 *   c2           the centre of camera 2 in the frame of camera 1, per candidate: c2[j] = -((R[0][j] t[0] + R[1][j] t[1]) + R[2][j] t[2])
 * Per used row and candidate:
 *   rays         d1 = ((x1 - cx1) / fx1, (y1 - cy1) / fy1, 1), d2 likewise with camera 2; r2 = R^T d2: r2[j] = (R[0][j] d2[0] + R[1][j] d2[1]) + R[2][j]
 *   midpoint     a = (d1[0]^2 + d1[1]^2) + 1, b = (d1[0] r2[0] + d1[1] r2[1]) + r2[2], c = (r2[0]^2 + r2[1]^2) + r2[2]^2,
 *                d = (d1[0] c2[0] + d1[1] c2[1]) + c2[2], e = (r2[0] c2[0] + r2[1] c2[1]) + r2[2] c2[2], den = a c - b b,
 *                lambda1 = (c d - b e) / den, lambda2 = (b d - a e) / den  (the depths along d1 and r2: the closest points of the two rays),
 *                X[j] = 0.5 ((lambda1 d1[j] + c2[j]) + lambda2 r2[j]) in the frame of camera 1 (j = 2: lambda1 itself for lambda1 d1[2])
 *   front        lambda1 > 0 and lambda2 > 0; a NaN is not front (den == 0 is not treated apart: it gives what IEEE division gives)
 *   cosang       b / sqrt(a c), the cosine of the angle between the two rays; a front row is WIDE iff cosang <= cos_min
 * The chosen pose is the candidate with the most front rows among the used rows; ties go to the first in the order above.  No used row:
 * MI_DEGENSAC_POSE_EMPTY.  With a status other than OK the pose is twelve zeros, the info row is (0, 0, 0, 0, status) and no row of
 * the entry is written.  Ranges must not overlap.
 * Outputs:
 *   d_pose [K, 12]          R row-major, then t, of the chosen candidate
 *   d_front [cap] uint8     1 for the used rows that are front under the chosen candidate; every other position keeps 0
 *   d_info [K, 5] int32     rows used, front rows of the chosen candidate, the largest front count of the other three, wide rows, status
 *   d_X [cap, 3], d_depth [cap, 2] = lambda1, lambda2, d_cosang [cap]   (each nullable) of the used rows under the chosen candidate;
 *                           positions that no entry owns, rows that are not used and rows of entries without a pose keep NaN
 *   d_cand [K, 4, 12], d_cand_front [K, 4] int32   (each nullable) all four candidates (zeros for TRUNCATED, BAD_CAMERA, BAD_MODEL) and
 *                           their front counts (zeros unless OK)
 * One workgroup per entry, no atomics, counts by wave ballots and integer adds: the same bits on every call.  Asynchronous on `stream`;
 * the call needs no temporaries.  d_corr_offsets and d_cam_idx are device data and are checked on the device, not on the host.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_entries < 0; cap < 0 or > 0x3fffffff; n_cams < 0; a cos_min that is NaN or outside [-1, 1]; NULL d_corr_offsets; for n_entries > 0
 * NULL d_F or d_cams, then NULL d_pose or d_info; for cap > 0 NULL d_pts or d_front.  n_entries == 0 and cap == 0 succeed (with
 * n_entries == 0 the fills are all that is written). */
enum { MI_DEGENSAC_POSE_OK = 0, MI_DEGENSAC_POSE_BAD_MODEL = 1, MI_DEGENSAC_POSE_BAD_CAMERA = 2, MI_DEGENSAC_POSE_TRUNCATED = 3,
       MI_DEGENSAC_POSE_EMPTY = 4 };
int mi_degensac_pose_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep /*nullable*/, const double *d_F,
                               const double *d_cams, int n_cams, const int32_t *d_cam_idx /*nullable*/, int n_entries, int64_t cap,
                               double cos_min, int device, void *stream, double *d_pose, uint8_t *d_front, int32_t *d_info,
                               double *d_X /*nullable*/, double *d_depth /*nullable*/, double *d_cosang /*nullable*/,
                               double *d_cand /*nullable*/, int32_t *d_cand_front /*nullable*/);
/* the same on host pointers (blocking): the inputs go to the device once, every output that is asked for comes back whole */
int mi_degensac_pose_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep /*nullable*/, const double *F,
                           const double *cams, int n_cams, const int32_t *cam_idx /*nullable*/, int n_entries, int64_t cap, double cos_min,
                           int device, double *pose, uint8_t *front, int32_t *info, double *X /*nullable*/, double *depth /*nullable*/,
                           double *cosang /*nullable*/, double *cand /*nullable*/, int32_t *cand_front /*nullable*/);
/* the tile constants: which = 0 rows per workgroup and step of a row pass, 1 the cap on the grid (-1 for any other value) */
int mi_degensac_pose_tile(int which);

/* ---- relative pose from a homography on exported correspondence lists (mi_pose_h.hip) ---------------------------------------------------
 * The pose call above takes (R, t) from F.  For a pair whose points lie on a plane, or whose cameras share a centre, F is degenerate: a
 * family of fundamental matrices fits and the estimator returns an arbitrary member, whose decomposition is a wrong pose.  Such a pair
 * (class 2 of the F + H verification) has its pose in the homography instead, which this call decomposes: G = K2^-1 H K1 = R + (t / d)
 * n^T for a plane n . X = d in the frame of camera 1, or G = R for a pure rotation.  Rows, offsets, keep, cameras and camera indices
 * exactly as mi_degensac_pose_lists_dev takes them; one more input per entry:
 *   H[p]         d_H[9 p ..], row-major, x2 ~ H x1 (any scale, either sign): the homography in the CALLER'S form, H = (M^T)^-1 for a
 *                model M in the driver's form as the estimator, the refit and dg_HDs take it.
 * Every step below is ONE IEEE float64 operation per written operator (+ - * / and sqrt only), no contraction; a sum of three terms is
 * (first + second) + third; a product with +-1 is exact.  Per entry (statuses in their order of precedence):
 *   range, cameras   as in mi_degensac_pose_lists_dev: MI_DEGENSAC_POSE_TRUNCATED, MI_DEGENSAC_POSE_BAD_CAMERA
 *   G = K2^-1 H K1   L = H K1: L[i][0] = H[i][0] fx1, L[i][1] = H[i][1] fy1, L[i][2] = (H[i][0] cx1 + H[i][1] cy1) + H[i][2]; then
 *                G[0][j] = (L[0][j] - cx2 L[2][j]) / fx2, G[1][j] = (L[1][j] - cy2 L[2][j]) / fy2, G[2][j] = L[2][j].
 *                m = the largest |G[i][j]|; an entry that is not finite, or m == 0: MI_DEGENSAC_POSE_BAD_MODEL.  A = G / m.
 *   V, sigma     the one-sided Jacobi rule of mi_degensac_pose_lists_dev on A, word for word: six sweeps, the same rotation, the same
 *                descending sort with ties keeping the lower column: v1, v2, v3, b1, b2, b3 (b_i = A v_i) and sigma1 >= sigma2 >= sigma3.
 *                sigma3 not > 0: BAD_MODEL (a homography has full rank).
 *   sign         s = -1 if det A < 0, else 1, with det A = (A00 (A11 A22 - A12 A21) - A01 (A10 A22 - A12 A20)) + A02 (A10 A21 - A11 A20):
 *                s A / sigma2 has the middle singular value 1 and both cameras on one side of the plane.
 *   rotation     if sigma1 - sigma3 <= rotation_eps sigma2 the status is MI_DEGENSAC_POSE_ROTATION: u_i = b_i / sigma_i (i = 1, 2, 3),
 *                R[r][c] = (u1[r] v1[c] + u2[r] v2[c]) + u3[r] v3[c], negated when its determinant (the formula above) is < 0; a number
 *                that is not finite: BAD_MODEL.  The single candidate is (R, t = 0) in slot 0, there is no normal, t_over_d = 0.
 *   solutions    otherwise, by the construction of Ma, Soatto, Kosecka & Sastry (An Invitation to 3-D Vision, theorem 5.19) from V alone:
 *                N = s A / sigma2 (N[i][j] = s (A[i][j] / sigma2)), h_i = N v_i taken as h_i[r] = s (b_i[r] / sigma2),
 *                k1 = sigma1 / sigma2, k3 = sigma3 / sigma2, p = sqrt((1 - k3) (1 + k3)), q = sqrt((k1 - 1) (k1 + 1)),
 *                w = sqrt((k1 - k3) (k1 + k3)).  For the two signs, a = (p v1 + q v3) / w and g = (p h1 + q h3) / w, then a = (p v1 - q v3)
 *                / w and g = (p h1 - q h3) / w (g = N a): v2 and a are the unit vectors whose length N keeps, so with
 *                n = v2 x a, rn = h2 x g (cross products as in the pose call: (1 2 - 2 1), (2 0 - 0 2), (0 1 - 1 0)):
 *                R[r][c] = (h2[r] v2[c] + g[r] a[c]) + rn[r] n[c],   T[r] = ((N[r][0] n[0] + N[r][1] n[1]) + N[r][2] n[2]) - rn[r]   (= t / d),
 *                t_over_d = sqrt((T[0]^2 + T[1]^2) + T[2]^2), t = T / t_over_d.
 *   candidates   in this order, (Ra, ta, na) from the + sign and (Rb, tb, nb) from the - sign: 0: (Ra, ta, na), 1: (Rb, tb, nb),
 *                2: (Ra, -ta, -na), 3: (Rb, -tb, -nb); the meaning is X2 = R X1 + t, |t| = 1, n the unit normal of the plane in the frame
 *                of camera 1.  A candidate with a number that is not finite: BAD_MODEL.  c2 per candidate as in the pose call.
 * Per used row and candidate, rays, midpoint, lambda1, lambda2, X and cosang are the pose call's rule unchanged.  A row is
 *   front        iff lambda1 > 0 and lambda2 > 0 and (n[0] d1[0] + n[1] d1[1]) + n[2] > 0: it triangulates in front of both cameras and
 *                the plane is seen from its visible side; a NaN is not front.  Of a pair (q, q + 2) at most one passes the plane-side test,
 *                so two of the four survive by construction; what tells the remaining two apart is only the rows that lie beyond the
 *                other solution's plane, and info[2] says when there were none.
 *   rotation     front iff (R[2][0] d1[0] + R[2][1] d1[1]) + R[2][2] > 0 (the ray lies in front of camera 2); cosang as above (the
 *                angle that the rotation leaves between the two rays); there are no depths and no midpoint.
 * The chosen pose is the candidate with the most front rows among the used rows; ties go to the first in the order above.  No used row:
 * MI_DEGENSAC_POSE_EMPTY.  With a status other than OK and ROTATION the pose is twelve zeros, the info row is (0, 0, 0, 0, status) and no
 * row of the entry is written.  Ranges must not overlap.
 * Outputs:
 *   d_pose [K, 12]          R row-major, then t, of the chosen candidate (ROTATION: t = 0); goes into mi_degensac_pose_refine_lists_dev
 *                           (which answers t = 0 with REFINE_BAD_POSE) and mi_degensac_rotation_average_dev as the pose call's does
 *   d_front [cap] uint8     1 for the used rows that are front under the chosen candidate; every other position keeps 0
 *   d_info [K, 5] int32     rows used, front rows of the chosen candidate, the largest front count of the other three (ROTATION: 0), wide
 *                           rows (ROTATION: 0), status
 *   d_normal [K, 3]         n of the chosen candidate; zeros without a pose and for ROTATION
 *   d_t_over_d [K]          baseline over plane distance of the chosen candidate, before t was normalised; 0 likewise
 *   d_X [cap, 3], d_depth [cap, 2], d_cosang [cap]   (each nullable) as in the pose call; ROTATION writes cosang only
 *   d_cand [K, 4, 12], d_cand_normal [K, 4, 3], d_cand_front [K, 4] int32   (each nullable) all candidates and normals (zeros for
 *                           TRUNCATED, BAD_CAMERA, BAD_MODEL; ROTATION: slot 0 only) and their front counts (zeros unless OK or ROTATION)
 * One workgroup per entry, no atomics, counts by wave ballots and integer adds: the same bits on every call.  Asynchronous on `stream`;
 * the call needs no temporaries.  d_corr_offsets and d_cam_idx are device data and are checked on the device, not on the host.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_entries < 0; cap < 0 or > 0x3fffffff; n_cams < 0; a cos_min that is NaN or outside [-1, 1]; a rotation_eps that is NaN or < 0; NULL
 * d_corr_offsets; for n_entries > 0 NULL d_H or d_cams, then NULL d_pose, d_info, d_normal or d_t_over_d; for cap > 0 NULL d_pts or
 * d_front.  n_entries == 0 and cap == 0 succeed (with n_entries == 0 the fills are all that is written). */
enum { MI_DEGENSAC_POSE_ROTATION = 5 };
int mi_degensac_pose_h_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep /*nullable*/, const double *d_H,
                                 const double *d_cams, int n_cams, const int32_t *d_cam_idx /*nullable*/, int n_entries, int64_t cap,
                                 double cos_min, double rotation_eps, int device, void *stream, double *d_pose, uint8_t *d_front,
                                 int32_t *d_info, double *d_normal, double *d_t_over_d, double *d_X /*nullable*/, double *d_depth /*nullable*/,
                                 double *d_cosang /*nullable*/, double *d_cand /*nullable*/, double *d_cand_normal /*nullable*/,
                                 int32_t *d_cand_front /*nullable*/);
/* the same on host pointers (blocking): the inputs go to the device once, every output that is asked for comes back whole */
int mi_degensac_pose_h_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep /*nullable*/, const double *H,
                             const double *cams, int n_cams, const int32_t *cam_idx /*nullable*/, int n_entries, int64_t cap, double cos_min,
                             double rotation_eps, int device, double *pose, uint8_t *front, int32_t *info, double *normal, double *t_over_d,
                             double *X /*nullable*/, double *depth /*nullable*/, double *cosang /*nullable*/, double *cand /*nullable*/,
                             double *cand_normal /*nullable*/, int32_t *cand_front /*nullable*/);
/* the tile constants: which = 0 rows per workgroup and step of a row pass, 1 the cap on the grid (-1 for any other value) */
int mi_degensac_pose_h_tile(int which);

/* ---- refinement of relative poses on exported correspondence lists ---------------------------------------------------------------------
 * The pose call takes (R, t) from E = K2^T F K1 of an uncalibrated F, which is no essential matrix, and snaps it to one without looking
 * at the rows again.  This call follows it with what every structure-from-motion front end runs next: a Levenberg-Marquardt refinement
 * of the five degrees of freedom of (R, t / |t|) on the Sampson distance, in pixels, of the used rows.  Per list entry, on the device and
 * without a host synchronisation; rows, offsets, keep and cameras exactly as mi_degensac_pose_lists_dev takes them (the pose call's
 * d_front goes in as d_keep as it is), d_pose [K, 12] = R row-major then t as that call writes it.
 * Every step below is ONE IEEE float64 operation per written operator, no contraction; a sum of three terms is (a + b) + c, one of four
 * ((a + b) + c) + d.  Only + - * / sqrt, comparisons and |x| occur: no sin, cos, acos or exp.
 * Statuses, in their order of precedence:
 *   TRUNCATED    not 0 <= o[p] <= o[p + 1] <= cap
 *   BAD_CAMERA   i1 or i2 outside [0, n_cams), or an fx / fy that is zero or not finite (as in the pose call)
 *   BAD_POSE     one of the twelve pose numbers is not finite, or (t[0] t[0] + t[1] t[1]) + t[2] t[2] is not > 0 (the twelve zeros of a
 *                failed pose entry)
 *   SHORT        fewer than 5 used rows
 *   NOT_FINITE   the cost of the start pose is not finite
 *   CONVERGED, STALLED, MAX_TRIALS   the three ends of a run (below)
 * With one of the first five the pose is copied through unchanged (BAD_POSE: twelve zeros are written), both costs are NaN, no row of
 * d_resid is written, the info row is (used, 0, 0, status) with used = 0 for the first three.
 * Notation: cross(x, y) = (x[1] y[2] - x[2] y[1], x[2] y[0] - x[0] y[2], x[0] y[1] - x[1] y[0]); for a vector x and a matrix M,
 * [x]x M is the matrix whose column j is cross(x, column j of M); dot(x, x) = (x[0] x[0] + x[1] x[1]) + x[2] x[2].
 * Model at a pose (R, t) (t is used as it is given; the cost does not depend on its length):
 *   E = [t]x R
 *   i = the index of the smallest |t[i]|, ties to the lowest index; c = cross(e_i, t) written out: i = 0: (0, -t[2], t[1]), i = 1:
 *   (t[2], 0, -t[0]), i = 2: (-t[1], t[0], 0); u = c / sqrt(dot(c, c)) (three divisions); v = cross(t, u)
 *   five generators: G_0 = (0, E_2, -E_1), G_1 = (-E_2, 0, E_0), G_2 = (E_1, -E_0, 0) by columns (E_j = column j of E: G_k = E [e_k]x, the
 *   right-hand rotation R <- R C(w)), G_3 = [u]x R, G_4 = [v]x R.  The zero columns are stored as +0.0 and take part like any number.
 * Per used row, with d1 = ((x1 - cx1) / fx1, (y1 - cy1) / fy1, 1) and d2 likewise with camera 2, for a 3 x 3 matrix M define
 * epi(M) = (n, a0, a1, b0, b1):
 *   a[i] = (M[i][0] d1[0] + M[i][1] d1[1]) + M[i][2],  b[j] = (M[0][j] d2[0] + M[1][j] d2[1]) + M[2][j]   (b[2] is not needed)
 *   n = (d2[0] a[0] + d2[1] a[1]) + a[2];  a0 = a[0] / fx2, a1 = a[1] / fy2, b0 = b[0] / fx1, b1 = b[1] / fy1
 * With (n, a0, a1, b0, b1) = epi(E):  s = ((a0 a0 + a1 a1) + b0 b0) + b1 b1, q = sqrt(s), r = n / q: the signed Sampson distance of
 * F = K2^-T E K1^-1 in pixels.  With (n_k, c0, c1, e0, e1) = epi(G_k), k = 0 .. 4:
 *   h_k = ((a0 c0 + a1 c1) + b0 e0) + b1 e1,  J_k = n_k / q - (n h_k) / (s q)
 * The 21 sums of a pass, in this order: cost = sum r r; g_k = sum J_k r (k = 0 .. 4); A_kl = sum J_k J_l for k <= l in the order 00 01 02
 * 03 04 11 12 13 14 22 23 24 33 34 44.  Each sum: thread tau of the 256 adds the terms of the used rows i == tau (mod 256) of the entry
 * (i counted from the entry's first row) in ascending i into an accumulator that starts as +0.0; a row that is not used adds nothing.
 * Inside each wave of 64, for m = 32, 16, 8, 4, 2, 1: lane l < m takes v[l] + v[l + m]; lane 0 holds the wave's sum w.  The sum is
 * ((w0 + w1) + w2) + w3 over the four waves.
 * The run: lambda = 1e-3; one pass at the start pose gives cost, g, A (cost not finite: NOT_FINITE); the start cost is kept.  Then up to
 * max_trials trials; before each, if max_trials trials have run the status is MAX_TRIALS.  One trial:
 *   M[k][k] = A_kk + lambda A_kk, M[k][l] = A_lk for l < k.  Unpivoted Cholesky M = L L^T, for j = 0 .. 4: x = M[j][j], then x = x -
 *   L[j][k] L[j][k] for k = 0 .. j - 1 in turn; x not > 0 (a NaN included): the trial is REJECTED and has no pass; L[j][j] = sqrt(x); for
 *   i = j + 1 .. 4: x = M[i][j], x = x - L[i][k] L[j][k] for k = 0 .. j - 1 in turn, L[i][j] = x / L[j][j].
 *   y: for i = 0 .. 4: x = -g_i, x = x - L[i][k] y[k] for k = 0 .. i - 1 in turn, y[i] = x / L[i][i].
 *   delta: for i = 4 .. 0: x = y[i], x = x - L[k][i] delta[k] for k = i + 1 .. 4 in turn, delta[i] = x / L[i][i].
 *   w = delta[0 .. 2], a = 0.5 w, aa = dot(a, a), p = 1 - aa, d = 1 + aa; the Cayley rotation (exact, rational):
 *   C[i][i] = (p + w[i] a[i]) / d;  C[0][1] = (w[0] a[1] - w[2]) / d, C[0][2] = (w[0] a[2] + w[1]) / d, C[1][0] = (w[1] a[0] + w[2]) / d,
 *   C[1][2] = (w[1] a[2] - w[0]) / d, C[2][0] = (w[2] a[0] - w[1]) / d, C[2][1] = (w[2] a[1] + w[0]) / d
 *   R'[i][j] = (R[i][0] C[0][j] + R[i][1] C[1][j]) + R[i][2] C[2][j];  z[j] = (t[j] + delta[3] u[j]) + delta[4] v[j], t' = z /
 *   sqrt(dot(z, z)) (three divisions)
 *   one pass at (R', t') gives cost', g', A'.  ACCEPTED iff cost' < cost (a NaN is not), else REJECTED.
 *   accepted: the pose and its sums become the current ones; lambda = max(lambda / 10, 1e-12); if (cost - cost') <= ftol cost with the
 *   cost before the step, the status is CONVERGED.  rejected: lambda = 10 lambda; if lambda > 1e12 the status is STALLED.
 * max_trials = 0 scores only (MAX_TRIALS, end cost = start cost).
 * Outputs:
 *   d_pose_out [K, 12]      the final pose; may be d_pose itself (an entry reads its twelve numbers before it writes them), must not
 *                           overlap it otherwise
 *   d_cost [K, 2]           cost at the start and at the final pose
 *   d_info [K, 4] int32     used rows, trials run (rejected ones included), trials accepted, status
 *   d_resid [cap]           (nullable) r of the used rows under the final pose, from one more pass; every other position keeps NaN
 *   d_F [K, 9]              (nullable) F = K2^-T E K1^-1 of the final pose (x2^T F x1 = 0, row-major): H[i][0] = E[i][0] / fx1, H[i][1] =
 *                           E[i][1] / fy1, H[i][2] = (E[i][2] - H[i][0] cx1) - H[i][1] cy1; F[0][j] = H[0][j] / fx2, F[1][j] = H[1][j] /
 *                           fy2, F[2][j] = (H[2][j] - F[0][j] cx2) - F[1][j] cy2.  Nine zeros for TRUNCATED, BAD_CAMERA and BAD_POSE;
 *                           for SHORT and NOT_FINITE the F of the pose that was copied through.
 * One workgroup of 256 threads per entry, no atomics, a fixed order of every sum: the same bits on every call.  Asynchronous on `stream`;
 * no temporaries.  Ranges must not overlap.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_entries < 0; cap < 0 or > 0x3fffffff; n_cams < 0; max_trials outside 0 .. 100; an ftol that is NaN or < 0; NULL d_corr_offsets; for
 * n_entries > 0 NULL d_pose or d_cams, then NULL d_pose_out, d_cost or d_info; for cap > 0 NULL d_pts.  n_entries == 0 and cap == 0
 * succeed (with n_entries == 0 the NaN fill of d_resid is all that is written). */
enum { MI_DEGENSAC_REFINE_CONVERGED = 0, MI_DEGENSAC_REFINE_STALLED = 1, MI_DEGENSAC_REFINE_MAX_TRIALS = 2, MI_DEGENSAC_REFINE_SHORT = 3,
       MI_DEGENSAC_REFINE_NOT_FINITE = 4, MI_DEGENSAC_REFINE_BAD_POSE = 5, MI_DEGENSAC_REFINE_BAD_CAMERA = 6,
       MI_DEGENSAC_REFINE_TRUNCATED = 7 };
int mi_degensac_pose_refine_lists_dev(const double *d_pts, const int64_t *d_corr_offsets, const uint8_t *d_keep /*nullable*/,
                                      const double *d_pose, const double *d_cams, int n_cams, const int32_t *d_cam_idx /*nullable*/,
                                      int n_entries, int64_t cap, int max_trials, double ftol, int device, void *stream,
                                      double *d_pose_out, double *d_cost, int32_t *d_info, double *d_resid /*nullable*/,
                                      double *d_F /*nullable*/);
/* the same on host pointers (blocking): the inputs go to the device once, every output that is asked for comes back whole */
int mi_degensac_pose_refine_lists(const double *pts, const int64_t *corr_offsets, const uint8_t *keep /*nullable*/, const double *pose,
                                  const double *cams, int n_cams, const int32_t *cam_idx /*nullable*/, int n_entries, int64_t cap,
                                  int max_trials, double ftol, int device, double *pose_out, double *cost, int32_t *info,
                                  double *resid /*nullable*/, double *F /*nullable*/);
/* the tile constants: which = 0 rows per workgroup and step of a row pass, 1 the cap on the grid (-1 for any other value) */
int mi_degensac_pose_refine_tile(int which);

/* ---- triangulation of tracks under known camera poses (mi_triangulate.hip) ------------------------------------------------------------
 * The tracks call ends the pair-list pipeline with tables nobody consumed.  With poses from elsewhere (a previous reconstruction, a SLAM
 * front end, a rig, GPS/INS) every track becomes a 3-D point with its reprojection errors: hloc's triangulation.py, COLMAP's
 * point_triangulator.  Per track, on the device and without a host synchronisation: ranges and the number of tracks are read from
 * device memory.
 * Inputs (device arrays on one device), the first four exactly as mi_degensac_tracks_dev writes them, fills included:
 *   d_track_offsets [T + 1] int64   track k owns the positions o[k] .. o[k + 1] of d_obs / d_obs_image (T = n_tracks_max)
 *   d_obs [M] int32                 store rows (M = n_obs_max), d_obs_image [M] int32 their images; the -1 of the tails is never an index
 *   d_n_tracks [1] int64            (nullable: all T) only the first min(max(*d_n_tracks, 0), T) tracks are triangulated; every later one
 *                                   gets the outputs of an empty track: X, cost, cosang NaN, info (0, 0, 0, 0, SHORT)
 *   d_kps [rows, 2] float64         x, y per row of the ONE store the tracks were built on
 *   d_cams [n_images, 4] float64    pinhole fx, fy, cx, cy per image, as the pose call takes them
 *   d_poses [n_images, 12] float64  R row-major, then t: world to camera, X_cam = R X + t (the layout of d_pose)
 * Every step below is ONE IEEE float64 operation per written operator, no contraction; a sum of three terms is (a + b) + c, one of four
 * ((a + b) + c) + d.  Only + - * / sqrt, comparisons and |x| occur on the device.
 * Statuses, in their order of precedence:
 *   TRUNCATED    not 0 <= o[k] <= o[k + 1] <= M.  Nothing of the track is read; info (0, 0, 0, 0, TRUNCATED).
 *   SHORT        fewer than two USED observations.  The observation at position p is used when m = d_obs_image[p] lies in [0, n_images),
 *                r = d_obs[p] lies in [0, rows), x, y = d_kps[r] are finite, the twelve numbers of d_poses[m] are finite, and fx, fy of
 *                d_cams[m] are finite and not zero.  Anything else is skipped and never used as an index.  Two keypoints of one image
 *                are two observations.  info (used, 0, 0, 0, SHORT).
 *   DEGENERATE   the 3 x 3 system of the linear point is not positive definite, or the linear point is not finite.  info (used, 0, 0, 0,
 *                DEGENERATE).
 *   NARROW       a point exists and cosang > cos_min, cos_min = cos(min_angle_deg * (3.141592653589793 / 180.0)) by the C library's cos on
 *                the host.  Every output is written as for OK.
 *   OK
 * With one of the first three X, both costs and cosang are NaN and no position of d_err, d_ok, d_depth is written.
 * Per used observation: d0 = (x - cx) / fx, d1 = (y - cy) / fy; v[j] = (R[0][j] d0 + R[1][j] d1) + R[2][j] (R^T d with d[2] = 1);
 *   nn = sqrt((v[0] v[0] + v[1] v[1]) + v[2] v[2]); the unit ray w[j] = v[j] / nn;
 *   the centre c[j] = -((R[0][j] t[0] + R[1][j] t[1]) + R[2][j] t[2]);
 *   P = I - w w^T as P00 = 1 - w[0] w[0], P01 = -(w[0] w[1]), P02 = -(w[0] w[2]), P11 = 1 - w[1] w[1], P12 = -(w[1] w[2]), P22 = 1 - w[2] w[2];
 *   q[0] = (P00 c[0] + P01 c[1]) + P02 c[2], q[1] = (P01 c[0] + P11 c[1]) + P12 c[2], q[2] = (P02 c[0] + P12 c[1]) + P22 c[2].
 * The linear point (the N-view midpoint): the nine sums A = sum P in the order 00 01 02 11 12 22 and b = sum q; X = solve(A, b).
 * solve(M, r), M symmetric: the unpivoted Cholesky factor L00 = sqrt(M00), L10 = M01 / L00, L20 = M02 / L00, p = M11 - L10 L10, L11 =
 *   sqrt(p), L21 = (M12 - L20 L10) / L11, p = M22 - L20 L20, p = p - L21 L21, L22 = sqrt(p); a pivot (M00 and the two p) that is not > 0, a
 *   NaN included, FAILS the solve.  y0 = r[0] / L00, y1 = (r[1] - L10 y0) / L11, y2 = ((r[2] - L20 y0) - L21 y1) / L22; x[2] = y2 / L22,
 *   x[1] = (y1 - L21 x[2]) / L11, x[0] = ((y0 - L10 x[1]) - L20 x[2]) / L00.
 * One pass at a point X, per used observation: Xc = ((R[0][0] X[0] + R[0][1] X[1]) + R[0][2] X[2]) + t[0], Yc and Zc likewise with rows 1
 *   and 2; u = Xc / Zc, v = Yc / Zc; the residual rx = (fx u + cx) - x, ry = (fy v + cy) - y;
 *   ax = fx / Zc, ex = (fx u) / Zc, ay = fy / Zc, ey = (fy v) / Zc; the Jacobian with respect to X: Jx[j] = ax R[0][j] - ex R[2][j], Jy[j] =
 *   ay R[1][j] - ey R[2][j].
 *   The ten sums of a pass, each term ONE sum of two products: cost = sum (rx rx + ry ry); H_jk = sum (Jx[j] Jx[k] + Jy[j] Jy[k]) in the
 *   order 00 01 02 11 12 22; g_j = sum (Jx[j] rx + Jy[j] ry).
 * The run: one pass at the linear point gives cost, H, g; that cost is d_cost[k][0].  Then, while fewer than max_iters trials have been
 *   made: delta = solve(H, g); a failed solve ends the run (it is no trial).  The trial point is X'[j] = X[j] - delta[j]; one pass at X'
 *   gives cost', H', g'.  The trial is ACCEPTED iff cost' is finite and cost' < cost; the first trial that is not ends the run and the
 *   current point stays.  Accepted: X', cost', H', g' become the current ones; if (cost - cost') <= ftol cost with the cost before the
 *   step, the run ends.  max_iters = 0 returns the linear point.  A run is trials + 1 passes.
 * At the final point, per used observation: err = sqrt(rx rx + ry ry), depth = Zc, front = Zc > 0 (a NaN is not front), ok = front and
 *   err <= max_reproj_px.
 * cosang = the minimum of (w_i[0] w_j[0] + w_i[1] w_j[1]) + w_i[2] w_j[2] over the pairs i != j of used observations: the products
 *   commute, so it does not depend on an order.
 * The order of every sum (A, b, cost, H, g), with G = mi_degensac_triangulate_tile(0) lanes per track: lane l adds the terms of the used
 *   observations at the positions i == l (mod G) of the track (i counted from o[k]) in ascending i into an accumulator that starts as
 *   +0.0; an observation that is not used adds nothing.  Then for m = G / 2, G / 4, .., 1: every lane l takes v[l] + v[l xor m].  IEEE
 *   addition commutes, so all lanes hold the same bits: the tree in which lane 0 takes v[0] + v[m] with v[0] and v[m] the sums of the
 *   step before.  The counts are integer sums.
 * Outputs (T rows each, M positions each for the last three):
 *   d_X [T, 3]              the point in the world frame
 *   d_info [T, 5] int32     used observations, ok observations at the final point, accepted steps, trial steps, status
 *   d_cost [T, 2]           the cost in px^2 over the used observations at the linear and at the final point
 *   d_cosang [T]
 *   d_err [M], d_ok [M] uint8, d_depth [M]   (each nullable) per used observation of a track with a point; every other position, the
 *                           positions no track owns included, keeps NaN, 0, NaN
 * A group of G lanes per track, tracks by a grid stride over at most mi_degensac_triangulate_tile(1) workgroups of tile(2) groups; the
 * pair pass stages tile(3) unit rays at a time in LDS and recomputes them per chunk for a longer track, so a track of any length
 * works.  The pair pass is quadratic: a track of n observations costs n (n - 1) / 2 products inside its one group and, beyond tile(3)
 * observations, restages the rays once per pair of chunks, so one very long track holds its workgroup for that long (2049 observations:
 * 2.1 million products).  No atomics, no group waits for another: the same bits on every call.  Asynchronous on `stream`; no
 * temporaries.  Ranges must not overlap when d_err, d_ok or d_depth is given.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_tracks_max < 0 or > 0x3fffffff; n_obs_max < 0 or > 0x3fffffff; rows < 0 or > 0x7fffffff; n_images < 0; a min_angle_deg that is NaN or
 * outside [0, 180]; a max_reproj_px that is NaN or < 0; max_iters outside 0 .. 100; an ftol that is NaN or < 0; NULL d_track_offsets; for
 * n_obs_max > 0 NULL d_obs or d_obs_image; for n_tracks_max > 0 NULL d_X, d_info, d_cost or d_cosang; for rows > 0 NULL d_kps; for
 * n_images > 0 NULL d_cams or d_poses.  n_tracks_max == 0 and n_obs_max == 0 succeed (with n_tracks_max == 0 the fills of d_err, d_ok
 * and d_depth are all that is written). */
enum { MI_DEGENSAC_TRI_OK = 0, MI_DEGENSAC_TRI_NARROW = 1, MI_DEGENSAC_TRI_DEGENERATE = 2, MI_DEGENSAC_TRI_SHORT = 3,
       MI_DEGENSAC_TRI_TRUNCATED = 4 };
int mi_degensac_triangulate_tracks_dev(const int64_t *d_track_offsets, const int32_t *d_obs, const int32_t *d_obs_image,
                                       const int64_t *d_n_tracks /*nullable*/, const double *d_kps, int64_t rows, const double *d_cams,
                                       const double *d_poses, int n_images, int64_t n_tracks_max, int64_t n_obs_max, double min_angle_deg,
                                       double max_reproj_px, int max_iters, double ftol, int device, void *stream, double *d_X,
                                       int32_t *d_info, double *d_cost, double *d_cosang, double *d_err /*nullable*/,
                                       uint8_t *d_ok /*nullable*/, double *d_depth /*nullable*/);
/* the same on host pointers (blocking): the inputs go to the device once, every output that is asked for comes back whole; n_tracks is
 * passed by value, < 0 = all n_tracks_max */
int mi_degensac_triangulate_tracks(const int64_t *track_offsets, const int32_t *obs, const int32_t *obs_image, int64_t n_tracks,
                                   const double *kps, int64_t rows, const double *cams, const double *poses, int n_images,
                                   int64_t n_tracks_max, int64_t n_obs_max, double min_angle_deg, double max_reproj_px, int max_iters,
                                   double ftol, int device, double *X, int32_t *info, double *cost, double *cosang,
                                   double *err /*nullable*/, uint8_t *ok /*nullable*/, double *depth /*nullable*/);
/* the tile constants: which = 0 G = lanes per track, 1 the cap on the grid, 2 tracks (groups) per workgroup, 3 rays per staging area of
 * the pair pass (-1 for any other value) */
int mi_degensac_triangulate_tile(int which);

/* ---- refinement of camera poses against triangulated tracks (mi_camera_refine.hip) -----------------------------------------------------
 * The triangulation takes the poses as exact and gives every track a point; this call is the other block of the reprojection problem:
 * with the points held fixed, every camera's six degrees of freedom are refined on the reprojection error, in pixels, of its
 * observations (COLMAP's pose refinement after registration, the motion-only step of a SLAM back end).  Alternated with the
 * triangulation it is a block-coordinate bundle adjustment on the device with no host read between the steps.  Per image, on the device
 * and without a host synchronisation: ranges, the number of tracks and the number of observations per image are read from device memory.
 * Inputs (device arrays on one device): d_track_offsets [T + 1], d_obs [M], d_obs_image [M], d_n_tracks [1] (nullable: all T), d_kps
 * [rows, 2], d_cams [n_images, 4] and d_poses [n_images, 12] exactly as mi_degensac_triangulate_tracks_dev takes them, and
 *   d_X [T, 3] float64              the points as that call wrote them; a row with a number that is not finite is simply not used
 *   d_obs_keep [M] uint8            (nullable: all) the position p is used only where d_obs_keep[p] != 0; the triangulation's d_ok goes in
 *                                   as it is, and with it every used observation lies in front of its camera at the start
 *   d_refine [n_images] uint8       (nullable: all) an image with 0 is scored but not moved (status FIXED): this fixes the gauge when a
 *                                   caller alternates with the triangulation
 * Every step below is ONE IEEE float64 operation per written operator, no contraction; a sum of three terms is (a + b) + c.  Only + - * /
 * sqrt, comparisons and |x| occur on the device.
 * Used observations.  Let nt = min(max(*d_n_tracks, 0), T).  Track k < nt with 0 <= o[k] <= o[k + 1] <= M owns the positions o[k] ..
 * o[k + 1]; a track with another pair of offsets owns nothing.  The owned position p of track k is USED by image m = d_obs_image[p] when m
 * lies in [0, n_images), r = d_obs[p] lies in [0, rows), x, y = d_kps[r] are finite, the three numbers of d_X[k] are finite and d_obs_keep
 * allows p.  Anything else is skipped and never used as an index.  Whether a position is used does not depend on a pose or a camera.
 * The used observations of an image are ordered by ascending position p: that is the order i = 0, 1, .. of every sum below and of
 * d_img_obs.  The ranges of two tracks must not overlap.
 * Statuses of an image, in their order of precedence:
 *   BAD_CAMERA   fx or fy of d_cams[m] is zero or not finite
 *   BAD_POSE     one of the twelve numbers of d_poses[m] is not finite
 *   SHORT        fewer than 3 used observations
 *   NOT_FINITE   the cost of the start pose is not finite
 *   BEHIND       a used observation has a Zc that is not > 0 (a NaN included) at the start pose
 *   FIXED        d_refine[m] == 0: the start pose is scored, both costs are that cost, no trial is made
 *   CONVERGED, STALLED, MAX_TRIALS   the three ends of a run (below)
 * With one of the first five the pose is copied through unchanged (its bytes, whatever they are) and no position of d_err is written;
 * both costs are NaN for the first four, and for BEHIND both are the cost of the start pose (it is finite, or the status would be
 * NOT_FINITE).  The info row is (used, trials, accepted, status) with the used observations of the image whatever the status, and 0
 * trials for everything but the three ends of a run.
 * One pass at a pose (R, t), per used observation with its point X and keypoint x, y:
 *   P[i] = (R[i][0] X[0] + R[i][1] X[1]) + R[i][2] X[2];  Xc = P[0] + t[0], Yc = P[1] + t[1], Zc = P[2] + t[2]  (the triangulation's Xc, Yc,
 *   Zc, with the name P for the sum before t is added);  u = Xc / Zc, v = Yc / Zc;  rx = (fx u + cx) - x, ry = (fy v + cy) - y;
 *   ax = fx / Zc, ex = (fx u) / Zc, ay = fy / Zc, ey = (fy v) / Zc  (all as in the triangulation's pass).
 *   The update is a rotation on the left and a free translation, R' = C(w) R, t' = t + tau, so that X_cam' = C(w) (R X) + t + tau and at
 *   w = tau = 0 the derivative of X_cam is -[P]x with respect to w and I with respect to tau.  The Jacobian of (rx, ry) with respect to
 *   (w[0], w[1], w[2], tau[0], tau[1], tau[2]):
 *     Jx = (-(ex P[1]),  ax P[2] + ex P[0],  -(ax P[1]),  ax,  0,  -ex)
 *     Jy = (-(ay P[2] + ey P[1]),  ey P[0],  ay P[0],  0,  ay,  -ey)
 *   The two zeros are +0.0 and take part like any number.
 *   The 28 sums of a pass, each term ONE sum of two products, in this order: cost = sum (rx rx + ry ry); g_k = sum (Jx[k] rx + Jy[k] ry)
 *   for k = 0 .. 5; A_kl = sum (Jx[k] Jx[l] + Jy[k] Jy[l]) for k <= l in the order 00 01 02 03 04 05 11 12 13 14 15 22 23 24 25 33 34 35
 *   44 45 55.  Each sum: thread tau of the 256 adds the terms of the image's used observations i == tau (mod 256) in ascending i into an
 *   accumulator that starts as +0.0.  Inside each wave of 64, for m = 32, 16, 8, 4, 2, 1: lane l < m takes v[l] + v[l + m]; lane 0 holds
 *   the wave's sum w.  The sum is ((w0 + w1) + w2) + w3 over the four waves.  A pass also counts, as an integer, the used observations
 *   whose Zc is not > 0: `behind`.
 * The run: lambda = 1e-3; one pass at the start pose gives cost, g, A and behind (cost not finite: NOT_FINITE; else behind > 0: BEHIND;
 * else d_refine[m] == 0: FIXED); the start cost is kept.  Then up to max_trials trials; before each, if max_trials trials have run the
 * status is MAX_TRIALS.  One trial is the trial of mi_degensac_pose_refine_lists_dev with 6 in place of 5:
 *   M[k][k] = A_kk + lambda A_kk, M[k][l] = A_lk for l < k.  Unpivoted Cholesky M = L L^T, for j = 0 .. 5: x = M[j][j], then x = x -
 *   L[j][k] L[j][k] for k = 0 .. j - 1 in turn; x not > 0 (a NaN included): the trial is REJECTED and has no pass; L[j][j] = sqrt(x); for
 *   i = j + 1 .. 5: x = M[i][j], x = x - L[i][k] L[j][k] for k = 0 .. j - 1 in turn, L[i][j] = x / L[j][j].
 *   y: for i = 0 .. 5: x = -g_i, x = x - L[i][k] y[k] for k = 0 .. i - 1 in turn, y[i] = x / L[i][i].
 *   delta: for i = 5 .. 0: x = y[i], x = x - L[k][i] delta[k] for k = i + 1 .. 5 in turn, delta[i] = x / L[i][i].
 *   w = delta[0 .. 2], C = C(w) the Cayley rotation written out there (a = 0.5 w, aa = dot(a, a), p = 1 - aa, d = 1 + aa, ..).
 *   R'[i][j] = (C[i][0] R[0][j] + C[i][1] R[1][j]) + C[i][2] R[2][j];  t'[j] = t[j] + delta[3 + j].
 *   one pass at (R', t') gives cost', g', A', behind'.  ACCEPTED iff cost' < cost (a NaN is not) and behind' == 0, else REJECTED.
 *   accepted: the pose and its sums become the current ones; lambda = max(lambda / 10, 1e-12); if (cost - cost') <= ftol cost with the
 *   cost before the step, the status is CONVERGED.  rejected: lambda = 10 lambda; if lambda > 1e12 the status is STALLED.
 * max_trials = 0 scores only (MAX_TRIALS, end cost = start cost).
 * Outputs:
 *   d_poses_out [n_images, 12]   the final pose; may be d_poses itself (an image reads only its own twelve numbers, before it writes
 *                                them), must not overlap it otherwise
 *   d_cost [n_images, 2]         cost in px^2 at the start and at the final pose
 *   d_info [n_images, 4] int32   used observations, trials run (rejected ones included), trials accepted, status
 *   d_err [M]                    (nullable) sqrt(rx rx + ry ry) of the used observations of an image with one of the last four statuses
 *                                at its final pose, from one more pass, at the observation's TRACK-MAJOR position p, next to the
 *                                triangulation's d_err; every other position keeps NaN
 *   d_img_offsets [n_images + 1] int64, d_img_obs [M] int32   (each nullable) the image-major table the call builds: image m owns
 *                                d_img_obs[io[m] .. io[m + 1]], the positions p of its used observations in ascending order;
 *                                io[n_images] is the number of used observations, and every element of d_img_obs behind it is -1
 * Kernels: a fill and `mark` (the sort key of every position: its image when it is used, else n_images; and the track that owns it),
 * a stable rocprim::radix_sort_pairs of (key, position) over the key bits, `bounds` (io[m] = the lower bound of m in the sorted keys) and
 * `refine`: one workgroup of 256 threads per image, images by a grid stride over at most mi_degensac_camera_refine_tile(1) workgroups.
 * No atomics, no workgroup waits for another, a fixed order of every sum: the same bits on every call.  Asynchronous on `stream`; the
 * temporaries (20 bytes per position and rocprim's) are taken and returned stream-ordered.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_tracks_max < 0 or > 0x3fffffff; n_obs_max < 0 or > 0x3fffffff; rows < 0 or > 0x7fffffff; n_images < 0; max_trials outside 0 .. 100;
 * an ftol that is NaN or < 0; NULL d_track_offsets; for n_obs_max > 0 NULL d_obs or d_obs_image; for rows > 0 NULL d_kps; for
 * n_tracks_max > 0 NULL d_X; for n_images > 0 NULL d_cams or d_poses, then NULL d_poses_out, d_cost or d_info.  n_tracks_max == 0,
 * n_obs_max == 0 and n_images == 0 succeed: without observations every image is SHORT (or has a bad camera or pose); without images the
 * fills of d_err (NaN), d_img_offsets (one 0) and d_img_obs (-1) are all that is written, and with n_obs_max == 0 as well nothing is
 * written and no device is looked for. */
enum { MI_DEGENSAC_CAMREF_CONVERGED = 0, MI_DEGENSAC_CAMREF_STALLED = 1, MI_DEGENSAC_CAMREF_MAX_TRIALS = 2, MI_DEGENSAC_CAMREF_FIXED = 3,
       MI_DEGENSAC_CAMREF_BEHIND = 4, MI_DEGENSAC_CAMREF_NOT_FINITE = 5, MI_DEGENSAC_CAMREF_SHORT = 6, MI_DEGENSAC_CAMREF_BAD_POSE = 7,
       MI_DEGENSAC_CAMREF_BAD_CAMERA = 8 };
int mi_degensac_camera_refine_tracks_dev(const int64_t *d_track_offsets, const int32_t *d_obs, const int32_t *d_obs_image,
                                         const int64_t *d_n_tracks /*nullable*/, const double *d_kps, int64_t rows, const double *d_cams,
                                         const double *d_poses, int n_images, const double *d_X, const uint8_t *d_obs_keep /*nullable*/,
                                         const uint8_t *d_refine /*nullable*/, int64_t n_tracks_max, int64_t n_obs_max, int max_trials,
                                         double ftol, int device, void *stream, double *d_poses_out, double *d_cost, int32_t *d_info,
                                         double *d_err /*nullable*/, int64_t *d_img_offsets /*nullable*/, int32_t *d_img_obs /*nullable*/);
/* the same on host pointers (blocking): the inputs go to the device once, every output that is asked for comes back whole; n_tracks is
 * passed by value, < 0 = all n_tracks_max */
int mi_degensac_camera_refine_tracks(const int64_t *track_offsets, const int32_t *obs, const int32_t *obs_image, int64_t n_tracks,
                                     const double *kps, int64_t rows, const double *cams, const double *poses, int n_images, const double *X,
                                     const uint8_t *obs_keep /*nullable*/, const uint8_t *refine /*nullable*/, int64_t n_tracks_max,
                                     int64_t n_obs_max, int max_trials, double ftol, int device, double *poses_out, double *cost,
                                     int32_t *info, double *err /*nullable*/, int64_t *img_offsets /*nullable*/, int32_t *img_obs /*nullable*/);
/* the tile constants: which = 0 observations per workgroup and step of a row pass, 1 the cap on the grid of `refine`, 2 lanes per track
 * of `mark` (-1 for any other value) */
int mi_degensac_camera_refine_tile(int which);

/* ---- rotation averaging: global camera rotations from pairwise poses (mi_rotavg.hip) -----------------------------------------------------
 * The pose calls end with one (R, t) per PAIR, the track calls start from one world-to-camera pose per IMAGE.  This call is the first step
 * between them, the one global structure-from-motion front ends run first: from the two-view graph one rotation per image, and per pair
 * the cosine of the angle by which its relative rotation disagrees with them (the usual filter for pairs whose pose is wrong).  Camera
 * positions (translation averaging) are not part of it.  On the device and without a host synchronisation: the host never learns how
 * many sweeps were needed.
 * Inputs (device arrays on one device):
 *   d_pairs [K, 2] int32, d_R_rel [K, 9] float64   edge e joins the images i = pairs[e][0] and j = pairs[e][1] of ONE store of n_images
 *                                   images, X_j = R_rel[e] X_i: the pair list and the R of mi_degensac_pose_lists_dev /
 *                                   mi_degensac_pose_refine_lists_dev (the first nine numbers of their pose rows, so d_R_rel is read with
 *                                   a row length of 9: pass a compact copy)
 *   d_weight [K] float64            (nullable: 1) e.g. the wide rows of the pose call's info
 *   d_edge_keep [K] uint8           (nullable: all)
 *   d_R0 [n_images, 9], d_known [n_images] uint8   (both or neither) the cameras with d_known != 0 start SET with the nine numbers of
 *                                   d_R0 (their bytes, whatever they are) and are never moved.  With neither, camera `root` starts set
 *                                   with the identity and is never moved.  Such a camera is called KNOWN below.
 * Every step below is ONE IEEE float64 operation per written operator, no contraction; a sum of three terms is (a + b) + c.  Only + - * /
 * and comparisons occur on the device.
 * Used edges.  Edge e is USED when d_edge_keep[e] != 0, i and j lie in [0, n_images), i != j, d_weight[e] > 0 and finite, and
 * |s - 3| <= 1e-6 for s = the sum of r r over the nine numbers of R_rel[e] in their order (the zeros of a failed pose entry, a NaN and an
 * infinity fail it).  Anything else is unused and never used as an index.  Repeats and both orientations of a pair are separate edges.
 * Half-edges.  Edge e has the half-edges h = 2 e (camera i, other end j) and h = 2 e + 1 (camera j, other end i).  The half-edges of the
 * used edges are grouped by camera, ascending in h inside a camera: position 0, 1, .. deg - 1 of the camera.
 * State.  Per camera `set` (with the sweep in which it was set), a matrix R, `step` and `opposed`, in two buffers.  At the start a known
 * camera is set in sweep 0 with its matrix, every other camera is not set and has zeros; step is NaN and opposed 0 for all.  Sweep s =
 * 1, 2, .. reads the state sweep s - 1 left and nothing else (Jacobi: the result cannot depend on scheduling).  Per camera c:
 *   known: copied.
 *   The prediction of c over the half-edge h of edge e with other end o:  P = R_rel[e] R_o for h odd (c is the second image), P =
 *   R_rel[e]^T R_o for h even.  Every 3 x 3 product here is P[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j].
 *   not set: among its half-edges whose other end is set, the one with the largest weight, ties to the lowest position; R_c = its
 *     prediction, c is set in sweep s (a max-weight breadth-first start, one level per sweep).  Without one the camera is copied.
 *   set and not known: per half-edge whose other end is set, Q = P R_c^T (Q[i][j] = (P[i][0] R_c[j][0] + P[i][1] R_c[j][1]) + P[i][2]
 *     R_c[j][2]), q = 1 + ((Q[0][0] + Q[1][1]) + Q[2][2]).  If q > 2^-10 does not hold (a NaN included) the half-edge is OPPOSED: it is
 *     counted and adds nothing.  Else w = ((Q[2][1] - Q[1][2]) / q, (Q[0][2] - Q[2][0]) / q, (Q[1][0] - Q[0][1]) / q): the vector a with
 *     Q = Ca(a) for the rational Cayley map Ca(a) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), |a| = tan(angle / 2).  (The C(w) of
 *     the two refinements is Ca(0.5 w).)  m = (w0 w0 + w1 w1) + w2 w2.  f = weight, or with a robust_deg f = weight (g g) for g = s2 /
 *     (s2 + m), s2 = sigma sigma, sigma = tan(robust_deg pi / 360) computed once on the host.  The sums S = sum f and W_k = sum (f w_k):
 *     lane l of G = mi_degensac_rotation_average_tile(0) adds the terms of the positions l, l + G, .. in ascending order into an
 *     accumulator that starts as +0.0; then for m = G / 2, .., 2, 1 every lane takes v[l] + v[l xor m].  If S > 0: u_k = W_k / S, step_c =
 *     (u0 u0 + u1 u1) + u2 u2, a_k = damping u_k, b_k = a_k + a_k, aa = (a0 a0 + a1 a1) + a2 a2, p = 1 - aa, d = 1 + aa,
 *       C = ((p + b0 a0) / d, (b0 a1 - b2) / d, (b0 a2 + b1) / d;  (b1 a0 + b2) / d, (p + b1 a1) / d, (b1 a2 - b0) / d;
 *            (b2 a0 - b1) / d, (b2 a1 + b0) / d, (p + b2 a2) / d),   R_c <- C R_c.
 *     Otherwise R_c and step_c are copied.  opposed_c = the count of this sweep (0 for a camera that is known, not set, or set in s).
 *   damping = 0.5 is the lazy Jacobi step: it cannot oscillate on a bipartite graph, which the full step can.
 * Convergence.  Sweep s CHANGED something when it set a camera or gave some step_c > tol tol.  changed[0] = 1.  A sweep that finds
 * changed[s - 1] == 0 does nothing, and so does every later one; the outputs are the state after the last sweep that did something:
 * the first one that changed nothing, or sweep `sweeps`.  All `sweeps` launches are queued.
 * Outputs:
 *   d_R [n_images, 9]            the world-to-camera rotation; zeros for a camera that was never set
 *   d_info [n_images, 4] int32   (half-edges of used edges, the sweep in which the camera was set: 0 known, -1 never, opposed half-edges
 *                                in the last sweep that ran, status).  KNOWN; OK = set by the call; UNREACHED = has half-edges but
 *                                was not set; ISOLATED = not known and no half-edge
 *   d_step [n_images]            the last step_c the camera was given, NaN where none was
 *   d_summary [4] int64          (sweeps that changed something, cameras set, edges used, global status).  NO_ROOT = no known camera;
 *                                else CONVERGED = a sweep changed nothing; else MAX_SWEEPS (sweeps == 0 included)
 *   d_edge_cos [K]               (nullable) for a used edge whose two ends are set c = ((d0 + d1) + d2 - 1) / 2 with T = R_rel[e] R_i and
 *                                d_k = (T[k][0] R_j[k][0] + T[k][1] R_j[k][1]) + T[k][2] R_j[k][2]: the cosine of the angle between
 *                                R_rel and R_j R_i^T.  NaN elsewhere
 * Kernels: `mark` (the key of every half-edge: its camera, or n_images for an unused edge), a stable rocprim::radix_sort_pairs of (key,
 * half-edge) over the key bits, `init` (off[c] = the lower bound of c in the sorted keys, and the start state), one `sweep` launch per
 * sweep (G lanes per camera, 256 / G cameras per workgroup, further cameras by a grid stride over at most
 * mi_degensac_rotation_average_tile(1) workgroups, no barrier; the only atomic is the integer OR into changed[s]) and `finish` (an
 * integer add for the cameras set).  The same bits on every call.  Asynchronous on `stream`; the temporaries (16 bytes per
 * half-edge, 180 per camera, 4 per sweep and rocprim's) are taken and returned stream-ordered.
 * Refused with MI_DEGENSAC_EINVAL and a message in mi_degensac_match_last_error(), before a device is looked for and in this order:
 * n_images outside 1 .. 2^24; n_pairs < 0 or > 0x3fffffff; sweeps outside 0 .. 4096; a damping outside (0, 1]; a robust_deg that is
 * neither 0 (= no robust factor) nor in (0, 180); a tol that is NaN or < 0; root outside [0, n_images) (also when d_known is given);
 * for n_pairs > 0 NULL d_pairs or d_R_rel; exactly one of d_R0 and d_known; NULL d_R, d_info, d_step or d_summary.  n_pairs == 0
 * succeeds: every camera is KNOWN or ISOLATED. */
enum { MI_DEGENSAC_ROTAVG_KNOWN = 0, MI_DEGENSAC_ROTAVG_OK = 1, MI_DEGENSAC_ROTAVG_UNREACHED = 2, MI_DEGENSAC_ROTAVG_ISOLATED = 3 };
enum { MI_DEGENSAC_ROTAVG_CONVERGED = 0, MI_DEGENSAC_ROTAVG_MAX_SWEEPS = 1, MI_DEGENSAC_ROTAVG_NO_ROOT = 2 };
int mi_degensac_rotation_average_dev(const int32_t *d_pairs, const double *d_R_rel, const double *d_weight /*nullable*/,
                                     const uint8_t *d_edge_keep /*nullable*/, int64_t n_pairs, int n_images, const double *d_R0 /*nullable*/,
                                     const uint8_t *d_known /*nullable*/, int root, int sweeps, double damping, double robust_deg, double tol,
                                     int device, void *stream, double *d_R, int32_t *d_info, double *d_step, int64_t *d_summary,
                                     double *d_edge_cos /*nullable*/);
/* the same on host pointers (blocking): the inputs go to the device once, every output that is asked for comes back whole */
int mi_degensac_rotation_average(const int32_t *pairs, const double *R_rel, const double *weight /*nullable*/,
                                 const uint8_t *edge_keep /*nullable*/, int64_t n_pairs, int n_images, const double *R0 /*nullable*/,
                                 const uint8_t *known /*nullable*/, int root, int sweeps, double damping, double robust_deg, double tol, int device,
                                 double *R, int32_t *info, double *step, int64_t *summary, double *edge_cos /*nullable*/);
/* the tile constants: which = 0 G = lanes per camera, 1 the cap on the grid of a sweep, 2 cameras (groups) per workgroup (-1 for any
 * other value) */
int mi_degensac_rotation_average_tile(int which);

/* ---- unit-level device entry points (parity tests of the kernels' building blocks) ------------ */
/* score n_models fundamental (kind 0: Sampson, 1: symmetric epipolar) or homography (kind 10..14:
 * H Sampson, symm_sq_max, symm_max, symm_sq_sum, symm_sum) models against all n points: I (<= th)
 * and MSAC J per model, optionally the residual vectors [n_models*n]. Host pointers. */
int mi_degensac_score_models(const double *pts1, const double *pts2, int n, int dim,
                             const double *models, int n_models, int kind, double th, int device,
                             uint32_t *I, double *J, double *resid /*nullable*/);
/* the main-loop sample stream: for `iters` iterations the 7 (or 4) drawn ids in draw order.
 * seq_pool != 0 forces the sequential pool-swap stage. */
int mi_degensac_sample_stream(uint32_t seed, int n, int sample_size, int iters, int device,
                              int32_t *samples /*[iters*sample_size]*/);
int mi_degensac_sample_stream_ex(uint32_t seed, int n, int sample_size, int iters, int device,
                                 int seq_pool, int32_t *samples);
/* the 7-point solver + oriented-epipolar test on given samples: for each of n_samples 7-tuples of
 * ids (draw order) nsol[i] in 0..3 valid models (-1: null space not 2-dimensional) and up to 3 models
 * (27 doubles per sample) with the index of the cubic's root each came from. */
int mi_degensac_solve7(const double *pts1, const double *pts2, int n, int dim,
                       const int32_t *samples, int n_samples, int device,
                       int32_t *nsol, int32_t *root_idx /*[3*n_samples]*/, double *models /*[27*n_samples]*/);
/* the lane-level 3x3 routines of the DEGENSAC branch, one problem per lane: op 0 = in-place inverse (matutls/minv.c
 * order; in/out 9 doubles, flag = -1 when singular), op 1 = right singular vectors and singular values (matutls/svduv.c
 * order; in 9, out 9 + 3), op 2 = Hdetect (DegUtils.c:84-161; in F (9) + seven correspondences x1 y1 x2 y2 (28) + the
 * triplet as three doubles, out 9).  op 3 = the 9x9 symmetric eigen-solver (LAPACK dsyev as lap_eig calls it,
 * degensac/lapwrap.c:67-96), one problem per wave: in 81, out 9 eigenvalues (smallest first, the rest as the QL/QR
 * iteration left them) + 81 (column-major vectors, column 0 = the one of the smallest eigenvalue), flag = info.
 * op 4 = the real roots of a cubic as the 7-point solver takes them (Ftools.c:251-298; in 4 coefficients, out 3, flag =
 * the number of roots): the one routine of the path that calls the math library (pow / acos / cos).  The device takes their
 * correctly rounded values (dg_crmath.h), which the host's libm returns in all but ~0.1-0.2 % of its calls: the one place
 * where the device can differ from a host run of the reference in the last bits.
 * op 5 = op 3 with TWO problems per wave (dg_eig2.h: problem 2t in lanes 0..31 of wave t, 2t + 1 in lanes 32..63), same output.
 * op 6 / 7 = timing of op 3 / op 5: every wave solves its problem(s) flag[0] times (on entry) and leaves the 100 MHz ticks that took
 * in out[wave].
 * op 8 / 9 / 10 = dg_cr_cos / dg_cr_acos / dg_cr_pow13 (dg_crmath.h) as compiled for the device, one argument per lane: in 1, out 1,
 * flag = 0.  What op 4 calls, by itself: the correctly rounded cos on [0, pi], acos on [-1, 1] and pow(x, 1.0/3) on (1e-290, 1e290);
 * outside those ranges the device library's own value. */
int mi_degensac_mat3(int op, const double *in, int count, int device, double *out, int32_t *flag);
/* the screening counts of the scoring phase (dg_score_tiles.h) for given fundamental-matrix models over a point set:
 * c1[m] = level-1 count (single precision, loosest denominator, rounding-widened threshold), c2[m] = level-2 count
 * (double precision, the point's own denominator, threshold x (1 + 1e-6)); both must be >= the number of points whose
 * exact residual is < 9/4 th (kind 0 = Sampson, 1 = symmetric epipolar).  Models in batches of 64 per wave, as in the kernels. */
int mi_degensac_screen_counts(const double *pts1, const double *pts2, int n, int dim, const double *models, int n_models,
                              int kind, double th, int device, uint32_t *c1, uint32_t *c2);

/* the homography main loop's screen (dg_geom.h dg_HDs_maybe_below, swept by dg_h_screen4 four models per wave): cnt[m] = points
 * that may lie below 9/4 th under the Sampson metric of model m (division-free bound, threshold x (1 + 1e-6)); cand (nullable,
 * [n_models * n]) = the per-point verdicts.  Every point whose exact HDs residual (Htools.c:161-200) is < 9/4 th must be a
 * candidate, and cnt[m] must equal the number of candidates. */
int mi_degensac_screen_counts_h(const double *pts1, const double *pts2, int n, int dim, const double *models, int n_models,
                                double th, int device, uint32_t *cnt, uint8_t *cand);

/* the wave forms of the reference's srand() / rand() (one multiply-add per state word instead of 341 dependent steps; up to 31
 * outputs per step as three interleaved prefix sums): out[i] = the (skip + i + 1)-th rand() after srand(seed), generated `block`
 * (1..31) values at a time.  Must equal libc's sequence. */
int mi_degensac_rng_wave(uint32_t seed, int skip, int block, int count, int device, int32_t *out);

/* Where the time of ONE host-pointer call goes (the single-call latency of bench.py's `single_call_ms.breakdown`).  With timing on,
 * every host-pointer call of the calling thread leaves, in milliseconds: [0] the whole call (host clock), [1] packing the inputs into
 * the pinned block, [2] enqueueing (H2D copy, scratch set-up, launch, D2H copy), [3] waiting for the stream, [4] unpacking the
 * results; and from HIP events on the context's stream: [5] the H2D copy, [6] header memsets + kernel + error-word copy, [7] the
 * D2H copy.  Process-wide switch (returns the previous value), per-thread result; off by default (it costs four events per call). */
#define MI_DEGENSAC_TIMING_LEN 8
int mi_degensac_set_call_timing(int on);
int mi_degensac_last_call_timing(double *out /*[MI_DEGENSAC_TIMING_LEN]*/);

/* ---- misc -------------------------------------------------------------------------------------- */
int         mi_degensac_device_count(void);
const char *mi_degensac_last_error(void);
const char *mi_degensac_version(void);
/* name of the dominant kernel (for profiling) */
const char *mi_degensac_kernel_name(int homography);
/* result of the one-time LDS exchange-order self-check of `device` (1 = the parallel pool-swap stage is in use,
 * 0 = the check failed and the sequential stage is used, <0 = error) */
int         mi_degensac_pool_stage_parallel(int device);

#ifdef __cplusplus
}
#endif
#endif /* MI_DEGENSAC_H */
