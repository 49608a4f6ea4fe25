/* Internal interface between the estimator host (mi_degensac_host.inc, compiled into mi_degensac.hip next to the 512-thread kernels) and
 * the match-and-verify stage (mi_match_verify.hip): the error text of mi_degensac_last_error(), the HIP check and device guard that
 * report through it, and the four calls the stage makes.  Not part of the C-ABI: hidden symbols of libmi_degensac.so. */
#ifndef MI_ESTIMATOR_H
#define MI_ESTIMATOR_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"

/* the message mi_degensac_last_error() returns for the calling thread (a printf format with up to two %s) */
MT_HIDDEN void est_set_error(const char *fmt, const char *a = "", const char *b = "");
static inline void set_err(const char *fmt, const char *a = "", const char *b = "") { est_set_error(fmt, a, b); }

/* a failed call must not leave HIP's per-thread "last error" set: other users of the runtime in this process
 * (e.g. torch's lazy device initialisation) treat a stale error as their own */
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err("%s failed: %s", #x, hipGetErrorString(e_)); (void)hipGetLastError(); \
    return MI_DEGENSAC_EHIP; } } while (0)

/* the calling thread's current device is put back when an entry point returns (the library may be embedded next to
 * PyTorch, whose allocations follow the current device).  Unlike MiDevGuard (mi_host.h) it does not look at the device count: an index
 * that is not there fails in hipSetDevice, as EHIP. */
struct DevGuard {
    int prev = -1; bool armed = false;
    int enter(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != device) { HIPCHK(hipSetDevice(device)); armed = prev >= 0; }
        return 0;
    }
    ~DevGuard() { if (armed) (void)hipSetDevice(prev); }
};

/* the batched estimator, asynchronous on `stream`; the device must be current.  Takes the device's launch mutex.  d_err_copy: a device
 * word of the caller that receives the launch's error word (copied on `stream` right behind the kernel) */
MT_HIDDEN int est_launch_batch(int homography, const double *d_p1, const double *d_p2, const int64_t *d_off, const int64_t *h_off, int n_pairs,
                               int dim, const mi_degensac_params *prm, const uint32_t *d_seeds, int device, hipStream_t stream, double *d_model,
                               uint8_t *d_mask, int32_t *d_stats, const mi_degensac_diag *diag = nullptr, int *d_err_copy = nullptr);
/* what est_launch_batch would refuse in prm for this model and point dimension, without a device: 0 or EINVAL (message set) */
MT_HIDDEN int est_check_params(const mi_degensac_params *prm, int homography, int dim);
/* the stream (hipStreamNonBlocking) of the calling thread's own context on `device`; refuses a bad or absent device as
 * mi_degensac_ctx_create does */
MT_HIDDEN int est_thread_stream(int device, hipStream_t *stream);
/* the re-run of pairs discarded after a hand-over time-out (bit 10 of stats[15]): the host-pointer batch on the calling thread's context
 * without producer or helper workgroups, at depth 1 (a second time-out is an error); synchronises the context's stream */
MT_HIDDEN int est_rerun(int device, int homography, const double *p1, const double *p2, const int64_t *off, int n_pairs, int dim,
                        const mi_degensac_params *prm, const uint32_t *seeds, double *model, uint8_t *mask, int32_t *stats);
#endif /* MI_ESTIMATOR_H */
