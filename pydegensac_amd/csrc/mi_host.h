/* The host plumbing under the matcher, the guided stage and the list stages (correspondences, tracks, refit, pose, pose refinement,
 * triangulation): the HIP error check, the EINVAL refusal, the device guard, the stream-ordered scratch block and the staging block of
 * the host-pointer forms.  Not part of the C-ABI.  Every message goes through mt_set_error to mi_degensac_match_last_error().
 * (The estimator host and the match-and-verify stage have their own DevGuard / HIPCHK in mi_estimator.h: they report through
 * mi_degensac_last_error.) */
#ifndef MI_HOST_H
#define MI_HOST_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <vector>
#include "../../include/mi_degensac.h"
#include "mi_match_batch.h"

/* a failed HIP call: "<expr> failed: <reason>" as the thread's message, HIP's per-thread last error cleared, EHIP returned */
#define MICHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { char b_[256]; snprintf(b_, sizeof b_, "%s failed: %s", #x, hipGetErrorString(e_)); \
    mt_set_error(b_); (void)hipGetLastError(); return MI_DEGENSAC_EHIP; } } while (0)

static inline int mi_einval(const char *msg) { mt_set_error(msg); return MI_DEGENSAC_EINVAL; }

/* makes `device` current for the scope; the calling thread's previous device comes back on every return path, if it was known and differed */
struct MiDevGuard {
    int prev = -1; bool armed = false;
    int enter(int device)
    {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { (void)hipGetLastError(); mt_set_error("no HIP device: this library has no CPU path");
            return MI_DEGENSAC_ENODEV; }
        if (device < 0 || device >= n) { mt_set_error("device index out of range"); return MI_DEGENSAC_ENODEV; }
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != device) { MICHK(hipSetDevice(device)); armed = prev >= 0; }
        return 0;
    }
    ~MiDevGuard() { if (armed) (void)hipSetDevice(prev); }
};

/* the 256-byte step of every block layout here */
static inline size_t mi_up256(size_t b) { return (b + 255) / 256 * 256; }

/* the scratch of a _dev form: allocated stream-ordered on the caller's stream, freed on the same stream at scope exit; no synchronisation */
struct MiScratch {
    char *p = nullptr; hipStream_t s = nullptr;
    int alloc(size_t bytes, hipStream_t stream) { s = stream; MICHK(hipMallocAsync((void **)&p, bytes, s)); return 0; }
    ~MiScratch() { if (p) (void)hipFreeAsync(p, s); }
};

/* The staging block of a host-pointer form.  The caller declares its arrays in any order: in(host, bytes) / out(host, bytes) return the
 * slot's number, and late() is an output whose length is known only after the run (bytes = the most it can be).  A null host pointer is
 * an absent optional: its slot takes no room and dev() gives null for it, so the _dev form sees the same "absent".
 *   upload()   lays the slots out at 256-byte steps, makes the one hipMalloc (never for 0 bytes; freed at scope exit on every return path)
 *              and copies every input that is neither null nor empty;
 *   the caller runs its _dev form with dev<T>(slot), on the null stream or on a stream s of its own;
 *   finish(s)  the one hipStreamSynchronize of that stream, then every out() that is neither null nor empty comes back;
 *   fetch()    the first `bytes` of a late() slot, after finish(). */
struct MiStage {
    enum { IN, OUT, LATE };
    struct Slot { void *h; size_t bytes, at; int kind; };
    std::vector<Slot> sl;
    char *D = nullptr;
    ~MiStage() { (void)hipFree(D); }
    int add(const void *h, size_t bytes, int kind) { sl.push_back(Slot{const_cast<void *>(h), h ? bytes : 0, 0, kind}); return (int)sl.size() - 1; }
    int in(const void *h, size_t bytes) { return add(h, bytes, IN); }
    int out(void *h, size_t bytes) { return add(h, bytes, OUT); }
    int late(void *h, size_t bytes) { return add(h, bytes, LATE); }
    template <class T> T *dev(int i) const { return sl[i].h ? (T *)(D + sl[i].at) : nullptr; }
    int upload()
    {
        size_t all = 0;
        for (Slot &s : sl) { s.at = all; all += mi_up256(s.bytes); }
        MICHK(hipMalloc((void **)&D, all + 256));
        for (const Slot &s : sl)
            if (s.kind == IN && s.bytes) MICHK(hipMemcpy(D + s.at, s.h, s.bytes, hipMemcpyHostToDevice));
        return 0;
    }
    int finish(hipStream_t s = nullptr)
    {
        MICHK(hipStreamSynchronize(s));
        for (const Slot &s : sl)
            if (s.kind == OUT && s.bytes) MICHK(hipMemcpy(s.h, D + s.at, s.bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    int fetch(int i, size_t bytes)
    {
        if (sl[i].h && bytes) MICHK(hipMemcpy(sl[i].h, D + sl[i].at, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
};
#endif /* MI_HOST_H */
