// Internal: the host side that the stage handles share (nellie_hip_track.hip, nellie_hip_flow.hip, nellie_hip_reassign.hip,
// nellie_hip_voxfeat.hip, nellie_hip_nodefeat.hip, nellie_hip_branchfeat.hip, nellie_hip_adjacency.hip, nellie_hip_tracks.hip, nellie_hip_overlay.hip,
// nellie_hip_transitions.hip) -- argument checks of the create calls, the device / stream / event-pair base of a handle, growing
// device buffers and kernel timing.  Included by those ten units only.
#pragma once
#include <initializer_list>
#include "nl_host.h"

// Inside a create call: a failed HIP call becomes NL_ENOMEM / NL_EHIP with its message, then `cleanup` runs and the status is returned.
#define STAGE_HIP(expr, cleanup)                                                                                                \
    do {                                                                                                                        \
        hipError_t e_ = (expr);                                                                                                 \
        if (e_ != hipSuccess) {                                                                                                 \
            (void)hipGetLastError();                                                                                            \
            const int rc_ = nl_fail(err, errlen, e_ == hipErrorOutOfMemory ? NL_ENOMEM : NL_EHIP, "%s: %s%s", #expr,            \
                                    hipGetErrorString(e_), e_ == hipErrorOutOfMemory ? " [out of memory]" : "");                \
            cleanup;                                                                                                            \
            return rc_;                                                                                                         \
        }                                                                                                                       \
    } while (0)

// ---- argument checks of the create calls (before the device is looked at) --------------------------------------------------
// A (nz, ny, nx) frame with ndim spacings; a 2-D frame has nz = 1.  A handle without a frame shape passes 1, 1, 1.
static inline int stage_check_frame(int ndim, const double *spacing, int64_t nz, int64_t ny, int64_t nx, char *err, size_t errlen) {
    if (ndim != 2 && ndim != 3) return nl_fail(err, errlen, NL_EINVAL, "ndim must be 2 or 3");
    if (!spacing) return nl_fail(err, errlen, NL_EINVAL, "spacing is NULL");
    if (nz < 1 || ny < 1 || nx < 1 || (ndim == 2 && nz != 1)) return nl_fail(err, errlen, NL_EINVAL, "bad frame shape");
    if ((double)nz * (double)ny * (double)nx > 9e15) return nl_fail(err, errlen, NL_EINVAL, "frame too large");
    for (int a = 0; a < ndim; ++a)
        if (!(spacing[a] > 0.0) || !(spacing[a] < 1e300)) return nl_fail(err, errlen, NL_EINVAL, "spacing must be positive and finite");
    return NL_OK;
}

// what: "the radius", "the time step"
static inline int stage_check_positive(double v, const char *what, char *err, size_t errlen) {
    if (!(v > 0.0) || !(v < 1e300)) return nl_fail(err, errlen, NL_EINVAL, "%s must be positive and finite", what);
    return NL_OK;
}

static inline int stage_check_device(int device, char *err, size_t errlen) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return nl_fail(err, errlen, NL_ENODEV, "GPU backend requested but no HIP device is visible");
    }
    if (device < 0 || device >= count) return nl_fail(err, errlen, NL_ENODEV, "GPU backend requested but device %d does not exist", device);
    return NL_OK;
}

// ---- what every handle struct derives from -----------------------------------------------------------------------------------
struct StageBase {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;      // around timed kernels (stage_start / stage_stop); null in a handle that times nothing
};

#define STAGE_ENTER(h, noun)                                                \
    if (!(h)) return nl_fail(err, errlen, NL_EINVAL, noun " is NULL");      \
    NL_HIP(hipSetDevice((h)->device));

static inline int stage_open(StageBase &b, int device, bool timed, char *err, size_t errlen) {
    b.device = device;
    STAGE_HIP(hipSetDevice(device), (void)0);
    STAGE_HIP(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking), (void)0);
    if (timed) {
        STAGE_HIP(hipEventCreate(&b.ev_a), (void)0);
        STAGE_HIP(hipEventCreate(&b.ev_b), (void)0);
    }
    return NL_OK;
}

// The whole of a destroy call but the delete: waits for the stream, frees the device and the pinned buffers (null ones skipped),
// then the events and the stream.  Safe on a half-built handle.
static inline void stage_close(StageBase &b, const std::vector<void *> &dev, std::initializer_list<void *> pinned) {
    hipSetDevice(b.device);
    if (b.stream) hipStreamSynchronize(b.stream);
    for (void *p : dev) if (p) hipFree(p);
    for (void *p : pinned) if (p) hipHostFree(p);
    if (b.ev_a) hipEventDestroy(b.ev_a);
    if (b.ev_b) hipEventDestroy(b.ev_b);
    if (b.stream) hipStreamDestroy(b.stream);
    (void)hipGetLastError();
}

// ---- device buffers ------------------------------------------------------------------------------------------------------------
// Frees *p, then allocates max(count, 1) elements.  After an error *p is null or (hipFree failed) unchanged.
template <typename P> static hipError_t stage_alloc(P **p, i64 count, size_t elem) {
    if (*p) {
        const hipError_t e = hipFree(*p);
        if (e != hipSuccess) return e;
    }
    *p = nullptr;
    return hipMalloc((void **)p, (size_t)(count > 0 ? count : 1) * elem);
}

struct StageBuf {                     // a buffer of a group: `elem` bytes per unit of the group's capacity
    void **p;
    size_t elem;
    template <typename P> StageBuf(P **q, size_t e) : p((void **)q), elem(e) {}
};

// The buffers that share the capacity *cap: nothing when need <= *cap, else all of them are reallocated for new_cap units (the
// caller's policy: need itself, or stage_doubled).  An error leaves *cap = 0 and every buffer freed, null or newly allocated.
static inline int stage_grow(i64 *cap, i64 need, i64 new_cap, std::initializer_list<StageBuf> bufs, char *err, size_t errlen) {
    if (need <= *cap) return NL_OK;
    *cap = 0;
    for (const StageBuf &b : bufs) NL_HIP(stage_alloc(b.p, new_cap, b.elem));
    *cap = new_cap;
    return NL_OK;
}
static inline i64 stage_doubled(i64 cap, i64 need) { return need > 2 * cap ? need : 2 * cap; }

// `count` elements of `size` bytes from the host into *buf (capacity *cap, bytes), grown when it is too small; on the handle's stream
static inline int stage_upload(StageBase &b, void **buf, i64 *cap, const void *host, i64 count, size_t size, char *err, size_t errlen) {
    const i64 bytes = count * (i64)size;
    if (int rc = stage_grow(cap, bytes, bytes, {{buf, 1}}, err, errlen)) return rc;
    if (bytes > 0) NL_HIP(hipMemcpyAsync(*buf, host, (size_t)bytes, hipMemcpyHostToDevice, b.stream));
    return NL_OK;
}

// ---- kernel timing ---------------------------------------------------------------------------------------------------------------
// stage_start .. stage_stop around kernels: the device time between them is added to *ms.  stage_stop synchronises the stream; a
// caller that enqueues copies behind the kernels calls its two halves, stage_stop_record before them and stage_stop_wait after.
static inline int stage_start(StageBase &b, char *err, size_t errlen) {
    NL_HIP(hipEventRecord(b.ev_a, b.stream));
    return NL_OK;
}
static inline int stage_stop_record(StageBase &b, char *err, size_t errlen) {
    NL_HIP(hipEventRecord(b.ev_b, b.stream));
    return NL_OK;
}
static inline int stage_stop_wait(StageBase &b, float *ms, char *err, size_t errlen) {
    NL_HIP(hipStreamSynchronize(b.stream));
    float t = 0.f;
    NL_HIP(hipEventElapsedTime(&t, b.ev_a, b.ev_b));
    *ms += t;
    return NL_OK;
}
static inline int stage_stop(StageBase &b, float *ms, char *err, size_t errlen) {
    if (int rc = stage_stop_record(b, err, errlen)) return rc;
    return stage_stop_wait(b, ms, err, errlen);
}
