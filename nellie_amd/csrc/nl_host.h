// Internal: what the translation units of libnellie_hip.so share on the host side -- the communicator dispatch, the entry-point macros,
// a few launch helpers and the declarations of what one unit defines for the others (at the end of this file):
//   nellie_hip.hip      Filter: context lifetime, cascade, device chain, 2-D path, epilogue      -> upload_convert, store_planes, ...
//   nellie_walk.hip     the Hessian walk: divisors, launch plan and launcher, resolve launch     -> set_spacing, spec_enqueue, resolve_*, walk_plan
//   nellie_sample.hip   lattice / flat sampling, histogram records and thresholds               -> the sample_* rounds, fetch_counted, host_edges
//   nellie_comm.hip     RCCL loader, loopback transport, communicator pool, collectives         -> rccl(), comm_release, reduce_*, ag_reserve, allgather_sizes
//   nellie_label.hip    Label / Network / streaming                                             -> nl_launch_threshold_pack
//   nellie_markers.hip  Markers                                                                 -> nl_launch_pack_labels
//   nellie_hip_network.hip  Network behind the thinning (clean, seed, per-object relabel)        -> nw_release
//   nellie_hip_thin.hip     the 3-D thinning (Lee94 as skimage runs it)                           -> thin_device
//   nellie_gauss.hip, nellie_gzyx.hip, nellie_hv.hip: kernels behind gauss_launch.h / hv_launch.h (nellie_hv.hip: the pair and the wave-autonomous
//   walk, launched by nellie_walk.hip); the eight stage handles share nl_stage.h.
// gfx950 only.
#pragma once
#include <stdarg.h>
#include <stdlib.h>
#include <type_traits>
#include <thread>
#include <mutex>
#include <vector>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include "nl_common.h"

#define NL_MASK_SLOTS 2      // cumulative h_mask bit planes (ping-pong between consecutive scales)
#define NL_VERSION "nellie_amd-hip 0.1.0 (gfx950)"
#define NL_PREZERO_DEFAULT 1 // NELLIE_PREZERO when unset (nl_chain_begin)
#define SCAN_CHUNK 4096      // elements per workgroup of the exclusive scans (label_voxels.inc)

// What the entry points call: RCCL's names, dispatched per communicator -- a communicator created from a loopback id
// (nl_comm_loopback_id) lives in loopback.inc, every other one is RCCL's (dlopen()ed on first use).  Defined in nellie_comm.hip.
struct CommApi {
    std::atomic<int> n_real{0};
    ncclResult_t GetUniqueId(ncclUniqueId *id);
    ncclResult_t CommInitRank(ncclComm_t *comm, int world, ncclUniqueId id, int rank);
    ncclResult_t CommDestroy(ncclComm_t comm);
    const char *GetErrorString(ncclResult_t r);
    ncclResult_t GroupStart();
    ncclResult_t GroupEnd();
    ncclResult_t Send(const void *buf, size_t count, ncclDataType_t dt, int peer, ncclComm_t comm, hipStream_t st);
    ncclResult_t Recv(void *buf, size_t count, ncclDataType_t dt, int peer, ncclComm_t comm, hipStream_t st);
    ncclResult_t AllReduce(const void *src, void *dst, size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm_t comm, hipStream_t st);
    ncclResult_t AllGather(const void *src, void *dst, size_t count, ncclDataType_t dt, ncclComm_t comm, hipStream_t st);
    ncclResult_t Broadcast(const void *src, void *dst, size_t count, ncclDataType_t dt, int root, ncclComm_t comm, hipStream_t st);
};
CommApi &rccl();

#include "device_math.inc"
#include "convert.inc"
#include "gauss_launch.h"

// 2-D images: 256 columns per workgroup in x, rows by a stride loop in the kernel (~1024 workgroups = four per CU: the kernels end
// in one atomic per workgroup on one word, ~10 ns each -- with 4096 workgroups they were 40 of vesselness2d_kernel's 60 us at 2048^2)
static inline dim3 grid2d_rows(i64 nx, i64 ny) {
    const i64 gx = (nx + 255) / 256;
    i64 gy = (1024 + gx - 1) / gx;
    if (gy > ny) gy = ny;
    if (gy < 1) gy = 1;
    return dim3((unsigned)gx, (unsigned)gy, 1);
}
static inline unsigned int grid1d(i64 n, int block = 256, i64 cap = 256 * 32) {
    i64 g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned int)g;
}

// Zeroing a few counter words between kernels with a one-wave kernel of our own instead of the runtime's fill path
// (~35 of these per frame).  `bytes` is a multiple of 4.  (static: every translation unit has its own copy)
static __global__ void zero_words_kernel(unsigned int *p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0u;
}
static inline hipError_t zero_small(void *p, size_t bytes, hipStream_t st) {
    zero_words_kernel<<<1, 256, 0, st>>>((unsigned int *)p, (int)(bytes / 4));
    return hipGetLastError();
}

static float *gauss_cur(const nl_ctx *c) { return c->gauss_ext ? c->gauss_ext : c->f[c->i_gauss]; }
static inline float *field_ptr(nl_ctx *c, int field) {      // the fields that are a volume of their own
    if (field == NL_FIELD_GAUSS) return gauss_cur(c);
    if (field == NL_FIELD_FRANGI) return c->f[c->i_vmax];
    return nullptr;
}
// The cumulative h_mask bit planes of Filter ping-pong in m[0]: scale k writes slot k & 1 (cm) and reads the other (pm); wpr words per row.
// (k = c->mask_slots_used; the caller that commits the slot increments it.)
struct MaskSlots { unsigned long long *cm; const unsigned long long *pm; int wpr; };
static inline MaskSlots mask_slots(const nl_ctx *c, int k) {
    const int wpr = (int)((c->nx + 63) / 64);
    const i64 slot_words = c->nzl * c->ny * wpr;
    return MaskSlots{(unsigned long long *)c->m[0] + (i64)(k & 1) * slot_words, (unsigned long long *)c->m[0] + (i64)((k + 1) & 1) * slot_words, wpr};
}
#define NL_NAN_FLAG_OFF (52 << 10)      // byte offset in d_small of the "NaN Hessian solved" word (VessP::nan_flag), zeroed per frame
// the planes [z0, z1) of the vesselness volume are all zero already: the frame's first cascade step did it in passing (gauss_zyx.inc)
static inline bool vmax_is_zero(const nl_ctx *c, i64 z0, i64 z1) { return c->vmax_zero_hi > 0 && c->vmax_zero_lo <= z0 && z1 <= c->vmax_zero_hi; }
static inline HessP hessp(const nl_ctx *c) { return HessP{c->hz, c->hy, c->hx, c->hz2, c->hy2, c->hx2}; }
static VolGeom geom(const nl_ctx *c) {
    VolGeom v{c->nzl, c->ny, c->nx, c->gz0, c->gnz};
    // 128-element chunks read 128 + 2R elements for 128 outputs; 256 halves the excess (about 1 % of the Gaussian passes at 1024^3,
    // within run-to-run noise) but also halves the number of workgroups, so only where those are plentiful
    static int forced = -1;
    if (forced < 0) { const char *e = getenv("NELLIE_GM_CHUNK"); forced = e ? atoi(e) : 0; }
    // (a 2-D image has one plane: 32-row chunks, or its Gaussian passes run on a handful of workgroups)
    v.chunk = forced > 0 ? forced : (c->two_d ? 32 : (c->n >= ((i64)1 << 29) ? 256 : 128));
    return v;
}

static size_t dtype_size(int dt) {
    switch (dt) {
        case NL_U8: case NL_I8: return 1;
        case NL_U16: case NL_I16: return 2;
        case NL_U32: case NL_I32: case NL_F32: return 4;
        case NL_F64: case NL_U64: case NL_I64: return 8;
    }
    return 0;
}

#define NL_ENTER(c)                                                    \
    if (!(c)) return nl_fail(err, errlen, NL_EINVAL, "ctx is NULL");   \
    ++(c)->epoch;                                                      \
    NL_HIP(hipSetDevice((c)->device));

// The entry points between the frame's last cascade step and nl_label_run that leave the pre-zeroed volume alone (or say so: pz_touch):
// they carry its flag forward.  After any other entry point the volume counts as pre-zeroed no longer.
#define NL_ENTER_KEEP_PZ(c)                                            \
    NL_ENTER(c)                                                        \
    if ((c)->pz_epoch + 1 == (c)->epoch.load()) (c)->pz_epoch = (c)->epoch.load();

static inline bool pz_valid(const nl_ctx *c) { return c->pz_buf && c->pz_epoch == c->epoch.load(); }
static inline bool pz_is(const nl_ctx *c, const float *p) { return pz_valid(c) && p == c->pz_buf; }
static inline void pz_set(nl_ctx *c, float *p) { c->pz_buf = p; c->pz_epoch = c->epoch.load(); }
// `p` is about to be written by an entry point that carries the flag
static inline void pz_touch(nl_ctx *c, const float *p) { if (p == c->pz_buf) c->pz_buf = nullptr; }

// Entry points of the copy threads of nellie_amd/streaming.py (nl_input_load_async, nl_outputs_fetch_async, nl_outputs_wait):
// they run CONCURRENTLY with the compute thread's calls on the same context, touch only the copy streams, the input slots
// and the staging buffers, and therefore leave `epoch` (the compute state's version) alone.
#define NL_ENTER_IO(c)                                                 \
    if (!(c)) return nl_fail(err, errlen, NL_EINVAL, "ctx is NULL");   \
    NL_HIP(hipSetDevice((c)->device));

// nl_mask_volume_fused leaves the support of the Frangi frame (the opened mask, 1 bit/voxel) behind; nl_label_run may
// use it to skip the 98 % of the frame that is zero -- but only if nothing else ran in between.  Every entry point
// bumps `epoch`; the few that read the frame without touching it or the mask planes carry the validity forward.
#define NL_KEEP_SUPPORT(c) if ((c)->support_epoch + 1 == (c)->epoch.load()) (c)->support_epoch = (c)->epoch.load();
// the same for the label bits nl_label_run leaves in m[1] (read by nl_markers_begin): carried over entry points that write neither the
// label volume nor the bit planes
#define NL_KEEP_LABBITS(c) if ((c)->labbits_epoch + 1 == (c)->epoch.load()) (c)->labbits_epoch = (c)->epoch.load();

// Orders the main stream after whatever is still running on the side stream (the resolve kernel of the previous
// scale).  Called by every entry point that touches the vesselness volume, the mask planes or the queue.
#define NL_JOIN_SIDE(c)                                                            \
    if ((c)->side_pending) {                                                       \
        NL_HIP(hipStreamWaitEvent((c)->stream, (c)->ev_side, 0));                  \
        (c)->side_pending = 0;                                                     \
    }

#define NL_NCCL(expr)                                                                                  \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess) { c->comm_poisoned = 1; return nl_fail(err, errlen, NL_ECOMM, "%s: %s", #expr, rccl().GetErrorString(r_)); } \
    } while (0)


// ---- reductions across the ranks, on the device (nl_comm_fuse) ---------------------------------------------------------
// With a communicator in "fused" mode the sampling / statistics entry points below finish with the GLOBAL value: the RCCL
// collective sits on the context stream between the kernels, so a threshold costs one host round trip instead of one per
// pass plus one per host-level all-reduce.  Every rank must make the same calls in the same order (they do: the path is SPMD).
static inline bool fused(const nl_ctx *c) { return c->comm && c->fuse_reduce; }

// ---- defined in nellie_hip.hip ------------------------------------------------------------------------------------------
int upload_convert(nl_ctx *c, const void *host, int dtype, float *dst, i64 count, char *err, size_t errlen);
int store_planes(nl_ctx *c, const void *dev_base, void *host, size_t elem, int64_t z0, int64_t z1, char *err, size_t errlen);
bool gyx_tiled();
struct VessP;
// The two Hessian kernels of an image (filter2d.inc), enqueued in their profiling groups: the statistics into res[0..2]; the vesselness
// update, which commits the scale's mask slot (dev_params: as resolve_enqueue's)
int hessian2d_stats_enqueue(nl_ctx *c, unsigned int *res, char *err, size_t errlen);
int vesselness2d_enqueue(nl_ctx *c, const VessP &vp0, unsigned long long *d_cnt, const float *dev_params, char *err, size_t errlen);

// ---- defined in nellie_walk.hip -----------------------------------------------------------------------------------------
struct VqAlloc;
struct WalkPlan;
VqAlloc vq_alloc(int64_t nzl, int64_t ny, int64_t nx);                       // the eigen queue of a context (walk_plan.h), under the environment's switches
int64_t vq_alloc_entries(int64_t nzl, int64_t ny, int64_t nx);               // its 32-byte entries (the other stages borrow the queue as scratch)
WalkPlan walk_plan(const nl_ctx *c, int mode, int64_t z0, int64_t z1);       // the walk's launch plan for this context (walk_plan.h)
int set_spacing(nl_ctx *c, const double spacing[3], char *err, size_t errlen);
float mask_threshold_on_fsq(float max_abs, int use_thr, float thr);
int spec_enqueue(nl_ctx *c, const double spacing[3], float fsq_lo, float fsq_hi, int64_t z0, int64_t z1, unsigned int *res, unsigned long long *d_cnt,
                 const float *dev_lohi, char *err, size_t errlen);
int resolve_enqueue(nl_ctx *c, VessP vp, unsigned long long *d_cnt, const float *dev_params, char *err, size_t errlen, bool force_side = false);
bool resolve_defer_ok(const nl_ctx *c);
int resolve_deferred_launch(nl_ctx *c, bool on_side, char *err, size_t errlen);

// ---- defined in nellie_sample.hip ---------------------------------------------------------------------------------------
// A histogram record, contiguous so that one transfer brings it back: counts (u64 x nbins) | edges (f32 x nbins + 1, padded to
// 16 bytes) | res: [0] min bits, [1] max bits, [2..3] count, [4] flag (0 no positive sample, 1 ok, 2 range not finite), 32 bytes.
// ChainHist (chain.inc) is this layout at NL_CHAIN_BINS.
struct HistLayout { size_t off_edges, off_res, bytes; };
constexpr size_t hist_off_res(int nbins) { return (size_t)nbins * 8 + (((size_t)(nbins + 1) * 4 + 15) & ~(size_t)15); }
constexpr HistLayout hist_layout(int nbins) { return HistLayout{(size_t)nbins * 8, hist_off_res(nbins), hist_off_res(nbins) + 32}; }
// The first round of a scale, enqueued: the records of field_a and field_b on the lattice (sz, sy, sx) into dA / dB.  The Gaussian /
// raw-Frobenius pair takes one pass over the lattice where `pair_ok` and NELLIE_CHAIN_UNFUSED_SAMPLING allow, else two single
// sequences.  hA / hB: pinned mirrors the initial state is uploaded from, or NULL when the caller initialised the records (chain.inc).
int sample_first_round(nl_ctx *c, int field_a, int field_b, i64 sz, i64 sy, i64 sx, int nbins, char *dA, char *dB, char *hA, char *hB, bool pair_ok,
                       char *err, size_t errlen);
// The exact round of a scale on stream `st`: edges from the range already in the record, then the histogram of the cached frob_sq under
// the normalisation at norm_dev (device memory); reduce: the counts are summed across a fused communicator.
int sample_exact_round(nl_ctx *c, i64 sz, i64 sy, i64 sx, int nbins, char *rec, const float *norm_dev, hipStream_t st, bool reduce, char *err, size_t errlen);
// The positive lattice samples of `field`, compacted into dst with their number in *d_n (zeroed here), enqueued.  *total = the lattice
// points; a lattice of more than `cap` points enqueues nothing -- the caller reports that.
int sample_gather_pos_enqueue(nl_ctx *c, int field, i64 sz, i64 sy, i64 sx, float *dst, unsigned int *d_n, i64 cap, i64 *total, char *err, size_t errlen);
int fetch_counted(nl_ctx *c, const float *stage, const unsigned int *d_n, i64 max_count, float *out, i64 cap, int64_t *n, char *err, size_t errlen);
void host_edges(float first, float last, int nbins, float *edges);       // sample_edges_kernel on the host

// ---- defined in nellie_comm.hip -----------------------------------------------------------------------------------------
void comm_release(nl_ctx *c, void *comm, int role);      // RCCL communicators go back to a per-process pool (see nl_comm_init)
// small reductions across the ranks on the context stream, in place.  reduce_range: res = [min bits, max bits, count lo, count hi] of
// positive float32 samples (unsigned order = float order); two records (res_b != NULL) travel in one group, as do two count arrays
int reduce_range(nl_ctx *c, unsigned int *res, unsigned int *res_b, char *err, size_t errlen);
int reduce_u64_sum(nl_ctx *c, unsigned long long *v, size_t n, char *err, size_t errlen, unsigned long long *v_b = nullptr);
int reduce_u32_sum(nl_ctx *c, unsigned int *v, size_t n, char *err, size_t errlen);
int reduce_u32_max(nl_ctx *c, unsigned int *v, size_t n, char *err, size_t errlen);
// the all-gather staging of the context (d_ag on the device, h_ag page-locked) holds at least that many bytes afterwards
int ag_reserve(nl_ctx *c, size_t device_bytes, size_t host_bytes, char *err, size_t errlen);
// bytes_of[r] = rank r's nbytes (one collective and one wait, through the small scratch)
int allgather_sizes(nl_ctx *c, int64_t nbytes, int64_t *bytes_of, char *err, size_t errlen);

// ---- defined in nellie_label.hip ----------------------------------------------------------------------------------------
// nl_skel_pixel_class behind its upload: classes (f[2]) and branch bits of the int32 skeleton in f[3]
int nw_pixel_class_resident(nl_ctx *c, uint8_t *pixel_class_host, int64_t *n_skel, char *err, size_t errlen);

// ---- defined in nellie_hip_network.hip -----------------------------------------------------------------------------------
void nw_release(nl_ctx *c);                              // the Network stage's own buffers and events (nl_ctx_destroy)

// ---- defined in nellie_hip_thin.hip ---------------------------------------------------------------------------------------
// Thins c->nw_mask in place on the context's stream (3-D frames; f[0..3] are its work lists and state).  labels != NULL: the image is
// first made from labels > 0 (device pointer); else nw_mask holds it, any non-zero byte foreground.  Leaves thin_counts / thin_ms.
int thin_device(nl_ctx *c, const int *labels, int rounds_per_sync, char *err, size_t errlen);

// ---- kernels of one unit launched from another ---------------------------------------------------------------------------
void nl_launch_threshold_pack(unsigned int grid, hipStream_t st, const float *f, const unsigned long long *support, unsigned long long *bits,
                              int has_thr, float thr, int nx, i64 nrows, int wpr, const float *thr_dev);      // nellie_label.hip
void nl_launch_pack_labels(unsigned int grid, hipStream_t st, const int *lab, unsigned long long *bits, int nx, i64 nrows, int wpr);   // nellie_markers.hip
