/*
 * nellie_amd.h -- C-ABI of libnellie_hip.so, the MI355X (gfx950) native engine for
 * Nellie's `nellie/segmentation` hot path: Filter (multiscale Frangi) -> Label.
 *
 * The reference (aelefebv/nellie v1.0.3) is pure Python: its "FFI" for this path is the
 * `xp`/`ndi` module handle that swaps numpy/scipy.ndimage for cupy/cupyx
 * (nellie/segmentation/filtering.py:117-159, labelling.py:115-154).  This library is what
 * a third backend binds instead: every entry point below replaces one group of xp/ndi calls
 * of the reference, cited as `file:line` relative to the reference checkout.  The host side
 * stays Python (the nellie_amd.segmentation modules) and talks to this ABI through ctypes:
 * numpy in, numpy out, plain pointers and sizes, no torch / cupy types.
 *
 * Conventions
 *  - Every function returns an int status (NL_OK == 0) and, on failure, writes a
 *    NUL-terminated message into the caller's `err` buffer (`errlen` bytes, may be NULL/0).
 *    No exceptions cross the boundary.  The Python layer maps NL_ENODEV to
 *    RuntimeError("GPU backend requested but ...") and NL_ENOMEM to MemoryError so the
 *    reference's retry ladder (nellie/utils/adaptive_run.py:116-141) keeps working.
 *  - Volumes are C-contiguous (Z, Y, X), X fastest.  All host buffers are owned by the
 *    caller; all device buffers are owned by the context.  Inputs are never written.
 *  - A context is bound to one device and one local volume shape.  It may hold a Z-slab of
 *    a larger global volume (multi-GPU): `gz0` is the global index of local plane 0, `gnz`
 *    the global plane count, `[own_lo, own_hi)` the planes this rank owns (the rest are
 *    ghost planes).  Boundary rules (reflect padding, one-sided differences, zero border)
 *    apply only at true faces of the GLOBAL volume.  Single GPU: gz0 = 0, gnz = nz,
 *    own = [0, nz).
 *  - Entry points call hipSetDevice themselves and are synchronous on return unless noted
 *    (nl_* _async variants enqueue on the context stream; nl_sync waits).  One context must
 *    not be used from two threads at once; different contexts may be.  The one exception are
 *    the copy-thread calls of the frame streamer -- nl_input_load_async, nl_input_wait, nl_outputs_fetch_async,
 *    nl_outputs_wait -- which touch only the copy streams, the input slots and the staging
 *    volumes and may run beside the compute thread's calls on the same context.
 */
#ifndef NELLIE_AMD_H
#define NELLIE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define NL_OK      0
#define NL_EINVAL  1   /* bad argument */
#define NL_ENODEV  2   /* no usable HIP device */
#define NL_ENOMEM  3   /* device or host allocation failed (out of memory) */
#define NL_EHIP    4   /* any other HIP runtime error */
#define NL_ESTATE  5   /* call order violated */
#define NL_ECOMM   6   /* RCCL error */

/* numpy dtype codes accepted by the upload entry points */
#define NL_U8 0
#define NL_I8 1
#define NL_U16 2
#define NL_I16 3
#define NL_U32 4
#define NL_I32 5
#define NL_F32 6
#define NL_F64 7
#define NL_U64 8
#define NL_I64 9

/* fields a sampling call can read */
#define NL_FIELD_GAUSS  0  /* current Gaussian scale-space volume */
#define NL_FIELD_FROB   1  /* sqrt(frob_sq)/max_abs of the current scale, inf -> max finite (filtering.py:421-426, 562) */
#define NL_FIELD_FRANGI 2  /* the Filter output (after nl_filter_finish / nl_mask_volume) or the uploaded Frangi image */
#define NL_FIELD_VESSELNESS 3 /* vesselness * masks BEFORE nl_filter_finish: the running maximum seen through the
                                 cumulative mask bits (what NL_FIELD_FRANGI would hold after nl_filter_finish) */

typedef struct nl_ctx nl_ctx;

const char *nl_version(void);

/* Replaces cupy.cuda.runtime.getDeviceCount / memGetInfo (adaptive_run.py:23-43). */
int nl_device_count(int *count, char *err, size_t errlen);
int nl_device_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes, char *err, size_t errlen);
int nl_device_name(int device, char *name, size_t namelen, char *err, size_t errlen);

int nl_ctx_create(nl_ctx **out, int device,
                  int64_t nz_local, int64_t ny, int64_t nx,
                  int64_t gz0, int64_t gnz, int64_t own_lo, int64_t own_hi,
                  char *err, size_t errlen);
int nl_ctx_destroy(nl_ctx *ctx);
int nl_sync(nl_ctx *ctx, char *err, size_t errlen);
/* bytes of device memory a context of this shape allocates (for the low-memory decision,
   adaptive_run.py:88-100) */
int64_t nl_ctx_bytes(int64_t nz_local, int64_t ny, int64_t nx);

/* ------------------------------------------------------------------ Filter ------------ */

/* frame = xp.asarray(memmap[t], dtype=float32)  (filtering.py:917-924).
   Uploads local planes [z0, z1) from `host` (shape (z1-z0, ny, nx), dtype code) and
   converts to float32.  Also resets the per-frame state (vesselness = 0, masks = 1;
   filtering.py:807-808). */
int nl_filter_load(nl_ctx *ctx, const void *host, int dtype, int64_t z0, int64_t z1,
                   char *err, size_t errlen);

/* The same in two halves, so a caller can keep the raw frame resident in HBM and restart from
   it without touching the host again (what the reference's cupy path gets from keeping `frame`
   alive): nl_input_load = H2D of the raw planes (any dtype, extra device allocation of the
   frame's own size); nl_filter_begin = float32 conversion + per-frame reset, asynchronous. */
int nl_input_load(nl_ctx *ctx, const void *host, int dtype, int64_t z0, int64_t z1,
                  char *err, size_t errlen);
int nl_filter_begin(nl_ctx *ctx, char *err, size_t errlen);

/* One cascade step: ndi.gaussian_filter(gauss, sigma=delta, output=gauss, mode="reflect",
   truncate=3.0) (filtering.py:827-835) = up to three correlate1d passes, axis order Z, Y, X,
   float64 accumulation in scipy's symmetric order, float32 store after each pass.
   w* are the 2r+1 float64 kernel weights the host computed exactly like scipy
   (`_gaussian_kernel1d`); a NULL pointer skips that axis (sigma <= 1e-15).
   Output planes [z0, z1) are produced; the input must be valid on [z0-rz, z1+rz) clipped to
   the local slab (true global faces reflect). */
int nl_gauss_step(nl_ctx *ctx,
                  const double *wz, int rz, const double *wy, int ry, const double *wx, int rx,
                  int64_t z0, int64_t z1, char *err, size_t errlen);

/* The same step enqueued AHEAD on the context's side stream: the cascade step of scale s+1 only reads the Gaussian of
   scale s, so it can overlap the Hessian walk of scale s.  The result becomes NL_FIELD_GAUSS at nl_gauss_commit
   (call it before anything of scale s+1).  In between, only the per-scale calls of Filter are allowed (sampling by
   min/max + histogram, nl_hessian_stats, nl_vesselness_*); nl_sample_gather, nl_mask_volume* and Label use the free
   Gaussian volumes as scratch.
   Only steps that write at most TWO of the three ping-pong volumes can run ahead (a Z pass + a fused Y+X pass: equal
   in-plane radii up to nl_ctx_info("gauss_yx_max_r")); a step of one pass per axis would write its third pass into the
   volume the current scale reads and is refused with NL_ESTATE -- run it with nl_gauss_step, in order. */
int nl_gauss_step_ahead(nl_ctx *ctx, const double *wz, int rz, const double *wy, int ry, const double *wx, int rx,
                        int64_t z0, int64_t z1, char *err, size_t errlen);
int nl_gauss_commit(nl_ctx *ctx, char *err, size_t errlen);

/* arr[::sz, ::sy, ::sx] of a field on the owned planes (strides are those of the GLOBAL
   lattice; filtering.py:342-346, 355-356).  `out` receives the samples in C order, `*n`
   their number; `cap` is the capacity of `out` in elements. */
int nl_sample_gather(nl_ctx *ctx, int field, int64_t sz, int64_t sy, int64_t sx,
                     float *out, int64_t cap, int64_t *n, char *err, size_t errlen);

/* nl_sample_gather restricted to the positive samples, compacted on the device so that only they cross PCIe (every
   consumer takes arr[arr > 0] first: filtering.py:357, 957-959).  Order unspecified; `cap` >= number of lattice
   points; *n = number of positives written. */
int nl_sample_gather_positive(nl_ctx *ctx, int field, int64_t sz, int64_t sy, int64_t sx,
                              float *out, int64_t cap, int64_t *n, char *err, size_t errlen);
/* The same in two halves: _begin enqueues the compaction (and reports the number of lattice points = the capacity _end
   needs at most), _end waits and fetches.  Between the two the host is free; the only calls allowed on this context in
   between are nl_chain_finish / nl_chain_log (which enqueue nothing). */
int nl_sample_gather_positive_begin(nl_ctx *ctx, int field, int64_t sz, int64_t sy, int64_t sx, int64_t *n_lattice, char *err, size_t errlen);
int nl_sample_gather_positive_end(nl_ctx *ctx, float *out, int64_t cap, int64_t *n, char *err, size_t errlen);

/* min / max / count of the POSITIVE lattice samples (arr[arr > 0]; filtering.py:357 and the
   range=(min,max) of gpu_functions.py:31-35, 60-64).  npos == 0 leaves mn/mx untouched. */
int nl_sample_minmax(nl_ctx *ctx, int field, int64_t sz, int64_t sy, int64_t sx,
                     float *mn, float *mx, int64_t *npos, char *err, size_t errlen);

/* numpy.histogram(positive, bins=nbins, range=(first,last)) counts (gpu_functions.py:31, 60):
   float32 index computation + the +-1 correction against the float32 `edges` (nbins+1
   values from numpy.linspace, computed by the host).  counts[nbins] int64. */
int nl_sample_hist(nl_ctx *ctx, int field, int64_t sz, int64_t sy, int64_t sx,
                   const float *edges, int nbins, int64_t *counts, char *err, size_t errlen);

/* nl_sample_minmax followed by nl_sample_hist without a host round trip in between: numpy's float32 bin edges for
   range = (min, max) of the positive samples (`_get_outer_edges` / `np.linspace`, numpy/lib/_histograms_impl.py) are
   formed on the device.  *valid: 0 = no positive sample (counts are zero), 1 = ok, 2 = the range is not finite (numpy
   raises ValueError there; counts are zero).  `edges` (may be NULL) receives the nbins + 1 edges the device used;
   they equal np.linspace(np.float32(min), np.float32(max), nbins + 1, dtype=float32) bit for bit. */
int nl_sample_range_hist(nl_ctx *ctx, int field, int64_t sz, int64_t sy, int64_t sx, int nbins, float *mn, float *mx,
                         int64_t *n_positive, int64_t *counts, float *edges, int *valid, char *err, size_t errlen);
/* The same for two fields that need nothing from each other (the gamma samples of the Gaussian and the raw Frobenius
   samples of a scale: filtering.py:365-380, 421-444) in ONE device round trip; every output is an array of two (counts:
   2 x nbins, edges: 2 x (nbins + 1)), [0] = field_a. */
int nl_sample_range_hist2(nl_ctx *ctx, int field_a, int field_b, int64_t sz, int64_t sy, int64_t sx, int nbins, float *mn, float *mx,
                          int64_t *npos, int64_t *counts, float *edges, int *valid, char *err, size_t errlen);

/* The two histogram thresholds of nellie/utils/gpu_functions.py on a finished histogram (host arithmetic, no device
   work; callable without a context): `counts[nbins]` int64 as numpy.histogram returns them, `edges[nbins + 1]`
   float32 bin edges.  *otsu = centre of the bin maximising the between-class variance (gpu_functions.py:36-50),
   *triangle = the triangle-method bin centre (:64-94), both float32 values widened to double, computed with numpy's
   float64 operation order so that they carry numpy's bits.  *status: 0 ok, 1 = the triangle construction is degenerate
   (numpy raises "attempt to get argmax of an empty sequence" there; *triangle is 0, *otsu is valid). */
int nl_hist_thresholds(const int64_t *counts, const float *edges, int nbins, double *triangle, double *otsu, int *status,
                       char *err, size_t errlen);
/* The same for either edge type numpy.histogram produces: edges_f64 = 0 -> `edges` is float32[nbins + 1] (float32 data), 1 ->
   float64[nbins + 1] (integer and float64 data -- Label's intensity thresholds on the original image, labelling.py:414-431:
   the bin centres are then float64 like the reference's).  *otsu_var (may be NULL) = the between-class variance at the
   threshold, the second value of gpu_functions.py:50. */
int nl_hist_thresholds_ex(const int64_t *counts, const void *edges, int edges_f64, int nbins, double *triangle, double *otsu,
                          double *otsu_var, int *status, char *err, size_t errlen);
/* Host only: np.histogram(values, bins=nbins) of float32 data (range = its min .. max) and nl_hist_thresholds_ex of it in one
   call -- Label's log-domain threshold (labelling.py:448-455) on the few 10^4 samples the device compacted.  Same float32
   arithmetic as the device histogram.  *status: 0 ok, 1 degenerate triangle, 2 range not finite (numpy raises ValueError for
   both).  counts_out (nbins) / edges_out (nbins + 1): optional copies of the histogram. */
int nl_host_hist_thresholds_f32(const float *values, int64_t n, int nbins, double *triangle, double *otsu, int *status,
                                int64_t *counts_out, float *edges_out, char *err, size_t errlen);

/* Hessian by double finite differences of the current Gaussian volume (xp.gradient twice,
   filtering.py:518-536) on the owned planes; returns
     max_abs          = max over the six components of max|h|         (filtering.py:556-561; NOT yet mapped 0 -> 1)
     max_frob_sq      = largest finite frob_sq                         (filtering.py:538-543)
     any_inf          = 1 if some frob_sq is +inf                      (filtering.py:421-426)
   `spacing` = (dz, dy, dx) as the reference's python floats. */
int nl_hessian_stats(nl_ctx *ctx, const double spacing[3],
                     float *max_abs, float *max_frob_sq, int *any_inf, char *err, size_t errlen);

/* Fixes the normalisation NL_FIELD_FROB and nl_vesselness_step use: frob = sqrt(frob_sq)/max_abs,
   +inf replaced by max_finite (the host passes max_abs already mapped <=0 -> 1.0). */
int nl_set_frob_norm(nl_ctx *ctx, float max_abs, float max_finite, char *err, size_t errlen);

/* One scale of filtering.py:842-851 on the owned planes:
     h_mask     = use_thr ? frob > thr : frob > 0            (filtering.py:428-444)
     v          = Frangi(eigvalsh(H) sorted by |.|) on h_mask, 0 elsewhere (filtering.py:574-585, 744-766)
     vesselness = maximum(vesselness, v); masks &= h_mask    (filtering.py:850-851)
   The host calls it only when the mask is non-empty (filtering.py:843-844).
   Planes [z0, z1) are processed (z0 = z1 = -1: the owned planes; a slab passes own +-2 so that the
   opening of nl_mask_volume finds valid neighbours).  `mask_count` (may be NULL) receives the number
   of OWNED voxels in h_mask. */
int nl_vesselness_step(nl_ctx *ctx, float gamma_sq, float alpha_sq, float beta_sq,
                       int use_thr, float thr, int64_t z0, int64_t z1, int64_t *mask_count,
                       char *err, size_t errlen);

/* The grid spacing nl_hessian_stats would set, without the statistics pass (needed before NL_FIELD_FROB can be
   sampled for the bracket of nl_vesselness_spec). */
int nl_set_spacing(nl_ctx *ctx, const double spacing[3], char *err, size_t errlen);

/* nl_hessian_stats + nl_vesselness_step in ONE walk over the Hessian (filtering.py:555-585), for a mask threshold
   that is not known yet but predicted to satisfy  fsq_lo <= fsq_min <= fsq_hi  in units of frob_sq (the
   un-normalised squared Frobenius norm, filtering.py:538-543).  Voxels with frob_sq >= fsq_hi are treated as
   h_mask, below fsq_lo as not h_mask, the ones in between are parked.  Returns the statistics of
   nl_hessian_stats plus `overflow` (a queue region was too small).  Nothing is final until
   nl_vesselness_resolve confirms the bracket; if it cannot (or any_inf / overflow is set) the caller runs
   nl_vesselness_step as if this call had not happened.  Planes [z0, z1) must cover the owned planes.
   Availability: nl_ctx_info("vesselness_one_pass"). */
int nl_vesselness_spec(nl_ctx *ctx, const double spacing[3], float fsq_lo, float fsq_hi, int64_t z0, int64_t z1,
                       float *max_abs, float *max_frob_sq, int *any_inf, int *overflow, char *err, size_t errlen);

/* Device-resident threshold chain (csrc/chain.inc): the four data-dependent scalars of a scale -- gamma, the walk's bracket,
   max |H| and the Frobenius threshold (filtering.py:365-380, 421-444, 555-566) -- are computed by small kernels between the large
   ones, which read them from device memory, so a frame's scale loop is enqueued without a single wait:
     nl_chain_begin(n)            a frame of n scales (<= 16) starts
     nl_gauss_step ...            the cascade step of scale k, as always
     nl_chain_scale(...)          everything else of scale k: lattice histograms, thresholds, walk, exact histogram, resolve kernel
                                  (sz, sy, sx: lattice strides; division / margin / test_scale: frob_thresh_division, the relative
                                  half-width of the bracket, a factor on the predicted threshold (1.0; tests force misses with it))
     nl_chain_flush()             optional: start the download of the records now; kernels enqueued after it (the samples of the
                                  percentile threshold: nl_sample_gather_positive_begin) run while nl_chain_finish waits for the
                                  records alone and repeats the decisions on the host
     nl_chain_finish(...)         THE wait: per scale flags[k] (0 = stands), gamma, max |H|, the threshold, this context's h_mask count
   Every histogram and every derived scalar is logged, and nl_chain_finish repeats the arithmetic on the host with the code of
   the synchronous entry points and compares bit for bit: a difference, or any condition the fast path does not handle (no
   positive sample, degenerate triangle, +inf, queue overflow, bracket miss, empty scale), gives a non-zero flag and the caller
   redoes the frame with nl_sample_range_hist2 / nl_vesselness_spec / nl_vesselness_resolve.  Same results either way.
   nl_chain_log: test hook, the logged record of scale k (which: 0 Gaussian, 1 raw Frobenius, 2 normalised Frobenius samples). */
int nl_chain_begin(nl_ctx *ctx, int n_scales, char *err, size_t errlen);
int nl_chain_scale(nl_ctx *ctx, const double spacing[3], int64_t sz, int64_t sy, int64_t sx, double alpha_sq, double beta_sq,
                   double division, double margin, double test_scale, int64_t z0, int64_t z1, char *err, size_t errlen);
int nl_chain_flush(nl_ctx *ctx, char *err, size_t errlen);
int nl_chain_finish(nl_ctx *ctx, int *flags, double *gamma, double *max_abs, double *thr, int64_t *mask_count, char *err, size_t errlen);
int nl_chain_log(nl_ctx *ctx, int k, int which, int64_t *counts, float *edges, float *range, double *scalars, char *err, size_t errlen);

/* The scales of a frame walked OUT of sigma order.  The frame is max_s(v_s) * AND_s(m_s): any walk order gives the same bits, and a walk
   queues only voxels alive in the masks walked before it, so the most selective masks should come first.  A whole 3-D volume on one
   context whose cascade steps are all fused (nl_gauss_step_fused: one kernel, one volume read, one written), so that the Gaussians of
   three consecutive scales coexist in the three ping-pong volumes:
     nl_chain_begin_unordered(n)  instead of nl_chain_begin
     nl_gauss_step ...            the cascade step of scale k (sigma order); refused with NL_ESTATE while three scales are pending
     nl_chain_sample(k, ...)      right after it: lattice histograms, gamma, bracket, and the forecast of the scale's mask fraction;
                                  scale k is now pending -- its Gaussian and its lattice cache are kept until it is walked
     nl_chain_estimates(frac, n)  the forecasts of the scales sampled so far (< 0: none); waits for the newest sampling round.  They
                                  steer the order only
     nl_chain_walk(k, ...)        any pending scale: walk, exact histogram, resolve kernel; frees the scale's volume
     nl_chain_flush / nl_chain_finish / nl_chain_log as above: records, flags and results by sigma index k.
   The frame's last cascade step pre-zeroes the label volume (NELLIE_PREZERO) only if its third volume holds no pending scale. */
int nl_gauss_step_fused(nl_ctx *ctx, const double *wz, int rz, const double *wy, int ry, const double *wx, int rx, int *fused,
                        char *err, size_t errlen);
int nl_chain_begin_unordered(nl_ctx *ctx, int n_scales, char *err, size_t errlen);
int nl_chain_sample(nl_ctx *ctx, int k, const double spacing[3], int64_t sz, int64_t sy, int64_t sx, double division, double margin,
                    double test_scale, char *err, size_t errlen);
int nl_chain_estimates(nl_ctx *ctx, float *frac, int n, char *err, size_t errlen);
int nl_chain_walk(nl_ctx *ctx, int k, const double spacing[3], int64_t sz, int64_t sy, int64_t sx, double alpha_sq, double beta_sq,
                  double division, int64_t z0, int64_t z1, char *err, size_t errlen);

/* Second half of nl_vesselness_spec, with the arguments nl_vesselness_step takes (nl_set_frob_norm first).
   *hit = 1: the exact threshold lies inside the bracket; the parked voxels got the exact h_mask test and the scale
   is complete, bit-identical to nl_vesselness_step (`mask_count` as there).  *hit = 0: no effect. */
int nl_vesselness_resolve(nl_ctx *ctx, float gamma_sq, float alpha_sq, float beta_sq, int use_thr, float thr,
                          int *hit, int64_t *mask_count, char *err, size_t errlen);

/* The resolve kernel of nl_vesselness_resolve runs on a side stream so that the Gaussian cascade step of the next
   scale (which touches neither the vesselness volume nor the masks) can overlap it; every entry point that does
   touch them orders itself after it.  Passing mask_count = NULL to nl_vesselness_resolve keeps the call
   asynchronous; this returns the count later (and waits for the kernel). */
int nl_vesselness_count(nl_ctx *ctx, int64_t *mask_count, char *err, size_t errlen);

/* Host only (no context, no device): the launch plan of the Hessian walk (csrc/walk_plan.h) for a slab of nzl x ny x nx voxels with the
   owned planes [own_lo, own_hi), walked over [z0, z1) in `mode` (0 statistics -- always the owned planes --, 1 known threshold, 2 one
   pass), fast_div / fast_div2 as the divisors' proof came out (nl_ctx_info("fast_div") >= 1 / == 2), and the switches' values as the
   environment would give them: switches[7] = NELLIE_HV_RS, NELLIE_HV_NP, NELLIE_HV_DPP, NELLIE_HM_TY, NELLIE_HV_ZCHUNK, NELLIE_VQ_CAP
   (0: unset), NELLIE_SPEC_MAX_GB.  plan[13] = kernel family (0 one voxel per thread, 1 pair, 2 wave-autonomous), tile rows, rs, np,
   division form (0 float64, 1 three instructions, 2 two), planes per workgroup, tiles in X, tiles in Y, Z chunks, grid of a launch
   (workgroups; waves for family 2), its queue regions, queue entries per region, planes per launch. */
int nl_host_walk_plan(int mode, int64_t nzl, int64_t ny, int64_t nx, int64_t own_lo, int64_t own_hi, int64_t z0, int64_t z1, int fast_div,
                      int fast_div2, const int64_t switches[7], int64_t plan[13], char *err, size_t errlen);

/* ---- 2-D images (im_info.no_z): a context of shape (1, ny, nx) switched to 2-D ------------------------------
   nl_set_ndim(ctx, 2) makes nl_hessian_stats, NL_FIELD_FROB, nl_vesselness_step and nl_mask_volume follow the
   reference's 2-D branches: Hessian (hxx, hxy, hyy) by np.gradient twice (filtering.py:461-490), closed-form
   float32 eigenvalues (filtering.py:675-690), the two-eigenvalue Frangi response (filtering.py:732-741) and the
   4-connected binary_opening.  nl_gauss_step is called with wz = NULL. */
int nl_set_ndim(nl_ctx *ctx, int ndim, char *err, size_t errlen);

/* One sigma of the multi-scale blob response (filtering.py:779-789): current = -gaussian_laplace(gauss, (s, s)) * s^2
   [* masks], running element-wise maximum.  wy2/wy0/wx2/wx0: scipy's `_gaussian_kernel1d` of order 2 / 0 for the Y and
   X axes, 2r+1 float64 weights each (truncate 4.0); s2 = float32(s**2); `gauss` is the current NL_FIELD_GAUSS
   (the reference's in-place cascade leaves the LAST scale's Gaussian in `frame`, filtering.py:811, 927-928). */
int nl_log2d_step(nl_ctx *ctx, const double *wy2, const double *wy0, const double *wx2, const double *wx0, int r,
                  float s2, int first, int use_mask, char *err, size_t errlen);

/* filtering.py:792-795 + 928-930: clip at 0, divide by (max + 1e-12) and by 10, NL_FIELD_FRANGI =
   maximum(NL_FIELD_FRANGI, blob).  Call after nl_filter_finish.  n_positive = pixels > 0 afterwards. */
int nl_log2d_finish(nl_ctx *ctx, int64_t *n_positive, char *err, size_t errlen);

/* vesselness * masks (filtering.py:926) -> NL_FIELD_FRANGI on planes [z0, z1) (-1, -1: owned).
   n_positive = number of OWNED voxels > 0 (the `sum > 0` test of filtering.py:1016-1017). */
int nl_filter_finish(nl_ctx *ctx, int64_t z0, int64_t z1, int64_t *n_positive, char *err, size_t errlen);

/* `_remove_edges` (filtering.py:969-1000, called at :931-932 when remove_edges=True) on the frame nl_filter_finish left
   on the device: in every Z plane (a 2-D image is one plane) the rows that hold a non-zero value span [rmin, rmax];
   min(margin, rmax - rmin + 1) rows at each end of the span are zeroed (margin = 15 in the reference).
   *n_positive = values > 0 that remain on the owned planes (`float(sum(frame)) > 0`, filtering.py:1014). */
int nl_remove_edges(nl_ctx *ctx, int margin, int64_t *n_positive, char *err, size_t errlen);

/* filtering.py:964-966: mask = frangi > thr; binary_opening (6-connected cross, one
   iteration, border 0); frangi *= mask. */
int nl_mask_volume(nl_ctx *ctx, float thr, char *err, size_t errlen);

/* nl_filter_finish + nl_mask_volume in one go for the common case (filtering.py:926 + 964-966), called INSTEAD of
   nl_filter_finish after the last scale with the percentile threshold of the NL_FIELD_VESSELNESS samples:
   the threshold pass reads the vesselness only where the cumulative mask has bits, the final pass reads it only where
   the opened mask has bits and writes zeros elsewhere (12 instead of 27 bytes per voxel of traffic).
   n_positive = OWNED voxels of vesselness * masks that are > 0 (what nl_filter_finish reports).  Requires at least
   one evaluated scale. */
int nl_mask_volume_fused(nl_ctx *ctx, float thr, int64_t *n_positive, char *err, size_t errlen);
/* The same epilogue with NO host decision in it (round 4; csrc/percentile.inc): nl_tail_enqueue gathers the positive lattice samples
   of `vesselness * masks` (strides sz, sy, sx: filtering.py:348-363), selects their q-th percentile on the device with numpy's
   float32 'linear' rule (filtering.py:963) -- on Z slabs from histograms all-reduced between the kernels, no sample leaves its
   rank --, and runs the percentile mask, the opening and the product (filtering.py:964-966) with the threshold read from device
   memory.  Enqueue only.  nl_tail_finish waits and reports (samples, the two order statistics a <= b, the interpolation weight,
   the threshold, the positive voxels of the product: global on a fused communicator); commit != 0 makes the result the frame
   (as nl_mask_volume_fused does) unless there was no positive sample -- the caller then takes the plain path. */
int nl_tail_enqueue(nl_ctx *ctx, int64_t sz, int64_t sy, int64_t sx, double q, char *err, size_t errlen);
int nl_tail_finish(nl_ctx *ctx, int commit, int64_t *n_samples, float *a, float *b, float *gamma, float *thr, int64_t *n_positive,
                   char *err, size_t errlen);
/* _mask_volume (filtering.py:952-967) on the finished Frangi frame with the percentile selected on the device (samples, selection,
   `frame > thr`, opening, product; one wait): the epilogue of 2-D images, of remove_edges runs and of slabs without the fused
   epilogue.  Reports (n, a, b, gamma, thr) for the host's check; n = 0: the frame was left as it is. */
int nl_mask_volume_dev(nl_ctx *ctx, int64_t sz, int64_t sy, int64_t sx, double q, int64_t *n_samples, float *a, float *b, float *gamma,
                       float *thr, char *err, size_t errlen);
/* tests: numpy.percentile(values, q) of n positive float32 values by the device's selection */
int nl_debug_percentile(nl_ctx *ctx, const float *values, int64_t n, double q, float *thr, float *a, float *b, char *err, size_t errlen);

/* D2H of NL_FIELD_FRANGI local planes [z0, z1) (filtering.py:1023-1031). */
int nl_filter_store(nl_ctx *ctx, float *host, int64_t z0, int64_t z1, char *err, size_t errlen);

/* Debug / test access: D2H of the current Gaussian volume, local planes [z0, z1). */
int nl_gauss_store(nl_ctx *ctx, float *host, int64_t z0, int64_t z1, char *err, size_t errlen);

/* ------------------------------------------------------------------ Z-slabs ----------- */
/* The reference has no distributed code; these entry points are new functionality: a
   volume too large for one device is cut into Z-slabs, one context per GPU, ghost planes exchanged
   between Z neighbours over RCCL/xGMI, scalars and histograms all-reduced. */

/* D2H / H2D of arbitrary local planes of a float field (NL_FIELD_GAUSS / NL_FIELD_FRANGI): the
   host-mediated exchange used by tests and by communicators without RCCL. */
int nl_planes_get(nl_ctx *ctx, int field, int64_t z0, int64_t z1, float *host, char *err, size_t errlen);
int nl_planes_put(nl_ctx *ctx, int field, int64_t z0, int64_t z1, const float *host, char *err, size_t errlen);

/* RCCL communicator: rank 0 calls nl_comm_unique_id (128 bytes), distributes it out of band, every rank
   calls nl_comm_init on its context. */
int nl_comm_unique_id(char *id128, char *err, size_t errlen);
int nl_comm_init(nl_ctx *ctx, int world, int rank, const char *id128, char *err, size_t errlen);
/* Loopback transport: an id from nl_comm_loopback_id makes nl_comm_init / nl_comm_init2 build a communicator between
   `world` contexts of THIS process (one host thread per rank, any devices of the process -- typically all on one GPU).
   Every exchange above -- ghost planes, bit planes, fused reductions, variable all-gathers -- then runs through the same
   code with the same pointers, offsets, counts, streams and events as over RCCL, the data moving by device-to-device
   copies on those streams: the N >= 2 paths are testable on a one-GPU box.  NELLIE_LOOPBACK_DELAY_US=n puts a random
   0..n us spin in front of every transfer (stress for missing stream dependencies). */
int nl_comm_loopback_id(char *id128, char *err, size_t errlen);

/* Exchange `depth` ghost planes of a float field with both Z neighbours (ncclSend/ncclRecv in one group,
   asynchronous on the context stream). */
int nl_halo_exchange(nl_ctx *ctx, int field, int64_t depth, char *err, size_t errlen);
/* The same for the `depth` owned planes that start `offset` planes inside the boundary (they land at the same distance
   from the interface on the other side): the per-step exchange of the cascade -- a rank computes every scale on its owned
   planes +- 4 and fetches, per step, only the r_z(s) planes beyond that from the neighbour that owns them.  async != 0
   (needs nl_comm_init2: a second communicator with its own unique id) runs the exchange on a stream and communicator of
   its own, ordered after the work submitted so far; the next nl_gauss_step waits for it, everything else runs beside it. */
int nl_halo_exchange_at(nl_ctx *ctx, int field, int64_t offset, int64_t depth, int async, char *err, size_t errlen);
int nl_comm_init2(nl_ctx *ctx, int world, int rank, const char *id128, char *err, size_t errlen);

/* All-reduce of a few host values through RCCL: dtype 0 = int64, 1 = float32; op 0 = sum, 1 = min, 2 = max. */
int nl_allreduce(nl_ctx *ctx, void *host_inout, int64_t count, int dtype, int op, char *err, size_t errlen);

/* ------------------------------------------------------------------ Label ------------- */

/* frangi_in_mem = xp.asarray(frangi_view) (labelling.py:547): host float32 -> NL_FIELD_FRANGI. */
int nl_label_load_frangi(nl_ctx *ctx, const float *host, int64_t z0, int64_t z1,
                         char *err, size_t errlen);

/* frangi *= (original > thresh) (labelling.py:550-552); the comparison is done in float64 on
   the exactly converted original, `thresh` already rounded by the host as numpy would. */
int nl_label_intensity_mask(nl_ctx *ctx, const void *host_original, int dtype, double thresh,
                            char *err, size_t errlen);
/* The same on planes [z0, z1) of the context's frame; `host_original` holds those planes of the original image (a Z slab masks
   the planes it owns: Label's intensity thresholds on a sharded frame). */
int nl_label_intensity_mask_planes(nl_ctx *ctx, const void *host_original, int dtype, double thresh, int64_t z0, int64_t z1,
                                   char *err, size_t errlen);
/* The same against an integer threshold, for NL_U64 and NL_I64 images only: `thresh` is of the image's own type (for NL_U64 its
   bits) and the comparison is done on integers, as numpy compares a 64-bit integer array with an integer; in float64 the
   elements beyond 2^53 would round. */
int nl_label_intensity_mask_int(nl_ctx *ctx, const void *host_original, int dtype, int64_t thresh, int64_t z0, int64_t z1,
                                char *err, size_t errlen);

/* flat[offset::step] of a field (labelling.py:393, 412). */
int nl_flat_sample_gather(nl_ctx *ctx, int field, int64_t offset, int64_t step,
                          float *out, int64_t cap, int64_t *n, char *err, size_t errlen);

/* The same, positive samples only, compacted on the device (labelling.py:426-433); order unspecified. */
int nl_flat_sample_gather_positive(nl_ctx *ctx, int field, int64_t offset, int64_t step, float *out, int64_t cap,
                                   int64_t *n, char *err, size_t errlen);

/* labelling.py:467-509 on the device:
     mask = has_thr ? frangi > thr : 0; binary_fill_holes (6-conn) if fill_holes;
     label (26-conn); remove components with < min_area voxels; uniform_filter(3) > 0.5;
     label again.  Ids are int32, 1..K in raster order of each component's first voxel. */
int nl_label_run(nl_ctx *ctx, int has_thr, float thr, int64_t min_area, int fill_holes,
                 int64_t *n_labels, char *err, size_t errlen);

/* Label on Z-slabs.  The thresholded mask is 1 bit/voxel, so instead of stitching per-slab labellings
   every rank (1) packs `frangi > thr` of its OWN planes into a GLOBAL bit mask (nl_label_pack), (2) the bit
   planes are all-gathered (nl_label_bits_allgather over RCCL, or nl_label_bits_get/put through the host),
   (3) the run-level labelling of labelling.py:484-509 runs on the global mask on every rank
   (nl_label_run_global) and each rank paints only its own planes.  slab_plane0 has world+1 entries: the first
   global plane of every rank's slab, then gnz.  Rows are (global plane * ny + y). */
int nl_label_pack(nl_ctx *ctx, int has_thr, float thr, char *err, size_t errlen);
int nl_label_bits_get(nl_ctx *ctx, int64_t row0, int64_t nrows, uint64_t *host, char *err, size_t errlen);
int nl_label_bits_put(nl_ctx *ctx, int64_t row0, int64_t nrows, const uint64_t *host, char *err, size_t errlen);
int nl_label_bits_allgather(nl_ctx *ctx, const int64_t *slab_plane0, char *err, size_t errlen);
int nl_label_run_global(nl_ctx *ctx, int64_t min_area, int fill_holes, int64_t *n_labels, char *err, size_t errlen);

/* Label on Z-slabs WITHOUT replication (the production multi-GPU path; the reference's closest precedent is the chunk
   stitching of labelling.py:585-691 with its union-find :221-288, which however labels chunks independently and is not
   equivalent to the full-volume result -- this is).  Every rank labels its owned planes plus ONE ghost bit plane per
   interior side (exchanged with nl_slab_bits_exchange over RCCL, or nl_slab_bits_get / _put through the host).  A
   component that crosses an interface shows up on both ranks as a tree containing runs of the two planes both ranks see,
   and the k-th SEGMENT COMPONENT of such a plane (a connected piece of the plane's mask inside a band of rows: what the in-LDS
   level of the union-find joins) is the same voxels on both sides: `nl_slab_phase` hands those (tree, quantity) pairs -- a few
   hundred per plane -- to the host, which joins the trees of neighbouring ranks and patches the result back.  Three phases:
     phase 0 (fill)   6-connected background; quantity = 1 if the tree touches a face of the GLOBAL volume; after the
                      patch nl_slab_apply sets the enclosed background of the owned planes        (labelling.py:486)
     phase 1 (area)   26-connected foreground; quantity = voxels on the OWNED planes; after the patch (global sums)
                      nl_slab_apply(min_area) writes the kept-objects mask                        (labelling.py:489-501)
     nl_slab_majority majority filter of the kept-objects mask (its ghost planes exchanged first)  (labelling.py:503-505)
     phase 2 (number) 26-connected foreground; quantity = first run of the tree on the owned planes (INT32_MAX: none).
                      The owner of a component is the lowest rank holding voxels of it; nl_slab_number ranks the trees a
                      rank owns in raster order (and says which rank each tree of `set` got), nl_slab_paint adds the rank's
                      base id (exclusive sum of the lower ranks' counts) and takes the labels of trees owned elsewhere from
                      the host: ids 1..K in raster order of the first voxel, exactly scipy.ndimage.label's numbering of the
                      whole volume                                                                  (labelling.py:507)
   nl_slab_phase(phase, gather, block_ints, out, &need_ints, &nruns): one call per phase, one wait.  A rank's tables are a blob
   of int32: [n0 n1 n2 n3 | ints in the blob | overflow | runs | 0] [roots of plane 0..3] [values of plane 0..3], planes in the
   order ghost-low, first owned, last owned, ghost-high (n = 0 towards a side without a neighbour).  gather = 0: out receives
   this rank's blob (one block of block_ints); gather = 1 (needs nl_comm_init): the blobs of ALL ranks, all-gathered over RCCL
   on the context stream in fixed blocks (no size negotiation), rank r's at out + r * block_ints.  *need_ints: the largest blob;
   if it exceeds block_ints nothing was copied and the caller repeats with phase = -1 and a larger block (nothing is recomputed). */
int nl_slab_label_pack(nl_ctx *ctx, int has_thr, float thr, char *err, size_t errlen);
int nl_slab_bits_get(nl_ctx *ctx, int which, int64_t plane, uint64_t *host, char *err, size_t errlen);
int nl_slab_bits_put(nl_ctx *ctx, int which, int64_t plane, const uint64_t *host, char *err, size_t errlen);
int nl_slab_bits_exchange(nl_ctx *ctx, int which, char *err, size_t errlen);
int nl_slab_phase(nl_ctx *ctx, int phase, int gather, int64_t block_ints, int32_t *out, int64_t *need_ints, int64_t *nruns,
                  char *err, size_t errlen);
int nl_slab_patch(nl_ctx *ctx, int64_t n, const int32_t *roots, const int32_t *values, char *err, size_t errlen);
int nl_slab_apply(nl_ctx *ctx, int64_t min_area, char *err, size_t errlen);
int nl_slab_majority(nl_ctx *ctx, char *err, size_t errlen);
int nl_slab_number(nl_ctx *ctx, int64_t n_clear, const int32_t *clear, int64_t n_set, const int32_t *set, int64_t *n_local,
                   int32_t *ids_of_set, char *err, size_t errlen);
int nl_slab_paint(nl_ctx *ctx, int64_t base, int64_t n, const int32_t *roots, const int32_t *labels, char *err, size_t errlen);
/* Host only (no device, no context): joins the tables of `world` ranks (blobs as nl_slab_phase writes them, rank r's at
   blobs + r * block_ints).  One NODE per (rank, tree) that appears in a table, ranks in order, a rank's trees by ascending root;
   node_rank / node_root / node_val (int64, the tree's quantity) / node_comp receive up to `cap` nodes, *n_nodes their count,
   *n_comp the number of components after joining rank r's planes 2, 3 with rank r + 1's planes 0, 1 entry by entry; components
   are numbered in the order of their smallest node.  Returns NL_EINVAL if two ranks disagree about a shared plane.  Every rank
   calls it on the same gathered blobs and gets the same answer (the reference has no counterpart: SURVEY.md 8(e)). */
int nl_host_slab_join(int world, const int32_t *blobs, int64_t block_ints, int64_t cap, int64_t *n_nodes, int64_t *n_comp,
                      int64_t *node_rank, int32_t *node_root, int64_t *node_val, int64_t *node_comp, char *err, size_t errlen);

/* The positive samples of ALL ranks, compacted on the device, all-gathered over RCCL in fixed blocks and fetched, in one call with
   one wait: mode 0 = arr[::a, ::b, ::c] of `field` where > 0 (filtering.py:348-363, the samples of gamma / the percentile
   threshold), mode 1 = flat[a::b] where > 0 (labelling.py:418-433, Label's threshold).  block_items: a bound on the sample POINTS
   of any one rank, the same number on every rank (the callers derive it from the global shape).  out (cap floats) receives the
   samples rank by rank (order inside a rank unspecified: the consumers are order-free), counts[world] how many each rank gave. */
int nl_positive_samples_world(nl_ctx *ctx, int field, int mode, int64_t a, int64_t b, int64_t c, int64_t block_items,
                              float *out, int64_t cap, int64_t *counts, char *err, size_t errlen);
/* Variable-size all-gather of host bytes over RCCL (ncclAllGather on padded device staging): `recv` receives
   world * max_bytes bytes, rank r's block at r * max_bytes (its first bytes_of[r] bytes are valid; bytes_of has `world`
   entries and is filled here).  Used for the threshold samples and the slab tables, so that no data of the path
   travels through the control plane. */
int nl_allgather_bytes(nl_ctx *ctx, const void *send, int64_t nbytes, void *recv, int64_t max_bytes, int64_t *bytes_of,
                       char *err, size_t errlen);

/* The same when the caller does not know the largest block: the library gathers the sizes, uses their maximum (rounded up
   to 16) as the block size and lands the blocks in a page-locked buffer the CONTEXT owns: *recv (valid until the next
   call on this context), rank r's block at r * *stride. */
int nl_allgather_var(nl_ctx *ctx, const void *send, int64_t nbytes, void **recv, int64_t *stride, int64_t *bytes_of,
                     char *err, size_t errlen);

/* "Fused" reductions: with on != 0, nl_sample_minmax / nl_sample_hist / nl_sample_range_hist / nl_vesselness_spec return the
   value over ALL ranks of the communicator (range and counts of the lattice samples; max |H|, max frob_sq and the inf /
   overflow flags of the one-pass walk) -- the RCCL all-reduce runs on the context stream between the kernels, so the
   host-level nl_allreduce (one more device round trip each) is not needed for them.  The reference has no counterpart:
   its statistics are whole-volume numpy / cupy reductions (filtering.py:348-380, 555-562).  Requires nl_comm_init; every
   rank must issue the same sequence of calls. */
int nl_comm_fuse(nl_ctx *ctx, int on, char *err, size_t errlen);

/* D2H of the int32 label volume, local planes [z0, z1) (labelling.py:727-729). */
int nl_label_store(nl_ctx *ctx, int32_t *host, int64_t z0, int64_t z1, char *err, size_t errlen);

/* ------------------------------------------------------------------ frame streaming --- */
/* 3-D+T stacks: the reference moves every frame with a blocking xp.asarray / .get() (filtering.py:924, 1023;
   labelling.py:546, 727).  These entry points overlap the three legs instead: frame t+1 host->HBM on a copy
   stream (nl_input_load_async into slot 0/1, nl_input_select before nl_filter_begin), frame t computing, frame
   t-1's outputs HBM->host on a second copy stream (nl_outputs_stage: device copies into staging volumes;
   nl_outputs_fetch_async; nl_outputs_wait).  Host buffers must come from nl_pinned_alloc. */
int nl_pinned_alloc(void **ptr, int64_t bytes, char *err, size_t errlen);
int nl_pinned_free(void *ptr);
int nl_host_register(void *ptr, int64_t bytes, char *err, size_t errlen);   /* page-lock caller-owned memory */
int nl_host_unregister(void *ptr);
int nl_input_load_async(nl_ctx *ctx, int slot, const void *host_pinned, int dtype, char *err, size_t errlen);
int nl_input_select(nl_ctx *ctx, int slot, char *err, size_t errlen);
/* Blocks until the upload nl_input_load_async started into that slot has arrived.  The streamer with several lanes (contexts of one
   GPU working on different frames of a stack, nellie_amd/streaming.py) feeds them from ONE upload thread that keeps exactly one
   host -> HBM copy in flight: two concurrent copies share the link badly (measured: 2.49 ms alone, 3.57 ms each as a pair for a
   134 MB frame, profiles/r06_stream_lanes_trace.txt), and the upload is what bounds a float32 stack (filtering.py:917-924 is the
   blocking load this replaces). */
int nl_input_wait(nl_ctx *ctx, int slot, char *err, size_t errlen);
int nl_outputs_stage(nl_ctx *ctx, int with_labels, char *err, size_t errlen);
int nl_outputs_fetch_async(nl_ctx *ctx, float *frangi_pinned, int32_t *labels_pinned, char *err, size_t errlen);
int nl_outputs_wait(nl_ctx *ctx, char *err, size_t errlen);

/* Packed outputs.  Both products are ~98 % zeros; the dense download (8 B/voxel, the reference's blocking .get() per
   frame: filtering.py:1023, labelling.py:727) is what bounds a streamed stack.  nl_outputs_pack leaves in a staging buffer of
   the context, per volume: 1 bit per voxel (!= 0 / label > 0; rows padded to 64-voxel words), one u32 per row + 1 (index of
   the row's first item) and the items -- the non-zero float32 values in raster order, and ONE int32 label per maximal X-run
   of labelled voxels.  *nbytes = size of the blob; 0 = this frame does not pack (more than n / 4 items, or X-neighbours
   with different labels): fall back to nl_outputs_stage / nl_outputs_fetch_async.  nl_outputs_fetch_packed_async copies the
   blob to page-locked host memory on the download stream (nl_outputs_wait blocks until it landed; it is one of the
   copy-thread calls).  nl_outputs_unpack is host code: it expands a blob into dense (nz, ny, nx) arrays with `threads` host
   threads; dst_elems = elements each destination array holds -- a blob whose header describes another volume, or whose
   sections / row offsets do not fit its size, is refused before anything is written; zero_fill = 0 if the arrays are known
   to hold zeros (a freshly created file), rows without content are then not touched at all. */
int nl_outputs_pack(nl_ctx *ctx, int with_labels, int64_t *nbytes, char *err, size_t errlen);
/* on != 0: every nl_label_run of this context ends by enqueueing nl_outputs_pack(ctx, 1, ...) of its frame UNDER ITS OWN WAIT (the
   item counts stay on the device: no host round trip between counting and emitting); the nl_outputs_pack(ctx, 1, ...) that follows
   returns at once.  A streamed stack (labelling.py:701-734 has a blocking .get() per frame instead) loses two host waits per frame. */
int nl_outputs_pack_with_label(nl_ctx *ctx, int on, char *err, size_t errlen);
int nl_outputs_fetch_packed_async(nl_ctx *ctx, void *host_pinned, int64_t nbytes, char *err, size_t errlen);
int nl_outputs_unpack(const void *blob, int64_t nbytes, float *frangi, int32_t *labels, int64_t dst_elems, int zero_fill,
                      int threads, char *err, size_t errlen);
/* Host code: zero `bytes` bytes at `dst` with `threads` host threads.  For callers that unpack into arrays of their own (not
   freshly created sparse files): the fill of both dense outputs -- 8 B/voxel of host memory traffic, most of what an unpack
   with zero_fill = 1 takes -- can run on host threads WHILE the GPU still works on the frame, and the unpack (zero_fill = 0)
   then only scatters the non-zero items. */
int nl_host_zero(void *dst, int64_t bytes, int threads, char *err, size_t errlen);

/* ------------------------------------------------------------------ Hu-moment tracking -------- */
/* nellie/tracking/hu_tracking.py on the device (DESIGN.md "Tracking").  A tracker has its own stream and buffers (marker-sized ones
   grow with the marker count, never shrink); it keeps the features of the last two frames resident.
   nl_track_create   : frame shape (nz = 1 for ndim 2) and spacing ((Z,) Y, X in um) of the T stack.
   nl_track_frame    : uploads intensity (uint8 / uint16 / float32), frangi, distance (float32) and marker (uint8) of one frame
                       and computes its markers (np.argwhere order), radii, stats and log-Hu features; the frame before stays
                       resident as the "pre" frame.  n_markers = the frame's marker count.
   nl_track_features : which = 0 the last frame, 1 the one before: coords (n, ndim) int64, stats (n, 4) float32, log-Hu
                       (n, 6 | 18) float64; NULL pointers are skipped.
   nl_track_match    : last frame (rows) against the one before (columns); mode 0 dense, 1 sparse; row_* has n_post entries,
                       col_* n_pre; index -1 = no candidate (sparse); full (dense, may be NULL) = the float16 cost matrix.
   nl_host_half_round / nl_host_half_nansum : the float64 -> float16 cast and np.nansum of float16 rows the dense matcher uses.
   nl_host_np_sum_f32 : numpy's float32 np.sum of n floats (8192-item blocks, pairwise inside), the order of the float stats. */
typedef struct nl_track nl_track;
int nl_track_create(nl_track **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, char *err, size_t errlen);
int nl_track_destroy(nl_track *tracker);
int nl_track_frame(nl_track *tracker, const void *intensity, int dtype, const float *frangi, const float *distance, const uint8_t *marker,
                   int64_t *n_markers, char *err, size_t errlen);
int nl_track_features(nl_track *tracker, int which, int64_t *coords, float *stats, double *hu, char *err, size_t errlen);
int nl_track_match(nl_track *tracker, int mode, double max_distance, int32_t *row_idx, float *row_cost, int32_t *col_idx,
                   float *col_cost, uint16_t *full, char *err, size_t errlen);
int nl_host_half_round(const double *in, uint16_t *out, int64_t n, char *err, size_t errlen);
int nl_host_half_nansum(const uint16_t *in, int64_t rows, int k, uint16_t *out, char *err, size_t errlen);
int nl_host_np_sum_f32(const float *in, int64_t n, float *out, char *err, size_t errlen);

/* ------------------------------------------------------------------ flow-vector interpolation -------- */
/* nellie/tracking/flow_interpolation.py on the device.  A flow field has its own stream and buffers.
   nl_flow_create      : ndim 2 or 3, spacing ((Z,) Y, X in um) and the search radius r in um (max(max_distance_um * dt, 0.5)).
   nl_flow_load        : the rows of one time point and direction, float64: check coordinates (n, ndim) in voxels (the row's
                         position, forward; position + vector, backward), vectors (n, ndim) and costs (n).  They replace the
                         rows loaded before, are binned into a grid of cells of edge r and stay on the device.  n may be 0.
   nl_flow_interpolate : n query rows (n, ndim) float64 in voxels -> out (n, ndim) float64.  Neighbours of a query are the rows
                         with sum_axes (q*s - c*s)^2 <= r*r; a row without one (a NaN row included) is NaN.  n_found = the number
                         of rows that found a neighbour.  Inputs of any length: the library runs them in chunks.
   nl_flow_interpolate_dev : the same for n query rows and an output that are already on the field's device (device pointers),
                         in one launch: nothing crosses the host.  The caller's work on the queries must be complete.  With
                         no rows loaded nothing is written and n_found = 0.
   nl_flow_kernel_ms   : device time of the kernels of the last nl_flow_interpolate(_dev) call, transfers excluded.
   nl_flow_grid_info   : the plan of the loaded rows, read back from the device: dims[3] (a 2-D field has a leading axis of one
                         cell), the number of cells, the cell edge per axis in um (edge[3]; 0 where the plan resolves nothing), the
                         cell budget the plan was given and the number of rows in the fullest cell.  All 0 with no rows loaded.
                         Changes nothing. */
typedef struct nl_flow nl_flow;
int nl_flow_create(nl_flow **out, int device, int ndim, const double *spacing, double r, char *err, size_t errlen);
int nl_flow_destroy(nl_flow *field);
int nl_flow_load(nl_flow *field, const double *coords, const double *vectors, const double *costs, int64_t n, char *err, size_t errlen);
int nl_flow_interpolate(nl_flow *field, const double *queries, int64_t n, double *out, int64_t *n_found, char *err, size_t errlen);
int nl_flow_interpolate_dev(nl_flow *field, const double *d_queries, int64_t n, double *d_out, int64_t *n_found, char *err, size_t errlen);
int nl_flow_kernel_ms(nl_flow *field, float *ms, char *err, size_t errlen);
int nl_flow_grid_info(nl_flow *field, int *dims, int64_t *ncell, double *edge, int64_t *max_cells, int64_t *fullest, char *err, size_t errlen);

/* ------------------------------------------------------------------ voxel reassignment -------- */
/* nellie/tracking/voxel_reassignment.py on the device.  A reassigner has its own stream and buffers and
   keeps the last two frames of a label stack: union mask (1 bit / voxel), labelled voxels in raster order, their labels and
   their reassigned labels.
   nl_reassign_create  : ndim 2 or 3 (nz = 1 for 2), the frame's shape, spacing ((Z,) Y, X in um) and the radius r in um.
   nl_reassign_frame   : the next frame: branch and object labels (int32, frame shape).  The frame loaded before becomes
                         "prev".  seed != 0: the frame's reassigned labels are its labels (frame 0).  n_vox = labelled voxels.
   nl_reassign_pair    : matches the last two frames.  fw: a flow field with the forward rows of t loaded, bw: one with the
                         backward rows of t + 1; NULL gives no candidates of that direction.  The predicted centroids never
                         leave the device (nl_flow_interpolate_dev).  Writes the reassigned labels of the later frame.
                         n_candidates = 0: no candidate at all, the later frame stays unassigned.
   nl_reassign_fetch   : which = 0 the last frame, 1 the one before: linear voxel indices (n_vox, raster order), reassigned
                         branch / object labels per labelled voxel, and (which = 0, after a pair with candidates) per voxel the
                         rank of the best pair's source among the voxels of the frame before, -1 without a candidate.
                         NULL pointers are skipped.
   nl_reassign_kernel_ms : device time of the last nl_reassign_pair, its flow interpolation included, transfers excluded. */
typedef struct nl_reassign nl_reassign;
int nl_reassign_create(nl_reassign **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, double r,
                       char *err, size_t errlen);
int nl_reassign_destroy(nl_reassign *reassigner);
int nl_reassign_frame(nl_reassign *reassigner, const int32_t *branch, const int32_t *obj, int seed, int64_t *n_vox, char *err, size_t errlen);
int nl_reassign_pair(nl_reassign *reassigner, nl_flow *fw, nl_flow *bw, int64_t *n_candidates, char *err, size_t errlen);
int nl_reassign_fetch(nl_reassign *reassigner, int which, int64_t *vox, int32_t *re_branch, int32_t *re_obj, int32_t *best_src,
                      char *err, size_t errlen);
int nl_reassign_kernel_ms(nl_reassign *reassigner, float *ms, char *err, size_t errlen);

/* ------------------------------------------------------------------ voxel tracks of a label stack -------- */
/* LabelTracks of nellie/tracking/all_tracks_for_label.py on the device.  A track set has its own stream
   and buffers: `mask_slots` frame masks (labels > 0, 1 bit / voxel) that the caller keeps resident and replaces as it sees fit,
   the seeds, the coordinates of a run and its rows [id, frame, (z,) y, x] (float64).  The coordinates never cross the host; the
   surviving rows come down once.  A run is seed, begin, the backward steps, the forward steps, one filter call per frame with
   rows, finish, fetch.
   nl_tracks_create  : ndim 2 or 3 (nz = 1 for 2), the frame's shape and the number of mask slots.
   nl_tracks_mask    : the labels > 0 mask of a frame (int32, frame shape) into a slot.
   nl_tracks_seed    : the seeds: every skip-th voxel in raster order of the slot's mask (use_label = 0) or of labels == label.
                       labels != NULL: the start frame, uploaded for this call only; it also builds the slot's mask.  Seeding by
                       label needs it.  n_seeds = their number.
   nl_tracks_begin   : sizes the run's buffers before any work: n_seeds * (steps + 1) rows per direction (0 steps: the direction
                       does not run).  Ids are id0 + the seed's index.  NL_ENOMEM when that does not fit.
   nl_tracks_step    : one frame of a direction.  flow: a field with the direction's rows of frame_from loaded, NULL when there
                       are none.  When no coordinate finds a row nothing changes and n_rows = 0.  Otherwise a coordinate whose
                       vector row is all NaN is NaN from here on, every other one moves by + vector (backward: - vector) and emits
                       [id, frame_to, coord].  first != 0: the direction's first frame -- the coordinates start from the seeds and
                       a kept one emits [id, frame_from, old coord] before its new row.  Backward steps come first.
   nl_tracks_filter  : for the rows of one frame: a row stays if its coordinates, rounded half to even, lie inside the frame on a
                       set bit of the mask in `slot` (slot < 0: the frame is outside the stack, its rows go); a NaN or infinite
                       coordinate goes.  Also orders the backward rows: by id, within an id by ascending frame.
   nl_tracks_finish  : one scan and one compaction.  n_rows = rows that stay: the backward ones, then the forward ones as emitted.
   nl_tracks_fetch   : those rows, (n_rows, 2 + ndim) float64.
   nl_tracks_kernel_ms : device time of the kernels since the last nl_tracks_seed: ms[0] masks, [1] seeding, [2] flow
                       interpolation, [3] steps, [4] filter and order, [5] scan and compaction.  Transfers excluded. */
typedef struct nl_tracks nl_tracks;
int nl_tracks_create(nl_tracks **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, int mask_slots, char *err, size_t errlen);
int nl_tracks_destroy(nl_tracks *tracks);
int nl_tracks_mask(nl_tracks *tracks, int slot, const int32_t *labels, char *err, size_t errlen);
int nl_tracks_seed(nl_tracks *tracks, int slot, const int32_t *labels, int use_label, int32_t label, int skip, int64_t *n_seeds,
                   char *err, size_t errlen);
int nl_tracks_begin(nl_tracks *tracks, int64_t fw_steps, int64_t bw_steps, int64_t id0, char *err, size_t errlen);
int nl_tracks_step(nl_tracks *tracks, nl_flow *flow, int backward, int first, int64_t frame_from, int64_t frame_to, int64_t *n_rows,
                   char *err, size_t errlen);
int nl_tracks_filter(nl_tracks *tracks, int64_t frame, int slot, char *err, size_t errlen);
int nl_tracks_finish(nl_tracks *tracks, int64_t *n_rows, char *err, size_t errlen);
int nl_tracks_fetch(nl_tracks *tracks, double *rows, char *err, size_t errlen);
int nl_tracks_kernel_ms(nl_tracks *tracks, float *ms, char *err, size_t errlen);

/* ------------------------------------------------------------------ the analysis overlay -------- */
/* The overlay of nellie_napari/nellie_analysis.py on the device: a column of a feature table painted onto
   the labelled voxels of a frame.  An overlay object is made for one frame shape and has its own stream and buffers; the state of
   the loaded frame (mask, rows, groups) stays until the next load, so another column costs one small upload and the paint.
   nl_overlay_create : ndim 2 or 3 (nz = 1 for 2) and the frame's shape.
   nl_overlay_load   : the label frame (int32, frame shape).  Its voxels with label > 0, in raster order, are the rows; n_rows = V.
   nl_overlay_groups : the rows' groups.  group != NULL: one per row (V ints, -1: none).  Else a CSR: offsets (V + 1 entries from 0,
                       not decreasing, ending at n_idx) and idx (n_idx group indices, in any order, repeats allowed).  A group
                       index is 0 .. 2^31 - 2.
   nl_overlay_values : direct = 0: attr is the column by group index, n_attr entries, more than the largest group index.  A row's
                       value is the mean of attr[g] over its distinct groups g with attr[g] not NaN, NaN without one.  The sum is
                       np.sum's over the dense float64 column of n_attr entries, +0.0 where the row has no group or attr is NaN:
                       pairwise = 0: from +0.0, one add per entry in ascending g; else numpy's pairwise trees over pieces of 8192
                       entries, added in order.  direct != 0: attr holds the rows' values themselves, n_attr = V.
   nl_overlay_paint  : the dense frame, one streaming pass.  kind 0: float64, the row's value at a labelled voxel, NaN elsewhere;
                       1: float32, the value rounded once; 2: uint64 labels, the truncated value, 0 where it is NaN, negative,
                       infinite or 2^64 and above, 0 elsewhere.
   nl_overlay_fetch_values : the V values, float64.
   nl_overlay_fetch_frame  : the painted frame in the element type of its kind.
   nl_overlay_kernel_ms    : device time of the kernels of the last load (ms[0]), values (ms[1]) and paint (ms[2]) call. */
typedef struct nl_overlay nl_overlay;
int nl_overlay_create(nl_overlay **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, char *err, size_t errlen);
int nl_overlay_destroy(nl_overlay *overlay);
int nl_overlay_load(nl_overlay *overlay, const int32_t *labels, int64_t *n_rows, char *err, size_t errlen);
int nl_overlay_groups(nl_overlay *overlay, const int32_t *group, const int64_t *offsets, const int32_t *idx, int64_t n_idx, char *err,
                      size_t errlen);
int nl_overlay_values(nl_overlay *overlay, const double *attr, int64_t n_attr, int direct, int pairwise, char *err, size_t errlen);
int nl_overlay_paint(nl_overlay *overlay, int kind, char *err, size_t errlen);
int nl_overlay_fetch_values(nl_overlay *overlay, double *values, char *err, size_t errlen);
int nl_overlay_fetch_frame(nl_overlay *overlay, void *frame, char *err, size_t errlen);
int nl_overlay_kernel_ms(nl_overlay *overlay, float *ms, char *err, size_t errlen);

/* ------------------------------------------------------------------ voxel-level features -------- */
/* Voxels of nellie/feature_extraction/hierarchical.py on the device.  The object has its own stream and
   buffers and keeps one frame: mask (1 bit / voxel), the labelled voxels in raster order and their values.
   nl_voxfeat_create   : ndim 2 or 3 (nz = 1 for 2), the frame's shape, spacing ((Z,) Y, X in um) and the time step dt in s.
   nl_voxfeat_frame    : component and branch labels (int32), intensity and structure frames in their own dtypes (the dtype codes of
                         nl_filter_load).  Lists the voxels with component > 0 and gathers their four values.  n_vox = their number.
   nl_voxfeat_fetch_voxels : linear voxel indices (n_vox, raster order), the two labels, intensity and structure values (n_vox
                         elements of the uploaded dtypes).  NULL pointers are skipped.
   nl_voxfeat_motility : bw: a flow field with the backward rows of the frame's time point loaded (vec01), fw: one with its
                         forward rows (vec12); NULL: the direction does not exist.  The flow is interpolated at every voxel on
                         the device (nl_flow_interpolate_dev); a direction without a field, rows or any neighbour is all NaN.
                         Then the pivot voxel of every branch label and direction (smallest |vec|, lowest index on a tie) and the
                         motility features in float64.  n_found_*: voxels with a flow neighbour.
   nl_voxfeat_fetch_motility : out = 13 host pointers (NULL ones skipped), float32: vec01 (n, D), vec12 (n, D), linear_vel_vector
                         (n, D), linear_vel, angular_vel_vector ((n) in 2-D, (n, 3) in 3-D), angular_vel, linear_acc,
                         angular_acc, rel_linear_vel, rel_angular_vel, rel_linear_acc, rel_angular_acc, rel_directionality.
   nl_voxfeat_nodes    : pixel_class (any dtype code) and distance (float32 or float64) frames.  Nodes are the voxels with pixel
                         class > 0 in raster order; a node's box is trunc(radius * -+1 + index) per axis, upper limit + 1, clamped
                         to [0, size]; a voxel belongs to the node when every coordinate is within the limits, ends included.
   nl_voxfeat_fetch_nodes : the limits per axis (n_nodes, 2) int64 (lims2 in 3-D only) and both lists as CSR of int32 ranks:
                         node_start (n_nodes) / node_val (n_pairs): the voxels of every node, ascending; vox_start (n_vox) /
                         vox_val (n_pairs): the nodes of every voxel, ascending.  The last list ends at n_pairs.
   nl_voxfeat_kernel_ms : ms[5], device time since the last nl_voxfeat_frame: frame load and compaction, flow interpolation,
                         pivots, motility, node assignment.  Transfers excluded. */
typedef struct nl_voxfeat nl_voxfeat;
int nl_voxfeat_create(nl_voxfeat **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, double dt,
                      char *err, size_t errlen);
int nl_voxfeat_destroy(nl_voxfeat *voxfeat);
int nl_voxfeat_frame(nl_voxfeat *voxfeat, const int32_t *comp, const int32_t *branch, const void *raw, int raw_dtype, const void *structure,
                     int struct_dtype, int64_t *n_vox, char *err, size_t errlen);
int nl_voxfeat_fetch_voxels(nl_voxfeat *voxfeat, int64_t *vox, int32_t *comp, int32_t *branch, void *raw, void *structure, char *err, size_t errlen);
int nl_voxfeat_motility(nl_voxfeat *voxfeat, nl_flow *bw, nl_flow *fw, int64_t *n_found_bw, int64_t *n_found_fw, char *err, size_t errlen);
int nl_voxfeat_fetch_motility(nl_voxfeat *voxfeat, float *const *out, char *err, size_t errlen);
int nl_voxfeat_nodes(nl_voxfeat *voxfeat, const void *pixel_class, int class_dtype, const void *distance, int dist_dtype, int64_t *n_nodes,
                     int64_t *n_pairs, char *err, size_t errlen);
int nl_voxfeat_fetch_nodes(nl_voxfeat *voxfeat, int64_t *lims0, int64_t *lims1, int64_t *lims2, int32_t *node_start, int32_t *node_val,
                           int32_t *vox_start, int32_t *vox_val, char *err, size_t errlen);
int nl_voxfeat_kernel_ms(nl_voxfeat *voxfeat, float *ms, char *err, size_t errlen);

/* ------------------------------------------------------------------ node-level features -------- */
/* Nodes and aggregate_stats_for_class of nellie/feature_extraction/hierarchical.py on the device.  The
   object has its own stream and buffers.  It keeps one frame's node list and border mask (1 bit / voxel), and one set of groups:
   lists of indices into value arrays, over which any number of value arrays are aggregated.  Every sum is numpy's sum of a row
   padded to L, the longest group of the set: the row in blocks of 8192 elements (numpy's ufunc buffer) added in order from 0.0,
   each block summed pairwise.
   nl_nodefeat_create  : ndim 2 or 3 (nz = 1 for 2), the frame's shape and spacing ((Z,) Y, X in um).  An object that only
                         aggregates may have any shape.
   nl_nodefeat_frame   : pixel class, component labels, branch labels and border mask, each in its own dtype (the dtype codes of
                         nl_filter_load).  Nodes are the voxels with pixel class > 0 in raster order; their labels are gathered;
                         their thickness is 2 * the distance in um to the nearest voxel with border != 0 (per axis node * s -
                         border * s, squares added in axis order, sqrt of the minimum), NaN without a border voxel.
   nl_nodefeat_fetch   : coordinates (n_nodes, D) int64, the two labels (n_nodes elements of the uploaded dtypes), thickness
                         (n_nodes float64).  NULL pointers are skipped.
   nl_nodefeat_groups  : group j = idx[offsets[j] .. offsets[j + 1]), in the order given, neither sorted nor disjoint; offsets has
                         n_groups + 1 entries from 0.  At most 2^31 - 1 indices in all.  longest = L.
   nl_nodefeat_set_wide_from : from the next nl_nodefeat_groups on, groups of at least wide_from values are summed one block of
                         8192 elements per wave and the blocks' sums added in order, the others one group
                         per wave; 0 = never.  The results are the same bits either way; the default is a measured choice.
   nl_nodefeat_aggregate : values (float32, float64 or integers of at most 32 bits; n_values above every index) as float64.
                         out (5, n_groups) float64 = mean, std_dev, min, max, sum: nanmean, nanstd, nanmin, nanmax and nansum of
                         the rows of the groups' matrix padded with NaN to L columns.  A group without a number: NaN, sum 0.
   nl_nodefeat_node_stats : the groups are the nodes' voxel lists (n_groups = n_nodes): indices into coords (n_vox, D) int64 and
                         vec01 / vec12 (n_vox, D) float32, NULL = all NaN.  out (6, n_nodes) float64 = z, y, x (mean voxel
                         coordinate * spacing, z NaN in 2-D), divergence, convergence, vergere; NaN for a node without voxels.
   nl_nodefeat_kernel_ms : ms[4], device time: node list and labels, border mask and thickness, node statistics (since the last
                         nl_nodefeat_frame), aggregation (since the last nl_nodefeat_groups).  Transfers excluded. */
typedef struct nl_nodefeat nl_nodefeat;
int nl_nodefeat_create(nl_nodefeat **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, char *err,
                       size_t errlen);
int nl_nodefeat_destroy(nl_nodefeat *nodefeat);
int nl_nodefeat_frame(nl_nodefeat *nodefeat, const void *pixel_class, int class_dtype, const void *comp, int comp_dtype, const void *branch,
                      int branch_dtype, const void *border, int border_dtype, int64_t *n_nodes, char *err, size_t errlen);
int nl_nodefeat_fetch(nl_nodefeat *nodefeat, int64_t *coords, void *comp, void *branch, double *thickness, char *err, size_t errlen);
int nl_nodefeat_groups(nl_nodefeat *nodefeat, const int64_t *offsets, const int64_t *idx, int64_t n_groups, int64_t *longest, char *err,
                       size_t errlen);
int nl_nodefeat_set_wide_from(nl_nodefeat *nodefeat, int64_t wide_from, char *err, size_t errlen);
int nl_nodefeat_aggregate(nl_nodefeat *nodefeat, const void *values, int dtype, int64_t n_values, double *out, char *err, size_t errlen);
int nl_nodefeat_node_stats(nl_nodefeat *nodefeat, const int64_t *coords, const float *vec01, const float *vec12, int64_t n_vox, double *out,
                           char *err, size_t errlen);
int nl_nodefeat_kernel_ms(nl_nodefeat *nodefeat, float *ms, char *err, size_t errlen);

/* ------------------------------------------------------------------ branch-level features -------- */
/* Branches of nellie/feature_extraction/hierarchical.py: everything of the branch level that touches voxels.  The object has its own
   stream and buffers.  It keeps one frame's skeleton list (the voxels with skeleton label > 0, in raster order) with what is known
   per skeleton voxel and per skeleton label, and one frame's regions (the distinct labels > 0 of the full branch-label volume) with
   their sums.  Per-label arrays have one row per label present, ascending, whatever the label values (at most 2^31 - 2).
   nl_branchfeat_create  : ndim 2 or 3 (nz = 1 for 2), the frame's shape and spacing ((Z,) Y, X in um).
   nl_branchfeat_frame   : skeleton labels (an integer dtype), component labels and border mask, each in its own dtype (the dtype
                         codes of nl_filter_load).  Counts the skeleton voxels, their distinct labels, the tips (degree 1) and the
                         lone tips (degree 0).
   nl_branchfeat_fetch   : per skeleton voxel: coordinates (n, D) int64, labels (n) int64, degree (n) uint8 = the neighbours (26 or 8)
                         inside the frame with the same label, radius (n) float64 = the distance in um to the nearest voxel with
                         border != 0 (as nl_nodefeat_frame measures it), NaN without one; tips (n_tips) and lone (n_lone) int64:
                         positions in the list, ascending.  Per label: branch_label (B) int64; comp (B elements of the uploaded
                         dtype) = the component label at the label's first voxel; edges (B, 13 or 4) uint32 = same-label pairs per
                         offset whose first non-zero component is +1, offsets in the order dz, dy, dx each over -1, 0, 1; count (B)
                         int32 = its voxels; median (B) float64 = np.median of 2 * radius over them.  NULL pointers are skipped.
   nl_branchfeat_regions : the branch-label volume (an integer dtype; every extent at most 2^15) and, or NULL, the reassigned labels
                         (an integer dtype, values in [0, 2^31)).
   nl_branchfeat_regions_rows : nl_branchfeat_regions with the sums taken per run of equal labels along X (closed forms, one set
                         of atomics per run) instead of per voxel: the same regions, sums and mode, bit for bit.  Neither call
                         needs nl_branchfeat_frame first.
   nl_branchfeat_fetch_regions : labels (R) int64 ascending; sums (F, R) int64 with F = 1 + 3 D + D (D + 1) / 2: the voxel count, per
                         axis the smallest coordinate, the largest, the sum of the coordinates, then the sums of the products
                         c_a * c_b for a <= b in row order, all exact; mode (R) int64 = the most frequent reassigned label over the
                         region, the smallest among equals, -1 when none were given.
   nl_branchfeat_kernel_ms : ms[5], device time: skeleton list and labels, degree and edge counts, border mask and radii, per-label
                         lists with medians and tips (since the last nl_branchfeat_frame), regions (since the last
                         nl_branchfeat_regions).  Transfers excluded.
   nl_branchfeat_convex  : the convex counts of the loaded regions: per region the number of lattice points in the closed convex hull
                         of its voxels' diamonds (every voxel centre moved by +-1/2 along every axis), which is skimage's
                         area_convex / pixel volume; 0 for a 3-D region whose voxel centres lie in one plane (skimage's all-zero
                         convex image).  Works on the label frame that the last nl_branchfeat_regions / _regions_rows call left
                         on the device, so it follows that call directly (NL_ESTATE after nl_branchfeat_frame).  Exact integers:
                         coordinates are below 2^15, doubled box-relative differences below 2^17, facet normals below 2^35 per
                         component and N . p below 2^54, so int64 holds everything.  The hulls are built on the host.
   nl_branchfeat_fetch_convex : count (R) int64; facets (R) int64 = facets of every region's hull; rows (R) int64 = rows (z, y) of its
                         bounding box.  NULL pointers are skipped.
   nl_branchfeat_convex_ms : ms[4] of the last nl_branchfeat_convex: device time of the row extremes, the per-plane hulls and the
                         count (transfers excluded), then the host time of the hulls.
   nl_branchfeat_convex_limits : limits[3]: box rows per workgroup of the count kernel, facets per staging chunk, workgroups per
                         launch.
   nl_host_convex_facets : host only: the hull's facets (k, 4) int64 = (N_z, N_y, N_x, d), N . p <= d inside in doubled coordinates
                         (voxel c -> 2 c), of n voxels coords (n, ndim) int64 in [0, 2^15); k = 0 for a 3-D set of affine rank
                         < 3.  Writes at most cap facets; *n_facets = k. */
typedef struct nl_branchfeat nl_branchfeat;
int nl_branchfeat_create(nl_branchfeat **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, char *err,
                         size_t errlen);
int nl_branchfeat_destroy(nl_branchfeat *branchfeat);
int nl_branchfeat_frame(nl_branchfeat *branchfeat, const void *skel, int skel_dtype, const void *comp, int comp_dtype, const void *border,
                        int border_dtype, int64_t *n_voxels, int64_t *n_labels, int64_t *n_tips, int64_t *n_lone, char *err, size_t errlen);
int nl_branchfeat_fetch(nl_branchfeat *branchfeat, int64_t *coords, int64_t *labels, uint8_t *degree, double *radius, int64_t *tips, int64_t *lone,
                        int64_t *branch_label, void *comp, uint32_t *edges, int32_t *count, double *median, char *err, size_t errlen);
int nl_branchfeat_regions(nl_branchfeat *branchfeat, const void *labels, int dtype, const void *reassigned, int reassigned_dtype,
                          int64_t *n_regions, char *err, size_t errlen);
int nl_branchfeat_regions_rows(nl_branchfeat *branchfeat, const void *labels, int dtype, const void *reassigned, int reassigned_dtype,
                               int64_t *n_regions, char *err, size_t errlen);
int nl_branchfeat_fetch_regions(nl_branchfeat *branchfeat, int64_t *labels, int64_t *sums, int64_t *mode, char *err, size_t errlen);
int nl_branchfeat_kernel_ms(nl_branchfeat *branchfeat, float *ms, char *err, size_t errlen);
int nl_branchfeat_convex(nl_branchfeat *branchfeat, char *err, size_t errlen);
int nl_branchfeat_fetch_convex(nl_branchfeat *branchfeat, int64_t *count, int64_t *facets, int64_t *rows, char *err, size_t errlen);
int nl_branchfeat_convex_ms(nl_branchfeat *branchfeat, float *ms, char *err, size_t errlen);
int nl_branchfeat_convex_limits(int64_t *limits, char *err, size_t errlen);
int nl_host_convex_facets(const int64_t *coords, int64_t n, int ndim, int64_t *facets, int64_t cap, int64_t *n_facets, char *err, size_t errlen);

/* ------------------------------------------------------------------ adjacency maps -------- */
/* The edge lists of Hierarchy._save_adjacency_maps (nellie/feature_extraction/hierarchical.py): every list is (m, 2) int64 rows
   (row, column), ascending in the row.  The object has its own stream and buffers and no frame shape.  An operation computes its
   rows on the device and reports their number; nl_adjacency_fetch downloads the rows of the last operation.
   nl_adjacency_pairs  : labels (n elements, NL_I32 or NL_I64) -> (i, labels[i] - bias) for every i with labels[i] > 0.
   nl_adjacency_expand : the CSR of one list of values per row (offsets: n_rows + 1 entries that start at 0, do not decrease and end
                         at the number of values; otherwise NL_EINVAL before any launch) -> (row, value), the values of a row in
                         their order.
   nl_adjacency_lookup : (i, j) with j the last position of child[i] in parent (p labels), for every child that occurs there.  A
                         child above the largest parent label is NL_EINVAL, the message naming its row and label (found by the
                         kernel, read by the host afterwards; the object stays usable); so is a negative label on either side
                         (checked on the host).  No parents: no rows.  Labels are at most 2^31 - 2.
   nl_adjacency_fetch  : out (n_edges, 2) int64 of the last operation (NL_ESTATE without one).
   nl_adjacency_kernel_ms : ms[3], device time of the last call of pairs, expand and lookup.  Transfers excluded.
   At most 2^31 - 1 edges per list. */
typedef struct nl_adjacency nl_adjacency;
int nl_adjacency_create(nl_adjacency **out, int device, char *err, size_t errlen);
int nl_adjacency_destroy(nl_adjacency *adjacency);
int nl_adjacency_pairs(nl_adjacency *adjacency, const void *labels, int dtype, int64_t n, int64_t bias, int64_t *n_edges, char *err, size_t errlen);
int nl_adjacency_expand(nl_adjacency *adjacency, const int64_t *offsets, const int64_t *values, int64_t n_rows, int64_t *n_edges, char *err,
                        size_t errlen);
int nl_adjacency_lookup(nl_adjacency *adjacency, const int64_t *child, int64_t n, const int64_t *parent, int64_t p, int64_t *n_edges, char *err,
                        size_t errlen);
int nl_adjacency_fetch(nl_adjacency *adjacency, int64_t *out, char *err, size_t errlen);
int nl_adjacency_kernel_ms(nl_adjacency *adjacency, float *ms, char *err, size_t errlen);

/* ------------------------------------------------------------------ label transitions -------- */
/* Label transition counts from voxel matches: for a frame pair, every match row (a voxel of frame t, a voxel
   of frame t + 1) is turned into the pair of labels found there, and the distinct pairs are counted.  A transitions object is made
   for one frame shape and has its own stream and buffers; two label frames stay on the device.
   nl_trans_create  : ndim 2 or 3 (nz = 1 for 2) and the frame's shape.
   nl_trans_frame   : the next label frame (NL_I32 or NL_I64, frame shape): the resident "next" frame becomes "prev", this one "next".
   nl_trans_begin   : begins a pair with a cleared table of `slots` slots (a power of two).  Needs two frames.
   nl_trans_count   : rows row0 .. row0 + n of the pair: prev, next (n, ndim) coordinates of NL_U16, NL_U32 or NL_U64.  Any number of
                      calls, rows ascending; all count into the same table.  A coordinate outside the frame is NL_EINVAL naming the
                      lowest such row (found by the kernel; the object stays usable).  *overflow: the table is too small.
   nl_trans_finish  : ends the pair.  A gathered label below 0 or above 2^31 - 1 is NL_EINVAL naming the lowest such row.  *overflow:
                      repeat the pair with more slots.  Else *n_entries distinct pairs, *n_dropped rows with a label of 0 at either
                      end, *n_heads runs of equal neighbouring rows that touched the table (one atomic add each).
   nl_trans_fetch   : out (n_entries, 2) uint64: (prev label << 32 | next label, count), in no particular order.
   nl_trans_label_max : the largest label of the "next" frame.
   nl_trans_relabel : the "next" frame through lut (n_lut int32): label b in (0, n_lut) becomes lut[b], everything else 0.
   nl_trans_fetch_frame : that frame, int32.
   nl_trans_kernel_ms   : ms[4], device time of the clear, the count launches and the compaction of the last pair, and of the last
                          relabel.  Transfers excluded, except that the compaction's figure spans the scan's one-word round trip
                          to the host between its kernels.
   At most 2^31 rows per nl_trans_count, 2^34 slots, 2^31 - 1 distinct pairs. */
typedef struct nl_trans nl_trans;
int nl_trans_create(nl_trans **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, char *err, size_t errlen);
int nl_trans_destroy(nl_trans *trans);
int nl_trans_frame(nl_trans *trans, const void *labels, int dtype, char *err, size_t errlen);
int nl_trans_begin(nl_trans *trans, int64_t slots, char *err, size_t errlen);
int nl_trans_count(nl_trans *trans, const void *prev, const void *next, int coord_dtype, int64_t n, int64_t row0, int *overflow, char *err,
                   size_t errlen);
int nl_trans_finish(nl_trans *trans, int64_t *n_entries, int64_t *n_dropped, int64_t *n_heads, int *overflow, char *err, size_t errlen);
int nl_trans_fetch(nl_trans *trans, uint64_t *out, char *err, size_t errlen);
int nl_trans_label_max(nl_trans *trans, int64_t *top, char *err, size_t errlen);
int nl_trans_relabel(nl_trans *trans, const int32_t *lut, int64_t n_lut, char *err, size_t errlen);
int nl_trans_fetch_frame(nl_trans *trans, int32_t *frame, char *err, size_t errlen);
int nl_trans_kernel_ms(nl_trans *trans, float *ms, char *err, size_t errlen);

/* ------------------------------------------------------------------ test hooks -------- */
/* Known-answer hook for the fused device routine (filtering.py:581-585 + 744-766): for n explicit
   Hessians h6[n][6] = (hxx,hxy,hxz,hyy,hyz,hzz) writes out4[n][4] = (l1,l2,l3 sorted by |.|, Frangi
   response).  impl 0 = production eigen-solve, 1 = libm acos/cos form. */
int nl_debug_eig_frangi(nl_ctx *ctx, const float *h6, int64_t n, int impl, float alpha_sq, float beta_sq,
                        float gamma_sq, float *out4, char *err, size_t errlen);

/* Introspection: "fast_div" (2 / 1 when the 2- / 3-instruction constant division was proven exact for the
   current spacings, 0: the float64 form), "hessian_tile_rows", "device_bytes", "gauss_yx_max_r" (largest in-plane
   radius whose Y and X passes share a kernel: see nl_gauss_step_ahead), "last_label_path" (what nl_label_run's last frame
   took: 0 the run-level labelling, 1 the voxel-level kernels because a row exceeds 65535 voxels, 2 the voxel-level kernels
   after a run set exceeded the scratch capacity of n / 2 runs, 3 the voxel-level kernels forced by NELLIE_LABEL_VOXEL). */
int nl_ctx_info(nl_ctx *ctx, const char *key, double *value);

/* ------------------------------------------------------------------ timing ------------ */
/* HIP-event timing on the context stream (bench.py's roofline figures). */
int nl_timer_begin(nl_ctx *ctx, char *err, size_t errlen);
int nl_timer_end_ms(nl_ctx *ctx, float *ms, char *err, size_t errlen);
/* accumulated HIP-event time and launch count of one named kernel group since the last
   reset; names: "gauss", "hessian_stats", "vesselness", "sample", "finish", "mask_volume", "label" */
int nl_prof_enable(nl_ctx *ctx, int on);
int nl_prof_get(nl_ctx *ctx, const char *name, double *ms, int64_t *launches);
int nl_prof_reset(nl_ctx *ctx);

/* ---- Markers stage (nellie/segmentation/mocap_marking.py:648-703, use_im = 'distance', 3-D volumes) -----------------
   The stage after Label: distance transform of the labelled objects, their border shell, multi-scale LoG peaks of
   the distance image, intensity-based non-maximum suppression.  All three products are bit-exact.
   nl_markers_begin : mask = labels > 0 (mocap_marking.py:658-659); labels = NULL uses the labels nl_label_run left on
                      the device, intensity = NULL the resident input of nl_input_load (any dtype, cast to float32 as
                      `score_img[...] = intensity_im[...]` does, :595-596).
   nl_markers_distance : border = binary_dilation(mask) ^ mask; distance = float32(distance_transform_edt(mask)) clamped
                      at `clamp` = float32(2 * max_radius_px) (:440-448).  Exact: only background within floor(clamp)
                      voxels can matter.  n_mask (may be NULL) = object voxels.
   nl_markers_log_step : one sigma of :488-508 -- response = float32(-gaussian_laplace(distance, (s/z_ratio, s, s)) * s^2)
                      clamped at 0; a valid voxel (mask & distance > 0) whose response equals the maximum of its 3x3x3
                      neighbourhood (mode 'nearest') and beats every earlier scale becomes a peak.  Weights: scipy's
                      `_gaussian_kernel1d` of order 2 / 0, truncate 4.0, 2r+1 float64 values each, s2 = float32(s**2).
                      Radii 1 ... 63 on every axis (a 0.065 um pixel gives 21); in-plane radii above 12, or above ny, take
                      one-thread-per-voxel passes with scipy's multiple reflection (one more float32 volume, allocated then).
                      2-D image (context of shape (1, ny, nx)): wz2 = wz0 = NULL, sigma_vec = (s, s) (:323-324) -- the two
                      in-plane terms only; distance transform, border, 3x3 maxima and the suppression window are the
                      nz = 1 cases of the 3-D kernels.
   nl_markers_finish : :569-606 -- a peak survives if its float32 intensity is positive and equals the maximum over the
                      peaks within +-peak_min_distance.
   nl_markers_store  : marker (uint8 0/1), distance (float32), border (uint8 0/1); NULL pointers are skipped. */
int nl_markers_begin(nl_ctx *ctx, const int32_t *labels_host, const void *intensity_host, int dtype, char *err, size_t errlen);
int nl_markers_distance(nl_ctx *ctx, float clamp, int64_t *n_mask, char *err, size_t errlen);
/* use_im = 'frangi' (mocap_marking.py:675-679): the LoG of nl_markers_log_step runs on this float32 image (whole
   volume, host) instead of the distance image; NULL switches back.  Call between nl_markers_begin and the first step. */
int nl_markers_use_image(nl_ctx *ctx, const float *image, char *err, size_t errlen);
int nl_markers_log_step(nl_ctx *ctx, const double *wz2, const double *wz0, int rz, const double *wy2, const double *wy0,
                        const double *wx2, const double *wx0, int ryx, float s2, char *err, size_t errlen);
int nl_markers_finish(nl_ctx *ctx, int peak_min_distance, int64_t *n_markers, char *err, size_t errlen);
int nl_markers_store(nl_ctx *ctx, uint8_t *marker, float *distance, uint8_t *border, char *err, size_t errlen);

/* ---- Network stage, the two dense per-voxel steps (nellie/segmentation/networking.py; 3-D volumes and 2-D images) ----
   The skeletonisation itself (skimage, networking.py:394-409) is the last block of this file (3-D) or the caller's (2-D); the rest of
   the stage is the next block.
   nl_skel_pixel_class  : `_get_pixel_class_impl` (networking.py:672-683) -- skel_mask = skel > 0;
                          class = min(4, convolve(skel_mask, ones(3,3,3), mode="constant", cval=0)) * skel_mask, uint8:
                          1 isolated, 2 tip, 3 edge, 4 junction.  n_skel (may be NULL) = skeleton voxels.
   nl_skel_branch_labels: `_get_branch_skel_labels` (networking.py:758-800) -- label((pc > 0) & (pc != 4),
                          structure = ones(3,3,3)): int32 ids 1..K in raster order of each component's first voxel.
                          pixel_class = NULL uses the classes the previous nl_skel_pixel_class left on the device.
   A context of shape (1, ny, nx) gives the reference's 2-D branch (ones(3,3)). */
int nl_skel_pixel_class(nl_ctx *ctx, const int32_t *skel, uint8_t *pixel_class, int64_t *n_skel, char *err, size_t errlen);
int nl_skel_branch_labels(nl_ctx *ctx, const uint8_t *pixel_class, int32_t *labels, int64_t *n_labels, char *err, size_t errlen);

/* ---- Network stage behind the thinning (networking.py:828-851), one frame resident on the context from upload to download ----
   Whole volumes of fewer than 2^31 voxels; ndim = 2 needs a context of shape (1, ny, nx).  Labels are int32 and not negative.
   nl_network_load       : labels, the thinning's mask (uint8, non-zero = skeleton voxel) and the Frangi frame (float32) go up;
                           skel = labels * mask (networking.py:408).  max_label (may be NULL) = the largest label.
   nl_network_clean_seed : `_remove_connected_label_pixels_impl` (networking.py:261-296) -- a skeleton voxel whose 3x3x3 (2-D: 3x3)
                           neighbourhood, centre included, outside = background, holds two different labels is zeroed, voxels on a
                           face of the frame never; then `_add_missing_skeleton_labels` (networking.py:342-387) -- every label
                           without a skeleton voxel gets one at the maximum of the Frangi frame over its voxels.  Among equal
                           maxima the lowest raster index wins and NaN ranks above every number (the reference's pick follows no
                           rule there).  n_removed / n_seeded (may be NULL): voxels zeroed / labels seeded.
   nl_network_classes    : networking.py:839-847 -- the kernels of nl_skel_pixel_class and nl_skel_branch_labels on the resident
                           skeleton.  n_skel / n_branches may be NULL.
   nl_network_relabel_load: step 5 alone -- labels and branch labels (int32) go up, nl_network_relabel may follow.
   nl_network_relabel    : `_relabel_objects` (networking.py:485-577) -- per label L in its bounding box, every voxel of L takes the
                           branch label of the seed (branch > 0 and label == L) that scipy.ndimage.distance_transform_edt(~seeds,
                           sampling = spacing, return_indices = True) picks, ties included; objects without a seed and the
                           background stay 0.  spacing: ndim values.  scratch_voxels: box voxels one batch of objects may hold
                           (<= 0: half of the free HBM), never less than one frame; objects are not split.  n_objects (objects with a
                           seed), box_volume (the sum of their box volumes) and n_batches may be NULL.
   nl_network_fetch      : the branch skeleton labels (int32), the pixel classes (uint8) and the relabelled volume (uint32); each may
                           be NULL.
   nl_network_kernel_ms  : ms[4] = stream time of clean, seed, classes, relabel of the current frame, transfers excluded. */
int nl_network_load(nl_ctx *ctx, const int32_t *labels, const uint8_t *skel_mask, const float *frangi, int ndim, int64_t *max_label,
                    char *err, size_t errlen);
int nl_network_clean_seed(nl_ctx *ctx, int64_t *n_removed, int64_t *n_seeded, char *err, size_t errlen);
int nl_network_classes(nl_ctx *ctx, int64_t *n_skel, int64_t *n_branches, char *err, size_t errlen);
int nl_network_relabel_load(nl_ctx *ctx, const int32_t *labels, const int32_t *branch, int ndim, int64_t *max_label, char *err, size_t errlen);
int nl_network_relabel(nl_ctx *ctx, const double *spacing, int64_t scratch_voxels, int64_t *n_objects, int64_t *box_volume,
                       int64_t *n_batches, char *err, size_t errlen);
int nl_network_fetch(nl_ctx *ctx, int32_t *branch, uint8_t *pixel_class, uint32_t *relabelled, char *err, size_t errlen);
int nl_network_kernel_ms(nl_ctx *ctx, float *ms, char *err, size_t errlen);

/* ---- The 3-D thinning (skimage.morphology.skeletonize of a volume: Lee, Kashyap & Chu 1994; networking.py:394-409) ----
   Whole 3-D volumes of fewer than 2^31 voxels, axes (z, y, x), background outside the frame; ndim != 3 is refused (skimage thins 2-D
   images by another rule).  The result equals skimage 0.18.3's voxel for voxel, its quirks included: a frame of one plane runs the four
   in-plane directions only, and the sequential re-check is the component test alone (a solid 6 x 30 x 34 block thins to nothing).
   rounds_per_sync: rounds of the re-check launched between two read-backs of the counters (<= 0: the default, 8); it changes no result.
   nl_thin               : stand-alone -- mask (uint8, non-zero = foreground) up, skeleton (uint8, 0 / 1) down.  n_skel may be NULL.
   nl_network_load_thin  : nl_network_load with the mask thinned on the device from labels > 0: labels and the Frangi frame go up (8
                           bytes per voxel), no mask.  max_label / n_mask (the mask's voxels) may be NULL.
   nl_network_fetch_mask : the mask the last nl_network_load_thin or nl_thin left on the context (uint8, 0 / 1).
   nl_thin_info          : of that thinning, each may be NULL -- counts[7] = foreground voxels in, skeleton voxels out, outer iterations,
                           sub-iterations, rounds that had work, candidates, voxels removed; ms[1] = its time on the stream, the waits
                           for the counters included.
   nl_thin_decide_host   : the kernels' decision functions on the host (no context, no device): flags[i] = bit 0 endpoint, bit 1
                           Euler-invariant, bit 2 simple of the 27-bit neighbourhood nbhd[i], bit (dz+1)*9 + (dy+1)*3 + (dx+1). */
int nl_thin(nl_ctx *ctx, const uint8_t *mask, uint8_t *skel, int ndim, int rounds_per_sync, int64_t *n_skel, char *err, size_t errlen);
int nl_network_load_thin(nl_ctx *ctx, const int32_t *labels, const float *frangi, int ndim, int rounds_per_sync, int64_t *max_label,
                         int64_t *n_mask, char *err, size_t errlen);
int nl_network_fetch_mask(nl_ctx *ctx, uint8_t *skel_mask, char *err, size_t errlen);
int nl_thin_info(nl_ctx *ctx, int64_t *counts, float *ms, char *err, size_t errlen);
int nl_thin_decide_host(const uint32_t *nbhd, int64_t n, uint8_t *flags);

#ifdef __cplusplus
}
#endif
#endif /* NELLIE_AMD_H */
