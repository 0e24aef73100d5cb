// Translation unit of libnellie_hip.so (gfx950): the 3-D thinning in front of the Network stage (skimage.morphology.skeletonize of a
// volume, networking.py:394-409).  C-ABI in include/nellie_amd.h; kernels, decision functions and the algorithm in thin.inc.
// The thinning runs before anything else of a Network frame, so all of the context's volumes are free:
//   nw_mask  the working image, one byte per voxel; what is left of it is the skeleton mask
//   f[0]     the foreground voxels' indices (compacted once)       f[1], f[3]  the undecided candidates of a round, ping-pong
//   f[2]     the state volume (thin.inc)
// Rounds are launches on the context's stream, `rounds_per_sync` of them blind between two read-backs of the counters; a launch behind
// a sub-iteration's last round finds an empty list and returns.  No kernel waits for another.
#include "nl_host.h"
#include "thin.inc"

#define THIN_SMALL_OFF 1024               // the counters' place in d_small / h_small (Network's own scalars sit below)

static inline ThinCnt *thin_cnt(nl_ctx *c) { return (ThinCnt *)((char *)c->d_small + THIN_SMALL_OFF); }

static int thin_read(nl_ctx *c, ThinCnt *out, char *err, size_t errlen) {
    ThinCnt *h = (ThinCnt *)((char *)c->h_small + THIN_SMALL_OFF);
    NL_HIP(hipMemcpyAsync(h, thin_cnt(c), sizeof(ThinCnt), hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    *out = *h;
    return NL_OK;
}

int thin_device(nl_ctx *c, const int *labels, int rounds_per_sync, char *err, size_t errlen) {
    if (c->n >= ((i64)1 << 31)) return nl_fail(err, errlen, NL_EINVAL, "the thinning holds voxel indices in 32 bits: frames of 2^31 voxels or more are not supported");
    for (hipEvent_t &e : c->thin_ev) if (!e) NL_HIP(hipEventCreate(&e));
    hipStream_t st = c->stream;
    const ThinGeom g{(int)c->nzl, (int)c->ny, (int)c->nx};
    uint8_t *img = c->nw_mask;
    int *vox = (int *)c->f[0], *list[2] = {(int *)c->f[1], (int *)c->f[3]}, *state = (int *)c->f[2];
    ThinCnt *tc = thin_cnt(c);
    c->thin_valid = 0;
    NL_HIP(hipEventRecord(c->thin_ev[0], st));
    if (labels) thin_from_labels_kernel<<<grid1d(c->n, 256, 2048), 256, 0, st>>>(labels, img, c->n);
    else thin_normalise_kernel<<<grid1d(c->n, 256, 2048), 256, 0, st>>>(img, c->n);
    NL_CHECK_LAUNCH();
    NL_HIP(zero_small(tc, sizeof(ThinCnt), st));
    NL_HIP(hipMemsetAsync(state, 0, (size_t)c->n * 4, st));
    thin_compact_kernel<<<grid1d(c->n, 256, 2048), 256, 0, st>>>(img, c->n, vox, tc);
    NL_CHECK_LAUNCH();
    ThinCnt h;
    if (int rc = thin_read(c, &h, err, errlen)) return rc;
    const i64 n_fg = h.n_fg;
    const int ndirs = thin_ndirs(c->nzl), batch = thin_batch(rounds_per_sync);
    i64 outer = 0, subiters = 0;
    unsigned int serial = 0;
    int unchanged = 0;
    if (n_fg == 0) { outer = 1; subiters = ndirs; unchanged = ndirs; }          // nothing to judge: the one outer iteration that changes nothing
    while (unchanged < ndirs) {
        ++outer;
        NL_HIP(zero_small(tc->sub_removed, sizeof(tc->sub_removed), st));
        for (int d = 0; d < ndirs; ++d) {
            ++subiters;
            const i64 alive = n_fg - (i64)h.removed;
            ++serial;
            thin_candidates_kernel<<<thin_grid(n_fg), 256, 0, st>>>(img, g, vox, d, serial, state, list[(serial + 1u) & 1u], tc);
            NL_CHECK_LAUNCH();
            i64 bound = alive;                                      // the candidates are among the voxels still set
            for (;;) {
                for (int r = 0; r < batch; ++r) {
                    ++serial;
                    thin_round_kernel<<<thin_grid(bound), 256, 0, st>>>(img, g, list[serial & 1u], d, serial, state, list[(serial + 1u) & 1u], tc);
                }
                NL_CHECK_LAUNCH();
                if (int rc = thin_read(c, &h, err, errlen)) return rc;
                bound = h.cnt[(serial + 1u) % 3u];                  // what the next launch would read
                if (bound == 0) break;
            }
        }
        unchanged = 0;
        for (int d = 0; d < ndirs; ++d) unchanged += h.sub_removed[d] == 0u;
    }
    NL_HIP(hipEventRecord(c->thin_ev[1], st));
    NL_HIP(hipStreamSynchronize(st));
    NL_HIP(hipEventElapsedTime(&c->thin_ms, c->thin_ev[0], c->thin_ev[1]));
    const i64 counts[7] = {n_fg, n_fg - (i64)h.removed, outer, subiters, (i64)h.rounds, (i64)h.candidates, (i64)h.removed};
    for (int k = 0; k < 7; ++k) c->thin_counts[k] = counts[k];
    c->thin_valid = 1;
    return NL_OK;
}

// Stand-alone: the mask (one byte per voxel, non-zero = foreground) goes up, its skeleton (0 / 1) comes down.  n_skel may be NULL.
extern "C" int nl_thin(nl_ctx *c, const uint8_t *mask, uint8_t *skel, int ndim, int rounds_per_sync, int64_t *n_skel, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_JOIN_SIDE(c);
    if (!mask || !skel) return nl_fail(err, errlen, NL_EINVAL, "nl_thin: NULL mask or skel");
    if (ndim != 3) return nl_fail(err, errlen, NL_EINVAL, "the thinning on the device is the 3-D one: ndim = %d is not supported (thin 2-D frames on the host)", ndim);
    if (c->own_lo != 0 || c->own_hi != c->nzl || c->gnz != c->nzl) return nl_fail(err, errlen, NL_EINVAL, "the thinning runs on a whole volume");
    if (!c->nw_mask) NL_HIP(hipMalloc((void **)&c->nw_mask, (size_t)c->n));
    // the thinning takes over the four volumes, and the Network frame's mask
    c->i_labels = -1; c->frangi_ready = 0; c->gauss_ext = nullptr; c->fsq_cache_valid = 0; c->mk_state = 0; c->nw_state = 0; c->nw_stage = 0;
    NL_HIP(hipMemcpyAsync(c->nw_mask, mask, (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    if (int rc = thin_device(c, nullptr, rounds_per_sync, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(skel, c->nw_mask, (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    if (n_skel) *n_skel = c->thin_counts[1];
    return NL_OK;
}

// The mask the last thinning on this context left (one byte per voxel, 0 / 1).
extern "C" int nl_network_fetch_mask(nl_ctx *c, uint8_t *skel_mask, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!skel_mask) return nl_fail(err, errlen, NL_EINVAL, "skel_mask is NULL");
    if (!c->thin_valid) return nl_fail(err, errlen, NL_ESTATE, "nl_network_fetch_mask needs nl_network_load_thin or nl_thin first");
    NL_HIP(hipMemcpyAsync(skel_mask, c->nw_mask, (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

// counts[7]: n_in, n_out, outer, subiters, rounds, candidates, removed of the last thinning; ms[1]: its time on the stream, from the
// first kernel to the last, the waits for the counters included.  Either may be NULL.
extern "C" int nl_thin_info(nl_ctx *c, int64_t *counts, float *ms, char *err, size_t errlen) {
    if (!c) return nl_fail(err, errlen, NL_EINVAL, "ctx is NULL");
    if (!c->thin_valid) return nl_fail(err, errlen, NL_ESTATE, "nl_thin_info needs nl_network_load_thin or nl_thin first");
    if (counts) for (int k = 0; k < 7; ++k) counts[k] = c->thin_counts[k];
    if (ms) ms[0] = c->thin_ms;
    return NL_OK;
}

// The decision functions the kernels use, evaluated on the host: flags[i] = bit 0 endpoint, bit 1 Euler-invariant, bit 2 simple of the
// 27-bit neighbourhood nbhd[i].
extern "C" int nl_thin_decide_host(const uint32_t *nbhd, int64_t n, uint8_t *flags) {
    if (n < 0 || (n > 0 && (!nbhd || !flags))) return NL_EINVAL;
    for (int64_t i = 0; i < n; ++i) flags[i] = thin_decide(nbhd[i] & 0x7ffffffu);
    return NL_OK;
}
