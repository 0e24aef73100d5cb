// Translation unit of libnellie_hip.so (gfx950): voxel-level features (Voxels of nellie/feature_extraction/hierarchical.py).
// C-ABI in include/nellie_amd.h; kernels in voxfeat.inc.  The object owns its buffers and stream and keeps one frame on the
// device; the flow vectors come from two flow fields (nellie_hip_flow.hip) through nl_flow_interpolate_dev, device to device.
#include <math.h>
#include <string.h>
#include "nl_stage.h"
#include "voxfeat.inc"

#define VF_MAX_ROWS ((i64)1 << 30)          // labelled voxels (and nodes) per frame: ranks are ints
#define VF_MAX_PAIRS (((i64)1 << 31) - 1)   // (node, voxel) pairs per frame: CSR offsets are ints
enum { VF_MS_LOAD, VF_MS_FLOW, VF_MS_PIVOT, VF_MS_MOTILITY, VF_MS_NODES, VF_MS_PARTS };

struct nl_voxfeat : StageBase {
    int ndim = 3;
    VfGeom g{};
    i64 words = 0;                                  // mask words per frame (a multiple of 4: one workgroup of rank_mask_kernel writes 4)
    // the frame as uploaded (dense): labels, and two 8-byte-per-voxel buffers for raw / structure, then pixel class / distance
    int *d_comp = nullptr, *d_branch = nullptr;
    void *d_a = nullptr, *d_b = nullptr;
    u64 *bits = nullptr, *nbits = nullptr;          // masks: labelled voxels, nodes
    int *pre = nullptr, *npre = nullptr, *d_wcount = nullptr;
    RankScan scan;
    int *d_maxlab = nullptr, *h_maxlab = nullptr;
    // labelled voxels
    i64 n = 0, cap = 0; int raw_size = 1, st_size = 1, nlab = 0; bool has_frame = false;
    i64 *vox = nullptr; int *lab_c = nullptr, *lab_b = nullptr; void *raw_c = nullptr, *st_c = nullptr;
    // motility
    double *d_q = nullptr, *d_v01 = nullptr, *d_v12 = nullptr; float *d_out = nullptr; i64 m_cap = 0; bool has_motility = false;
    u64 *d_best = nullptr; int *d_pivot = nullptr; i64 lab_cap = 0;
    // nodes
    i64 m = 0, node_cap = 0, pairs = 0, pair_cap = 0, vcnt_cap = 0; bool has_nodes = false;
    i64 *node_vox = nullptr, *lims = nullptr; double *radius = nullptr;
    int *ncount = nullptr, *nstart = nullptr, *vcount = nullptr, *vstart = nullptr, *cursor = nullptr, *node_val = nullptr, *vox_val = nullptr;
    float ms[VF_MS_PARTS] = {0.f, 0.f, 0.f, 0.f, 0.f};
};

extern "C" int nl_voxfeat_destroy(nl_voxfeat *h) {
    if (!h) return NL_OK;
    stage_close(*h, {h->d_comp, h->d_branch, h->d_a, h->d_b, h->bits, h->nbits, h->pre, h->npre, h->d_wcount, h->scan.d_bsum, h->scan.d_total,
                     h->d_maxlab, h->vox, h->lab_c, h->lab_b, h->raw_c, h->st_c, h->d_q, h->d_v01, h->d_v12, h->d_out, h->d_best, h->d_pivot,
                     h->node_vox, h->lims, h->radius, h->ncount, h->nstart, h->vcount, h->vstart, h->cursor, h->node_val, h->vox_val},
                {h->scan.h_total, h->h_maxlab});
    delete h;
    return NL_OK;
}

extern "C" int nl_voxfeat_create(nl_voxfeat **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, double dt,
                                 char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = stage_check_frame(ndim, spacing, nz, ny, nx, err, errlen)) return rc;
    if (int rc = stage_check_positive(dt, "the time step", err, errlen)) return rc;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_voxfeat *h = new nl_voxfeat();
    h->ndim = ndim;
    h->g.nz = nz; h->g.ny = ny; h->g.nx = nx; h->g.n = nz * ny * nx;
    for (int a = 0; a < 3; ++a) h->g.s[a] = a < ndim ? spacing[a] : 1.0;
    h->g.dt = dt;
    h->words = ((h->g.n + 255) / 256) * 4;
    const i64 n = h->g.n;
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_voxfeat_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->d_comp, n, 4), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_branch, n, 4), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_a, n, 8), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_b, n, 8), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->bits, h->words, 8), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->nbits, h->words, 8), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->pre, h->words, 4), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->npre, h->words, 4), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wcount, h->words, 4), nl_voxfeat_destroy(h));
    // the workgroup sums are sized once for the longest scan a frame of this shape can ask for
    STAGE_HIP(stage_alloc(&h->scan.d_bsum, rank_scan_sums(h->words > n ? h->words : n), 8), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_voxfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_maxlab, 1, 4), nl_voxfeat_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_voxfeat_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->h_maxlab, 4, hipHostMallocDefault), nl_voxfeat_destroy(h));
    *out = h;
    return NL_OK;
}

// A frame: component and branch labels (int32), intensity and structure frames in their own dtypes (NL_U8 .. NL_I64), all of the
// object's shape.  The voxels with component > 0 are listed in raster order with their four values.  n_vox = their number.
extern "C" int nl_voxfeat_frame(nl_voxfeat *h, const int32_t *comp, const int32_t *branch, const void *raw, int raw_dtype, const void *structure,
                                int struct_dtype, int64_t *n_vox, char *err, size_t errlen) {
    STAGE_ENTER(h, "voxel-feature object");
    if (!comp || !branch || !raw || !structure || !n_vox) return nl_fail(err, errlen, NL_EINVAL, "NULL frame or n_vox");
    const size_t rs = dtype_size(raw_dtype), ss = dtype_size(struct_dtype);
    if (!rs || !ss) return nl_fail(err, errlen, NL_EINVAL, "unsupported dtype code");
    hipStream_t st = h->stream;
    const i64 n = h->g.n;
    h->has_frame = h->has_motility = h->has_nodes = false;
    h->n = 0;
    for (float &v : h->ms) v = 0.f;
    NL_HIP(hipMemcpyAsync(h->d_comp, comp, (size_t)n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(h->d_branch, branch, (size_t)n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(h->d_a, raw, (size_t)n * rs, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(h->d_b, structure, (size_t)n * ss, hipMemcpyHostToDevice, st));
    if (int rc = stage_start(*h, err, errlen)) return rc;
    const unsigned gv = (unsigned)((n + 255) / 256);
    rank_mask_kernel<<<gv, 256, 0, st>>>(VfPositive{h->d_comp, NL_I32}, n, h->bits, h->d_wcount);
    NL_CHECK_LAUNCH();
    i64 total = 0;
    if (int rc = rank_scan(h->scan, st, h->d_wcount, h->words, h->pre, VF_MAX_ROWS, "labelled voxels in one frame", &total, err, errlen)) return rc;
    if (int rc = stage_grow(&h->cap, total, total, {{&h->vox, 8}, {&h->lab_c, 4}, {&h->lab_b, 4}, {&h->raw_c, 8}, {&h->st_c, 8}}, err, errlen)) return rc;
    NL_HIP(hipMemsetAsync(h->d_maxlab, 0, 4, st));
    if (total > 0) {
        vf_compact_kernel<<<gv, 256, 0, st>>>(h->d_comp, h->d_branch, h->d_a, (int)rs, h->d_b, (int)ss, n, h->bits, h->pre, h->vox, h->lab_c,
                                              h->lab_b, h->raw_c, h->st_c, h->d_maxlab);
        NL_CHECK_LAUNCH();
    }
    NL_HIP(hipMemcpyAsync(h->h_maxlab, h->d_maxlab, 4, hipMemcpyDeviceToHost, st));
    if (int rc = stage_stop(*h, &h->ms[VF_MS_LOAD], err, errlen)) return rc;          // the host arrays may go away after the call
    h->n = total;
    h->raw_size = (int)rs;
    h->st_size = (int)ss;
    h->nlab = *h->h_maxlab + 1;
    h->has_frame = true;
    *n_vox = total;
    return NL_OK;
}

// Downloads the frame's voxel list: linear indices (n_vox, raster order), component and branch labels, intensity and structure
// values (n_vox elements of the uploaded dtypes).  NULL pointers are skipped.
extern "C" int nl_voxfeat_fetch_voxels(nl_voxfeat *h, int64_t *vox, int32_t *comp, int32_t *branch, void *raw, void *structure, char *err, size_t errlen) {
    STAGE_ENTER(h, "voxel-feature object");
    if (!h->has_frame) return nl_fail(err, errlen, NL_ESTATE, "no frame loaded");
    hipStream_t st = h->stream;
    if (h->n > 0) {
        if (vox) NL_HIP(hipMemcpyAsync(vox, h->vox, (size_t)h->n * 8, hipMemcpyDeviceToHost, st));
        if (comp) NL_HIP(hipMemcpyAsync(comp, h->lab_c, (size_t)h->n * 4, hipMemcpyDeviceToHost, st));
        if (branch) NL_HIP(hipMemcpyAsync(branch, h->lab_b, (size_t)h->n * 4, hipMemcpyDeviceToHost, st));
        if (raw) NL_HIP(hipMemcpyAsync(raw, h->raw_c, (size_t)h->n * h->raw_size, hipMemcpyDeviceToHost, st));
        if (structure) NL_HIP(hipMemcpyAsync(structure, h->st_c, (size_t)h->n * h->st_size, hipMemcpyDeviceToHost, st));
    }
    NL_HIP(hipStreamSynchronize(st));
    return NL_OK;
}

// One direction's flow vectors at the frame's voxels into d_v; all NaN without a field, without rows or without any neighbour.
static int vf_direction(nl_voxfeat *h, nl_flow *flow, double *d_v, int64_t *found, char *err, size_t errlen) {
    *found = 0;
    if (flow) {
        if (int rc = nl_flow_interpolate_dev(flow, h->d_q, h->n, d_v, found, err, errlen)) return rc;
        float ms = 0.f;
        if (int rc = nl_flow_kernel_ms(flow, &ms, err, errlen)) return rc;
        h->ms[VF_MS_FLOW] += ms;
        NL_HIP(hipSetDevice(h->device));
    }
    if (*found == 0) NL_HIP(hipMemsetAsync(d_v, 0xff, (size_t)h->n * h->ndim * 8, h->stream));      // every byte 0xff: a NaN
    return NL_OK;
}

// The motility features of the loaded frame.  bw: a flow field with the backward rows of the frame's time point loaded (vec01),
// fw: one with its forward rows (vec12); NULL: the direction does not exist.  n_found_*: voxels with a flow neighbour.
extern "C" int nl_voxfeat_motility(nl_voxfeat *h, nl_flow *bw, nl_flow *fw, int64_t *n_found_bw, int64_t *n_found_fw, char *err, size_t errlen) {
    STAGE_ENTER(h, "voxel-feature object");
    if (!n_found_bw || !n_found_fw) return nl_fail(err, errlen, NL_EINVAL, "n_found is NULL");
    if (!h->has_frame) return nl_fail(err, errlen, NL_ESTATE, "no frame loaded");
    *n_found_bw = *n_found_fw = 0;
    h->ms[VF_MS_FLOW] = h->ms[VF_MS_PIVOT] = h->ms[VF_MS_MOTILITY] = 0.f;
    h->has_motility = false;
    const i64 n = h->n;
    const int D = h->ndim;
    if (n == 0) { h->has_motility = true; return NL_OK; }
    hipStream_t st = h->stream;
    int off[VF_OUT_BLOCKS + 1];
    vf_out_layout(D, off);
    if (int rc = stage_grow(&h->m_cap, n, n, {{&h->d_q, (size_t)D * 8}, {&h->d_v01, (size_t)D * 8}, {&h->d_v12, (size_t)D * 8},
                                              {&h->d_out, (size_t)off[VF_OUT_BLOCKS] * 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->lab_cap, h->nlab, h->nlab, {{&h->d_best, 2 * 8}, {&h->d_pivot, 2 * 4}}, err, errlen)) return rc;      // two tables each
    const unsigned gq = (unsigned)((n + 255) / 256);
    if (int rc = stage_start(*h, err, errlen)) return rc;
    rank_coords_kernel<<<gq, 256, 0, st>>>(h->vox, n, h->g.ny, h->g.nx, D, h->d_q);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->ms[VF_MS_FLOW], err, errlen)) return rc;          // the queries are complete before the fields read them
    if (int rc = vf_direction(h, bw, h->d_v01, n_found_bw, err, errlen)) return rc;
    if (int rc = vf_direction(h, fw, h->d_v12, n_found_fw, err, errlen)) return rc;
    const int nlab = h->nlab;
    u64 *best01 = h->d_best, *best12 = h->d_best + nlab;
    int *piv01 = h->d_pivot, *piv12 = h->d_pivot + nlab;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    NL_HIP(hipMemsetAsync(h->d_best, 0xff, (size_t)2 * nlab * 8, st));
    NL_HIP(hipMemsetAsync(h->d_pivot, 0x7f, (size_t)2 * nlab * 4, st));
    const double *vs[2] = {h->d_v01, h->d_v12};
    u64 *bests[2] = {best01, best12};
    int *pivs[2] = {piv01, piv12};
    const int64_t founds[2] = {*n_found_bw, *n_found_fw};
    for (int d = 0; d < 2; ++d) {
        if (founds[d] == 0) continue;                                     // every vector is NaN: no label has a pivot
        if (D == 3) {
            vf_pivot_norm_kernel<3><<<gq, 256, 0, st>>>(vs[d], n, h->g, h->lab_b, nlab, bests[d]);
            vf_pivot_index_kernel<3><<<gq, 256, 0, st>>>(vs[d], n, h->g, h->lab_b, nlab, bests[d], pivs[d]);
        } else {
            vf_pivot_norm_kernel<2><<<gq, 256, 0, st>>>(vs[d], n, h->g, h->lab_b, nlab, bests[d]);
            vf_pivot_index_kernel<2><<<gq, 256, 0, st>>>(vs[d], n, h->g, h->lab_b, nlab, bests[d], pivs[d]);
        }
        NL_CHECK_LAUNCH();
    }
    if (int rc = stage_stop(*h, &h->ms[VF_MS_PIVOT], err, errlen)) return rc;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    if (D == 3) vf_motility_kernel<3><<<gq, 256, 0, st>>>(h->vox, n, h->g, h->lab_b, nlab, h->d_v01, h->d_v12, piv01, piv12, h->d_out);
    else vf_motility_kernel<2><<<gq, 256, 0, st>>>(h->vox, n, h->g, h->lab_b, nlab, h->d_v01, h->d_v12, piv01, piv12, h->d_out);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->ms[VF_MS_MOTILITY], err, errlen)) return rc;
    h->has_motility = true;
    return NL_OK;
}

// Downloads the float32 results of nl_voxfeat_motility, in the order of voxfeat.inc's layout: vec01 (n, D), vec12 (n, D),
// linear_vel_vector (n, D), linear_vel, angular_vel_vector ((n) in 2-D, (n, 3) in 3-D), angular_vel, linear_acc, angular_acc,
// rel_linear_vel, rel_angular_vel, rel_linear_acc, rel_angular_acc, rel_directionality.  out: 13 host pointers, NULL ones skipped.
extern "C" int nl_voxfeat_fetch_motility(nl_voxfeat *h, float *const *out, char *err, size_t errlen) {
    STAGE_ENTER(h, "voxel-feature object");
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    if (!h->has_motility) return nl_fail(err, errlen, NL_ESTATE, "no motility results to fetch");
    int off[VF_OUT_BLOCKS + 1];
    vf_out_layout(h->ndim, off);
    hipStream_t st = h->stream;
    if (h->n > 0)
        for (int j = 0; j < VF_OUT_BLOCKS; ++j)
            if (out[j]) NL_HIP(hipMemcpyAsync(out[j], h->d_out + (size_t)off[j] * h->n, (size_t)(off[j + 1] - off[j]) * h->n * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    return NL_OK;
}

// The node assignment of the loaded frame.  pixel_class (any NL_* dtype) and distance (NL_F32 or NL_F64) have the object's shape.
// Nodes are the voxels with pixel class > 0 in raster order.  n_nodes, n_pairs: nodes, (node, voxel) pairs.
extern "C" int nl_voxfeat_nodes(nl_voxfeat *h, const void *pixel_class, int class_dtype, const void *distance, int dist_dtype, int64_t *n_nodes,
                                int64_t *n_pairs, char *err, size_t errlen) {
    STAGE_ENTER(h, "voxel-feature object");
    if (!pixel_class || !distance || !n_nodes || !n_pairs) return nl_fail(err, errlen, NL_EINVAL, "NULL frame or counter");
    if (!h->has_frame) return nl_fail(err, errlen, NL_ESTATE, "no frame loaded");
    const size_t cs = dtype_size(class_dtype);
    if (!cs) return nl_fail(err, errlen, NL_EINVAL, "unsupported dtype code");
    if (dist_dtype != NL_F32 && dist_dtype != NL_F64) return nl_fail(err, errlen, NL_EINVAL, "the distance frame must be float32 or float64");
    hipStream_t st = h->stream;
    const i64 n = h->g.n, nv = h->n;
    const int D = h->ndim;
    h->has_nodes = false;
    h->ms[VF_MS_NODES] = 0.f;
    *n_nodes = *n_pairs = 0;
    NL_HIP(hipMemcpyAsync(h->d_a, pixel_class, (size_t)n * cs, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(h->d_b, distance, (size_t)n * dtype_size(dist_dtype), hipMemcpyHostToDevice, st));
    if (int rc = stage_start(*h, err, errlen)) return rc;
    const unsigned gv = (unsigned)((n + 255) / 256);
    rank_mask_kernel<<<gv, 256, 0, st>>>(VfPositive{h->d_a, class_dtype}, n, h->nbits, h->d_wcount);
    NL_CHECK_LAUNCH();
    i64 m = 0, pairs = 0, pairs_v = 0;
    if (int rc = rank_scan(h->scan, st, h->d_wcount, h->words, h->npre, VF_MAX_ROWS, "nodes in one frame", &m, err, errlen)) return rc;
    if (int rc = stage_grow(&h->node_cap, m, m, {{&h->node_vox, 8}, {&h->radius, 8}, {&h->lims, 6 * 8}, {&h->ncount, 4}, {&h->nstart, 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->vcnt_cap, nv, nv, {{&h->vcount, 4}, {&h->vstart, 4}, {&h->cursor, 4}}, err, errlen)) return rc;
    if (m > 0) {
        const unsigned gm = (unsigned)((m + 255) / 256);
        vf_node_compact_kernel<<<gv, 256, 0, st>>>(h->d_b, dist_dtype, n, h->nbits, h->npre, h->node_vox, h->radius);
        NL_CHECK_LAUNCH();
        vf_node_lims_kernel<<<gm, 256, 0, st>>>(h->node_vox, h->radius, m, h->g, D, h->lims);
        NL_CHECK_LAUNCH();
        if (nv > 0) {
            NL_HIP(hipMemsetAsync(h->vcount, 0, (size_t)nv * 4, st));
            vf_node_count_kernel<<<gm, 256, 0, st>>>(h->lims, m, h->g, D, h->bits, h->pre, h->ncount, h->vcount);
            NL_CHECK_LAUNCH();
            if (int rc = rank_scan(h->scan, st, h->ncount, m, h->nstart, VF_MAX_PAIRS, "(node, voxel) pairs in one frame", &pairs, err, errlen)) return rc;
            if (int rc = rank_scan(h->scan, st, h->vcount, nv, h->vstart, VF_MAX_PAIRS, "(node, voxel) pairs in one frame", &pairs_v, err, errlen)) return rc;
            if (pairs_v != pairs) return nl_fail(err, errlen, NL_ESTATE, "node and voxel pair counts disagree");
            if (int rc = stage_grow(&h->pair_cap, pairs, pairs, {{&h->node_val, 4}, {&h->vox_val, 4}}, err, errlen)) return rc;
            if (pairs > 0) {
                NL_HIP(hipMemcpyAsync(h->cursor, h->vstart, (size_t)nv * 4, hipMemcpyDeviceToDevice, st));
                vf_node_place_kernel<<<gm, 256, 0, st>>>(h->lims, m, h->g, D, h->bits, h->pre, h->nstart, h->node_val, h->cursor, h->vox_val);
                NL_CHECK_LAUNCH();
                vf_sort_lists_kernel<<<(unsigned)((nv + 255) / 256), 256, 0, st>>>(nv, h->vstart, h->vcount, h->vox_val);
                NL_CHECK_LAUNCH();
            }
        } else {
            NL_HIP(hipMemsetAsync(h->ncount, 0, (size_t)m * 4, st));
            NL_HIP(hipMemsetAsync(h->nstart, 0, (size_t)m * 4, st));
        }
    }
    if (int rc = stage_stop(*h, &h->ms[VF_MS_NODES], err, errlen)) return rc;
    h->m = m;
    h->pairs = pairs;
    h->has_nodes = true;
    *n_nodes = m;
    *n_pairs = pairs;
    return NL_OK;
}

// Downloads the results of nl_voxfeat_nodes: the box limits per axis (n_nodes, 2) int64 (lims2 only in 3-D), and both lists as
// CSR with int32 ranks: node_start (n_nodes) and node_val (n_pairs, the voxels of every node, ascending), vox_start (n_vox) and
// vox_val (n_pairs, the nodes of every voxel, ascending).  A list ends where the next one starts, the last at n_pairs.  NULL
// pointers are skipped.
extern "C" int nl_voxfeat_fetch_nodes(nl_voxfeat *h, int64_t *lims0, int64_t *lims1, int64_t *lims2, int32_t *node_start, int32_t *node_val,
                                      int32_t *vox_start, int32_t *vox_val, char *err, size_t errlen) {
    STAGE_ENTER(h, "voxel-feature object");
    if (!h->has_nodes) return nl_fail(err, errlen, NL_ESTATE, "no node assignment to fetch");
    hipStream_t st = h->stream;
    const i64 m = h->m;
    int64_t *ls[3] = {lims0, lims1, lims2};
    if (m > 0) {
        for (int a = 0; a < h->ndim; ++a)
            if (ls[a]) NL_HIP(hipMemcpyAsync(ls[a], h->lims + (size_t)a * m * 2, (size_t)m * 16, hipMemcpyDeviceToHost, st));
        if (node_start) NL_HIP(hipMemcpyAsync(node_start, h->nstart, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    }
    if (h->pairs > 0) {
        if (node_val) NL_HIP(hipMemcpyAsync(node_val, h->node_val, (size_t)h->pairs * 4, hipMemcpyDeviceToHost, st));
        if (vox_val) NL_HIP(hipMemcpyAsync(vox_val, h->vox_val, (size_t)h->pairs * 4, hipMemcpyDeviceToHost, st));
    }
    if (h->n > 0 && vox_start) {
        if (m > 0) NL_HIP(hipMemcpyAsync(vox_start, h->vstart, (size_t)h->n * 4, hipMemcpyDeviceToHost, st));
        else memset(vox_start, 0, (size_t)h->n * 4);
    }
    NL_HIP(hipStreamSynchronize(st));
    return NL_OK;
}

// Device time (ms) of the kernels since the last nl_voxfeat_frame, per part: ms[0] frame load and compaction, [1] flow
// interpolation, [2] pivots, [3] motility, [4] node assignment.  Transfers excluded.
extern "C" int nl_voxfeat_kernel_ms(nl_voxfeat *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "voxel-feature object or ms is NULL");
    for (int j = 0; j < VF_MS_PARTS; ++j) ms[j] = h->ms[j];
    return NL_OK;
}
