"""numpy restatement of the voxel level of the hierarchy (the rules of DESIGN.md section 13), test infrastructure only -- never
imported by the package.  Plain functions on one frame; `voxels()` runs a stack and returns the attributes as lists per frame.

Frame: the voxels with component label > 0 in raster order, their labels, intensity and structure value.
Flow: tests/flow_interpolation_restatement.py at the voxel coordinates, backward field of t (vec01) and forward field of t
(vec12); a direction that does not exist, or in which no voxel has a flow neighbour, is (n, D) of NaN.
Pivot: per direction and branch label (0 included) the voxel with the smallest |vec * spacing| among non-NaN rows, the lowest
index on a tie; -1 when the label has no such row.
Motility: float64 numpy operations in the reference's order, cast to float32 at the end.
Nodes: the voxels with pixel class > 0 in raster order; box limits trunc(float64(radius) * (-1, +1) + index), upper + 1, clamped
to [0, shape]; a voxel belongs to a node when every coordinate is within the limits, both ends included -- one direct box test
per node, no nodes x voxels mask.
"""
import numpy as np

import flow_interpolation_restatement as fr

FLOAT_ATTRS = ("vec01", "vec12", "linear_vel_vector", "linear_vel", "angular_vel_vector", "angular_vel", "linear_acc", "angular_acc",
               "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc", "rel_directionality")


def frame_voxels(comp, branch, raw, struct):
    coords = np.argwhere(comp > 0)
    at = tuple(coords.T)
    return coords, comp[at], branch[at], raw[at], struct[at]


def node_boxes(pixel_class, distance):
    """(node coordinates (m, D), [limits (m, 2) int64 per axis])"""
    nodes = np.argwhere(pixel_class > 0)
    radius = distance[tuple(nodes.T)]
    lims = []
    for ax, size in enumerate(pixel_class.shape):
        lim = (radius[:, None] * np.array([-1, 1]) + nodes[:, ax, None]).astype(int)
        lim[:, 1] += 1
        lim[lim < 0] = 0
        lim[lim > size] = size
        lims.append(lim)
    return nodes, lims


def node_assignment(lims, coords):
    """CSR (offsets, values) of the voxels of every node (ascending voxel index) and of the nodes of every voxel (ascending node
    index)"""
    m, n = len(lims[0]), len(coords)
    per_node = []
    for i in range(m):
        inside = np.ones(n, bool)
        for ax, lim in enumerate(lims):
            inside &= (lim[i, 0] <= coords[:, ax]) & (lim[i, 1] >= coords[:, ax])
        per_node.append(np.nonzero(inside)[0])
    node_off = np.concatenate([[0], np.cumsum([len(v) for v in per_node])]).astype(np.int64)
    node_val = np.concatenate(per_node).astype(np.int64) if m else np.zeros(0, np.int64)
    owner = np.repeat(np.arange(m, dtype=np.int64), np.diff(node_off))
    order = np.lexsort((owner, node_val))
    vox_off = np.concatenate([[0], np.cumsum(np.bincount(node_val, minlength=n))]).astype(np.int64)
    return (node_off, node_val), (vox_off, owner[order])


def pivots(vec, branch_labels):
    """(pivot voxel per branch label 0 .. max label, -1 without one; smallest relative gap between the smallest norm of a label
    and the next larger one)"""
    if len(branch_labels) == 0:
        return np.zeros(0, np.int64), np.inf
    norm = np.linalg.norm(vec, axis=1)
    labels = np.asarray(branch_labels, np.int64)
    out = np.full(int(labels.max()) + 1, -1, np.int64)
    gap = np.inf
    for lbl in np.unique(labels):
        idx = np.nonzero((labels == lbl) & ~np.isnan(norm))[0]
        if len(idx) == 0:
            continue
        vals = norm[idx]
        out[lbl] = idx[np.argmin(vals)]                      # the first of equal minima
        larger = vals[vals > vals.min()]
        if len(larger):
            gap = min(gap, float((larger.min() - vals.min()) / larger.min()))
    return out, gap


def _ref_coords(coords_a, coords_b, pivot, branch_labels, vec):
    p = pivot[np.asarray(branch_labels, np.int64)]
    ref_a, ref_b = coords_a[np.maximum(p, 0)], coords_b[np.maximum(p, 0)]
    ref_a[p < 0] = np.nan
    ref_b[p < 0] = np.nan
    ref_a[np.isnan(vec)] = np.nan
    ref_b[np.isnan(vec)] = np.nan
    return ref_a, ref_b


def _linear(ra, rb, dt):
    vel = (rb - ra) / dt
    return vel, np.linalg.norm(vel, axis=1)


def _angular(ra, rb, dt):
    if ra.shape[1] == 2:
        delta = np.arctan2(rb[:, 1], rb[:, 0]) - np.arctan2(ra[:, 1], ra[:, 0])
        delta = (delta + np.pi) % (2 * np.pi) - np.pi
        vel = delta / dt
        return vel, np.abs(vel)
    cross = np.cross(ra, rb, axis=1)
    norm = np.linalg.norm(ra, axis=1) * np.linalg.norm(rb, axis=1)
    disp = np.divide(cross.T, norm.T).T
    disp[norm == 0] = np.nan
    vel = disp / dt
    return vel, np.linalg.norm(vel, axis=1)


def _pair(coords_a, coords_b, vec, branch_labels, dt):
    """velocities of one direction: absolute, and relative to the branch pivots"""
    lin, lin_mag = _linear(coords_a, coords_b, dt)
    ang, ang_mag = _angular(coords_a, coords_b, dt)
    pivot, gap = pivots(vec, branch_labels)
    ref_a, ref_b = _ref_coords(coords_a, coords_b, pivot, branch_labels, vec)
    rel_a, rel_b = coords_a - ref_a, coords_b - ref_b
    lin_rel, lin_rel_mag = _linear(rel_a, rel_b, dt)
    ang_rel, ang_rel_mag = _angular(rel_a, rel_b, dt)
    return dict(lin=lin, lin_mag=lin_mag, ang=ang, ang_mag=ang_mag, lin_rel=lin_rel, lin_rel_mag=lin_rel_mag, ang_rel=ang_rel,
                ang_rel_mag=ang_rel_mag, rel_a=rel_a, rel_b=rel_b, pivot=pivot, gap=gap)


def motility(coords, branch_labels, vec01_px, vec12_px, spacing, dt):
    """every motility attribute of one frame (float32) from the flow vectors in voxels ((n, D) float64, NaN rows where there is
    none), plus `pivot01`, `pivot12` and `gap` (the smallest pivot gap of the frame)"""
    with np.errstate(all="ignore"):
        px = coords.astype("float32")
        n, D = px.shape
        spacing = tuple(spacing)
        vec01, vec12 = vec01_px * spacing, vec12_px * spacing
        c1 = px * spacing
        c0 = (px - vec01_px) * spacing
        c2 = (px + vec12_px) * spacing
        a = _pair(c0, c1, vec01, branch_labels, dt)
        b = _pair(c1, c2, vec12, branch_labels, dt)
        r1, r2 = np.linalg.norm(b["rel_a"], axis=1), np.linalg.norm(b["rel_b"], axis=1)
        denom = r2 + r1
        direct = np.full(n, np.nan)
        np.divide(np.abs(r2 - r1), denom, out=direct, where=denom != 0)
        lin_acc = np.linalg.norm((b["lin"] - a["lin"]) / dt, axis=1)
        lin_acc_rel = np.linalg.norm((b["lin_rel"] - a["lin_rel"]) / dt, axis=1)
        ang_acc, ang_acc_rel = (b["ang"] - a["ang"]) / dt, (b["ang_rel"] - a["ang_rel"]) / dt
        if D == 2:
            ang_acc, ang_acc_rel = np.abs(ang_acc), np.abs(ang_acc_rel)
        else:
            ang_acc, ang_acc_rel = np.linalg.norm(ang_acc, axis=1), np.linalg.norm(ang_acc_rel, axis=1)
    f32 = lambda x: np.ascontiguousarray(x).astype(np.float32)   # noqa: E731
    return dict(vec01=f32(vec01), vec12=f32(vec12), linear_vel_vector=f32(b["lin"]), linear_vel=f32(b["lin_mag"]),
                angular_vel_vector=f32(b["ang"]), angular_vel=f32(b["ang_mag"]), linear_acc=f32(lin_acc), angular_acc=f32(ang_acc),
                rel_linear_vel=f32(b["lin_rel_mag"]), rel_angular_vel=f32(b["ang_rel_mag"]), rel_linear_acc=f32(lin_acc_rel),
                rel_angular_acc=f32(ang_acc_rel), rel_directionality=f32(direct), pivot01=a["pivot"], pivot12=b["pivot"],
                gap=min(a["gap"], b["gap"]))


def flow_at(flow, spacing, r, coords, t, forward):
    """(vectors (n, D) in voxels with NaN rows, neighbour counts, largest |vector| per row, membership margin)"""
    out, k, vmax, margin = fr.interpolate_coord(flow, spacing, r, coords.astype("float32"), t, forward)
    if len(out) != len(coords):
        out = np.full((len(coords), len(spacing)), np.nan)
    return out, k, vmax, margin


def voxels(comp, branch, raw, struct, pixel_class, distance, flow, spacing, dt, skip_nodes=False, enable_motility=True,
           max_distance_um=0.5, vectors=None):
    """The attributes of a stack as lists per frame.  vectors: {(t, "bw" | "fw"): (n, D) float64} replaces the interpolation
    (the tests feed the reference's own vectors to check the motility bit for bit).  Extra keys: `flow_px` (the vectors used),
    `flow_k`, `flow_vmax`, `margin` (interpolation membership), `gap` (pivots), `min_max_k` (the smallest, over the interpolation
    calls that found a neighbour, of the largest neighbour count)."""
    T, D = len(comp), comp.ndim - 1
    r = max(max_distance_um * dt, 0.5)
    out = {k: [] for k in ("time", "coords", "x", "y", "z", "intensity", "structure", "branch_labels", "component_labels") + FLOAT_ATTRS}
    out.update(node_lims=[], node_voxels=[], voxel_nodes=[], flow_px={}, flow_k={}, flow_vmax={}, pivot01=[], pivot12=[],
               margin=np.inf, gap=np.inf, min_max_k=np.iinfo(np.int64).max)
    for t in range(T):
        coords, cl, bl, inten, st = frame_voxels(comp[t], branch[t], raw[t], struct[t])
        n = len(coords)
        out["time"].append(np.ones(n, dtype=int) * t)
        out["coords"].append(coords)
        out["z"].append(coords[:, 0] if D == 3 else np.full(n, np.nan))
        out["y"].append(coords[:, D - 2])
        out["x"].append(coords[:, D - 1])
        for key, val in (("intensity", inten), ("structure", st), ("branch_labels", bl), ("component_labels", cl)):
            out[key].append(val)
        if not skip_nodes:
            _, lims = node_boxes(pixel_class[t], distance[t])
            nv, vn = node_assignment(lims, coords)
            out["node_lims"].append(lims)
            out["node_voxels"].append(nv)
            out["voxel_nodes"].append(vn)
        vecs = {}
        for key, forward, exists in (("bw", False, t > 0), ("fw", True, t < T - 1)):
            vec = np.full((n, D), np.nan)
            if enable_motility and T >= 2 and exists:
                if vectors is not None:
                    given = np.asarray(vectors[(t, key)], np.float64)
                    vec = given if len(given) == n else vec
                else:
                    vec, k, vmax, margin = flow_at(flow, spacing, r, coords, t, forward)
                    out["flow_k"][(t, key)], out["flow_vmax"][(t, key)] = k, vmax
                    out["margin"] = min(out["margin"], margin)
                    if k.any():
                        out["min_max_k"] = min(out["min_max_k"], int(k.max()))
            vecs[key] = vec
            out["flow_px"][(t, key)] = vec
        m = motility(coords, bl, vecs["bw"], vecs["fw"], spacing, dt)
        for key in FLOAT_ATTRS:
            out[key].append(m[key])
        out["pivot01"].append(m["pivot01"])
        out["pivot12"].append(m["pivot12"])
        out["gap"] = min(out["gap"], m["gap"])
    return out
