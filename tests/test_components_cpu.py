"""CPU tests of the organelle level of the hierarchy: the numpy restatement (tests/component_features_restatement.py) against every
golden of the reference's Components (tests/golden/components), the package's host arithmetic (feature_extraction/components.py and
branches.region_columns: what is left once the device has touched the voxels) against the restatement from numpy-made sums, a
line-by-line emulation of the row-run kernel's decomposition (bands of rows, 64-voxel chunks, runs, closed forms) against direct
sums, the CSR builder against the reference's argwhere lists, and the text of features_organelles.  The GPU tests
(tests/test_hip_components.py) lean on these."""
from types import SimpleNamespace

import numpy as np
import pytest

import branch_goldens as bg
import component_features_restatement as cr
import component_goldens as cg
import component_scenes as cs

NAMES = cg.names()
BAND = 16                                                         # BF_ROWS_BAND of csrc/branchfeat.inc: no sum depends on it
ALL_ONES = 2 ** 64 - 1


def restated(g, regions=True, **extra):
    own = cr.Components(cg.double_of(g, **extra))
    own.run(regions=regions)
    return own


def test_the_public_names_exist():
    from nellie_amd import feature_extraction as fe
    assert {"Components", "ComponentFeatures", "Branches", "BranchFeatures"} <= set(fe.__all__)
    assert fe.Components.__module__ == fe.ComponentFeatures.__module__ == "nellie_amd.feature_extraction.components"
    assert issubclass(fe.ComponentFeatures, fe.BranchFeatures)
    c = fe.Components(SimpleNamespace())
    assert c.stats_to_aggregate == cg.STATS_TO_AGGREGATE and c.features_to_save == cg.STATS_TO_AGGREGATE + ["x", "y", "z"]
    assert c._engine is None and c._aggregator is None and c.kernel_ms == [] and c.aggregate_branch_metrics == []


def test_the_goldens_cover_the_cases():
    assert [n[len("components_"):] for n in NAMES] == [n[len("branches_"):] for n in bg.names()] and len(NAMES) == 12
    counts = {name: [len(a) for a in cg.load(name)["ref"]["component_label"]] for name in NAMES}
    assert counts["components_3d_empty_frame"][2] == 0 and all(counts["components_3d_empty_frame"][t] for t in (0, 1, 3))
    assert cg.load("components_3d_skip_nodes")["ref"]["agg_node"] == [] and cg.load("components_3d_t_without_flow")["no_t"]
    assert {cg.load(name)["base"]["D"] for name in NAMES} == {2, 3} and len(set(cg.load("components_3d_aniso")["base"]["spacing"])) > 1
    seen = set()
    for name in NAMES:
        g = cg.load(name)
        h = cg.double_of(g)
        for t in range(g["base"]["T"]):
            for child, what in ((h.nodes, "nodes"), (h.branches, "branches")):
                if what == "nodes" and g["base"]["skip_nodes"]:
                    continue
                mine = set(np.asarray(child.component_label[t]).tolist())
                if any(l not in mine for l in g["ref"]["component_label"][t].tolist()):
                    seen.add("component without " + what)
            if counts[name][t]:                                   # an empty group: a NaN row with sum 0
                agg = g["ref"]["agg_branch"][t]["branch_length"]
                if np.isnan(agg["mean"]).any():
                    assert (agg["sum"][np.isnan(agg["mean"])] == 0).all()
                    seen.add("empty group")
    assert seen == {"component without nodes", "component without branches", "empty group"}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_golden(name):
    g = cg.load(name)
    own = restated(g, regions=False)
    cg.assert_same_components(own, g["ref"], g["base"])
    assert all(getattr(own, k)[t] == [] for k in cg.REGION for t in range(g["base"]["T"]))


@pytest.mark.parametrize("name", NAMES)
def test_host_arithmetic_of_the_package_equals_the_restatement(name):
    """region_columns with the organelle prefix from sums made by numpy, with and without reassigned labels, against the
    restatement's columns straight from the coordinates; the branch prefix gives the same values under the branch names"""
    from nellie_amd.feature_extraction.branches import REGION_STATS, region_columns
    from nellie_amd.feature_extraction.components import REGION_STATS as ORGANELLE_STATS
    assert ORGANELLE_STATS == cg.REGION and REGION_STATS == bg.REGION
    g = cg.load(name)
    base = g["base"]
    rng = np.random.default_rng(4)
    for t in range(base["T"]):
        labels, sums = cr.region_sums(base["comp"][t])
        reassigned = rng.integers(0, 3, base["comp"][t].shape)
        for re in (None, reassigned):
            mode = np.full(len(labels), -1, np.int64) if re is None else cr.mode_of(base["comp"][t], re)
            got = region_columns(sums, mode, base["spacing"], base["D"], prefix="organelle")
            want = cr.region_columns(base["comp"][t], base["spacing"], re)
            assert tuple(got) == cg.REGION and np.array_equal(labels, want["label"])
            for k in cg.REGION:
                assert got[k].dtype == np.float64 and cg.same(got[k], want[k]), (k, t)
            assert np.isnan(got["organelle_solidity"]).all() and np.isnan(got["reassigned_label"]).all() == (re is None or len(labels) == 0)
            old = region_columns(sums, mode, base["spacing"], base["D"])
            assert tuple(old) == bg.REGION and all(cg.same(a, b) for a, b in zip(old.values(), got.values()))


def test_groups_are_the_references_lists():
    """the CSR against a given label list: labels that do not occur (empty groups, first, last and in the middle), a child without
    rows, unsigned and signed dtypes mixed, positions ascending"""
    from nellie_amd.feature_extraction.components import _groups_of
    import node_features_restatement as nr
    rng = np.random.default_rng(9)
    cases = [(np.array([2, 5, 9, 11], np.int32), rng.integers(0, 12, 300).astype(np.uint16)),
             (np.array([1, 2, 3], np.int64), np.zeros(0, np.int32)),
             (np.array([4], np.uint16), np.array([0, 0, 7], np.int64)),
             (np.array([7, 40000], np.uint16), np.array([40000, 0, 7, 7, 40000, 3], np.uint16)),
             (np.zeros(0, np.int32), np.array([1, 2], np.int32))]
    for label_list, labels in cases:
        off, idx = _groups_of(label_list, labels)
        want_off, want_idx = nr.as_csr(cr.label_groups(label_list, labels)) if len(label_list) else (np.zeros(1, np.int64), np.zeros(0, np.int64))
        assert off.dtype == idx.dtype == np.int64 and np.array_equal(off, want_off) and np.array_equal(idx, want_idx), (label_list, labels)
    for name in ("components_3d_sparse_flow", "components_2d"):   # the goldens' own lists
        g = cg.load(name)
        h = cg.double_of(g)
        for t in range(g["base"]["T"]):
            label_list = g["ref"]["component_label"][t]
            for labels in (h.voxels.component_labels[t], h.nodes.component_label[t], h.branches.component_label[t]):
                off, idx = _groups_of(label_list, labels)
                want_off, want_idx = nr.as_csr(cr.label_groups(label_list, labels))
                assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)


def emulate_rows(lab):
    """bf_region_rows_kernel line by line in Python integers: (labels, sums (F, R) as a list of lists, runs).  Every intermediate
    of the closed forms is checked against the bound the kernel's comment states."""
    lab = np.asarray(lab)
    D = lab.ndim
    vol = lab.reshape((1,) * (3 - D) + lab.shape)
    nz, ny, nx = vol.shape
    F = 1 + 3 * D + D * (D + 1) // 2
    found = np.unique(lab[lab > 0])
    acc = [[ALL_ONES if 1 <= f <= D else 0 for _ in range(len(found))] for f in range(F)]
    runs = 0
    for z in range(nz):
        for y0 in range(0, ny, BAND):                              # a workgroup
            for wave in range(4):
                for y in range(y0 + wave, min(y0 + BAND, ny), 4):
                    for xc in range(0, nx, 64):
                        chunk = np.zeros(64, np.int64)
                        chunk[:min(64, nx - xc)] = np.maximum(vol[z, y, xc:xc + 64], 0)
                        heads = np.concatenate([[True], chunk[1:] != chunk[:-1]])
                        for lane in np.flatnonzero(heads & (chunk > 0)).tolist():
                            rest = np.flatnonzero(heads[lane + 1:])
                            n = int(rest[0]) + 1 if len(rest) else 64 - lane
                            x0 = xc + lane
                            assert x0 + n <= nx and (vol[z, y, x0:x0 + n] == chunk[lane]).all()
                            r = int(np.searchsorted(found, chunk[lane]))
                            c = [z, y, x0][3 - D:]
                            sx = n * x0 + n * (n - 1) // 2
                            qxx = n * x0 * x0 + x0 * n * (n - 1) + (n - 1) * n * (2 * n - 1) // 6
                            v = [n] + c + c[:-1] + [x0 + n - 1] + [ca * n for ca in c[:-1]] + [sx]
                            v += [c[a] * c[b] * n if b < D - 1 else c[a] * sx if a < D - 1 else qxx for a in range(D) for b in range(a, D)]
                            assert len(v) == F and all(0 <= x < 2 ** 47 for x in v)
                            runs += 1
                            for f in range(F):
                                acc[f][r] = min(acc[f][r], v[f]) if 1 <= f <= D else max(acc[f][r], v[f]) if D < f <= 2 * D else acc[f][r] + v[f]
    return found.astype(np.int64), acc, runs


@pytest.mark.parametrize("name", sorted(cs.FRAMES))
def test_row_run_decomposition_equals_direct_sums(name):
    lab = cs.frame(name)
    labels, sums = cs.direct(name)
    got_labels, acc, runs = emulate_rows(lab)
    assert np.array_equal(got_labels, labels) and len(labels) > 0
    assert all(max(row) < 2 ** 61 for row in acc) and np.array_equal(np.array(acc, dtype=np.int64), sums)
    rows = lab.size // lab.shape[-1]
    assert runs >= len(labels)
    if name == "scatter":
        band = np.unique(lab[0, :BAND][lab[0, :BAND] > 0])
        assert len(band) == cs.SCATTERED + 1 and (sums[0][labels >= 10] == 1).all()
    if name in ("box", "longest_run"):                            # a run per chunk, never longer: the largest closed-form terms
        assert len(labels) == 1 and np.array_equal(sums, cs.box_sums(lab.shape)) and runs == rows * -(-lab.shape[-1] // 64)


def test_the_scenes_show_what_they_are_for():
    assert cs.frame("longest_run").shape == (3, 32768) and cs.frame("box").size == 312_000
    wrap = cs.frame("wrap")
    assert (wrap[..., -1] == wrap[..., 0]).all() and (wrap[..., 0] > 0).all()
    adj = cs.frame("adjacent")
    assert (adj[0, :, 49] == 3).all() and (adj[0, :, 50] == 7).all() and (np.diff(adj[1, 0]) != 0).all()
    st = cs.frame("straddle")
    assert st[0, 0, 63] == st[0, 0, 64] == 2 and st[0, 0, 127] == st[0, 0, 128] == 3 and st[0, 1, 63] != st[0, 1, 64] and st[0, 2, 127] != st[0, 2, 128]
    co = cs.frame("corners")
    assert (co > 0).sum() == 8 and all(co[tuple(-1 if v else 0 for v in c)] > 0 for c in np.ndindex(2, 2, 2))
    assert 1_500_000 <= cs.direct("sparse")[0].min() and cs.direct("sparse")[0].max() == 2_000_000
    for name, shape in cs.GENERIC.items():
        assert cs.frame(name).shape == shape and len(cs.direct(name)[0]) >= 3


def _table_of(components, tmp_path, name="table.csv"):
    from nellie_amd.feature_extraction.hierarchy import write_table
    path = str(tmp_path / name)
    write_table(components, path, components.component_label)
    return open(path).read()


@pytest.mark.parametrize("name", ["components_3d_empty_frame", "components_2d", "components_3d_skip_nodes"])
def test_the_organelle_table_has_the_reference_columns(name, tmp_path):
    g = cg.load(name)
    rng = np.random.default_rng(3)
    own = restated(g, reassigned=rng.integers(0, 3, g["base"]["comp"].shape))
    header, want = cr.feature_table(own)
    got = _table_of(own, tmp_path)
    assert got == want and got.splitlines()[0] == ",".join(header)
    assert len(header) == 2 + (0 if g["base"]["skip_nodes"] else 20) + 55 + 45 + 9 and header[:2] == ["t", "label"]
    assert header[-9:] == [k + "_raw" for k in cg.STATS_TO_AGGREGATE + ["x", "y", "z"]]
    first = "linear_vel_mean" if g["base"]["skip_nodes"] else "divergence_mean"
    assert header[2] == first and "branch_length_mean" in header and header.index("intensity_sum") < header.index("branch_length_mean")
    rows = got.splitlines()[1:]
    assert len(rows) == sum(len(a) for a in g["ref"]["component_label"])
    assert sorted({int(float(r.split(",")[0])) for r in rows}) == [t for t in range(g["base"]["T"]) if len(g["ref"]["component_label"][t])]


def test_the_organelle_table_without_rows_and_with_a_clash(tmp_path):
    g = cg.load("components_3d_empty_frame")
    own = restated(g)
    empty = cr.Components(SimpleNamespace())
    for k in cg.PER_COMPONENT + cg.REGION + ("aggregate_voxel_metrics", "aggregate_node_metrics", "aggregate_branch_metrics"):
        setattr(empty, k, [getattr(own, k)[2]])
    text = _table_of(empty, tmp_path, "empty.csv")
    assert text == ",".join(["t", "label"] + [k + "_raw" for k in empty.features_to_save]) + "\n"
    own.aggregate_branch_metrics[0] = dict(own.aggregate_branch_metrics[0], intensity=own.aggregate_voxel_metrics[0]["intensity"])
    with pytest.raises(AssertionError, match="intensity"):        # dict.update would overwrite: concatenating is no longer the same
        _table_of(own, tmp_path, "clash.csv")
