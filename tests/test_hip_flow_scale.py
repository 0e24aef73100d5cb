"""GPU tests of flow-vector interpolation (csrc/flow.inc, nellie_hip_flow.hip) at tracker-scale row counts and capped grids: the
scenes of tests/flow_scenes.py through FlowInterpolator and through hipnative.FlowField, every query compared with the numpy
restatement (tests/flow_interpolation_restatement.py) and a sample with a grid-free brute force; the plan the device made is read
with FlowField.grid() and held to each scene's expectations.

Bound: rs.tolerance, unchanged -- NaN rows identical, values within 16 * k * 2^-52 * max(1, max|v|) per row.  No query is left out
and membership is never excused: tests/test_flow_scenes_cpu.py asserts that no pair of a scene lies within 1e-9 of the radius (or,
for `round_spacing`, that both sides form the same float64 d2 from the same operations)."""
import time

import numpy as np
import pytest

import flow_interpolation_restatement as rs
import flow_scenes as fs
from test_hip_flow import hip, im_double  # noqa: F401  (hip is the fixture)

pytestmark = pytest.mark.gpu


def check_plan(g, expect, what):
    """grid() against the scene's expectations"""
    print(f"{what}: dims {g['dims']}, {g['ncell']} cells of {tuple(round(e, 4) for e in g['cell_edge'])} um, budget {g['max_cells']}, "
          f"fullest cell {g['fullest']} rows")
    assert g["ncell"] == int(np.prod(g["dims"])) <= g["max_cells"]
    assert g["max_cells"] == expect["max_cells"]
    assert g["dims"] == tuple(expect["dims"])
    assert g["cell_edge"] == expect["cell_edge"]                     # r (1 + 2^-20) times the expected doublings, 0 where unresolved
    assert expect["fullest"][0] <= g["fullest"] <= expect["fullest"][1]


def load(field, name, forward=True):
    """loads the scene's rows; returns (scene with the face block at the cell edge the device reports, grid(), load ms)"""
    sc = fs.scene(name, forward)
    cc, v, c = fs.check_rows(sc.flow, sc.expect["ndim"], forward)
    t0 = time.perf_counter()
    field.load(cc, v, c)
    ms = (time.perf_counter() - t0) * 1e3
    g = field.grid()
    return fs.scene(name, forward, g["cell_edge"]), g, ms


def interpolate_checked(field, name, sc, what):
    """all queries of the scene through the field against the reference; (result bytes' array, found)"""
    want, k, vmax, _ = fs.reference(name, True, field.grid()["cell_edge"])
    got, found = field.interpolate(sc.queries)
    rs.assert_close(got, want, k, vmax, what)
    assert found == int((k > 0).sum())
    return got


@pytest.mark.parametrize("name", fs.ORDER)
def test_scene(hip, tmp_path, name):
    """the plan the device reports, then every query through FlowField and through FlowInterpolator against the restatement (the
    brute force where the restatement cannot hold the extent), and the 2 000-query sample against the brute force"""
    from nellie_amd import hipnative
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    D = fs.scene(name).expect["ndim"]
    with hipnative.FlowField(D, fs.scene(name).spacing, 0.5) as field:
        assert field.grid() == dict(dims=(0, 0, 0), ncell=0, cell_edge=(0.0, 0.0, 0.0), max_cells=0, fullest=0)
        _, _, first_ms = load(field, name)                           # the first load also allocates the row buffers
        sc, g, load_ms = load(field, name)
        check_plan(g, sc.expect, name)
        direct = interpolate_checked(field, name, sc, f"{name}, FlowField")
        print(f"{name}: nl_flow_load {load_ms:.2f} ms (upload included; {first_ms:.2f} ms the first time), flow_interp_kernel {field.kernel_ms():.3f} ms")
        assert field.grid() == g                                     # reading the plan changes nothing
    fi = FlowInterpolator(im_double(tmp_path, sc.flow, sc.spacing, 1.0), max_distance_um=0.5, forward=True)
    assert fi.max_distance_um == sc.r
    got = fi.interpolate_coord(sc.queries, fs.T_ROWS)
    assert fi.device_field(fs.T_ROWS).grid() == g
    fi.close()
    want, k, vmax, _ = fs.reference(name, True, g["cell_edge"])
    rs.assert_close(got, want, k, vmax, f"{name}, FlowInterpolator")
    assert got.tobytes() == direct.tobytes()
    pick, (bwant, bk, bvmax, _) = fs.brute_reference(name, True, g["cell_edge"])
    rs.assert_close(got[pick], bwant, bk, bvmax, f"{name}, sample against the brute force")
    nb = sc.expect["n_body"]                                         # the face block: r (1 - 1e-6) out finds a row
    assert np.isfinite(got[nb:][0::5]).all()


def test_cap_edge_on_one_field(hip):
    """32 767 rows, then 32 768 on the same field: the budget 8 * rows moves from 262 136 to the cap 2^18, both answers right"""
    from nellie_amd import hipnative
    with hipnative.FlowField(3, fs.ANISO, 0.5) as field:
        for name, budget in (("cap_edge_32767", 262_136), ("cap_edge_32768", 1 << 18)):
            sc, g, _ = load(field, name)
            check_plan(g, sc.expect, name)
            assert g["max_cells"] == budget
            interpolate_checked(field, name, sc, f"{name}, one field")


@pytest.mark.parametrize("name", ["dense_small", "clustered"])
def test_determinism_in_full_cells(hip, name):
    """cells of a hundred to hundreds of rows: whatever order the placement's atomics gave, the per-cell sort restores row order --
    two loads on one field and one on another give the same bytes"""
    from nellie_amd import hipnative
    out = []
    with hipnative.FlowField(3, fs.ANISO, 0.5) as a, hipnative.FlowField(3, fs.ANISO, 0.5) as b:
        for field in (a, a, b):
            sc, g, _ = load(field, name)
            assert g["fullest"] >= sc.expect["fullest"][0]
            out.append(field.interpolate(sc.queries))
    assert np.isfinite(out[0][0]).any()
    assert out[0][0].tobytes() == out[1][0].tobytes() == out[2][0].tobytes() and out[0][1] == out[1][1] == out[2][1]


def test_one_handle_across_regimes(hip):
    """capped grid, unresolved one-cell plan, small dense grid, an empty time point, the capped grid again, on one field: each answer
    right, the last the first byte for byte -- nothing of a plan (start, cursor, grid, row capacity) survives into the next"""
    from nellie_amd import hipnative
    sp = fs.SCENES["cube_1024"]["spacing"]
    res = {}
    with hipnative.FlowField(3, sp, 0.5) as field:
        for step, name in enumerate(("cube_1024", "unresolved", "dense_small", None, "cube_1024")):
            if name is None:
                field.load(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))
                assert field.grid()["ncell"] == 0 and field.grid()["fullest"] == 0
                got, found = field.interpolate(fs.scene("cube_1024").queries)
                assert found == 0 and np.isnan(got).all()
                continue
            # the field keeps cube_1024's spacing: the other scenes' rows are compared at that spacing, against the brute force
            sc = fs.scene(name)
            cc, v, c = fs.check_rows(sc.flow, 3)
            field.load(cc, v, c)
            g = field.grid()
            if tuple(sc.spacing) == tuple(sp):
                check_plan(g, sc.expect, f"step {step}, {name}")
                want, k, vmax, _ = fs.reference(name, True, g["cell_edge"])
                q = fs.scene(name, True, g["cell_edge"]).queries
            else:
                q = sc.queries[fs.sample(sc)]                        # the other scenes' 2 000-query samples, face block included
                want, k, vmax, margin = _at_spacing(name, sp)
                assert margin > 1e-9                                 # unambiguous at this spacing too
                if name == "unresolved":
                    assert g["ncell"] == 1 and g["cell_edge"] == (0.0, 0.0, 0.0) and g["fullest"] == len(cc)
                else:
                    assert g["ncell"] < 4096 and g["fullest"] >= sc.expect["fullest"][0]
            got, found = field.interpolate(q)
            rs.assert_close(got, want, k, vmax, f"step {step}, {name}")
            assert found == int((k > 0).sum()) > 0
            res[step] = got
    assert res[0].tobytes() == res[4].tobytes()


_AT = {}


def _at_spacing(name, sp):
    """the brute force on the sample of a scene's queries at another spacing than the scene's own"""
    if name not in _AT:
        sc = fs.scene(name)
        cc, v, c = fs.check_rows(sc.flow, 3)
        _AT[name] = fs.brute(cc, v, c, sp, sc.r, sc.queries[fs.sample(sc)])
    return _AT[name]


def test_backward_direction(hip, tmp_path):
    """`aniso_1024` backward: the check coordinate is position + vector, so the rows' box and with it the plan differ from the
    forward ones"""
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    name = "aniso_1024"
    sc = fs.scene(name, False)
    fi = FlowInterpolator(im_double(tmp_path, sc.flow, sc.spacing, 1.0), max_distance_um=0.5, forward=False)
    g = fi.device_field(fs.T_ROWS + 1).grid()
    print(f"{name} backward: dims {g['dims']}, fullest {g['fullest']}")
    assert g["dims"] != tuple(sc.expect["dims"]) and g["cell_edge"] == sc.expect["cell_edge"] and g["ncell"] <= g["max_cells"] == 1 << 18
    sc = fs.scene(name, False, g["cell_edge"])
    got = fi.interpolate_coord(sc.queries, fs.T_ROWS + 1)
    cc, _, _ = fs.check_rows(sc.flow, 3, False)
    assert np.array_equal(fi.check_coords, cc)
    fi.close()
    want, k, vmax, _ = fs.reference(name, False, g["cell_edge"])
    rs.assert_close(got, want, k, vmax, f"{name} backward")
    pick, (bwant, bk, bvmax, _) = fs.brute_reference(name, False, g["cell_edge"])
    rs.assert_close(got[pick], bwant, bk, bvmax, f"{name} backward, sample against the brute force")
