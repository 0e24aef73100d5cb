"""CPU tests of the scenes of tests/flow_scenes.py (no device): every scene decides membership unambiguously (or, for
`round_spacing`, sits on the radius on purpose), the numpy restatement equals a grid-free brute force on a sample of every scene bit
for bit, and every scene reaches what it is there for."""
import numpy as np
import pytest

import flow_interpolation_restatement as rs
import flow_scenes as fs


def restated(name):
    return fs.scene(name), fs.reference(name)


@pytest.mark.parametrize("name", fs.ORDER)
def test_scene_shape(name):
    sc = fs.scene(name)
    D = sc.expect["ndim"]
    assert sc.flow.shape == (sc.expect["rows"], 2 * D + 2) and np.all(sc.flow[:, 0] == fs.T_ROWS) and np.isfinite(sc.flow).all()
    assert sc.queries.shape == (sc.expect["queries"] + 10 * (D + 1), D)
    assert np.isnan(sc.queries[:sc.expect["n_body"]]).any() and np.isfinite(sc.queries[sc.expect["n_body"]:]).all()
    cc, _, _ = fs.check_rows(sc.flow, D)
    assert np.array_equal(cc.min(axis=0), cc[0])                     # the planted corners are the box
    if "far" not in sc.expect:
        assert np.array_equal(cc.max(axis=0), cc[1])
    again = fs._rows(np.random.default_rng([fs.ORDER.index(name), 20261021]), fs.SCENES[name])
    assert np.array_equal(again, sc.flow)                            # seeded


@pytest.mark.parametrize("name", fs.ORDER)
def test_margin(name):
    """no candidate pair (the face block's included: it is part of the queries) within 1e-9 of the radius; `round_spacing`
    instead has at least 1 000 pairs exactly on it"""
    sc, (_, k, _, margin) = restated(name)
    print(f"{name}: smallest |d2 - r^2| / r^2 = {margin:.3g}")
    if "exact_on_radius" not in sc.expect:
        assert margin > 1e-9
        return
    assert margin == 0.0
    s = np.asarray(sc.spacing)
    cc, _, _ = fs.check_rows(sc.flow, sc.expect["ndim"])
    q = sc.queries[np.isfinite(sc.queries).all(axis=1)]
    _, _, d2 = rs.neighbour_pairs(cc * s, q * s, sc.r)
    on, r2 = int((d2 == sc.r * sc.r).sum()), sc.r * sc.r
    near = int(((d2 != r2) & (np.abs(d2 - r2) < 1e-9 * r2)).sum())
    print(f"{name}: {on} candidate pairs with d2 == r^2, {near} more within 1e-9 of it")
    assert on >= sc.expect["exact_on_radius"]


@pytest.mark.parametrize("name", fs.ORDER)
def test_restatement_equals_brute_force(name):
    """on 2 000 seeded queries, the face block among them: k identical, values bit for bit (both sum in (d2, row) order)"""
    sc, (want, k, vmax, _) = restated(name)
    pick = fs.sample(sc)
    assert len(pick) == fs.BRUTE_SAMPLE and np.all(pick[-10 * (sc.expect["ndim"] + 1):] >= sc.expect["n_body"])
    pick2, (got, kb, vb, _) = fs.brute_reference(name)
    assert np.array_equal(pick, pick2)
    assert np.array_equal(kb, k[pick]) and np.array_equal(vb, vmax[pick])
    assert got.tobytes() == want[pick].tobytes()
    assert int((kb > 0).sum()) > 100


@pytest.mark.parametrize("name", fs.ORDER)
def test_scene_earns_its_place(name):
    sc, (_, k, _, _) = restated(name)
    share = float((k > 0).mean())
    print(f"{name}: {share:.3f} of the queries have a neighbour, k up to {int(k.max())}")
    assert 0.05 <= share <= 0.95
    lo, hi = sc.expect.get("k_max", (1, 10 ** 6))
    assert lo <= int(k.max()) <= hi
    # the face block: the first displacement of every face and corner finds its planted row, the second does not
    s = np.asarray(sc.spacing)
    cc, _, _ = fs.check_rows(sc.flow, sc.expect["ndim"])
    nb = sc.expect["n_body"]
    fq, frow = sc.queries[nb:], sc.expect["face_rows"]
    d2 = np.zeros(len(fq))
    for ax in range(len(s)):
        d2 = d2 + (fq[:, ax] * s[ax] - cc[frow, ax] * s[ax]) ** 2
    r2 = sc.r * sc.r
    assert np.all(d2[0::5] <= r2) and np.all(k[nb:][0::5] >= 1)
    assert np.all(d2[1::5] > r2)
    if sc.expect["mult"][-1] > 1:                                    # cells wider than r: a cell edge out is out of reach
        assert np.all(d2[2::5] > r2) and np.all(d2[4::5] > 4 * r2)


def test_backward_scene():
    """`aniso_1024` backward (check coordinate position + vector): another box than forward, and as unambiguous"""
    name = "aniso_1024"
    sc, fw = fs.scene(name, False), fs.scene(name, True)
    cb, cf = fs.check_rows(sc.flow, 3, False)[0], fs.check_rows(fw.flow, 3, True)[0]
    assert np.array_equal(sc.flow, fw.flow) and not np.array_equal(cb.min(axis=0), cf.min(axis=0))
    want, k, vmax, margin = fs.reference(name, False)
    assert margin > 1e-9 and 0.05 <= float((k > 0).mean()) <= 0.95
    pick, (got, kb, vb, _) = fs.brute_reference(name, False)
    assert np.array_equal(kb, k[pick]) and got.tobytes() == want[pick].tobytes()
