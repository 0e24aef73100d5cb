"""
The launch plan of the Hessian walk (csrc/walk_plan.h) pinned on the CPU: nl_host_walk_plan -- the arithmetic every launch site, the resolve
kernel's region count and nl_ctx_info("queue_entries") share -- must return the integers recorded in tests/golden/walk_plans.json for every
geometry and switch setting of the table.  The table was recorded from the launch code as it stood before the plan existed (three launch
sites with their own arithmetic), so it pins the plan to that code, not to itself.  The library is loaded, no GPU is touched.
"""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_plans.json")


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        return json.load(f)


def _plan(row):
    from nellie_amd import hipnative
    return hipnative.host_walk_plan(row["mode"], row["shape"], tuple(row["own"]), tuple(row["planes"]), row["fast_div"], row["fast_div2"], **row["switches"])


def test_plans_equal_the_recorded_ones(table):
    from nellie_amd import hipnative
    assert table["fields"] == list(hipnative.WALK_PLAN_FIELDS)
    bad = []
    for k, row in enumerate(table["rows"]):
        got = _plan(row)
        if [got[f] for f in table["fields"]] != row["plan"]:
            bad.append((k, {f: row[f] for f in ("mode", "shape", "own", "planes", "switches")}, dict(zip(table["fields"], row["plan"])), got))
    assert not bad, f"{len(bad)} of {len(table['rows'])} plans differ from the recorded ones, the first: {bad[0]}"


def test_the_table_has_rows_on_both_sides_of_every_change_over(table):
    """What the table must hold for the test above to mean something."""
    rows = table["rows"]
    col = {f: k for k, f in enumerate(table["fields"])}
    shapes = {tuple(r["shape"]) for r in rows}
    assert {63, 64, 65, 120, 121, 130} <= {s[2] for s in shapes}                       # the 64-column tiles and the 60-column strips
    assert {3, 4, 7, 8, 15, 16, 17, 37} <= {s[1] for s in shapes}
    assert {1, 32, 33, 64, 65, 70, 128, 129, 130, 192, 193} <= {r["planes"][1] - r["planes"][0] for r in rows}
    assert any(r["planes"][0] < r["own"][0] and r["planes"][1] > r["own"][1] for r in rows)            # ghost planes
    assert {(r["mode"], r["plan"][col["family"]]) for r in rows} >= {(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (2, 2)}
    assert {r["plan"][col["tile_rows"]] for r in rows if r["plan"][col["family"]] == 0} == {8, 16}
    assert {0, 32, 64, 128} <= {r["switches"].get("NELLIE_HV_ZCHUNK", 0) for r in rows}
    # 128-plane chunks forced, chosen by the frame's size alone (above 2^26 voxels), and refused where 2 * c128 > c64
    big = [r for r in rows if r["mode"] == 2 and not r["switches"] and r["shape"][0] * r["shape"][1] * r["shape"][2] > 1 << 26]
    assert {r["plan"][col["zchunk"]] for r in big if r["plan"][col["family"]] == 1} == {64, 128}
    assert any(r["switches"].get("NELLIE_HV_ZCHUNK") == 128 and r["plan"][col["zchunk"]] == 64 and r["plan"][col["family"]] == 1 and r["mode"] == 2 for r in rows)
    # the wave-autonomous walk asked for and refused (the queue cannot be shared out): the pair kernel's plan
    assert any(r["switches"].get("NELLIE_HV_DPP") == 1 and r["mode"] == 2 and r["plan"][col["family"]] == 1 for r in rows)
    # several known-threshold launches: a queue of exactly one chunk's entries
    assert any(r["mode"] == 1 and "NELLIE_VQ_CAP" in r["switches"] and r["plan"][col["launch_planes"]] == 64 < r["planes"][1] - r["planes"][0] for r in rows)
    # a chunk of 2^32 bytes and more selects the one-voxel kernel without a switch
    assert any(not r["switches"] and r["plan"][col["family"]] == 0 and 68 * r["shape"][1] * r["shape"][2] * 4 >= 1 << 32 for r in rows)


def test_bad_arguments_are_refused():
    from nellie_amd import hipnative
    for kw in (dict(mode=3, shape=(8, 8, 8)), dict(mode=2, shape=(8, 0, 8)), dict(mode=2, shape=(8, 8, 8), own=(4, 4)),
               dict(mode=1, shape=(8, 8, 8), planes=(0, 9))):
        with pytest.raises(ValueError):
            hipnative.host_walk_plan(**kw)
