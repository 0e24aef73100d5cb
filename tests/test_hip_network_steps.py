"""The Network stage behind the thinning on the MI355X (nellie_amd.segmentation.networking.Network): every product is compared for
equality -- integers, no tolerance, nothing left out -- with the reference's recorded steps (tests/golden/network_steps) and with the
numpy restatement (tests/network_steps_restatement.py), whose feature transform tests/test_network_steps_cpu.py holds against scipy."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import network_scenes as scenes  # noqa: E402
import network_steps_restatement as rs  # noqa: E402
from test_network_steps_cpu import STEP_CASES, load_steps  # noqa: E402

pytestmark = pytest.mark.gpu

ISO, ANISO_03, ANISO_029 = (1.0, 1.0, 1.0), (0.3, 0.1, 0.1), (0.29, 0.11, 0.11)
SPACINGS = [ISO, ANISO_03, ANISO_029]


def network(spacing, **kw):
    from nellie_amd.segmentation.networking import Network
    ndim = len(spacing)
    info = scenes.network_im_info(np.zeros((1,) + (2,) * ndim, np.int32), np.zeros((1,) + (2,) * ndim, np.float32), spacing)
    return Network(info, **kw)


# ---- 1. the reference's recorded steps, through files ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STEP_CASES)
def test_goldens_through_network_on_files(name):
    from nellie_amd.segmentation.networking import Network
    g = load_steps(name)
    info = scenes.network_im_info(g["labels"][None], g["frangi"][None], tuple(g["spacing"]))
    status = type("Viewer", (), {"status": ""})()
    net = Network(info, viewer=status, skeletonize=lambda mask: g["skel_mask"].copy())
    net.run()
    assert sorted(info.created) == ["pixel_class", "skel", "skel_relabelled"]
    skel, pc, rel = info.store["skel"], info.store["pixel_class"], info.store["skel_relabelled"]
    assert (skel.dtype, pc.dtype, rel.dtype) == (np.int32, np.uint8, np.uint32)
    assert np.array_equal(skel[0], g["frame_branch"]) and np.array_equal(pc[0], g["frame_pixel_class"])
    assert np.array_equal(rel[0], g["frame_relabelled"])
    assert status.status == "Extracting branches. Frame: 1 of 1."
    assert len(net.kernel_ms) == 1 and set(net.kernel_ms[0]) >= {"clean", "seed", "classes", "relabel"}
    assert net.frame_stats[0]["n_removed"] == int(g["n_removed"]) and net.frame_stats[0]["n_seeded"] == int(g["n_seeded"])


# ---- 2. relabel scenes against the restatement -------------------------------------------------------------------------------------------
def _seed_branches(rng, labels, positions):
    """Branch labels: a different id per seed position (a list of index tuples), kept where the voxel belongs to an object."""
    branch = np.zeros(labels.shape, np.int32)
    ids = rng.permutation(len(positions)) + 1
    for k, p in zip(ids, positions):
        if labels[p] > 0:
            branch[p] = k
    return branch


def nested_ls(shape=(3, 30, 30), n=4, step=1):
    """n nested L-shaped objects (a column and a row each), every one's box inside the one before: the boxes overlap, each is more
    than half the frame.  Several branches per object: seeds along both arms."""
    nz, ny, nx = shape
    labels = np.zeros(shape, np.int32)
    seeds = []
    for k in range(n):
        o = k * step
        labels[:, o:ny - o, o] = k + 1
        labels[:, ny - 1 - o, o:nx] = k + 1
        seeds += [(k % nz, o + 1 + 5 * j, o) for j in range(4)] + [((k + 1) % nz, ny - 1 - o, o + 3 + 6 * j) for j in range(4)]
    return labels, seeds


def scene_overlapping(rng):
    labels, seeds = nested_ls()
    return labels, _seed_branches(rng, labels, seeds)


def scene_whole_frame(rng):
    shape = (8, 22, 26)
    labels = np.zeros(shape, np.int32)
    labels[0], labels[-1], labels[:, 0], labels[:, -1], labels[:, :, 0], labels[:, :, -1] = 1, 1, 1, 1, 1, 1       # a shell: its box is the frame
    labels[2:5, 3:8, 4:9] = 2
    labels[3:6, 10:18, 12:20] = 3
    labels[3, 4, 15] = 4
    pos = [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(400)]
    return labels, _seed_branches(rng, labels, pos)


def scene_long_line(rng, axis):
    shape = tuple([5, 7][:axis] + [300] + [5, 7][axis:])                # 300 x 5 x 7, 5 x 300 x 7, 5 x 7 x 300
    labels = np.zeros(shape, np.int32)
    bar = [slice(1, 4)] * 3
    bar[axis] = slice(None)
    labels[tuple(bar)] = 1
    seeds = []
    for p in scenes.irregular_seeds(rng, 300):
        idx = [int(rng.integers(1, 4)) for _ in range(3)]
        idx[axis] = p
        seeds.append(tuple(idx))
    return labels, _seed_branches(rng, labels, seeds)


def scene_label_gaps(rng):
    shape = (6, 20, 24)
    labels = np.zeros(shape, np.int32)
    labels[1:4, 2:9, 2:10] = 1
    labels[2:5, 6:14, 8:16][labels[2:5, 6:14, 8:16] == 0] = 2
    labels[0:6, 12:20, 3:9] = 7
    labels[1:5, 10:19, 14:23][labels[1:5, 10:19, 14:23] == 0] = 1000
    pos = [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(150)]
    return labels, _seed_branches(rng, labels, pos)


def scene_single_voxels(rng):
    shape = (5, 9, 11)
    labels = np.zeros(shape, np.int32)
    cells = [(z, y, x) for z in range(0, 5, 2) for y in range(0, 9, 2) for x in range(0, 11, 2)]
    for k, c in enumerate(cells):
        labels[c] = k + 1
    return labels, _seed_branches(rng, labels, [c for k, c in enumerate(cells) if k % 4])


def scene_symmetric(rng):
    """One 9^3 block; seeds at the corners, the face centres and pairs mirrored about the centre: under isotropic spacing most voxels
    are equidistant from several seeds, in every axis pass."""
    shape = (11, 11, 11)
    labels = np.zeros(shape, np.int32)
    labels[1:10, 1:10, 1:10] = 1
    pos = [(z, y, x) for z in (1, 9) for y in (1, 9) for x in (1, 9)]
    pos += [(1, 5, 5), (9, 5, 5), (5, 1, 5), (5, 9, 5), (5, 5, 1), (5, 5, 9), (3, 3, 5), (7, 7, 5), (3, 5, 7), (7, 5, 3)]
    return labels, _seed_branches(rng, labels, pos)


SCENES = {"overlapping": scene_overlapping, "whole_frame": scene_whole_frame, "long_z": functools.partial(scene_long_line, axis=0),
          "long_y": functools.partial(scene_long_line, axis=1), "long_x": functools.partial(scene_long_line, axis=2),
          "label_gaps": scene_label_gaps, "single_voxels": scene_single_voxels, "symmetric": scene_symmetric}


@functools.lru_cache(maxsize=None)
def scene(name):
    labels, branch = SCENES[name](np.random.default_rng([len(name), 7]))
    labels.setflags(write=False)
    branch.setflags(write=False)
    return labels, branch


@functools.lru_cache(maxsize=None)
def expected(name, spacing):
    labels, branch = scene(name)
    out, n_obj, vol = rs.relabel(branch, labels, spacing)
    out.setflags(write=False)
    return out, n_obj, vol


def device_relabel(labels, branch, spacing, scratch_voxels=None):
    from nellie_amd import hipnative
    shape = (1,) * (3 - labels.ndim) + labels.shape
    with hipnative.Context(shape) as ctx:
        ctx.network_relabel_load(labels, branch)
        stats = ctx.network_relabel(spacing, scratch_voxels)
        return ctx.network_fetch(branch=False, pixel_class=False)[2], stats


@pytest.mark.parametrize("spacing", SPACINGS, ids=["iso", "aniso03", "aniso029"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_relabel_scene_equals_the_restatement(name, spacing):
    labels, branch = scene(name)
    want, n_obj, vol = expected(name, spacing)
    got, (objs, box_volume, batches) = device_relabel(labels, branch, spacing)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert (objs, box_volume) == (n_obj, vol) and batches == (1 if n_obj else 0)
    assert not got[labels == 0].any()


def test_symmetric_scene_has_ties_in_every_pass():
    """The scene is only worth its name if picking another of the equidistant seeds changes the result."""
    labels, branch = scene("symmetric")
    want = expected("symmetric", ISO)[0]
    flipped = rs.relabel(branch[::-1, ::-1, ::-1], labels[::-1, ::-1, ::-1], ISO)[0][::-1, ::-1, ::-1]
    assert (flipped != want).sum() > 50


def test_relabel_function_form_and_2d():
    from nellie_amd.segmentation.networking import relabel_objects
    rng = np.random.default_rng(3)
    labels = np.zeros((40, 52), np.int32)
    labels[2:20, 3:30] = 1
    labels[15:38, 20:50][labels[15:38, 20:50] == 0] = 2
    labels[30:36, 2:9] = 3                                            # no seed
    pos = [(int(rng.integers(0, 30)), int(rng.integers(10, 52))) for _ in range(60)]
    branch = _seed_branches(rng, labels, pos)
    for sp in ((1.0, 1.0), (0.107, 0.083), (2.5, 1.0)):
        want = rs.relabel(branch, labels, sp)[0]
        assert want[labels == 3].max() == 0 and want[labels == 1].min() > 0
        assert np.array_equal(relabel_objects(branch, labels, sp), want)


@pytest.mark.parametrize("seedless_every", [0, 3])
def test_many_single_voxel_objects(seedless_every):
    """72 900 objects, more than a grid dimension holds: each is its own seed and keeps its own branch label."""
    labels = np.zeros((540, 540), np.int32)
    labels[::2, ::2] = np.arange(1, 270 * 270 + 1, dtype=np.int32).reshape(270, 270)
    rng = np.random.default_rng(11)
    branch = np.zeros_like(labels)
    ids = rng.permutation(270 * 270).astype(np.int32) + 1
    branch[::2, ::2] = ids.reshape(270, 270)
    if seedless_every:
        branch[labels % seedless_every == 0] = 0
    got, (objs, vol, batches) = device_relabel(labels, branch, (0.11, 0.11))
    assert np.array_equal(got, branch.astype(np.uint32))              # what the reference does with one-voxel crops
    assert objs == vol == int((branch > 0).sum()) and batches == 1
    some = np.zeros_like(labels)                                      # and the restatement itself, on a corner of the lattice
    some[:40, :40] = labels[:40, :40]
    assert np.array_equal(rs.relabel(branch, some, (0.11, 0.11))[0][:40, :40], got[:40, :40])


# ---- 3. batching ------------------------------------------------------------------------------------------------------------------------
def _greedy_batches(volumes, budget):
    n, used = 0, None
    for v in volumes:
        if used is None or used + v > budget:
            n, used = n + 1, 0
        used += v
    return n


def test_batches_do_not_change_the_result():
    labels, branch = scene("overlapping")
    want, n_obj, vol = expected("overlapping", ANISO_029)
    volumes = [rs.ndi.find_objects(labels)[k] for k in range(n_obj)]
    volumes = [int(np.prod([s.stop - s.start for s in sl])) for sl in volumes]
    assert sum(volumes) == vol and min(volumes) > labels.size // 2      # at the floor, one frame, no two objects share a batch
    floor_out, (_, _, floor_batches) = device_relabel(labels, branch, ANISO_029, scratch_voxels=1)
    assert floor_batches == n_obj == 4 and np.array_equal(floor_out, want)
    three = next(b for b in range(labels.size, vol + 1) if _greedy_batches(volumes, b) == 3)
    out3, (_, _, batches3) = device_relabel(labels, branch, ANISO_029, scratch_voxels=three)
    assert batches3 == 3 and np.array_equal(out3, want)
    whole, (_, _, one) = device_relabel(labels, branch, ANISO_029, scratch_voxels=vol)
    assert one == 1 and np.array_equal(whole, want)


# ---- 4. clean and seed edge cases ----------------------------------------------------------------------------------------------------
def _frame_equals_restatement(net, labels, mask, frangi):
    assert rs.unique_maxima(labels, frangi)
    want = rs.frame(labels, mask, frangi, net.scaling)
    branch, pc, rel = net.frame(labels, frangi, skel_mask=mask)
    assert np.array_equal(branch, want["branch"]) and np.array_equal(pc, want["pixel_class"]) and np.array_equal(rel, want["relabelled"])
    assert np.array_equal(pc > 0, want["skel_seeded"] > 0)
    return want, net.frame_stats[-1]


@pytest.mark.parametrize("shape", [(5, 6, 7), (6, 9)], ids=["3d", "2d"])
def test_ambiguous_voxels_stay_on_the_faces_and_go_one_voxel_in(shape):
    rng = np.random.default_rng(5)
    labels = (1 + np.indices(shape).sum(0) % 2).astype(np.int32)       # a checkerboard of two labels: every voxel is ambiguous
    mask = np.ones(shape, bool)
    net = network(ANISO_029[3 - len(shape):])
    want, stats = _frame_equals_restatement(net, labels, mask, scenes.unique_frangi(rng, shape))
    inner = np.zeros(shape, bool)
    inner[(slice(1, -1),) * len(shape)] = True
    assert np.array_equal(want["skel_clean"] > 0, ~inner)               # every face, edge and corner kept; everything inside gone
    assert stats["n_removed"] == int(inner.sum()) and stats["n_seeded"] == 0
    net.close()


@pytest.mark.parametrize("shape", [(5, 8, 9), (8, 9)], ids=["3d", "2d"])
def test_a_label_that_loses_its_skeleton_is_seeded_again(shape):
    rng = np.random.default_rng(6)
    labels = np.ones(shape, np.int32)
    labels[..., shape[-1] // 2:] = 2
    mask = np.zeros(shape, bool)
    mid = tuple(s // 2 for s in shape[:-1])
    mask[mid + (shape[-1] // 2 - 1,)] = mask[mid + (shape[-1] // 2,)] = True      # two skeleton voxels, neighbours across the border
    frangi = scenes.unique_frangi(rng, shape)
    net = network(ISO[3 - len(shape):])
    want, stats = _frame_equals_restatement(net, labels, mask, frangi)
    assert stats["n_removed"] == 2 and stats["n_seeded"] == 2
    for L in (1, 2):
        at = np.flatnonzero((want["skel_seeded"] == L).ravel())
        assert at.size == 1 and at[0] == np.flatnonzero(labels.ravel() == L)[np.argmax(frangi.ravel()[labels.ravel() == L])]
    net.close()


@pytest.mark.parametrize("shape", [(4, 6, 9), (7, 9)], ids=["3d", "2d"])
def test_seeds_at_the_first_the_last_and_an_inner_voxel(shape):
    rng = np.random.default_rng(7)
    n = int(np.prod(shape))
    labels = np.zeros(n, np.int32)
    labels[:n // 3], labels[n // 3 + 2:2 * n // 3], labels[2 * n // 3 + 2:] = 1, 2, 3
    frangi = scenes.unique_frangi(rng, (n,)) * np.float32(0.5)
    inner = n // 2
    frangi[0], frangi[inner], frangi[n - 1] = 0.75, 0.875, 1.0
    labels, frangi = labels.reshape(shape), frangi.reshape(shape)
    net = network(ANISO_03[3 - len(shape):])
    want, stats = _frame_equals_restatement(net, labels, np.zeros(shape, bool), frangi)
    assert stats["n_seeded"] == 3
    assert np.array_equal(np.flatnonzero(want["skel_seeded"].ravel()), [0, inner, n - 1])
    net.close()


# ---- 5. residency and determinism -------------------------------------------------------------------------------------------------------
def test_one_handle_many_frames():
    ga, gb = load_steps("net_3d_seeding"), load_steps("net_3d_seedless")
    assert ga["labels"].shape == gb["labels"].shape
    net = network(tuple(ga["spacing"]))
    first = net.frame(ga["labels"], ga["frangi"], skel_mask=ga["skel_mask"])
    net.scaling = tuple(gb["spacing"])
    second = net.frame(gb["labels"], gb["frangi"], skel_mask=gb["skel_mask"])
    net.scaling = tuple(ga["spacing"])
    again = net.frame(ga["labels"], ga["frangi"], skel_mask=ga["skel_mask"])
    for got, g in ((first, ga), (second, gb), (again, ga)):
        assert np.array_equal(got[0], g["frame_branch"]) and np.array_equal(got[1], g["frame_pixel_class"])
        assert np.array_equal(got[2], g["frame_relabelled"])
    assert len(net.kernel_ms) == 3
    net.close()


def test_uneven_frames_of_a_stack_and_repeat_runs():
    from nellie_amd.segmentation.networking import Network
    shape, sp = (9, 30, 34), ANISO_029
    rng = np.random.default_rng(8)
    frames = [scenes.walks_scene(rng, shape, n_obj=7, drop=2), (np.zeros(shape, np.int32), np.zeros(shape, bool), scenes.unique_frangi(rng, shape)),
              scenes.walks_scene(rng, shape, n_obj=2, blocks=2), scenes.walks_scene(rng, shape, n_obj=4, touching=True)]
    labels = np.stack([f[0] for f in frames]).astype(np.uint16)       # an integer dtype that is not int32
    frangi = np.stack([f[2] for f in frames])
    masks = {f[0].tobytes(): f[1] for f in frames}
    outs = []
    for _ in range(2):
        info = scenes.network_im_info(labels, frangi, sp)
        net = Network(info, skeletonize=lambda m: masks[next(f[0] for f in frames if np.array_equal(f[0] > 0, m)).tobytes()])
        net.run()
        outs.append([np.array(info.store[k]) for k in ("skel", "pixel_class", "skel_relabelled")])
        assert len(net.kernel_ms) == 4
    for t, (lab, mask, fr) in enumerate(frames):
        want = rs.frame(lab, mask, fr, sp, transform=rs.scipy_transform)
        for got, key in zip(outs[0], ("branch", "pixel_class", "relabelled")):
            assert np.array_equal(got[t], want[key]), (t, key)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    info = scenes.network_im_info(labels, frangi, sp)
    net = Network(info, num_t=2, skeletonize=lambda m: masks[next(f[0] for f in frames if np.array_equal(f[0] > 0, m)).tobytes()])
    net.run()
    assert np.array_equal(info.store["skel_relabelled"][:2], outs[0][2][:2]) and not info.store["skel_relabelled"][2:].any()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    shape = (4, 6, 8)
    rng = np.random.default_rng(9)
    labels = np.zeros(shape, np.int64)
    labels[1:3, 2:5, 2:6] = 1
    mask, frangi = np.zeros(shape, bool), scenes.unique_frangi(rng, shape)
    net = network(ISO)
    big = labels.copy()
    big[0, 0, 0] = 1 << 31
    with pytest.raises(ValueError, match="refusing a cast"):
        net.frame(big, frangi, skel_mask=mask)
    with pytest.raises(ValueError, match="refusing a cast"):
        net.frame(big.astype(np.uint32), frangi, skel_mask=mask)
    with pytest.raises(ValueError, match="refusing a cast"):
        net.frame(labels + 0.5, frangi, skel_mask=mask)
    with pytest.raises(ValueError, match="not negative"):
        net.frame(-labels, frangi, skel_mask=mask)
    with pytest.raises(ValueError, match="shape"):
        net.frame(labels, frangi[:, :, :-1], skel_mask=mask)
    with pytest.raises(ValueError, match="shape"):
        net.frame(labels, frangi, skel_mask=mask[1:])
    with pytest.raises(ValueError, match="shape"):
        net.frame(labels[0], frangi[0], skel_mask=mask[0])                # a 2-D frame on a 3-D stage
    net.skeletonize = lambda m: m[:, :, 1:]
    with pytest.raises(ValueError, match="skeletonize returned shape"):
        net.frame(labels, frangi)
    net.skeletonize, net._thin = None, None
    ok = net.frame(labels, frangi, skel_mask=mask)                        # the handle still works after every refusal
    want = rs.frame(labels, mask, frangi, ISO)
    assert np.array_equal(ok[2], want["relabelled"]) and np.array_equal(ok[0], want["branch"])
    net.close()
