"""Reading tests/golden/adjacency/*.npz (written by tests/golden/make_golden_adjacency.py) back into the reference's edge lists, and
the hierarchy double they were captured from; test infrastructure only.  A fixture `adjacency_<case>.npz` sits on the image golden
`image_<case>.npz` (tests/image_goldens.py): the double is that golden's, with the `time` list of the node golden added to its
`nodes` (the reference counts the node frames with it).  Per key of v_b, v_n, v_o, n_b, n_o, b_o the fixture holds the frames'
(m, 2) int64 arrays stacked and transposed, `<key>` (2, edges) in the smallest signed dtype that holds its values (the files stay
small that way; `load` gives int64 back), and their offsets `<key>_off` (frames + 1 entries; one entry for a list without frames)."""
import glob
import os

import numpy as np

import image_goldens as ig
from adjacency_restatement import KEYS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "adjacency")


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "adjacency_*.npz")))


def double_of_image(gi):
    """the hierarchy double of the image golden gi with what the adjacency maps read beyond it"""
    h = ig.double_of(gi)
    h.nodes.time = list(gi["components"]["branches"]["nodes"]["ref"]["time"])
    return h


def pack(lists):
    out = {}
    for key in KEYS:
        frames = [np.asarray(a, np.int64).reshape(-1, 2) for a in lists[key]]
        stacked = (np.concatenate(frames) if frames else np.zeros((0, 2), np.int64)).T
        small = next(d for d in (np.int8, np.int16, np.int32, np.int64) if stacked.size == 0 or
                     (np.iinfo(d).min <= stacked.min() and stacked.max() <= np.iinfo(d).max))
        out[key] = np.ascontiguousarray(stacked.astype(small))
        assert np.array_equal(out[key].astype(np.int64), stacked)
        out[key + "_off"] = np.cumsum([0] + [len(a) for a in frames]).astype(np.int64)
    return out


_CACHE = {}


def load(name):
    """dict: `image` (the image golden) and `ref` = {key: list of (m, 2) int64 arrays per frame}.  Read once and shared."""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    ref = {key: [np.ascontiguousarray(z[key][:, a:b].T.astype(np.int64)) for a, b in zip(z[key + "_off"][:-1], z[key + "_off"][1:])] for key in KEYS}
    out = dict(name=name, image=ig.load(str(z["base"])), ref=ref)
    _CACHE[name] = out
    return out


def double_of(g):
    return double_of_image(g["image"])
