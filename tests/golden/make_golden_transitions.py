"""
Captures tests/golden/transitions/transitions_*.npz from the reference's own `accumulate_pair_counts`
(scripts/voxel_reassignment_demo.py:15-48):

    python tests/golden/make_golden_transitions.py /path/to/nellie-reference

The script imports `nellie.im_info.verifier` and `nellie.tracking.voxel_reassignment` at its top, which the capture does not need:
stand-in modules go into sys.modules and the script file is loaded on its own; its `main()` is never called.  The function runs
with use_gpu=False: its numpy branch, `np.add.at` on a uint32 matrix.

A fixture holds only: `src_ids`, `dst_ids` (0-based, int64), `n_src`, `n_dst` and the uint32 `matrix` out.  Nothing is written unless
tests/match_transitions_restatement.py's `dense` of the table of (src_ids + 1, dst_ids + 1) equals the matrix.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import match_transitions_restatement as mr  # noqa: E402

GOLDEN_DIR = os.path.join(HERE, "transitions")


def load_accumulate(ref):
    for name, attrs in (("nellie", {}), ("nellie.im_info", {}), ("nellie.im_info.verifier", {"FileInfo": object, "ImInfo": object}),
                        ("nellie.tracking", {}), ("nellie.tracking.voxel_reassignment", {"VoxelReassigner": object})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("reference_voxel_reassignment_demo", os.path.join(ref, "scripts", "voxel_reassignment_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.accumulate_pair_counts


def cases():
    """name -> (src_ids, dst_ids, n_src, n_dst): at most 200 x 200"""
    rng = np.random.default_rng(26)
    runs = np.repeat(rng.integers(0, 40, 300), rng.integers(1, 9, 300))
    return {
        "empty": (np.zeros(0, np.int64), np.zeros(0, np.int64), 5, 7),
        "one_pair": (np.full(300, 3), np.full(300, 1), 4, 2),
        "random_200": (rng.integers(0, 200, 5000), rng.integers(0, 200, 5000), 200, 200),
        "runs_40x60": (runs, (runs * 7 + rng.integers(0, 2, len(runs))) % 60, 40, 60),
        "wide_1x150": (np.zeros(2000, np.int64), rng.integers(0, 150, 2000), 1, 150),
    }


def main():
    ref = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.environ.get("NELLIE_REFERENCE", "")
    accumulate = load_accumulate(ref)
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    for name, (src, dst, n_src, n_dst) in cases().items():
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        matrix = accumulate(src, dst, n_src, n_dst, use_gpu=False)
        table, dropped = mr.table_of(src + 1, dst + 1)
        own = mr.dense(table, n_src, n_dst)
        assert dropped == 0 and own.dtype == matrix.dtype == np.uint32 and own.shape == matrix.shape and np.array_equal(own, matrix), \
            (name, "the restatement differs from the reference")
        path = os.path.join(GOLDEN_DIR, f"transitions_{name}.npz")
        np.savez_compressed(path, src_ids=src, dst_ids=dst, n_src=np.int64(n_src), n_dst=np.int64(n_dst), matrix=matrix)
        assert os.path.getsize(path) < 200_000, (name, os.path.getsize(path))
        print(f"{name}: {len(src)} ids, {int((matrix > 0).sum())} non-zero entries, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
