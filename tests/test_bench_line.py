"""bench.py at N = 1: a plain run prints the headline line only (the rest of the figures are behind --full), and --dump-outputs
writes what the last timed step computed -- equal to the same frame run through FramePipeline directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (24, 48, 48)


def test_plain_run_is_the_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    args = bench.parse_args()
    assert not args.full and args.dump_outputs is None and args.steps == 4 and args.warmup == 2


def test_dump_outputs_refuses_more_than_one_gpu():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    proc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--dump-outputs", "unused"],
                          env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode != 0 and "--dump-outputs" in proc.stderr


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--shape", *map(str, SHAPE), "--dump-outputs", str(out_dir)]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-1200:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-600:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mvoxel/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["roofline"] is None and line["cpu_baseline"] is None and "io" not in line and "accuracy" not in line

    fr, lab, n = (np.load(out_dir / f"{k}.npy") for k in ("frangi", "labels", "n_labels"))
    assert fr.dtype == np.float32 and lab.dtype == np.float64 and n.dtype == np.float64
    assert fr.shape == SHAPE and lab.shape == SHAPE and n.shape == (1,)

    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    pipe = pl.FramePipeline(SHAPE)
    pipe.load_input(make_volume(SHAPE, 2345))
    pipe.filter(None, pl.FilterParams(dim_res=ISO_01))
    n_ref = pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
    fr_ref, lab_ref = pipe.download_frangi(), pipe.download_labels()
    pipe.close()
    assert np.array_equal(fr, fr_ref) and np.array_equal(lab, lab_ref.astype(np.float64)) and int(n[0]) == n_ref
    assert int(n[0]) == line["config"]["labels"]
