"""bench.py's command line: a plain run is the headline figure alone, --full
switches the other legs on, --dump-outputs writes the last timed step's
frame and counters as .npy files (whole, or a fixed seeded sample above the
size limit)."""
from __future__ import annotations

import importlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    return importlib.import_module("bench")


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    b = bench.parse()
    assert b.full and b.dump_outputs == "somewhere"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_whole_frame(tmp_path):
    import torch
    bench = _bench()
    rows, w = 5, 7
    frame = torch.arange(rows * w * 3, dtype=torch.float32) / 8
    names = bench.dump_outputs(tmp_path / "o", frame, rows, w, 300, 100, 4, 0, 1)
    assert names == ["counters.npy", "frame.npy"]
    f = np.load(tmp_path / "o" / "frame.npy")
    assert f.dtype == np.float32 and f.shape == (rows, w, 3) and np.array_equal(f.ravel(), frame.numpy())
    c = np.load(tmp_path / "o" / "counters.npy")
    assert c.dtype == np.float64 and c.tolist() == [75.0, 25.0]
    # rank 1 of 2 names its own files
    assert bench.dump_outputs(tmp_path / "o", frame, rows, w, 300, 100, 4, 1, 2) == \
        ["counters_rank1.npy", "frame_rank1.npy"]


def test_dump_outputs_samples_a_frame_above_the_limit(tmp_path, monkeypatch):
    import torch
    bench = _bench()
    rows, w = 64, 96   # 73,728 bytes of pixels against a 40,000-byte limit
    monkeypatch.setattr(bench, "DUMP_LIMIT", 40000)
    frame = torch.arange(rows * w * 3, dtype=torch.float32)
    for d in ("a", "b"):
        names = bench.dump_outputs(tmp_path / d, frame, rows, w, 10, 10, 1, 0, 1)
        assert names == ["counters.npy", "frame_sample.npy", "frame_sample_index.npy"]
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    idx = got["frame_sample_index.npy"]
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < rows * w
    px = got["frame_sample.npy"]
    assert px.dtype == np.float32 and px.shape == (len(idx), 3)
    assert np.array_equal(px, frame.numpy().reshape(-1, 3)[idx.astype(np.int64)])
    assert len(idx) > rows * w // 4   # most of the limit is used
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 40000
    # the same pixels on every run
    assert all(np.array_equal(got[n], np.load(tmp_path / "b" / n)) for n in names)


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_frame(gpu_lib, tmp_path):
    """One plain bench.py process on a light frame (C1 at 2 spp): the line
    carries the headline fields and none of --full's legs, and the dumped
    frame and counters are rt_render's of the same scene, camera and seed."""
    from rtclj import raytracing as R
    from rtclj import scenes
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--spp", "2", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "Mray-samples/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(1200 * 675 * 2 / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-6)
    for leg in ("pipelined", "sustained", "stats_build", "end_to_end", "cpu_baseline", "parity"):
        assert d[leg] is None, leg
    assert d["dispatch_order"]["kernel_ms"] is None
    assert d["outputs"]["files"] == ["counters.npy", "frame.npy"]
    frame = np.load(out / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (675, 1200, 3)
    st = {}
    ref = R.render(scenes.cover(11, 42), scenes.cover_camera(1200, 675), 1200, 675, 2, 50, seed=1,
                   n_devices=1, stats=st)
    assert np.array_equal(frame, ref)
    assert np.load(out / "counters.npy").tolist() == [float(st["segments"]), float(st["samples"])]
