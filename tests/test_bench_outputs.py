"""bench.py --dump-outputs: the frames of the last timed step as float32 B, G, R planes, whole when
they fit bench.DUMP_BUDGET and as one fixed seeded pixel sample otherwise; and a plain run's result
line (no --full): the timed steps alone."""
import hashlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _repack(bgr):
    """The BGRA8 words (alpha 0) of a dumped [..., 3] float32 array."""
    b = bgr.astype(np.uint32)
    return b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16


def _fake_work(scenes, w, h, nsets, last_set, seed=5):
    rng = np.random.default_rng(seed)
    px = [[rng.integers(0, 1 << 24, w * h, dtype=np.uint32) for _ in scenes] for _ in range(nsets)]
    work = types.SimpleNamespace(
        scenes=[(sid, None, None, None) for sid in scenes], last_set=last_set,
        bufs=[[torch.from_numpy(p.view(np.int32)) for p in s] for s in px])
    return work, px


def test_dump_outputs_whole_frames(tmp_path, monkeypatch):
    """Frames within the budget: [H, W, 3] float32 of the set the last step rendered into."""
    monkeypatch.setattr(bench, "SCENES", (1, 8))
    monkeypatch.setattr(bench, "W", 37)
    monkeypatch.setattr(bench, "H", 11)
    work, px = _fake_work((1, 8), 37, 11, 2, last_set=1)
    bench.dump_outputs(work, 1, str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["scene1.npy", "scene8.npy"]
    for i, sid in enumerate((1, 8)):
        a = np.load(tmp_path / "out" / f"scene{sid}.npy")
        assert a.dtype == np.float32 and a.shape == (11, 37, 3)
        np.testing.assert_array_equal(_repack(a).reshape(-1), px[1][i])


def test_dump_outputs_sampled(tmp_path, monkeypatch):
    """Frames over the budget: the same seeded, ascending pixel sample of every frame, the files
    together within the budget, and the same sample on a second run."""
    monkeypatch.setattr(bench, "SCENES", (0, 1, 2))
    monkeypatch.setattr(bench, "W", 64)
    monkeypatch.setattr(bench, "H", 48)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 * (1024 + 12 * 1000))
    work, px = _fake_work((0, 1, 2), 64, 48, 1, last_set=0)
    bench.dump_outputs(work, 1, str(tmp_path / "a"))
    bench.dump_outputs(work, 1, str(tmp_path / "b"))
    idx = np.sort(np.random.default_rng(0).choice(64 * 48, 1000, replace=False))
    total = 0
    for i, sid in enumerate((0, 1, 2)):
        a = np.load(tmp_path / "a" / f"scene{sid}.npy")
        assert a.dtype == np.float32 and a.shape == (1000, 3)
        np.testing.assert_array_equal(_repack(a), px[0][i][idx])
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f"scene{sid}.npy"))
        total += os.path.getsize(tmp_path / "a" / f"scene{sid}.npy")
    assert total <= bench.DUMP_BUDGET


@pytest.mark.gpu
def test_bench_plain_run_dumps_reference_frames(tmp_path, golden):
    """A plain one-GPU run: --steps sets the timed steps, the line carries the headline fields and
    none of the --full legs, and the frames its last timed step rendered (the overlapped one launch
    per frame on two streams) are the reference renderer's 1920x1080x4 frames, byte for byte."""
    out_dir = tmp_path / "frames"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("{")))
    assert out["steps"] == 3 and out["warmup"] == 2 and out["full"] is False
    assert out["unit"] == "Msamples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 1920 * 1080 * 4 / out["ms_per_step"] / 1e3) <= 1e-3 * out["value"]
    for k in ("end_to_end", "moving_camera", "one_stream", "per_scene_steps", "first_frame_ms", "distributed"):
        assert k not in out
    assert out["roofline"] is None and out["cpu_baseline"] is None
    for sid in (1, 8):
        a = np.load(out_dir / f"scene{sid}.npy")
        assert a.dtype == np.float32 and a.shape == (1080, 1920, 3)
        assert hashlib.sha256(_repack(a).tobytes()).hexdigest() == golden["frames_1080p4"][str(sid)]["bgra_sha256"]
