"""bench.py's command line: a plain run times the headline leg only, --full adds the other legs,
--dump-outputs writes the last timed step's accumulator as float32 .npy files."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

torch = pytest.importorskip("torch")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_options(monkeypatch, tmp_path):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--no-pt", "--dump-outputs", str(tmp_path))
    assert a.full and a.no_pt and a.dump_outputs == str(tmp_path)
    with pytest.raises(SystemExit):  # the leg choices belong to --full: a plain run is the C3 path trace
        _parse(monkeypatch, "--no-pt")


def test_dump_output_whole_array(tmp_path):
    t = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    bench.dump_output(str(tmp_path / "d"), "radiance", t)
    assert sorted(os.listdir(tmp_path / "d")) == ["radiance.npy"]
    a = np.load(tmp_path / "d" / "radiance.npy")
    assert a.dtype == np.float32 and np.array_equal(a, t.numpy())


def test_dump_output_samples_rows_over_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 8 * 4)  # ten rows of eight floats
    t = torch.arange(37 * 8, dtype=torch.float32).reshape(37, 8)
    for d in ("a", "b"):
        bench.dump_output(str(tmp_path / d), "x", t)
    a, rows = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "x_rows.npy")
    assert a.dtype == np.float32 and rows.dtype == np.float64
    assert a.nbytes + rows.nbytes <= 10 * 8 * 4 + 10 * 8 and a.shape == (10, 8)
    idx = rows.astype(np.int64)
    assert len(set(idx.tolist())) == 10 and np.array_equal(a, t.numpy()[idx])
    assert np.array_equal(a, np.load(tmp_path / "b" / "x.npy"))  # the same rows every run
    assert np.array_equal(rows, np.load(tmp_path / "b" / "x_rows.npy"))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_accumulator(monkeypatch, capsys, tmp_path, native_lib):
    """A plain run at a small frame: --steps timed steps, ms_per_step in the line, none of --full's legs,
    the accumulator of the last step in radiance.npy."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    W, H = 96, 64
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--width", str(W),
                                      "--height", str(H), "--spp", "2", "--triangles", "170000",
                                      "--dump-outputs", str(tmp_path / "out")])
    bench.main()
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "Mrays/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["metric"] == bench.METRIC
    # rays of the two timed steps only (2 spp each): at least one extension ray per sample
    assert d["rays_per_step"] >= W * H * 2
    for leg in ("roofline", "pt_wavefront", "viewer_1spp", "bvh_gpu", "gs", "hybrid", "c1", "torus", "capture", "c5",
                "cpu_baseline"):
        assert leg not in d
    assert os.listdir(tmp_path / "out") == ["radiance.npy"]
    a = np.load(tmp_path / "out" / "radiance.npy")
    assert a.dtype == np.float32 and a.shape == (H, W, 4)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
