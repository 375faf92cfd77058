"""bench.py --dump-outputs: the file layout of a dumped frame (float32 bytes of
each pixel word, the stored rows' global indices), the size limit's fixed row
sample, and the options' defaults (a plain run is not --full)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _capture(n, w, seed=3):
    img = np.random.default_rng(seed).integers(0, 2 ** 32, size=(n, w), dtype=np.uint32)
    return 7, 4 * np.arange(n), img


def test_dump_outputs_whole_frame(tmp_path):
    import bench
    cap = _capture(24, 40)
    d = str(tmp_path / "out" / "dir")
    bench.dump_outputs(d, cap)
    assert sorted(os.listdir(d)) == ["frame.npy", "frame_rows.npy"]
    f, rows = np.load(os.path.join(d, "frame.npy")), np.load(os.path.join(d, "frame_rows.npy"))
    assert f.dtype == np.float32 and f.shape == (24, 40, 4) and rows.dtype == np.float64
    assert np.array_equal(rows, cap[1])
    # the four bytes of each word, in memory order, exactly
    assert np.array_equal(f.astype(np.uint8).reshape(24, 160).view(np.uint32), cap[2])


def test_dump_outputs_row_sample_is_fixed_and_within_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096 + 10 * (40 * 16 + 8))
    cap = _capture(24, 40)
    for k in "ab":
        bench.dump_outputs(str(tmp_path / k), cap)
    fa, ra = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "frame_rows.npy")
    assert fa.shape == (10, 40, 4) and np.all(np.diff(ra) > 0)
    assert fa.nbytes + ra.nbytes <= bench.DUMP_MAX_BYTES
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= bench.DUMP_MAX_BYTES
    assert np.array_equal(fa.astype(np.uint8).reshape(10, 160).view(np.uint32), cap[2][(ra // 4).astype(int)])
    assert np.array_equal(fa, np.load(tmp_path / "b" / "frame.npy"))
    assert np.array_equal(ra, np.load(tmp_path / "b" / "frame_rows.npy"))


def test_default_limit_holds_the_headline_frame():
    import bench
    assert bench.DUMP_MAX_BYTES <= 64 * 10 ** 6
    assert 1080 * (1920 * 16 + 8) + 4096 <= bench.DUMP_MAX_BYTES     # 1920x1080 is dumped whole


def test_plain_run_is_not_full(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "x"
