"""CPU tests of bench.py's command line and of the files --dump-outputs writes (no GPU call)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(monkeypatch):
    # bench.py sets a default for GPU_MAX_HW_QUEUES at import; keep the test process's environment as it was
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    import bench
    return bench


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_writes_float32_and_samples_large_images(monkeypatch, tmp_path):
    bench = _bench(monkeypatch)
    rng = np.random.default_rng(5)
    big_h, big_w = 1500, 1500                                  # more pixels than DUMP_SAMPLE_PX
    assert big_h * big_w > bench.DUMP_SAMPLE_PX
    hdr = rng.uniform(-4, 4, (big_h, big_w, 4)).astype(np.float16).view(np.uint16)
    depth = np.arange(big_h * big_w, dtype=np.float32).reshape(big_h, big_w, 1)      # each pixel's own index (exact in float32)
    small = rng.integers(0, 256, (30, 20, 3), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), [("hdr", hdr), ("depth", depth), ("small", small)])
    bench.dump_outputs(str(tmp_path / "b"), [("hdr", hdr), ("depth", depth), ("small", small)])

    total = 0
    for name in ("hdr", "depth", "small"):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy")), f"{name}: not the same sample twice"
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64 << 20

    s = np.load(tmp_path / "a" / "small.npy")
    assert np.array_equal(s, small.reshape(-1, 3).astype(np.float32))
    h = np.load(tmp_path / "a" / "hdr.npy")
    d = np.load(tmp_path / "a" / "depth.npy")
    assert h.shape == (bench.DUMP_SAMPLE_PX, 4) and d.shape == (bench.DUMP_SAMPLE_PX, 1)
    # one fixed set of pixels, in ascending order, for every image of the frame's size
    rows = d[:, 0].astype(np.int64)
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(h, hdr.reshape(-1, 4)[rows].view(np.float16).astype(np.float32))
