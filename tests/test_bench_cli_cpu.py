"""CPU: bench.py's options that need no GPU -- the secondary measurements need --full, and --dump-outputs keeps a batch
of waveforms under its size limit as a fixed sample of whole rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("args", [["--latency-b1", "10"], ["--cpu-utts", "2"], ["--detail", "x.txt"], ["--steps", "0"]])
def test_rejected_without_full(args):
    r = subprocess.run([sys.executable, "bench.py", *args], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "error" in r.stderr, r.stderr


def test_dump_outputs_sample_and_mask(tmp_path):
    B, F = 64, 422  # the headline batch: 64 rows of 600 * F float32 samples exceed the limit
    rng = np.random.default_rng(5)
    audio = rng.standard_normal((B, 600 * F), dtype=np.float32)
    frames = np.full(B, F, dtype=np.int32)
    frames[3] = F - 10  # a shorter row: its tail is not the caller's
    bench.dump_outputs(str(tmp_path / "a"), audio, frames)
    bench.dump_outputs(str(tmp_path / "b"), audio, frames)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 10 ** 6
    a, rows = np.load(tmp_path / "a" / "audio.npy"), np.load(tmp_path / "a" / "audio_rows.npy")
    assert a.dtype == np.float32 and rows.dtype == np.float64 and len(rows) == a.shape[0] < B
    assert (np.diff(rows) > 0).all() and np.array_equal(rows, np.load(tmp_path / "b" / "audio_rows.npy"))
    ri = rows.astype(int)
    for i, r in enumerate(ri):
        n = 600 * frames[r]
        assert np.array_equal(a[i, :n], audio[r, :n]) and not a[i, n:].any()
    assert np.array_equal(np.load(tmp_path / "a" / "frames.npy"), frames.astype(np.float64))


def test_synthetic_blob_outside_an_unwritable_tree(tmp_path, monkeypatch):
    """A checkout the benchmarking user cannot write: the weight file goes to the user's cache, whole, and is reused."""
    from kokorox_amd import weights as W
    (tmp_path / "ro").write_text("")  # a file where the package's directory would be: it cannot be created
    monkeypatch.setenv("KOKOROX_AMD_CACHE", str(tmp_path / "ro" / "build"))
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "cache"))
    p = bench.synthetic_blob()
    assert p == str(tmp_path / "cache" / "kokorox_amd" / os.path.basename(W.default_blob_path()))
    assert os.listdir(os.path.dirname(p)) == [os.path.basename(p)]  # no temporary left behind
    assert sum(a.size for a in W.read_blob(p).values()) > 80e6
    t = os.path.getmtime(p)
    assert bench.synthetic_blob() == p and os.path.getmtime(p) == t
