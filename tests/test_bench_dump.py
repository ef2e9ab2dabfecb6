"""bench.py --dump-outputs without a GPU: the writer keeps whole arrays under its 64 MB cap, and above it a seeded sample that is
the same in every run; bench.py refuses a step count that would time nothing.  (The GPU runs of the option itself:
tests/test_parallel_gpu.py::test_bench_plain_line and ::test_bench_single_gpu_line_schema.)"""
import os
import subprocess
import sys

import numpy as np
import torch

import bench
import cases


def _arrays(n):
    # distinct values (exact in float32 below 2**24) so that a sampled value names the flat index it came from
    return {"o": torch.arange(n, dtype=torch.float32).reshape(2, 1, n // 2), "z": -1.0 - torch.arange(n // 4, dtype=torch.float64).reshape(2, 4, n // 32)}


def test_dump_outputs_whole_arrays_under_the_cap(tmp_path):
    arrays = _arrays(4096)
    info = bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["o.npy", "z.npy"]
    for name, t in arrays.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(t.shape) and np.array_equal(a, t.float().numpy())
        assert info[name] == {"shape": list(t.shape), "dtype": "float32", "sampled": False}


def test_dump_outputs_sample_is_capped_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    arrays = _arrays(1 << 18)                                        # 1.3 MB of float32
    a_info = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 200_000
    for name, t in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a_info[name]["sampled"] and a.dtype == np.float32 and a.ndim == 1 and a.size == a_info[name]["elements"] > 0
        assert np.array_equal(a, b)
        idx = (a if name == "o" else -1.0 - a).astype(np.int64)     # the flat indices the sample took, ascending and without repeats
        assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < t.numel()
        assert np.array_equal(a, t.float().numpy().reshape(-1)[idx])


def test_steps_must_time_at_least_one_step():
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr[-2000:]


def test_bench_weights_are_generated_in_process(tmp_path, monkeypatch):
    """bench.py takes its weights from cases.full_model_weights(file_cache=False): generated in the run's own process, with no file
    read or written, and equal to what the file-cached path hands the tests."""
    import tempfile
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    monkeypatch.setattr(cases, "_FULL_SD", {})
    fresh = cases.full_model_weights(skip_enc_q=True, file_cache=False)
    assert os.listdir(tmp_path) == []
    cases.full_model_weights(skip_enc_q=True)                       # generates and writes the file ...
    monkeypatch.setattr(cases, "_FULL_SD", {})
    cached = cases.full_model_weights(skip_enc_q=True)              # ... which this call reads back
    assert len(os.listdir(tmp_path)) == 1
    assert list(fresh) == list(cached) and all(fresh[k].dtype == np.float32 and np.array_equal(fresh[k], cached[k]) for k in fresh)
