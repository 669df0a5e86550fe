"""bench.py without a GPU (this container): it must refuse loudly — there is no CPU fallback to time — whatever launch
form is asked for, and `--gpus N` as typed must not demand a launcher any more (round 2 did)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="a HIP device is present: the GPU contract tests cover bench.py")
@pytest.mark.parametrize("argv", [[], ["--gpus", "8"], ["--gpus", "8", "--loopback"], ["--gpus", "1", "--force-group"], ["--mode", "stream"]])
def test_bench_refuses_to_run_without_a_device(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", *argv, "--steps", "1", "--warmup", "0"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0
    msg = r.stderr + r.stdout
    assert "no CPU fallback" in msg
    assert "torch.distributed.run" not in msg            # `--gpus N` needs no launcher
    assert not any(line.startswith("{") for line in r.stdout.splitlines())      # and no JSON line is faked


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_exact_float_columns(tmp_path):
    import numpy as np
    bench = _bench_module()
    rec = np.zeros(5, np.dtype([("good_count", "<u4"), ("min_dist", "<u2"), ("n_train", "<u2")]))
    rec["good_count"], rec["min_dist"], rec["n_train"] = [0, 1, 7, 2000, 65535], [0, 3, 256, 99, 65535], [1, 2, 3, 4, 65535]
    isum = np.array([0, 1, 2**31 + 5, 2**32 - 1, 12345], np.uint32)
    bench.dump_outputs(str(tmp_path), bench.score_fields(rec, isum))
    assert sorted(os.listdir(tmp_path)) == ["good_count.npy", "index_checksum.npy", "min_dist.npy", "n_train.npy"]
    for name in ("good_count", "min_dist", "n_train"):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, rec[name].astype(np.int64))
    a = np.load(tmp_path / "index_checksum.npy")
    assert a.dtype == np.float64 and np.array_equal(a.astype(np.int64), isum.astype(np.int64))


def test_dump_outputs_samples_the_same_rows_above_the_cap(tmp_path, monkeypatch):
    import numpy as np
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    n = 10000
    col = np.arange(n, dtype=np.int64) * 3
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), {"a": (col, np.float64), "b": (col, np.float32)})
    sel = np.load(tmp_path / "0" / "sample_index.npy")
    a = np.load(tmp_path / "0" / "a.npy")
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in os.listdir(tmp_path / "0")) < 4096 + 3 * 256
    assert len(sel) == len(a) > 0 and np.all(np.diff(sel) > 0) and np.array_equal(a, col[sel.astype(np.int64)])
    for f in ("sample_index.npy", "a.npy", "b.npy"):
        assert np.array_equal(np.load(tmp_path / "0" / f), np.load(tmp_path / "1" / f))
