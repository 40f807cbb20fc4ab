"""bench.py's host logic that needs no GPU: the launcher, the world-size check, the PMC-profile freshness check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


@pytest.mark.parametrize("extra", [[], ["--train"]])
def test_world_size_must_equal_gpus(extra):
    """VERDICT r1 / ADVICE: `--gpus 8` in a one-rank world used to print an n_gpus: 1 line.  Now: non-zero exit, no line."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--no-cpu-baseline"] + extra,
                         env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "WORLD_SIZE=1 but --gpus 2" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_gpus_n_without_launcher_spawns_n_ranks():
    """With WORLD_SIZE unset the parent starts torch.distributed.run itself (before any GPU call) and relays the ranks' exit code.
    There is no GPU here, so both ranks stop at 'needs a GPU' -- what is checked is that TWO ranks were started by the parent and
    that their failure is the parent's failure (no silent single-rank line)."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"],
                         env=_env(AKE_REHEARSE_ONE_GPU="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert "2-rank launch failed" in out.stderr
    assert out.stderr.count("bench.py needs a GPU") >= 2 or ("rank: 1" in out.stderr or "local_rank: 1" in out.stderr)
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, BENCH, "--steps", "0"], env=_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--steps must be at least 1" in out.stderr


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    """--dump-outputs: float32 (float64 kept) .npy files; over the byte limit every array keeps the same seeded sample of rows."""
    sys.path.insert(0, REPO)
    import bench
    rng = np.random.default_rng(1)
    small = {"key": rng.normal(size=(8, 12)).astype(np.float32), "loss": np.float32(0.5), "x64": rng.normal(size=3)}
    bench.dump_outputs(str(tmp_path / "a"), small)
    for k, v in small.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert got.dtype == np.asarray(v).dtype and np.array_equal(got, v)
    big = {"key": rng.normal(size=(1000, 12)).astype(np.float32), "tonic": rng.normal(size=(1000, 12)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "b"), big, max_bytes=10_000)
    bench.dump_outputs(str(tmp_path / "c"), big, max_bytes=10_000)
    got = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in big}
    assert 0 < sum(a.nbytes for a in got.values()) <= 10_000
    rows = [int(np.flatnonzero((big["key"] == r).all(1))[0]) for r in got["key"]]
    assert rows == sorted(set(rows)) and np.array_equal(got["tonic"], big["tonic"][rows])
    for k in big:
        assert np.array_equal(got[k], np.load(tmp_path / "c" / f"{k}.npy"))


def test_pmc_traffic_is_refused_when_stale(tmp_path, monkeypatch):
    sys.path.insert(0, REPO)
    import bench
    h = bench.kernel_set_hash()
    assert len(h) == 16 and h == bench.kernel_set_hash()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "REPO", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_set_hash", lambda: h)
    (prof / "r09_a_pmc_traffic.json").write_text(json.dumps({"kernel_set": "0123456789abcdef", "kernels": {"k": {"hbm_bytes": 1}}}))
    name, kernels, why = bench.pmc_traffic()
    assert kernels == {} and "STALE" in why and name == "r09_a_pmc_traffic.json"
    (prof / "r09_b_pmc_traffic.json").write_text(json.dumps({"kernel_set": h, "kernels": {"k": {"hbm_bytes": 1}}}))
    name, kernels, why = bench.pmc_traffic()
    assert kernels == {"k": {"hbm_bytes": 1}} and why is None and name == "r09_b_pmc_traffic.json"
