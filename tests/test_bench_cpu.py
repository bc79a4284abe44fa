"""bench.py without a GPU: the plain run's result line (gloo dry runs) and the --dump-outputs sampler."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*argv, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                          timeout=timeout, env=env)


def test_plain_run_prints_the_headline_and_nothing_of_full():
    for gpus in ("1", "2"):
        r = _bench("--gpus", gpus, "--steps", "4", "--warmup", "1", "--dry-run-cpu")
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        res = json.loads(lines[0])
        assert all(k in res for k in HEADLINE), res
        assert res["steps"] == 4 and res["warmup"] == 1 and res["full"] is False and res["higher_is_better"] is True
        assert res["ms_per_step"] == max(res["per_rank_ms_per_step"]) and len(res["per_rank_ms_per_step"]) == int(gpus)
        for k in ("secondary", "in_run_single_gpu", "cpu_baseline", "repeat_regions"):
            assert k not in res, k
        assert res["cold_protocol"] is None and res["parity_rel_err_vs_oracle"] is None


def test_bench_rejects_arguments_it_cannot_honour():
    r = _bench("--steps", "0", "--dry-run-cpu")
    assert r.returncode != 0 and "--steps" in r.stderr
    r = _bench("--steps", "2", "--dry-run-cpu", "--dump-outputs", os.path.join(ROOT, "nonexistent_dump_dir"))
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
    assert not os.path.exists(os.path.join(ROOT, "nonexistent_dump_dir"))


def test_dump_outputs_writes_all_or_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    B, T, sd = 12, 7, 5
    out = torch.arange(B * T * sd, dtype=torch.float64).reshape(B, T, sd)
    status = torch.zeros(B * sd, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "all"), out, status)
    y = np.load(tmp_path / "all" / "mlpg_out.npy")
    assert y.dtype == np.float64 and np.array_equal(y, out.numpy())
    assert np.array_equal(np.load(tmp_path / "all" / "mlpg_out_utterances.npy"), np.arange(B))
    st = np.load(tmp_path / "all" / "status.npy")
    assert st.dtype == np.float64 and st.shape == (B * sd,) and not st.any()
    # larger than the limit: whole utterances, the same ones every time, within the limit
    monkeypatch.setattr(bench, "DUMP_LIMIT", 5 * T * sd * 8)
    picks = []
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), out.float(), None)
        idx = np.load(tmp_path / d / "mlpg_out_utterances.npy").astype(np.int64)
        y = np.load(tmp_path / d / "mlpg_out.npy")
        assert y.dtype == np.float64 and y.nbytes <= bench.DUMP_LIMIT and len(idx) == 5
        assert np.all(np.diff(idx) > 0) and np.array_equal(y, out.numpy()[idx])
        assert not os.path.exists(tmp_path / d / "status.npy")
        picks.append(idx)
    assert np.array_equal(picks[0], picks[1])
