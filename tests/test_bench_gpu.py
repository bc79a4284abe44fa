"""bench.py on the GPU: a plain run's line and --dump-outputs (what the timed path computed, checked against the oracle
and against a second run with the same arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]


def _plain(dump_dir, B, T, sd):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--frames", str(T), "--static-dim", str(sd), "--dump-outputs", dump_dir],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_dumps_what_the_timed_path_computed(tmp_path):
    import torch
    from oracle import mlpg as O
    B, T, sd = 128, 1000, 60                     # 61 MB of trajectories: more than the dump limit, a sample is written
    res = _plain(str(tmp_path / "a"), B, T, sd)
    assert res["steps"] == 3 and res["full"] is False and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["unit"] == "frames/s" and res["dtype"] == "f64" and res["higher_is_better"] is True
    assert "secondary" not in res and "cpu_baseline" not in res and res["roofline"]["peak_measured"] is None
    y = np.load(tmp_path / "a" / "mlpg_out.npy")
    idx = np.load(tmp_path / "a" / "mlpg_out_utterances.npy").astype(np.int64)
    st = np.load(tmp_path / "a" / "status.npy")
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert y.dtype == np.float64 and y.shape == (len(idx), T, sd) and 1 <= len(idx) < B and total <= 64e6
    assert st.shape == (B * sd,) and not st.any()
    # the inputs bench.py generates (seeded torch.Generator on the device), against the oracle
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1234)
    means = torch.randn(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
    variances = torch.rand(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
    for k in (0, len(idx) - 1):
        b = int(idx[k])
        yo = O.mlpg(means[b].cpu().numpy(), variances[b].cpu().numpy(), WINDOWS)
        assert np.abs(y[k] - yo).max() / np.abs(yo).max() < 1e-9, b
    # the same arguments: the same inputs, the same utterances, the same outputs
    _plain(str(tmp_path / "b"), B, T, sd)
    assert np.array_equal(np.load(tmp_path / "b" / "mlpg_out_utterances.npy"), idx.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "b" / "mlpg_out.npy"), y)
