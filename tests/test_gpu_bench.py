"""bench.py as a command: a plain run prints the headline line and nothing that
needs runs of its own, and --dump-outputs writes the last timed step's outputs
(the Swimmer config, 25 x 500 rows: the smallest the benchmark has)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_prints_headline_and_dumps_outputs(tmp_path):
    import bench
    from oracle import npg_cpu as O
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    cfg = bench.CONFIGS["c2"]
    T = cfg["paths"] * cfg["horizon"]
    assert d["metric"] == cfg["metric"] and d["unit"] == "timesteps/s" and d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(T / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert d["dtype"].startswith("f32")
    # the companion measurements belong to --full
    assert d["full"] is False and d["roofline"] is None and d["f32_ms_per_step"] is None
    assert not {"cpu_baseline", "vs_cpu_baseline", "e2e_from_host", "e2e_stream"} & set(d)

    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(arrays) == ["advantages", "npg_grad", "stats", "theta_new", "vpg_grad"]
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    nd = sum(int(np.prod(s)) for s in bench.param_shapes(cfg))
    for k in ("theta_new", "vpg_grad", "npg_grad"):
        assert arrays[k].dtype == np.float32 and arrays[k].shape == (nd,) and np.isfinite(arrays[k]).all(), k
    assert np.abs(arrays["theta_new"] - bench.initial_theta(cfg)).max() > 0
    # the advantages depend on the seeded inputs alone, and the GAE pass is exact
    obs, _, rew = bench.make_paths(0, cfg["paths"], cfg=cfg)
    base = bench.baseline_coeffs(cfg)
    bl = np.concatenate([base.predict(dict(observations=o.astype(np.float64), rewards=r)) for o, r in zip(obs, rew)])
    lengths = np.full(cfg["paths"], cfg["horizon"], dtype=np.int64)
    _, adv = O.returns_and_advantages(np.concatenate(rew), bl, lengths, np.zeros(len(lengths), bool), bench.GAMMA,
                                      bench.LAM)
    assert arrays["advantages"].dtype == np.float64 and np.array_equal(arrays["advantages"], adv)
    st = dict(zip(bench.DUMP_STATS, arrays["stats"]))
    assert arrays["stats"].dtype == np.float64 and len(arrays["stats"]) == len(bench.DUMP_STATS) + 4
    assert 1 <= st["cg_iters"] <= bench.CG_ITERS and st["alpha"] > 0 and st["kl_dist"] > 0
