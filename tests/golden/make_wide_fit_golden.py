"""Golden vectors of the reference's minibatch fits on policies wider than 64 hidden units
(mjrl/algos/behavior_cloning.py:11-68, behavior_cloning_2.py:11-77, ppo_clip.py:23-120): the
bc_case / bc2_case / ppo_case recipes of make_golden.py and make_bc2_golden.py at the widths
the fused "hip_wide" backend exists for.  bc_wide.npz, bc2_wide.npz and ppo_wide.npz next to
this file, with the keys of bc.npz / bc2.npz / ppo.npz.

Build-container only, like make_golden.py (whose import recipe and path helpers this reuses;
importing it runs no case): the reference is not on the GPU box, which reads only the
committed .npz.  The fixtures are data: the inputs and what the reference's own run produced.

    python tests/golden/make_wide_fit_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as G  # noqa: E402  (installs the gym stub, puts the reference on sys.path)
import numpy as np  # noqa: E402

BC_HIDDEN = (96, 160)
PPO_HIDDEN = (128, 128)


def _bc_paths():
    rs = np.random.RandomState(61)
    n, m = 6, 3
    lengths = [100, 80, 120]
    paths = G.make_paths(rs, n, m, lengths, [False] * 3)
    for p in paths:
        p["observations"] = p["observations"] * 3.0 + 1.0
        p["actions"] = np.tanh(p["observations"][:, :m]) + 0.1 * p["actions"]
    return n, m, lengths, paths


def _save_bc(name, paths, lengths, policy, bc, **extra):
    t = policy.model.transformations
    np.savez_compressed(os.path.join(G.OUT, name), obs=G.concat(paths, "observations"),
                        act=G.concat(paths, "actions"), lengths=np.array(lengths),
                        final=policy.get_param_values(), loss=np.array(bc.logger.log["loss"], dtype=np.float64),
                        in_shift=t["in_shift"], in_scale=t["in_scale"], out_shift=t["out_shift"],
                        out_scale=t["out_scale"], np_seed=np.int64(17), **extra)
    print(name, "losses", bc.logger.log["loss"])


def bc_wide_case():
    """Reference BC, hidden (96, 160), epochs 2 of 9 minibatches of 32 after np.random.seed(17)."""
    from mjrl.algos.behavior_cloning import BC as RefBC
    n, m, lengths, paths = _bc_paths()
    policy = G.MLP(G.EnvSpec(n, m, 120, 1), hidden_sizes=BC_HIDDEN, seed=5)
    init = policy.get_param_values()
    bc = RefBC(paths, policy, epochs=2, batch_size=32, lr=1e-3)
    np.random.seed(17)
    bc.train()
    _save_bc("bc_wide.npz", paths, lengths, policy, bc, init=init)


def bc2_wide_case():
    """Reference MSE behaviour cloning on the same rows and widths."""
    from mjrl.algos.behavior_cloning_2 import BC as RefBC
    n, m, lengths, paths = _bc_paths()
    policy = G.MLP(G.EnvSpec(n, m, 120, 1), hidden_sizes=BC_HIDDEN, seed=5)
    init = policy.get_param_values()
    bc = RefBC(paths, policy, epochs=2, batch_size=32, lr=1e-3)
    after_init = policy.get_param_values()
    groups = bc.optimizer.param_groups
    assert len(groups) == 1 and len(groups[0]["params"]) == 6
    np.random.seed(17)
    bc.train()
    assert np.array_equal(policy.get_param_values()[-m:], after_init[-m:])   # log_std is not trained
    _save_bc("bc2_wide.npz", paths, lengths, policy, bc, init=init, after_init=after_init)


def ppo_wide_case():
    """Reference PPO train_from_paths, hidden (128, 128), two iterations (the Adam state carries
    over; the second runs in the aliased form) after np.random.seed(23) / (24)."""
    from mjrl.algos.ppo_clip import PPO as RefPPO
    rs = np.random.RandomState(71)
    n, m = 6, 2
    lengths = [150, 90, 200, 160]
    policy = G.MLP(G.EnvSpec(n, m, 200, 1), hidden_sizes=PPO_HIDDEN, seed=3, init_log_std=-0.5)
    ppo = RefPPO(None, policy, None, clip_coef=0.2, epochs=2, mb_size=64, learn_rate=3e-3, save_logs=True)
    out = dict(init=policy.get_param_values(), lengths=np.array(lengths))
    for it, seed in enumerate((23, 24)):
        paths = G.make_paths(rs, n, m, lengths, [False] * 4)
        for p in paths:
            p["advantages"] = rs.randn(len(p["rewards"])) * 2.0 + 0.3
        np.random.seed(seed)
        stats = ppo.train_from_paths(paths)
        for k, key in (("obs", "observations"), ("act", "actions"), ("rew", "rewards"), ("adv", "advantages")):
            out["%s%d" % (k, it)] = G.concat(paths, key)
        out["np_seed%d" % it] = np.int64(seed)
        out["base_stats%d" % it] = np.array(stats, dtype=np.float64)
        out["params%d" % it] = policy.get_param_values()
        for k in ("kl_dist", "surr_improvement", "running_score"):
            out["%s%d" % (k, it)] = np.float64(ppo.logger.log[k][-1])
    np.savez_compressed(os.path.join(G.OUT, "ppo_wide.npz"), **out)
    print("ppo_wide kl", out["kl_dist0"], out["kl_dist1"], "surr", out["surr_improvement0"],
          out["surr_improvement1"])


if __name__ == "__main__":
    bc_wide_case()
    bc2_wide_case()
    ppo_wide_case()
