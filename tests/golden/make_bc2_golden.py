"""Golden vectors of the reference's MSE behaviour cloning
(mjrl/algos/behavior_cloning_2.py:11-77), the bc_case recipe of make_golden.py run
on that class: bc2.npz next to this file.

Build-container only, like make_golden.py (whose import recipe and path helpers
this reuses; importing it runs no case): the reference is not on the GPU box, which
reads only the committed .npz.  The fixture is data: the inputs and what the
reference's own run produced.

    python tests/golden/make_bc2_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as G  # noqa: E402  (installs the gym stub, puts the reference on sys.path)
import numpy as np  # noqa: E402


def bc2_case():
    """Minibatch Adam on MSELoss(policy.model(obs), act) over policy.model.parameters(),
    minibatches from np.random.choice after np.random.seed(17): the transformations
    and the log_std the constructor sets (after_init), the per-epoch full-data losses,
    the final parameters."""
    from mjrl.algos.behavior_cloning_2 import BC as RefBC
    rs = np.random.RandomState(61)
    n, m = 6, 3
    lengths = [100, 80, 120]
    paths = G.make_paths(rs, n, m, lengths, [False] * 3)
    for p in paths:
        p["observations"] = p["observations"] * 3.0 + 1.0
        p["actions"] = np.tanh(p["observations"][:, :m]) + 0.1 * p["actions"]
    policy = G.MLP(G.EnvSpec(n, m, 120, 1), hidden_sizes=(32, 32), seed=5)
    init = policy.get_param_values()
    bc = RefBC(paths, policy, epochs=2, batch_size=32, lr=1e-3)
    after_init = policy.get_param_values()
    groups = bc.optimizer.param_groups
    assert len(groups) == 1 and len(groups[0]["params"]) == 6
    np.random.seed(17)
    bc.train()
    final = policy.get_param_values()
    assert np.array_equal(final[-m:], after_init[-m:])   # log_std is not trained
    t = policy.model.transformations
    np.savez_compressed(os.path.join(G.OUT, "bc2.npz"), obs=G.concat(paths, "observations"),
                        act=G.concat(paths, "actions"), lengths=np.array(lengths), init=init, after_init=after_init,
                        final=final, loss=np.array(bc.logger.log["loss"], dtype=np.float64),
                        in_shift=t["in_shift"], in_scale=t["in_scale"], out_shift=t["out_shift"],
                        out_scale=t["out_scale"], np_seed=np.int64(17))
    print("bc2 losses", bc.logger.log["loss"])


if __name__ == "__main__":
    bc2_case()
