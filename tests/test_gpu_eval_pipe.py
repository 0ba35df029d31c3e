"""The pipelined EVAL kernel (csrc/kxe.h, k_kx_eval_pipe) against the serial EVAL
instance of k_kx, bit for bit: the eval sums stats[S_EVAL : S_EVAL + 2] and the
per-workgroup rpart records.

The pipelined kernel changes where tile t+1's first-layer products are issued
(inside tile t's chain), not one operation of the arithmetic, so equality is
exact: every comparison here is on bytes.  mjrl_eval_pipe(0 / 1) selects the
kernel; mjrl_eval_grid gives the launch's workgroup count, from which the row
counts with 1 / 2 and 2 / 3 tiles per workgroup are chosen (the grid never
exceeds the tile count, so no workgroup of a launch is without a tile: asserted;
the kernel's prologue handles one all the same).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = (64, 64)
# every (MP, KG) the library instantiates k_kx for: (n, m) -> np = 32 KG, mp = MP
SHAPES = {(16, 4): (120, 6), (16, 8): (250, 6), (16, 12): (376, 6),
          (32, 4): (120, 17), (32, 8): (250, 17), (32, 12): (376, 17)}
SMALL_T = [1, 31, 32, 33, 63, 65]
T_MAX = 25000
SENTINEL = 777.25


@pytest.fixture(autouse=True)
def _restore_setting():
    from mjrl_amd import _lib
    K = _lib.calls()
    was = K.mjrl_eval_pipe(-1)
    yield
    K.mjrl_eval_pipe(was)


def _d(n, m):
    return 64 * n + 64 + 64 * 64 + 64 + m * 64 + m + m


def _grid_rows(K, shape):
    """Row counts in 8k .. 25k whose launch gives its workgroups 1 / 2 and 2 / 3
    tiles, each with a whole and with a partial last tile."""
    found = {}
    for T in range(8192, T_MAX + 1):
        nt = (T + 31) // 32
        G = K.mjrl_eval_grid(shape, T)
        assert 1 <= G <= nt, (T, G)   # no workgroup without a tile
        key = (len(range(G - 1, nt, G)), len(range(0, nt, G)), T % 32 != 0)
        if key[:2] in ((1, 2), (2, 3)) and key not in found:
            found[key] = T
    assert len(found) == 4, found
    return sorted(found.values())


class _Case:
    """An engine with rows loaded and the a1 / mu0 / ll0 caches of a real forward pass."""

    def __init__(self, n, m, obs, seed):
        from mjrl_amd.engine import UpdateEngine
        rs = np.random.RandomState(seed)
        T = obs.shape[0]
        self.eng = eng = UpdateEngine(n, m, H, device="cuda:0", precision="split")
        assert eng.K.mjrl_split_supported(eng.shape)
        eng.load_rows(obs, rs.randn(T, m), rs.randn(T))
        theta = (rs.randn(_d(n, m)) * 0.05).astype(np.float32)
        theta[-m:] = np.linspace(-1.0, 0.3, m)
        eng.forward_pass(torch.from_numpy(theta).cuda(), T)
        self.theta1 = torch.from_numpy(theta + (rs.randn(theta.size) * 2e-3).astype(np.float32)).cuda()

    def run(self, T, pipe, skip=None):
        """One eval pass over the first T rows; (the two eval sums, the rpart records) as bytes."""
        from mjrl_amd import _lib
        from mjrl_amd.engine import S_EVAL
        eng = self.eng
        K, s = eng.K, eng.shape
        assert K.mjrl_eval_pipe(pipe) in (0, 1) and K.mjrl_eval_pipe(-1) == pipe
        G = K.mjrl_eval_grid(s, T)
        eng.stats[S_EVAL:S_EVAL + 2].fill_(SENTINEL)
        eng.ws["rpart"][:2 * G].fill_(SENTINEL)
        st = _lib.stream_ptr()
        K.mjrl_pack_params(s, eng._pad(self.theta1, "theta_new"), eng.packed_new, 1, eng.min_log_std, st)
        _, _, osh, osc = eng.transforms
        args = (s, eng._rows(T, eng.ws["adv32"]), T, eng.packed_new, eng.packed_theta, osh, osc, eng._scratch(T),
                eng.stats[S_EVAL:])
        if skip is None:
            K.mjrl_policy_eval(*args, st)
        else:
            K.mjrl_policy_eval_if(*args, skip, st)
        torch.cuda.synchronize()
        return (eng.stats[S_EVAL:S_EVAL + 2].cpu().numpy().tobytes(), eng.ws["rpart"][:2 * G].cpu().numpy().tobytes())


@pytest.mark.parametrize("mp,kg", sorted(SHAPES))
def test_pipelined_eval_is_bit_identical(mp, kg):
    n, m = SHAPES[(mp, kg)]
    rs = np.random.RandomState(10 * mp + kg)
    c = _Case(n, m, rs.randn(T_MAX, n), seed=kg)
    assert (c.eng.shape.mp, c.eng.shape.np) == (mp, 32 * kg)
    rows = SMALL_T + _grid_rows(c.eng.K, c.eng.shape) + [T_MAX]
    sentinel = np.full(2, SENTINEL).tobytes()
    for T in rows:
        serial, piped = c.run(T, 0), c.run(T, 1)
        assert serial[0] != sentinel and np.all(np.isfinite(np.frombuffer(serial[0])))
        assert SENTINEL not in np.frombuffer(serial[1])
        assert piped[0] == serial[0], (T, np.frombuffer(piped[0]), np.frombuffer(serial[0]))
        assert piped[1] == serial[1], T


def test_wide_range_observation_columns():
    """Observation columns spanning 1e-6 .. 1e3 (as test_gpu_split.py), with
    always-zero columns and an all-zero row."""
    n, m = SHAPES[(32, 12)]
    rs = np.random.RandomState(5)
    T = 9000
    obs = rs.randn(T, n) * 10.0 ** rs.uniform(-6, 3, size=n)
    obs[:, :5] = 0.0
    obs[7, :] = 0.0
    c = _Case(n, m, obs / 50.0, seed=6)
    for T_ in (T, 33):
        assert c.run(T_, 1) == c.run(T_, 0)


def test_skip_flag_leaves_the_outputs_untouched():
    """mjrl_policy_eval_if: with the flag set neither kernel writes anything; with
    it clear both give mjrl_policy_eval's bytes."""
    n, m = SHAPES[(32, 12)]
    c = _Case(n, m, np.random.RandomState(7).randn(9000, n), seed=8)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    for T in (9000, 65):
        G = c.eng.K.mjrl_eval_grid(c.eng.shape, T)
        untouched = (np.full(2, SENTINEL).tobytes(), np.full(2 * G, SENTINEL).tobytes())
        ref = c.run(T, 0)
        for pipe in (0, 1):
            flag.fill_(1)
            assert c.run(T, pipe, skip=flag) == untouched
            flag.fill_(0)
            assert c.run(T, pipe, skip=flag) == ref


@pytest.mark.parametrize("algo", ["trpo", "npg"])
def test_updates_are_identical_with_either_eval(algo):
    """One update (TRPO: the device line search, mjrl_policy_eval_if; NPG), eager
    and as a replayed graph, with the serial and with the pipelined EVAL: the same
    parameters and statistics, bit for bit."""
    from mjrl_amd.engine import UpdateEngine, DeviceBatch, S_EVAL
    n, m = SHAPES[(16, 4)]
    rs = np.random.RandomState(11)
    lengths = np.array([700, 1, 650, 33, 900, 416])
    T = int(lengths.sum())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    obs = rs.randn(T, n).astype(np.float32).astype(np.float64)
    act = rs.randn(T, m).astype(np.float32).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    tensors = (t(obs), t(act), t(rs.randn(T)), t(rs.randn(T)), t(off), t(np.zeros(len(lengths), np.uint8)))
    theta = t((rs.randn(_d(n, m)) * 0.1).astype(np.float32))
    args = dict(algo="trpo", kl_dist=0.05, trpo_verbose=False) if algo == "trpo" else dict(algo="npg", n_step_size=0.1)
    records = []
    for pipe in (0, 1):
        eng = UpdateEngine(n, m, H, device="cuda:0")
        assert eng.split and eng.K.mjrl_eval_pipe(pipe) in (0, 1)
        if algo == "trpo":
            assert eng.trpo_device_trials > 0
        b = DeviceBatch(*tensors)
        for graph in (False, True, True, True):   # eager; eager + capture; two replays
            eng.graphs = graph
            res = eng.update(b, theta, gamma=0.99, gae_lambda=0.95, **args)
            torch.cuda.synchronize()
            keys = ("alpha", "gx", "kl_dist", "surr_after", "surr_before", "cg_iters", "base_stats")
            records.append((pipe, graph, {k: res[k] for k in keys}, res["trials"],
                            eng.vec["theta_new"].cpu().numpy().tobytes(),
                            eng.stats[S_EVAL:S_EVAL + 2].cpu().numpy().tobytes()))
        assert eng._gstate.get("graph") is not None
    for r in records[1:]:
        assert r[2:] == records[0][2:], (r[:4], records[0][:4])
