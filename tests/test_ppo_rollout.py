"""PPO from device rollouts, the parts that need no GPU: the NumPy definition of the
device minibatch draw (algos/_device_sgd.py: minibatch_indices_reference), and the
errors of PPO.minibatch_draw and PPO.train_from_rollout, raised before the GPU
library is loaded."""
import numpy as np
import pytest
import torch

H, E = 5, 3


@pytest.fixture
def no_gpu_library(monkeypatch):
    from mjrl_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the GPU library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "calls", refuse)


# ---- the draw's definition ----

@pytest.mark.parametrize("T,N,bound", [(7, 70_000, 22.46), (264, 264_000, 339.0)])
def test_reference_range_and_uniformity(T, N, bound):
    """Chi-square of the counts against the uniform law, below the 0.001 point at
    T - 1 degrees of freedom."""
    from mjrl_amd.algos._device_sgd import minibatch_indices_reference
    d = minibatch_indices_reference(1, 0, N, T)
    assert d.dtype == np.int64 and d.shape == (N,)
    assert d.min() >= 0 and d.max() < T
    c = np.bincount(d, minlength=T)
    chi = float(((c - N / T) ** 2 / (N / T)).sum())
    print("T = %d: chi-square %.2f (bound %.2f)" % (T, chi, bound))
    assert chi < bound


def test_reference_partition_and_large_T():
    from mjrl_amd.algos._device_sgd import minibatch_indices_reference as ref
    whole = ref(1, 0, 1001, 1000)
    assert np.array_equal(whole, np.concatenate([ref(1, 0, 333, 1000), ref(1, 333, 668, 1000)]))   # an odd first
    assert np.array_equal(whole[5:6], ref(1, 5, 1, 1000)) and ref(1, 7, 0, 1000).shape == (0,)
    T = 2 ** 40 + 11
    big = ref(1, 0, 64, T)
    assert big.min() >= 0 and big.max() < T and big.max() > 2 ** 32
    assert not np.array_equal(ref(1, 0, 64, 1000), ref(2, 0, 64, 1000))
    assert not np.array_equal(ref(1, 0, 64, 1000), ref(1 + (1 << 32), 0, 64, 1000))   # the seed's high word counts
    assert np.all(ref(3, 11, 9, 1) == 0)
    for bad in ((0, 1, 0), (-1, 1, 5), (0, -1, 5)):
        with pytest.raises(ValueError, match="minibatch_indices_reference"):
            ref(1, *bad)


def test_reference_is_the_stated_formula():
    """Draw by draw in Python integers: the block's words, the 64-bit word of the
    draw's parity, the high half of the 128-bit product."""
    from mjrl_amd.algos._device_sgd import minibatch_indices_reference
    from mjrl_amd.samplers.device_actor import philox4x32
    seed, first = (5 << 32) + 9, 3
    for T in (1, 7, 2 ** 31 + 11, 2 ** 40 + 11, 2 ** 63 - 1):
        got = minibatch_indices_reference(seed, first, 9, T)
        for i, g in enumerate(range(first, first + 9)):
            b = g >> 1
            x = [int(w) for w in philox4x32((b & 0xFFFFFFFF, b >> 32, 0, 0), (9, 5 ^ 0x4D425849))]
            u = (x[2] | x[3] << 32) if g & 1 else (x[0] | x[1] << 32)
            assert int(got[i]) == (u * T) >> 64, (T, g)


# ---- errors before the GPU library is loaded ----

class _Env:
    env_id = "rollout-v0"


def _agent(**kw):
    from mjrl_amd.algos.ppo_clip import PPO
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    spec = EnvSpec(4, 2, 1000, 1)
    return PPO(_Env(), MLP(spec, hidden_sizes=(64, 64), seed=0), LinearBaseline(spec), **kw)


def _rollout():
    done = torch.zeros(H, E, dtype=torch.uint8)
    done[2, 0] = 1
    return dict(observations=torch.zeros(H, E, 4), actions=torch.zeros(H, E, 2), rewards=torch.zeros(H, E), done=done)


def _paths():
    rs = np.random.RandomState(0)
    return [dict(observations=rs.randn(6, 4), actions=rs.randn(6, 2), rewards=rs.randn(6), advantages=rs.randn(6))]


def test_minibatch_draw_errors(no_gpu_library, monkeypatch):
    from mjrl_amd.algos.ppo_clip import PPO
    for var in ("MJRL_AMD_DEVICES", "WORLD_SIZE", "RANK"):
        monkeypatch.delenv(var, raising=False)
    assert PPO.minibatch_draw == "numpy"
    agent = _agent()
    agent.minibatch_draw = "philox"
    for call in (lambda: agent.train_from_paths(_paths()), lambda: agent.train_from_rollout(**_rollout())):
        with pytest.raises(ValueError, match=r"PPO\.minibatch_draw.*'philox'"):
            call()
    cpu = _agent(device="cpu")
    cpu.minibatch_draw = "device"
    for call in (lambda: cpu.train_from_paths(_paths()), lambda: cpu.train_from_rollout(**_rollout())):
        with pytest.raises(ValueError, match=r'PPO\.minibatch_draw = "device".*cpu'):
            call()
    # set on the class, as fit_backend is
    monkeypatch.setattr(PPO, "minibatch_draw", "host")
    with pytest.raises(ValueError, match=r"PPO\.minibatch_draw"):
        _agent().train_from_paths(_paths())


def test_train_from_rollout_argument_errors_name_ppo(no_gpu_library, monkeypatch):
    for var in ("MJRL_AMD_DEVICES", "WORLD_SIZE", "RANK"):
        monkeypatch.delenv(var, raising=False)
    with pytest.raises(ValueError, match="PPO.*is a CPU tensor"):
        _agent().train_from_rollout(**_rollout())
    with pytest.raises(ValueError, match="PPO.*steps"):
        _agent().train_from_rollout(steps=[1, 2], **_rollout())
    # the fused backends' limits come first, by name too
    agent = _agent(mb_size=128)
    agent.fit_backend = "hip"
    with pytest.raises(ValueError, match=r'PPO\.fit_backend = "hip"'):
        agent.train_from_rollout(**_rollout())

    class TwoRanks:
        world_size, rank, sharded = 2, 0, True
    with pytest.raises(ValueError, match="PPO.*world size 2"):
        _agent(comm=TwoRanks()).train_from_rollout(**_rollout())


def test_draw_counter_is_pickled():
    import pickle
    agent = _agent(seed=3)
    assert agent._draw_first == 0
    agent._draw_first = 1234
    again = pickle.loads(pickle.dumps(agent))
    assert again._draw_first == 1234 and again.seed == 3 and again.minibatch_draw == "numpy"
