"""Host side of the device rollout ingest (mjrl_amd/samplers/rollout_ingest.py): the
cut of a step-major rollout into paths, written out by hand, the equivalent
sampler-format paths, and every argument error of DeviceBatch.from_rollout /
train_from_rollout, raised before the GPU library is loaded."""
import numpy as np
import pytest
import torch

from mjrl_amd.samplers import rollout_ingest as RI

H, E = 5, 3
STEPS = [5, 0, 3]
#            env 0  1  2
DONE = np.array([[1, 1, 0],    # t = 0: a done at t = 0 (env 0); env 1 has no valid step
                 [1, 1, 0],    # t = 1: the second of two consecutive dones
                 [0, 0, 0],
                 [0, 1, 1],    # env 2's cell is past its 3 steps: never read
                 [1, 1, 1]],   # env 0: a done on its last valid step, no trailing path
                dtype=np.uint8)
TERM = np.array([[1, 0, 0],
                 [0, 1, 0],    # env 0's second end was a time limit
                 [1, 0, 1],    # set where done is not: never read
                 [0, 0, 1],
                 [1, 0, 0]], dtype=np.uint8)


def hand_case():
    return DONE.copy(), TERM.copy(), list(STEPS)


def test_hand_written_segmentation():
    seg = RI.segment_rollout_reference(DONE, TERM, STEPS)
    assert seg["P"] == 4 and seg["T"] == 8
    assert seg["paths"] == [(0, 0, 1, True), (0, 1, 1, False), (0, 2, 3, True), (2, 0, 3, False)]
    assert seg["path_off"].tolist() == [0, 1, 2, 5, 8] and seg["path_off"].dtype == np.int64
    assert seg["path_term"].tolist() == [1, 0, 1, 0] and seg["path_term"].dtype == np.uint8
    assert seg["R"].tolist() == [0, 5, 5, 8]
    # terminated None: every done is a termination; steps None: every env runs H steps
    seg = RI.segment_rollout_reference(DONE)
    assert seg["paths"] == [(0, 0, 1, True), (0, 1, 1, True), (0, 2, 3, True),
                            (1, 0, 1, True), (1, 1, 1, True), (1, 2, 2, True), (1, 4, 1, True),
                            (2, 0, 4, True), (2, 4, 1, True)]
    assert seg["R"].tolist() == [0, 5, 10, 15] and seg["path_off"][-1] == 15
    # bool boards and torch tensors cut the same way
    seg_b = RI.segment_rollout_reference(torch.from_numpy(DONE).bool(), torch.from_numpy(TERM).bool(), STEPS)
    assert seg_b["paths"] == RI.segment_rollout_reference(DONE, TERM, STEPS)["paths"]
    empty = RI.segment_rollout_reference(DONE, TERM, [0, 0, 0])
    assert empty["P"] == 0 and empty["T"] == 0 and empty["path_off"].tolist() == [0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rollout_to_paths_wire_format(dtype):
    rs = np.random.RandomState(3)
    n, m = 4, 2
    obs = rs.randn(H, E, n).astype(dtype)
    act = rs.randn(H, E, m).astype(dtype)
    rew = rs.randn(H, E).astype(dtype)
    for x in (obs, act, rew):   # cells past an env's steps are never read
        x[3:, 2] = np.nan
        x[:, 1] = np.nan
    paths = RI.rollout_to_paths(obs, act, rew, DONE, TERM, STEPS)
    assert len(paths) == 4
    lens = [1, 1, 3, 3]
    for p, L, t in zip(paths, lens, [True, False, True, False]):
        assert set(p) == {"observations", "actions", "rewards", "agent_infos", "env_infos", "terminated"}
        assert p["observations"].shape == (L, n) and p["observations"].dtype == np.float64
        assert p["actions"].shape == (L, m) and p["actions"].dtype == np.float64
        assert p["rewards"].shape == (L,) and p["rewards"].dtype == np.float64
        assert p["terminated"] is t and p["agent_infos"] == {} and p["env_infos"] == {}
    # the concatenation (npg_cg.py:87-89) is the valid cells in row order, env by env
    for key, x in (("observations", obs), ("actions", act), ("rewards", rew)):
        cat = np.concatenate([p[key] for p in paths])
        want = np.concatenate([x[:5, 0], x[:3, 2]]).astype(np.float64)
        assert np.array_equal(cat, want) and not np.isnan(cat).any()
        assert np.array_equal(RI.rollout_rows(x, STEPS), np.concatenate([x[:5, 0], x[:3, 2]]))
    # torch tensors give the same paths
    tp = RI.rollout_to_paths(torch.from_numpy(obs), torch.from_numpy(act), torch.from_numpy(rew),
                             torch.from_numpy(DONE), torch.from_numpy(TERM), STEPS)
    assert all(np.array_equal(a["observations"], b["observations"]) for a, b in zip(tp, paths))


# ---- argument errors, without the GPU library ----

@pytest.fixture
def no_gpu_library(monkeypatch):
    from mjrl_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the GPU library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "calls", refuse)


def _rollout(n=4, m=2, dtype=torch.float32):
    return dict(observations=torch.zeros(H, E, n, dtype=dtype), actions=torch.zeros(H, E, m, dtype=dtype),
                rewards=torch.zeros(H, E, dtype=dtype), done=torch.from_numpy(DONE.copy()))


BAD = [
    (dict(observations=torch.zeros(H, E)), "observations"),
    (dict(actions=torch.zeros(H, E + 1, 2)), "actions"),
    (dict(rewards=torch.zeros(H, E, 1)), "rewards"),
    (dict(done=torch.zeros(H + 1, E, dtype=torch.uint8)), "done"),
    (dict(terminated=torch.zeros(H, E + 1, dtype=torch.uint8)), "terminated"),
    (dict(actions=torch.zeros(H, E, 2, dtype=torch.float64)), "actions are torch.float64"),
    (dict(observations=torch.zeros(H, E, 4, dtype=torch.float16), actions=torch.zeros(H, E, 2, dtype=torch.float16)),
     "observations must be float32 or float64"),
    (dict(rewards=torch.zeros(H, E, dtype=torch.int32)), "rewards"),
    (dict(done=torch.zeros(H, E, dtype=torch.float32)), "done must be uint8 or bool"),
    (dict(observations=np.zeros((H, E, 4), np.float32)), "observations must be a torch tensor"),
    (dict(steps=[5, 0]), "steps"),
    (dict(steps=[5, 0, 6]), "steps"),
    (dict(steps=[5, -1, 3]), "steps"),
    (dict(steps=[5.0, 0.0, 3.0]), "steps"),
    (dict(), "is a CPU tensor"),
    (dict(observations=torch.zeros(H, E, 4, device="meta")), "one device"),
]


@pytest.mark.parametrize("change,match", BAD, ids=[("%d-%s" % (i, m)).replace(" ", "_") for i, (_, m) in enumerate(BAD)])
def test_from_rollout_argument_errors(no_gpu_library, change, match):
    from mjrl_amd.engine import DeviceBatch
    kw = dict(_rollout(), **change)
    with pytest.raises(ValueError, match=match):
        DeviceBatch.from_rollout(**kw)


class _Env:
    env_id = "rollout-v0"


def _spec(n=4, m=2):
    from mjrl_amd.utils.gym_env import EnvSpec
    return EnvSpec(n, m, 1000, 1)


@pytest.mark.parametrize("kind", ["MLPBaseline", "QuadraticBaseline", "Other"])
def test_from_rollout_refuses_baselines_that_need_host_paths(no_gpu_library, kind):
    from mjrl_amd.engine import DeviceBatch
    if kind == "MLPBaseline":
        from mjrl_amd.baselines.mlp_baseline import MLPBaseline
        base = MLPBaseline(_spec())
    elif kind == "QuadraticBaseline":
        from mjrl_amd.baselines.quadratic_baseline import QuadraticBaseline
        base = QuadraticBaseline(_spec())
    else:
        base = type("Other", (), {"predict": lambda self, p: None})()
    with pytest.raises(ValueError, match=kind):
        DeviceBatch.from_rollout(baseline=base, **_rollout())
    # the agent method names the class too, before anything else touches the GPU
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.policies.gaussian_mlp import MLP
    agent = NPG(_Env(), MLP(_spec(), hidden_sizes=(64, 64), seed=0), base)
    with pytest.raises(ValueError, match=kind):
        agent.train_from_rollout(**_rollout())


def test_from_rollout_accepts_the_device_baselines_up_to_the_device_check(no_gpu_library):
    """LinearBaseline, ZeroBaseline and None pass the class check: the next error is
    the CPU tensors'."""
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.baselines.zero_baseline import ZeroBaseline
    from mjrl_amd.engine import DeviceBatch
    for base in (None, ZeroBaseline(_spec()), LinearBaseline(_spec())):
        with pytest.raises(ValueError, match="is a CPU tensor"):
            DeviceBatch.from_rollout(baseline=base, **_rollout())


def _agent(cls, **kw):
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    return cls(_Env(), MLP(_spec(), hidden_sizes=(64, 64), seed=0), LinearBaseline(_spec()), **kw)


def test_train_from_rollout_refusals(no_gpu_library, monkeypatch):
    from mjrl_amd.algos.batch_reinforce import BatchREINFORCE
    from mjrl_amd.algos.dapg import DAPG
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.algos.ppo_clip import PPO
    from mjrl_amd.algos.trpo import TRPO
    for var in ("MJRL_AMD_DEVICES", "WORLD_SIZE", "RANK"):
        monkeypatch.delenv(var, raising=False)
    with pytest.raises(ValueError, match="DAPG"):
        _agent(DAPG).train_from_rollout(**_rollout())
    with pytest.raises(ValueError, match="PPO"):
        _agent(PPO).train_from_rollout(**_rollout())

    class MyDAPG(DAPG):
        pass
    with pytest.raises(ValueError, match="MyDAPG.*DAPG"):
        _agent(MyDAPG).train_from_rollout(**_rollout())
    with pytest.raises(ValueError, match="NPG.*devices= pool"):
        _agent(NPG, devices=[0, 1]).train_from_rollout(**_rollout())
    monkeypatch.setenv("MJRL_AMD_DEVICES", "2")
    with pytest.raises(ValueError, match="TRPO.*devices= pool"):
        _agent(TRPO).train_from_rollout(**_rollout())
    monkeypatch.delenv("MJRL_AMD_DEVICES")

    class TwoRanks:
        world_size, rank, sharded = 2, 0, True
    with pytest.raises(ValueError, match="NPG.*world size 2"):
        _agent(NPG, comm=TwoRanks()).train_from_rollout(**_rollout())
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "1")
    with pytest.raises(ValueError, match="BatchREINFORCE.*world size 4"):
        _agent(BatchREINFORCE).train_from_rollout(**_rollout())
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    # one process, one device: the arguments are checked next
    for cls in (BatchREINFORCE, NPG, TRPO):
        with pytest.raises(ValueError, match="is a CPU tensor"):
            _agent(cls).train_from_rollout(**_rollout())
        with pytest.raises(ValueError, match="actions are torch.float64"):
            _agent(cls).train_from_rollout(**dict(_rollout(), actions=torch.zeros(H, E, 2, dtype=torch.float64)))
        with pytest.raises(ValueError, match="steps"):
            _agent(cls).train_from_rollout(steps=[1, 2], **_rollout())
