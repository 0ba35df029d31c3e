"""Cases and fp64 truth of the policy-pass tests (test_gpu_policy_passes_fp64.py):
mjrl_policy_vpg / _fvp / _eval / _eval_if on every kernel that implements them
(k_rows, k_fused, k_ks, k_kx, k_kx_eval_pipe), against oracle.npg_cpu.Policy in
float64.  Importable without a GPU and without the HIP library; the conditions
the inputs must meet for the comparison to mean anything are asserted by
test_policy_pass_inputs.py with this module alone.

A case is a policy shape, a precision and what the dispatcher must pick for it.
Its inputs, for a row count T, are T_load = T + TAIL rows: the passes run over
the first T, and the GPU test poisons what the passes read of the TAIL rows after
them (poison()), so a row past T_eval that reaches a sum shows.

theta1 = theta0 + s delta, with s chosen from the fp64 oracle so that the mean KL
over the first T rows is KL_TARGET: an unscaled small step (KL ~ 2e-4) makes the
oracle's own fp32 evaluation cancel to 5e-4 of the surrogate's scale, which would
say nothing about a kernel held to 1e-4.

The poison of ll0.  A poisoned row must enter the surrogate sum with a large
likelihood ratio exp(LL_new - ll0).  ll0 = -50 does that while LL_new of an
ordinary row is well above -50; LL_new goes as -1.1 m for these inputs (down to
-88 over the tail rows at m = 64), where -50 would give a ratio of e^-38 and hide
the row.  So the poison is min(-50, min over the tail rows of the fp64 LL_new -
20): -50 for m up to 20, never weaker than -50, and a ratio of at least e^20
everywhere."""
import zlib
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

import vec_ref as V
from oracle import npg_cpu as O

F32, F64 = np.float32, np.float64

TAIL = 40            # rows loaded after the T the passes run over
KL_TARGET = 0.05     # fp64 mean KL(theta0 || theta1) over the first T rows
DAMPING = 1e-4
# the bars of the GPU test (the project's existing ones: test_gpu_rows_shapes.py for
# VPG / F v, test_gpu_parity.py's teacher-forced eval for the surrogate and the KL)
BAR_VEC, BAR_BLOCK, BAR_EVAL = 1e-5, 1e-4, 1e-4
ADV_POISON, MU0_POISON, LL0_POISON, LL0_MARGIN = 1e6, 1e3, -50.0, 20.0

# workgroup caps of the eval pass (mjrl_eval_grid): 512 workgroups of 32-row
# (hidden >= 128) or 64-row tiles on k_rows, 256 of 32-row tiles on k_ks / k_kx.
# One row more than cap x tile is the smallest T at which a workgroup runs two
# tiles (and the last tile is partial); the GPU test asks mjrl_eval_grid that this
# is so, and that one row fewer is still one tile per workgroup.
ROWS_CAP, KS_CAP = 512, 256


class Case(namedtuple("Case", "n m hidden precision expect family pipe identity extra")):
    """expect: what the GPU test asserts of the dispatch: dict(mp, np, path, split),
    path = eng.accumulate_path() (2 = k_ks / k_kx, 1 = k_fused, 0 = k_rows + the
    weight-gradient kernels).  family: the kernel of the VPG / F v passes.  pipe:
    mjrl_eval_pipe's setting (split cases).  identity: no transformations (null
    pointers).  extra: the family's case that also runs T = 1, 31 and a multi-tile T."""
    __slots__ = ()

    @property
    def kernel_hidden(self):
        if self.hidden == (0, 0):
            return (0, 0)
        w = min(w for w in (32, 64, 128, 256) if max(self.hidden) <= w)
        return (w, w)

    @property
    def kg(self):
        return self.expect["np"] // 32 if self.family in ("ks", "kx") else None

    @property
    def instance(self):
        """The kernel instance this case anchors: (kernel hidden, mp, family, KG, pipe)."""
        return (self.kernel_hidden, self.expect["mp"], self.family, self.kg, self.pipe)

    @property
    def id(self):
        h = "lin" if self.hidden == (0, 0) else "%dx%d" % self.hidden
        return "%s-n%d-m%d-%s%s%s" % (h, self.n, self.m, self.precision,
                                     "" if self.pipe is None else "-pipe%d" % self.pipe, "-id" if self.identity else "")

    def rows(self):
        """The row counts T this case runs."""
        if not self.extra:
            return (33, 97)
        if self.family in ("ks", "kx"):
            multi = KS_CAP * 32 + 1
        else:
            multi = ROWS_CAP * (32 if self.kernel_hidden[0] >= 128 else 64) + 1
        return (1, 31, 33, 97, multi)


def _case(n, m, hidden, family, path, precision="f32", pipe=None, identity=False, extra=False):
    kh = Case(n, m, hidden, precision, None, family, pipe, identity, extra).kernel_hidden
    s = V.make_shape(n, m, *kh)
    return Case(n, m, hidden, precision, dict(mp=s.mp, np=s.np, path=path, split=precision == "split"), family, pipe,
                identity, extra)


LIN, H32, H64, H128, H256 = (0, 0), (32, 32), (64, 64), (128, 128), (256, 256)
CASES = [
    # the linear policy: k_rows<0, 0, MP>
    _case(11, 3, LIN, "rows", 0, extra=True),
    _case(30, 20, LIN, "rows", 0),
    _case(30, 40, LIN, "rows", 0, identity=True),
    _case(70, 40, LIN, "rows", 0),                     # np = 80
    # (32, 32): VPG / F v on k_fused, EVAL on k_rows<32, 32, MP>; MP 64 on k_rows throughout
    _case(17, 6, H32, "fused", 1, extra=True),
    _case(12, 17, H32, "fused", 1, identity=True),
    _case(15, 40, H32, "rows", 0),
    # (64, 64) with EVAL on k_rows<64, 64, MP>
    _case(8, 2, H64, "fused", 1),
    _case(45, 20, H64, "fused", 1),
    _case(20, 6, H64, "fused", 1),                     # np = 32: KG = 1, which k_ks does not take
    _case(40, 33, H64, "rows", 0, identity=True),      # MP 64
]
# (64, 64) on k_ks: KG 2, 4, 6, 8, 12 x MP 16, 32
CASES += [_case(n, m, H64, "ks", 2, extra=(n, m) == (60, 17), identity=(n, m) == (120, 6))
          for n in (60, 120, 180, 250, 376) for m in (6, 17)]
# (64, 64) on k_kx (split-f16 first layer): KG 4, 8, 12 x MP 16, 32, the serial and the pipelined EVAL
CASES += [_case(n, m, H64, "kx", 2, "split", pipe, extra=(n, m) == (120, 17), identity=(n, m) == (250, 6))
          for n in (120, 250, 376) for m in (6, 17) for pipe in (0, 1)]
CASES += [
    _case(17, 6, H128, "rows", 0, extra=True),
    _case(45, 24, H128, "rows", 0, identity=True),
    _case(20, 40, H128, "rows", 0),
    _case(70, 40, H128, "rows", 0),                    # np = 80, MP 64: the k_wgrad fallback
    _case(11, 3, H256, "rows", 0, extra=True),
    _case(39, 28, H256, "rows", 0, identity=True),
    _case(20, 64, H256, "rows", 0),
    # a real shape the kernels run zero-padded to (64, 64) (UpdateEngine._pad / _unpad)
    _case(8, 2, (48, 32), "fused", 1),
]


def nrel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def block_offsets(c):
    """Offsets of the parameter blocks of the flat vector (oracle.param_shapes order)."""
    hidden = None if c.hidden == (0, 0) else c.hidden
    return np.cumsum([0] + [int(np.prod(s)) for s in O.param_shapes(c.n, c.m, hidden)])


def _policy(c, d, theta_old, theta_new, dtype):
    p = O.Policy(c.n, c.m, None if c.hidden == (0, 0) else c.hidden, np.asarray(theta_old, F64), d.transforms,
                 dtype=dtype)
    if theta_new is not None:
        p.set_params(np.asarray(theta_new, F64), set_new=True, set_old=False)
    return p


def eval_rows(p, obs, act):
    """Per row: the likelihood ratio, KL(old || new) (gaussian_mlp.py:124-140, as
    Policy.surrogate / Policy.kl before their means) and LL_new, as float64 arrays."""
    with torch.no_grad():
        mu_o, ll_o = p.mean_ll(p.old, obs, act)
        mu_n, ll_n = p.mean_ll(p.new, obs, act)
        so, sn = p.old[-1], p.new[-1]
        num = (mu_o - mu_n) ** 2 + torch.exp(so) ** 2 - torch.exp(sn) ** 2
        kl = torch.sum(num / (2 * torch.exp(sn) ** 2 + 1e-8) + sn - so, dim=1)
        return (torch.exp(ll_n - ll_o).double().numpy(), kl.double().numpy(), ll_n.double().numpy(),
                mu_n.double().numpy())


def _evals(c, d, dtype):
    """(surrogate mean, KL mean) over the first T rows from the oracle's own functions."""
    p = _policy(c, d, d.theta0, d.theta1, dtype)
    T = d.T
    return (float(p.surrogate(d.obs[:T], d.act[:T], d.adv[:T]).detach()), float(p.kl(d.obs[:T], d.act[:T]).detach()))


def _grads(c, d, dtype):
    """(VPG over T rows, VPG over T_load rows, F v + damping v over T rows) at theta0."""
    p = _policy(c, d, d.theta0, None, dtype)
    T = d.T
    v = d.v.astype(F64)
    return (p.flat_vpg(d.obs[:T], d.act[:T], d.adv_vpg[:T]).astype(F64),
            p.flat_vpg(d.obs, d.act, d.adv_vpg).astype(F64),
            np.asarray(p.fvp(d.obs[:T], d.act[:T], v, DAMPING), F64))


@lru_cache(maxsize=None)
def _make(n, m, hidden, identity, T):
    c = Case(n, m, hidden, None, None, None, None, identity, None)
    rs = np.random.RandomState(zlib.crc32(repr((n, m, hidden, identity, T)).encode()))
    d = SimpleNamespace(T=T, T_load=T + TAIL)
    R = d.T_load
    r32 = lambda a: a.astype(F32).astype(F64)   # the f32-rounded values, as the passes read them
    d.obs, eps, d.adv, d.adv_vpg = r32(rs.randn(R, n)), rs.randn(R, m), r32(rs.randn(R)), r32(rs.randn(R))
    offs = block_offsets(c)
    dim = int(offs[-1])
    d.theta0 = (0.1 * rs.randn(dim)).astype(F32)
    d.theta0[-m:] = np.linspace(-1.0, 0.3, m)
    d.v = (1e-2 * rs.randn(dim)).astype(F32)
    delta = rs.randn(dim)
    tr = (0.5 * rs.randn(n), rs.rand(n) + 0.5, 0.1 * rs.randn(m), rs.rand(m) + 0.5)
    d.transforms = None if identity else tuple(a.astype(F32) for a in tr)
    # actions as a rollout gives them, drawn from the policy at theta0: with actions
    # unrelated to the means the largest of 30,000 likelihood ratios passes 1,000
    p = _policy(c, d, d.theta0, None, torch.float64)
    with torch.no_grad():
        mu0 = p.mean(p.old, d.obs).numpy()
    d.act = r32(mu0 + np.exp(d.theta0[-m:].astype(F64)) * eps)
    # the step: KL goes as s^2, so a few rescalings reach the target
    s = 1e-2
    for _ in range(12):
        d.theta1 = (d.theta0 + s * delta).astype(F32)
        p.set_params(d.theta1.astype(F64), set_new=True, set_old=False)
        kl = float(p.kl(d.obs[:T], d.act[:T]).detach())
        if abs(kl / KL_TARGET - 1) < 0.02:
            break
        s *= np.sqrt(KL_TARGET / kl)
    d.step_scale = s
    # fp64 truth over the first T rows (and the VPG over all T_load rows: the shard form)
    lr, klr, ll_new, mu_new = eval_rows(p, d.obs, d.act)
    d.lr, d.kl_rows, d.ll_new, d.mu_new = lr, klr, ll_new, mu_new
    d.surr64, d.kl64 = _evals(c, d, torch.float64)
    d.absmean64 = float(np.mean(np.abs(lr[:T] * d.adv[:T])))
    d.vpg64, d.vpg64_load, d.fv64 = _grads(c, d, torch.float64)
    # the oracle's own fp32 evaluation of the same input, measured against fp64
    s32, k32 = _evals(c, d, torch.float32)
    g32, _, f32_ = _grads(c, d, torch.float32)
    d.err32 = dict(vpg=nrel(g32, d.vpg64), fvp=nrel(f32_, d.fv64), surr=abs(s32 - d.surr64) / d.absmean64,
                   kl=abs(k32 - d.kl64) / d.kl64)
    d.ll0_poison = float(min(LL0_POISON, ll_new[T:].min() - LL0_MARGIN))
    return d


def make_case(c, T):
    """The inputs and the fp64 truth of case c at T rows (cached: treat as read-only;
    the serial / pipelined pair of a split shape shares one)."""
    return _make(c.n, c.m, c.hidden, c.identity, T)


def poison(d, ws):
    """Overwrites what the passes read of the tail rows in the engine workspace `ws`
    (device tensors): the advantages of both kinds, the cached old means and
    log-likelihoods.  The actions stay ordinary: an action of 1e4 would drive
    exp(LL_new - LL_old) to 0 and hide the row."""
    T, R = d.T, d.T_load
    ws["adv32"][T:R].fill_(ADV_POISON)
    ws["adv_vpg"][T:R].fill_(ADV_POISON)
    ws["mu0"][T:R].fill_(MU0_POISON)
    ws["ll0"][T:R].fill_(d.ll0_poison)


def poisoned_row_moves(c, d, i):
    """What tail row i would add if a pass counted it, in the units of the GPU bars:
    (|surrogate term| / (T mean|lr adv|), |KL term| / (T KL), |VPG term| / (T |VPG|))."""
    T = d.T
    surr = np.exp(d.ll_new[i] - d.ll0_poison) * ADV_POISON
    sn = np.maximum(d.theta1[-c.m:].astype(F64), -3.0)
    so = np.maximum(d.theta0[-c.m:].astype(F64), -3.0)
    num = (MU0_POISON - d.mu_new[i]) ** 2 + np.exp(so) ** 2 - np.exp(sn) ** 2
    kl = np.sum(num / (2 * np.exp(sn) ** 2 + 1e-8) + sn - so)
    p = _policy(c, d, d.theta0, None, torch.float64)
    g = p.flat_vpg(d.obs[i:i + 1], d.act[i:i + 1], np.array([ADV_POISON]))
    return (abs(surr) / (T * d.absmean64), abs(kl) / (T * d.kl64),
            float(np.linalg.norm(g) / (T * np.linalg.norm(d.vpg64))))
