"""Parameter packing, the CG iteration in its four schedules and three init forms,
the NPG step and the device TRPO line search, each called through the C ABI alone
(no UpdateEngine, no policy pass) and compared BIT FOR BIT with the numpy
restatement of their documented arithmetic (vec_ref.py), and hence with each other.

The comparison can be exact because the inputs are chosen so (test_vec_ref.py): every
dot product's exact sum lies further from an f32 rounding boundary than any fp64
summation order can move it, and the log-std block's result does not depend on the
last bits of expf.  The only tolerances here are the fp64 summation bound of the
64-term p.z partials and the expf bracket of the wide log-std test.

Shapes (n, m, h0, h1), by the edge of the d-dependent code they hit:

    (3, 2, 0, 0)          d = 10       linear PackMap branch; less than one wave
    (5, 3, 32, 32)        1,350        2 workgroups; ragged 64- and 256-element tails
    (12, 17, 32, 32)      2,050        log-std entries 2033..2049 straddle a 1024- and a
                                       64-element boundary; mp = 32
    (59, 2, 64, 64)       8,132        k_cgm_xrp_f<8>, masked prefetch
    (60, 2, 64, 64)       8,196        first d on k_cgm_xrp_f<32>
    (376, 17, 64, 64)     29,410       Humanoid
    (39, 28, 256, 256)    83,256       tail loop past 32 x 1024 prefetched terms; 1,301 p.z partials
    (130, 3, 256, 256)    100,102      mjrl_cg_z / _xr_p refuse (1,565 > 1,536 chunks)
    (1756, 1, 256, 256)   515,842      504 workgroups: the last multi-workgroup d
    (1757, 1, 256, 256)   516,098      505: the single-workgroup k_cg_init, k_cg_step, k_npg_step

mjrl_shape_init supports all of them (hidden 0 / 32 / 64 / 256, mp 16 / 32)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vec_ref as V

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, U32 = np.float32, np.float64, np.uint32
NAN = U32(V.NAN_BITS).view(F32)
SHAPES = list(V.CG_SHAPES)
FUSED_MAX_D = 64 * (V.CG_STATE - V.CG_PZ_PARTS) // 2      # mjrl_cg_z / mjrl_cg_step_xr_p above it: MJRL_EINVAL
SCHEDULES = ("step", "z_xr_p", "step1", "update")


def _id(shape):
    return "d%d" % V.make_shape(*shape).d


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(n):
    """n words that an unwritten position keeps: the NaN pattern of vec_ref."""
    return _dev(np.full(n, NAN, F32))


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want, what):
    got = _host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.view(U32) != want.view(U32))[0]
    assert len(bad) == 0, "%s: %d of %d words differ, first at %s: got %r, reference %r" % (
        what, len(bad), got.size, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


@pytest.fixture(scope="module")
def K():
    from mjrl_amd import _lib
    return _lib.calls()


@pytest.fixture(scope="module")
def st():
    from mjrl_amd import _lib
    return _lib.stream_ptr()


def _shape(shape):
    """The library's structure for `shape`, which must equal the reference's."""
    from mjrl_amd import _lib
    s, r = _lib.make_shape(*shape), V.make_shape(*shape)
    assert tuple(getattr(s, k) for k in r._fields) == tuple(r), shape
    return s


# --------------------------------------------------------------------------
# mjrl_pack_params
# --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("clamp", [0, 1])
def test_pack_params(K, st, shape, clamp):
    """Bitwise vec_ref.pack; with the clamp, log-std entries below min_log_std and one
    equal to it.  Positions outside the written mask keep their pre-fill."""
    s, r = _shape(shape), V.make_shape(*shape)
    rs = np.random.RandomState(3)
    theta = rs.standard_normal(r.d).astype(F32)
    theta[r.d - r.m:] = np.linspace(-4.0, -2.0, r.m)
    theta[r.d - 1] = V.MIN_LS
    packed = _nan(r.packed)
    K.mjrl_pack_params(s, _dev(theta), packed, clamp, V.MIN_LS, st)
    want, mask = V.pack(r, theta, bool(clamp), V.MIN_LS, fill=NAN)
    _same(packed, want, "packed")


# --------------------------------------------------------------------------
# CG: device state of one case, the init forms and the schedules
# --------------------------------------------------------------------------
class Cg:
    """The device buffers of one CG run.  r and p are pairs: the one-launch schedules
    write the other buffer of the pair (`ri`, `pi` index the current one)."""

    def __init__(self, c, cg=None):
        r = c["s"]
        self.c, self.r, self.s = c, r, _shape(c["shape"])
        self.b = _dev(c["b"])
        self.x = _nan(r.d)
        self.rb = [_nan(r.d), _nan(r.d)]
        self.pb = [_nan(r.d), _nan(r.d)]
        self.z = _nan(r.d)
        self.packed_p = _nan(r.packed)
        self.packed_theta = _dev(V.pack(r, c["theta"])[0])
        self.cg = cg if cg is not None else torch.zeros(V.CG_STATE, dtype=torch.float32, device=DEV)
        self.done = torch.full((1,), 1, dtype=torch.int32, device=DEV)
        self.ri = self.pi = 0
        self.gs = [_dev(g) for g in c["gsums"]]
        self.zref = [_dev(stt["z"]) for stt in c["states"][1:]]

    def init(self, K, st, schedule):
        self.ri = self.pi = 0
        if schedule == "update":
            K.mjrl_cg_init_vec(self.r.d, self.b, self.x, self.rb[0], self.pb[0], self.cg, self.done, st)
        else:
            K.mjrl_cg_init(self.s, self.b, self.x, self.rb[0], self.pb[0], self.packed_p, self.cg, self.done, st)

    def iterate(self, K, st, schedule, k, tol):
        c, s = self.c, self.s
        r, p, ro, po = self.rb[self.ri], self.pb[self.pi], self.rb[1 - self.ri], self.pb[1 - self.pi]
        if schedule == "step":
            K.mjrl_cg_step(s, self.gs[k], c["inv_T"], c["damping"], self.packed_theta, self.x, r, p, self.z,
                           self.packed_p, self.cg, self.done, tol, st)
        elif schedule == "z_xr_p":
            K.mjrl_cg_z(s, self.gs[k], c["inv_T"], c["damping"], self.packed_theta, p, self.z, self.cg, self.done, st)
            K.mjrl_cg_step_xr_p(s, self.x, r, ro, p, self.z, self.packed_p, self.cg, self.done, tol, st)
        elif schedule == "step1":
            K.mjrl_cg_step1(s, self.gs[k], c["inv_T"], c["damping"], self.packed_theta, self.x, r, ro, p, po,
                            self.packed_p, self.cg, self.done, tol, st)
        else:
            K.mjrl_cg_update(self.r.d, self.zref[k], self.x, r, p, self.cg, self.done, tol, st)

    def advance(self, schedule):
        """The buffers a launch that was not skipped has moved on to."""
        if schedule in ("z_xr_p", "step1"):
            self.ri = 1 - self.ri
        if schedule == "step1":
            self.pi = 1 - self.pi

    def check(self, want, schedule, what, p=True, z=True):
        r = self.r
        ncg = 5 if want["cg"][1] > 0 else 2     # an init sets rdotr and the iteration count only
        _same(self.x, want["x"], what + " x")
        _same(self.rb[self.ri], want["r"], what + " r")
        if p:
            _same(self.pb[self.pi], want["p"], what + " p")
            if schedule != "update":
                _same(self.packed_p, V.pack(r, want["p"], fill=NAN)[0], what + " packed_p")
        if z and want["z"] is not None and schedule in ("step", "z_xr_p"):
            _same(self.z, want["z"], what + " z")
        _same(self.cg[:ncg], want["cg"][:ncg], what + " cg[0..%d] (rdotr, iterations, v, mu, p.z)" % (ncg - 1))
        assert int(_host(self.done)[0]) == want["done"], what + " done"
        assert _host(self.cg).view(U32)[8] == 0, what + " ticket not reset"

    def snapshot(self):
        return [_host(t).copy() for t in (self.x, self.rb[0], self.rb[1], self.pb[0], self.pb[1], self.packed_p,
                                          self.z, self.cg, self.done)]


def _schedules(r):
    return [sch for sch in SCHEDULES if sch != "z_xr_p" or r.d <= FUSED_MAX_D]


def _pz_partials(run, k):
    """Schedule 2's p.z partials of iteration k (doubles at cg[1024 + 2 i]): each within
    the summation bound 64 2^-53 sum|terms| of its 64 parameters' exact sum."""
    c, r = run.c, run.r
    ng = (r.d + 63) // 64
    got = _host(run.cg)[V.CG_PZ_PARTS:].view(F64)[:ng]
    ex, sabs = V.chunk_sums(c["states"][k]["p"], c["states"][k + 1]["z"], 64)
    bad = np.nonzero(np.abs(got - ex) > 64 * 2.0 ** -53 * sabs)[0]
    assert len(bad) == 0, (k, bad[:6].tolist(), got[bad[:6]].tolist(), ex[bad[:6]].tolist())


def _three_iterations(K, st, run, schedule, what):
    c = run.c
    run.init(K, st, schedule)
    run.check(c["states"][0], schedule, "%s %s init" % (what, schedule))
    for k in range(V.CG_ITERS):
        run.iterate(K, st, schedule, k, c["tol_never"])
        run.advance(schedule)
        run.check(c["states"][k + 1], schedule, "%s %s iteration %d" % (what, schedule, k + 1))
        if schedule == "z_xr_p":
            _pz_partials(run, k)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_cg_init_forms(K, st, shape):
    """mjrl_cg_init, mjrl_cg_init_scaled and mjrl_scale_vec + mjrl_cg_init: the same
    bits in g, x, r, p, packed_p, cg[0], cg[1] and done, all equal to the reference."""
    c = V.cg_case(shape)
    r = c["s"]
    want = c["states"][0]
    gsum0 = _dev(c["gsum0"])
    for form in ("init", "init_scaled", "scale_vec + init"):
        run = Cg(c)
        run.cg[1] = 7.0     # iterations of an earlier solve
        g = _nan(r.d)
        if form == "init":
            g = run.b
            K.mjrl_cg_init(run.s, g, run.x, run.rb[0], run.pb[0], run.packed_p, run.cg, run.done, st)
        elif form == "init_scaled":
            K.mjrl_cg_init_scaled(run.s, gsum0, c["scale"], g, run.x, run.rb[0], run.pb[0], run.packed_p, run.cg,
                                  run.done, st)
        else:
            K.mjrl_scale_vec(gsum0, r.d, c["scale"], g, st)
            K.mjrl_cg_init(run.s, g, run.x, run.rb[0], run.pb[0], run.packed_p, run.cg, run.done, st)
        _same(g, c["b"], form + " g")
        run.check(want, "step", form)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_cg_three_teacher_forced_iterations(K, st, shape):
    """Every schedule, three iterations, each checked bitwise against the reference
    (and hence against the other schedules): x, r, p, packed_p, z where it is stored,
    cg[0..4], done; schedule 2's p.z partials within their summation bound."""
    c = V.cg_case(shape)
    for schedule in _schedules(c["s"]):
        _three_iterations(K, st, Cg(c), schedule, "fresh state")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_cg_ticket_reuse(K, st, shape):
    """The whole sequence twice on one cg buffer, cg[8] never re-zeroed by the host:
    every launch leaves the ticket ready for the next, whichever schedule follows."""
    c = V.cg_case(shape)
    cg = torch.zeros(V.CG_STATE, dtype=torch.float32, device=DEV)
    for rep in range(2):
        for schedule in _schedules(c["s"]):
            _three_iterations(K, st, Cg(c, cg), schedule, "pass %d on one cg buffer" % rep)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_cg_convergence(K, st, shape):
    """residual_tol between r.r of iterations 1 and 2: after iteration 2, x, r, the
    scalars and done == 1 match the reference (p for the schedules documented to update
    it on the converging iteration), and a third launch changes no byte."""
    c = V.cg_case(shape)
    r = c["s"]
    single_wg = (r.d + 1023) // 1024 > (V.CG_PZ_PARTS - 16) // 2
    for schedule in _schedules(r):
        run = Cg(c)
        what = "converging " + schedule
        run.init(K, st, schedule)
        for k in range(2):
            run.iterate(K, st, schedule, k, float(c["tol_conv"]))
            run.advance(schedule)
            p_updated = k == 0 or schedule in ("step1", "update") or (schedule == "step" and single_wg)
            run.check(c["conv"][k + 1], schedule, "%s iteration %d" % (what, k + 1), p=p_updated)
        before = run.snapshot()
        run.iterate(K, st, schedule, 2, float(c["tol_conv"]))
        for a, b, name in zip(before, run.snapshot(), ("x", "r0", "r1", "p0", "p1", "packed_p", "z", "cg", "done")):
            assert np.array_equal(a.view(U32 if a.dtype != np.int32 else np.int32),
                                  b.view(U32 if b.dtype != np.int32 else np.int32)), \
                "%s: a launch after convergence changed %s" % (what, name)
        assert _host(run.cg)[1] == 2


@pytest.mark.parametrize("shape", [sh for sh in SHAPES if V.CG_SHAPES[sh] > FUSED_MAX_D], ids=_id)
def test_fused_schedule_refuses_large_d(K, st, shape):
    """Beyond the p.z partials the CG state holds, mjrl_cg_z and mjrl_cg_step_xr_p
    return MJRL_EINVAL and write nothing."""
    from mjrl_amd import _lib
    L = _lib.lib()
    c = V.cg_case(shape)
    run = Cg(c)
    run.init(K, st, "step")
    before = run.snapshot()
    sp, P = C.byref(run.s), _lib.ptr
    assert L.mjrl_cg_z(sp, P(run.gs[0]), c["inv_T"], c["damping"], P(run.packed_theta), P(run.pb[0]), P(run.z),
                       P(run.cg), P(run.done), st) == _lib.MJRL_EINVAL
    assert L.mjrl_cg_step_xr_p(sp, P(run.x), P(run.rb[0]), P(run.rb[1]), P(run.pb[0]), P(run.z), P(run.packed_p),
                               P(run.cg), P(run.done), 1e-10, st) == _lib.MJRL_EINVAL
    for a, b in zip(before, run.snapshot()):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_log_std_curvature_wide_range(K, st):
    """log_std over [-10, 2] (m = 64), across 2 sigma^2 = 1e-8 where the closed form's
    numerator changes sign: z on the log-std block from mjrl_cg_z and from mjrl_cg_step
    lies inside the fp64 closed form's values at exp(log_std) (1 -+ 2^-22) (what any
    f32 expf within two ulps can give), widened by one f32 ulp.  The bracket comes from
    the reference alone."""
    r = V.make_shape(*V.WIDE_SHAPE)
    s = _shape(V.WIDE_SHAPE)
    rs = np.random.RandomState(11)
    ls0 = r.d - r.m
    assert ls0 < 4096 < r.d and ls0 % 64      # the block across a workgroup boundary, starting inside a chunk
    log_std = np.linspace(-10.0, 2.0, r.m).astype(F32)
    theta = (0.1 * rs.standard_normal(r.d)).astype(F32)
    theta[ls0:] = log_std
    b = rs.standard_normal(r.d).astype(F32)
    gsum = (V.CG_T * 1.5 * b.astype(F64)).astype(F32)
    sg = np.exp(log_std.astype(F64))
    assert (2 * sg[0] ** 2 < 1e-8 < 2 * sg[-1] ** 2)
    pl = b[ls0:].astype(F64)
    cands = np.stack([(V.logstd_curv(sg * f) * pl).astype(F32) + F32(V.CG_DAMPING) * b[ls0:]
                      for f in (1 - 2.0 ** -22, 1.0, 1 + 2.0 ** -22)])
    lo = np.nextafter(cands.min(0), F32(-np.inf))
    hi = np.nextafter(cands.max(0), F32(np.inf))
    zmean = (gsum[:ls0].astype(F64) * (1.0 / V.CG_T)).astype(F32) + F32(V.CG_DAMPING) * b[:ls0]
    packed_theta = _dev(V.pack(r, theta)[0])
    for entry in ("mjrl_cg_z", "mjrl_cg_step"):
        x, rr_, p, z, pp = _nan(r.d), _nan(r.d), _nan(r.d), _nan(r.d), _nan(r.packed)
        cg = torch.zeros(V.CG_STATE, dtype=torch.float32, device=DEV)
        done = torch.zeros(1, dtype=torch.int32, device=DEV)
        K.mjrl_cg_init(s, _dev(b), x, rr_, p, pp, cg, done, st)
        if entry == "mjrl_cg_z":
            K.mjrl_cg_z(s, _dev(gsum), 1.0 / V.CG_T, V.CG_DAMPING, packed_theta, p, z, cg, done, st)
        else:
            K.mjrl_cg_step(s, _dev(gsum), 1.0 / V.CG_T, V.CG_DAMPING, packed_theta, x, rr_, p, z, pp, cg, done,
                           1e-10, st)
        zz = _host(z)
        _same(zz[:ls0], zmean, entry + " z on the mean block")
        bad = np.nonzero(~((lo <= zz[ls0:]) & (zz[ls0:] <= hi)))[0]
        assert len(bad) == 0, (entry, bad.tolist(), zz[ls0:][bad].tolist(), lo[bad].tolist(), hi[bad].tolist(),
                               log_std[bad].tolist())


# --------------------------------------------------------------------------
# mjrl_npg_step and mjrl_trpo_trial
# --------------------------------------------------------------------------
def _npg_buffers(c):
    r = c["s"]
    return dict(g=_dev(c["g"]), x=_dev(c["x"]), theta=_dev(c["theta"]), theta_new=_nan(r.d),
                packed_new=_nan(r.packed), out=torch.zeros(V.STEP_OUT, dtype=torch.float32, device=DEV))


def _npg_call(K, st, s, c, B, run):
    K.mjrl_npg_step(s, B["g"], B["x"], B["theta"], run["mode"], c["delta"], c["alpha_in"], run["const_lr"],
                    V.MIN_LS, B["theta_new"], B["packed_new"], B["out"], st)


@pytest.mark.parametrize("shape", V.NPG_SHAPES, ids=_id)
def test_npg_step(K, st, shape):
    """Modes 0, 1 and 1 with const_lr, one after another on the same out buffer (its
    ticket is reused), each twice: out[0..2], theta_new and the packed copy, bitwise."""
    c = V.npg_case(shape)
    r, s = c["s"], _shape(shape)
    B = _npg_buffers(c)
    for name in ("mode0", "mode1", "const_lr"):
        run = c["runs"][name]
        for rep in range(2):
            B["theta_new"].copy_(_nan(r.d))
            B["packed_new"].copy_(_nan(r.packed))
            _npg_call(K, st, s, c, B, run)
            what = "%s call %d" % (name, rep)
            _same(B["out"][:3], run["out"], what + " out[0..2] (alpha, g.x, delta)")
            _same(B["theta_new"], run["theta_new"], what + " theta_new")
            _same(B["packed_new"], V.pack(r, run["theta_new"], fill=NAN)[0], what + " packed_new")
            assert _host(B["out"]).view(U32)[8] == 0, what + " ticket not reset"


def _ls0():
    return np.full(V.LS_STATE, -7.0, F32)    # whatever an earlier search left: only written slots may change


@pytest.mark.parametrize("shape", V.TRPO_SHAPES, ids=_id)
def test_trpo_trial(K, st, shape):
    """After a mode-0 step: reject, reject (kl == kl_dist exactly), accept, then a trial
    after acceptance; and a rejecting trial with apply = 0.  The log, ls[1], ls[2],
    ls[8 + k], the f32 alpha chain, theta_new / packed_new after each trial, skip and
    out[0]."""
    from mjrl_amd import _lib
    c = V.npg_case(shape)
    r, s = c["s"], _shape(shape)
    run0 = c["runs"]["mode0"]
    T, kl_dist = 1024, 0.0625
    inv_T = 1.0 / T
    # (surrogate sum, KL sum) the host writes before each trial
    reject, on_the_bound, accept = (3.5 * T, 0.31 * T), (2.25 * T, kl_dist * T), (1.7 * T, 0.01 * T)
    assert F32(on_the_bound[1] * inv_T) == F32(kl_dist)
    for apply_last in (1, 0):
        B = _npg_buffers(c)
        _npg_call(K, st, s, c, B, run0)
        ls = _dev(_ls0())
        skip = torch.full((1,), 5, dtype=torch.int32, device=DEV)      # trial 1 starts the search: it sets the flag
        ref = V.TrpoSearch(r, c["x"], c["theta"], V.MIN_LS, run0["out"][0], run0["theta_new"], _ls0())
        seq = [(1, reject, 1), (2, on_the_bound, 1), (3, accept, 1), (4, reject, 1)] if apply_last else \
              [(1, reject, 1), (2, on_the_bound, 0)]      # apply = 0 ends a sequence
        for k, sums, apply in seq:
            K.mjrl_trpo_trial(s, B["x"], B["theta"], V.MIN_LS, B["theta_new"], B["packed_new"], B["out"],
                              _dev(np.array(sums, F64)), inv_T, kl_dist, k, apply, ls, skip, st)
            ref.trial(k, sums, inv_T, kl_dist, apply)
            what = "trial %d (apply %d)" % (k, apply)
            _same(ls, ref.ls, what + " ls")
            assert int(_host(skip)[0]) == ref.skip, what + " skip"
            _same(B["out"][:3], np.array([ref.out0, run0["out"][1], run0["out"][2]], F32), what + " out")
            _same(B["theta_new"], ref.theta_new, what + " theta_new")
            _same(B["packed_new"], V.pack(r, ref.theta_new, fill=NAN)[0], what + " packed_new")
        a0 = run0["out"][0]
        a1 = F32(0.9) * a0
        if apply_last:
            a2 = F32(0.9) * a1
            assert ref.skip == 1 and ref.ls[1] == 1 and ref.ls[2] == 3 and ref.out0 == a2
            assert ref.ls[9] == a1 and ref.ls[10] == a2 and ref.ls[11] == F32(-7.0)
            assert ref.ls[V.LS_LOG:V.LS_LOG + 9].tolist() == [a0, F32(0.31), F32(3.5), a1, F32(kl_dist), F32(2.25),
                                                              a2, F32(0.01), F32(1.7)]
        else:
            assert ref.skip == 0 and ref.ls[2] == 2 and ref.ls[9] == a1 and ref.ls[10] == F32(-7.0)
            assert np.array_equal(ref.theta_new, V.apply_step(r, c["theta"], c["x"], a1, V.MIN_LS))
    L = _lib.lib()
    P = _lib.ptr
    sums = _dev(np.array(reject, F64))
    before = [_host(t).copy() for t in (ls, skip, B["theta_new"], B["packed_new"], B["out"])]
    for k in (0, 24):
        assert L.mjrl_trpo_trial(C.byref(s), P(B["x"]), P(B["theta"]), V.MIN_LS, P(B["theta_new"]),
                                 P(B["packed_new"]), P(B["out"]), P(sums), inv_T, kl_dist, k, 1, P(ls), P(skip),
                                 st) == _lib.MJRL_EINVAL
    for a, t in zip(before, (ls, skip, B["theta_new"], B["packed_new"], B["out"])):
        assert np.array_equal(a.view(np.int32), _host(t).view(np.int32))
