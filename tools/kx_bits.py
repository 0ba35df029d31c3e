"""Output bits of the split-f16 policy passes (csrc/kx.h k_kx, csrc/kxe.h
k_kx_eval_pipe) on small seeded batches: FWD (separate pack and fused pack),
FVP (a random tangent and one whose W1 block is zero) and EVAL (serial and
pipelined), for every (MP, KG) the library instantiates.

    python tools/kx_bits.py            # print each array's SHA-256 and first values
    python tools/kx_bits.py --write    # write tests/golden/kx_bits.json
    python tools/kx_bits.py --check    # compare with tests/golden/kx_bits.json

tests/test_gpu_kx_bits.py runs `case_arrays` against the committed file.  The
file is written from the build of the commit BEFORE a change that must keep the
bits, never from the code under test (profiles/r09a/README.md names the commit).
MJRL_AMD_LIB selects the library build.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "kx_bits.json")
H = (64, 64)
# (MP, KG) -> (n, m): np = 32 KG, mp = MP; n % 4 == 0 (the fused pack's condition)
SHAPES = {(16, 4): (120, 6), (16, 8): (248, 6), (16, 12): (376, 6),
          (32, 4): (120, 17), (32, 8): (248, 17), (32, 12): (376, 17)}
T_ALL = (1, 33, 97)   # a lone ragged tile; one full tile + 1 row; three full tiles + 1 row
T_MAX = max(T_ALL)
CASES = [(mp, kg, T) for (mp, kg) in ((32, 12), (16, 4)) for T in T_ALL] + \
        [(mp, kg, 33) for (mp, kg) in sorted(SHAPES) if (mp, kg) not in ((32, 12), (16, 4))]


def case_name(mp, kg, T):
    return "mp%d_kg%d_T%d" % (mp, kg, T)


def _d(n, m):
    return 64 * n + 64 + 64 * 64 + 64 + m * 64 + m + m


def inputs(mp, kg):
    """Seeded rows (T_MAX of them; a case takes the first T) and parameters:
    observation columns spanning 1e-6 .. 1e3, column 3 all zero, row 32 all zero
    (the lone row of the ragged tile at T = 33), |adv| = 1e30 on row 0."""
    n, m = SHAPES[(mp, kg)]
    rs = np.random.RandomState(1000 * mp + kg)
    obs = rs.randn(T_MAX, n) * 10.0 ** np.linspace(-6, 3, n)[rs.permutation(n)] / 50.0
    obs[:, 3] = 0.0
    obs[32, :] = 0.0
    obs = obs.astype(np.float32)
    act = rs.randn(T_MAX, m).astype(np.float32)
    adv = rs.randn(T_MAX)
    adv[0] = -1e30
    d = _d(n, m)
    theta = (rs.randn(d) * 0.05).astype(np.float32)
    theta[-m:] = np.linspace(-1.0, 0.3, m)
    theta1 = theta + (rs.randn(d) * 2e-3).astype(np.float32)
    v = (rs.randn(d) * 0.1).astype(np.float32)
    v0 = v.copy()
    w1 = 64 * n + 64   # flat order W0, b0, W1, ...
    v0[w1:w1 + 64 * 64] = 0.0
    return dict(n=n, m=m, obs=obs, act=act, adv=adv, theta=theta, theta1=theta1, v=v, v0=v0)


def case_arrays(mp, kg, T, inp=None):
    """name -> numpy array of every output of the passes over the first T rows."""
    from mjrl_amd import _lib
    from mjrl_amd.engine import UpdateEngine, S_EVAL
    inp = inp or inputs(mp, kg)
    n, m = inp["n"], inp["m"]
    dev = torch.device("cuda:0")
    eng = UpdateEngine(n, m, H, device=dev, precision="split")
    K, s = eng.K, eng.shape
    assert (s.mp, s.np) == (mp, 32 * kg) and K.mjrl_split_supported(s)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {}
    cache = ("a0", "a1", "mu0", "ll0")

    def grab(prefix, names):
        torch.cuda.synchronize()
        for k in names:
            out[prefix + k] = eng.ws[k][:T].cpu().numpy().copy()

    # FWD over rows packed by the separate pack kernel
    eng.load_rows(inp["obs"][:T].astype(np.float64), inp["act"][:T].astype(np.float64), inp["adv"][:T])
    theta = t(inp["theta"])
    eng.forward_pass(theta, T)
    grab("fwd_", cache)
    out["fwd_gsum"] = eng.pvec["gsum"].cpu().numpy().copy()
    xs_ref = eng.ws["xs"][:T].cpu().numpy().copy()
    xu_ref = eng.ws["xu"][:T].cpu().numpy().copy()

    # FVP at those caches: a random tangent, and one whose W1 block is zero
    for key in ("v", "v0"):
        eng.fvp(t(inp[key]), damping=1e-4, T=T)
        torch.cuda.synchronize()
        out["fvp_%s_gsum" % key] = eng.pvec["gsum"].cpu().numpy().copy()

    # EVAL, serial and pipelined
    was = K.mjrl_eval_pipe(-1)
    try:
        for pipe in (0, 1):
            K.mjrl_eval_pipe(pipe)
            G = K.mjrl_eval_grid(s, T)
            eng.stats[S_EVAL:S_EVAL + 2].zero_()
            eng.ws["rpart"][:2 * G].zero_()
            eng.eval_pass(t(inp["theta1"]), T)
            torch.cuda.synchronize()
            tag = "eval_pipe_" if pipe else "eval_serial_"
            out[tag + "sums"] = eng.stats[S_EVAL:S_EVAL + 2].cpu().numpy().copy()
            out[tag + "rpart"] = eng.ws["rpart"][:2 * G].cpu().numpy().copy()
    finally:
        K.mjrl_eval_pipe(was)

    # FWD with the fused pack: caches cleared first, so they are this pass's
    st = _lib.stream_ptr()
    for k in cache + ("xs", "xu"):
        eng.ws[k][:T].zero_()
    obs32 = t(inp["obs"][:T])
    eng.ws["act32"][:T].copy_(t(inp["act"][:T]))
    eng._colscale(obs32, T, st)
    K.mjrl_pack_params(s, eng._pad(theta, "theta"), eng.packed_theta, 1, eng.min_log_std, st)
    _, _, osh, osc = eng.transforms
    K.mjrl_policy_vpg_pack(s, eng._rows(T, eng.ws["adv32"]), obs32, eng.packed_theta, osh, osc, eng._scratch(T),
                           eng.pvec["gsum"], st)
    grab("fwdpack_", cache + ("xs", "xu"))
    out["fwdpack_gsum"] = eng.pvec["gsum"].cpu().numpy().copy()
    # the two packs write the same rows (the fused pack's own contract)
    assert out["fwdpack_xs"].tobytes() == xs_ref.tobytes() and out["fwdpack_xu"].tobytes() == xu_ref.tobytes()
    return out


def digest(arrays):
    rec = {}
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        rec[k] = {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "dtype": str(a.dtype), "shape": list(a.shape),
                  "head": [repr(float(x)) for x in a.reshape(-1)[:8].astype(np.float64)]}
    return rec


def compare(name, got, want):
    """Names of the arrays of case `name` whose bytes differ from the record."""
    bad = []
    for k in sorted(set(got) | set(want)):
        if k not in got or k not in want or got[k]["sha256"] != want[k]["sha256"]:
            bad.append("%s/%s: got %s want %s" % (name, k, got.get(k, {}).get("head"), want.get(k, {}).get("head")))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write tests/golden/kx_bits.json")
    ap.add_argument("--check", action="store_true", help="compare with tests/golden/kx_bits.json")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    rec = {}
    for mp, kg, T in CASES:
        rec[case_name(mp, kg, T)] = digest(case_arrays(mp, kg, T))
    if args.write:
        with open(args.out, "w") as f:
            json.dump({"cases": rec}, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %s: %d cases" % (args.out, len(rec)))
    elif args.check:
        with open(args.out) as f:
            want = json.load(f)["cases"]
        bad = [b for name in rec for b in compare(name, rec[name], want[name])]
        print("\n".join(bad) if bad else "all %d cases identical to %s" % (len(rec), args.out))
        sys.exit(1 if bad else 0)
    else:
        for name in rec:
            for k, v in rec[name].items():
                print(name, k, v["sha256"][:16], v["head"][:3])


if __name__ == "__main__":
    main()
