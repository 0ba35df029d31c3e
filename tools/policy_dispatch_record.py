"""The host-side decisions of the policy-pass dispatch (csrc/policy.hip), over a
sweep of shapes and row counts: for every shape mjrl_shape_init's status and
(np, mp, d, packed), mjrl_fused_path and mjrl_split_supported; for every
(shape, T) mjrl_eval_grid and mjrl_scratch_size's three outputs.  Once as the
library decides by default and once with MJRL_AMD_WGRAD_OLD=1, which the library
reads once per process: each mode is probed in a child process of its own.

    python tools/policy_dispatch_record.py            # print the record of the built library
    python tools/policy_dispatch_record.py --write    # write tests/golden/policy_dispatch.json

tests/test_policy_dispatch.py compares the built library with the committed
file.  The file pins the dispatch across a change that must not move it, so it
is written from the build of the commit BEFORE such a change, never from the
code under test; --write stores the commit it ran at (and refuses a tree whose
csrc differs from that commit).  MJRL_AMD_LIB selects the library build.

Needs no GPU and imports neither torch nor the package: plain ctypes.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "policy_dispatch.json")
LIB_PATH = os.path.join(ROOT, "mjrl_amd", "lib", "libmjrl_amd.so")
MODES = {"default": None, "wgrad_old": "1"}   # the value of MJRL_AMD_WGRAD_OLD

# row counts: the first tiles of every tile size, the caps of the persistent grids
# (256 and 512 workgroups of 32- and 64-row tiles) and one row past them, the two
# tile counts between which ks_grid drops (8192 -> 256, 8224 -> 129), real batches
TS = [0, 1, 31, 32, 33, 64, 65, 256 * 32 - 1, 256 * 32, 256 * 32 + 1, 512 * 32 + 1, 512 * 64 + 1, 8192 * 32,
      8224 * 32, 125000, 1000000]

# shapes beyond tests/pass_ref.py's cases (one per kernel instance): those of
# test_abi.py's test_scratch_size_is_monotonic, shapes no kernel takes (a width
# without an instance, an action count past 64), and (70, 40, 128): H 128, MP 64,
# NPBM 8, the instance k_wgrad_all leaves to k_wgrad
EXTRA_SHAPES = [(6, 2, 0, 0), (8, 2, 64, 64), (17, 6, 128, 128), (376, 17, 64, 64), (39, 28, 256, 256),
                (15, 40, 32, 32), (45, 24, 128, 128),
                (10, 3, 48, 48), (10, 100, 64, 64), (10, 3, 64, 32),
                (70, 40, 128, 128), (120, 40, 128, 128), (140, 6, 128, 128)]


class Shape(C.Structure):   # mjrl_shape
    _fields_ = [(k, C.c_int32) for k in ("n", "m", "h0", "h1", "np", "mp", "d", "packed")]


def shape_key(n, m, h0, h1):
    return "n%d_m%d_h%dx%d" % (n, m, h0, h1)


def probe(lib, shapes, ts=TS, shape_type=Shape):
    """{shape key: record} from a raw library handle: a ctypes.CDLL, or _lib.load()
    with shape_type=_lib.Shape (the structure its argtypes name)."""
    out = {}
    for n, m, h0, h1 in shapes:
        s = shape_type()
        rec = {"init": int(lib.mjrl_shape_init(C.byref(s), n, m, h0, h1)),
               "shape": [s.np, s.mp, s.d, s.packed],
               "fused_path": int(lib.mjrl_fused_path(C.byref(s))),
               "split_supported": int(lib.mjrl_split_supported(C.byref(s))),
               "eval_grid": [], "scratch": []}
        for T in ts:
            rec["eval_grid"].append(int(lib.mjrl_eval_grid(C.byref(s), C.c_int64(T))))
            wf, rd, sl = C.c_int64(), C.c_int64(), C.c_int32()
            rc = lib.mjrl_scratch_size(C.byref(s), C.c_int64(T), C.byref(wf), C.byref(rd), C.byref(sl))
            rec["scratch"].append([int(rc), wf.value, rd.value, sl.value])
        out[shape_key(n, m, h0, h1)] = rec
    return out


def probe_in_child(mode, shapes):
    """probe() in a fresh process with MJRL_AMD_WGRAD_OLD set as the mode says."""
    env = dict(os.environ)
    env.pop("MJRL_AMD_WGRAD_OLD", None)
    if MODES[mode] is not None:
        env["MJRL_AMD_WGRAD_OLD"] = MODES[mode]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit", json.dumps(shapes)], env=env,
                       capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


def _cdll():
    path = os.environ.get("MJRL_AMD_LIB") or LIB_PATH
    if not os.path.isabs(path) and not os.path.exists(path):
        path = os.path.join(ROOT, path)
    return C.CDLL(path)


def _all_shapes():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import pass_ref
    shapes = [(c.n, c.m) + tuple(h) for c in pass_ref.CASES for h in (c.hidden, c.kernel_hidden)] + EXTRA_SHAPES
    return sorted(set(shapes))


def _commit():
    def git(*a):
        return subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True, check=True).stdout.strip()
    if git("status", "--porcelain", "--", "mjrl_amd/csrc", "include"):
        sys.exit("mjrl_amd/csrc or include differ from HEAD: record from a clean checkout of the parent commit")
    return git("rev-parse", "HEAD")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write tests/golden/policy_dispatch.json")
    ap.add_argument("--emit", metavar="SHAPES", help="(child) print probe() of these shapes as JSON")
    ap.add_argument("--commit", help="with --write: the commit the library was built at (default: HEAD, checked clean)")
    args = ap.parse_args()
    if args.emit:
        print(json.dumps(probe(_cdll(), json.loads(args.emit))))
        sys.exit(0)
    shapes = _all_shapes()
    rec = {"commit": (args.commit or _commit()) if args.write else None, "T": TS, "shapes": [list(s) for s in shapes]}
    for mode in MODES:
        rec[mode] = probe_in_child(mode, shapes)
    text = json.dumps(rec, indent=None, separators=(",", ":"), sort_keys=True)
    if args.write:
        with open(GOLDEN, "w") as f:
            f.write(text + "\n")
        print("wrote %s (%d shapes x %d row counts x %d modes, commit %s)"
              % (GOLDEN, len(shapes), len(TS), len(MODES), rec["commit"]))
    else:
        print(text)
