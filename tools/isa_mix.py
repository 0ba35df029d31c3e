"""Static instruction mix of a kernel's tile loop, per barrier interval, from the
compiler's assembly listing (the k_kx table).

    hipcc <the build's flags> --cuda-device-only -S mjrl_amd/csrc/policy.hip -o policy.s
    python tools/isa_mix.py policy.s _ZN...k_kx...        # a mangled name, or a unique part of it
    python tools/isa_mix.py policy.s --list               # the kernels in the listing, with their loops

The tile loop is the loop (a label with a backward branch to it) that holds the
most workgroup barriers; --loop N picks another.  Counts are per wave and per
pass over the loop body as laid out: every instruction between two barriers,
whichever branch it sits under.  Classes: MFMA (v_mfma*), VALU (every other v_*),
LDS (ds_*), vmem (global_* / buffer_* / flat_* / scratch_*), waits, SALU (the
remaining s_*, without s_nop / s_barrier / branches).  --ops adds the most frequent
opcodes of the loop.
"""
import argparse
import collections
import re
import sys

LABEL = re.compile(r"^([.\w$]+):")
INSN = re.compile(r"^\s+([a-z_][a-z0-9_]+)\b(.*)$")
BRANCH = re.compile(r"^s_(c?branch\w*)$")


def kernels(lines):
    """name -> (first, last) line of every function body in the listing."""
    out, cur = {}, None
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m and not m.group(1).startswith(".L"):
            cur = (m.group(1), i)
        elif cur and ln.lstrip().startswith(".Lfunc_end"):
            out[cur[0]] = (cur[1], i)
            cur = None
    return out


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.split("_")[0] in ("global", "buffer", "flat", "scratch"):
        return "vmem"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_barrier":
        return "barrier"
    if op == "s_nop" or BRANCH.match(op) or op in ("s_endpgm", "s_setpc_b64"):
        return "other"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def loops(lines, lo, hi):
    """(barriers, first, last) of every label .. backward-branch span in [lo, hi)."""
    labels = {}
    found = []
    for i in range(lo, hi):
        m = LABEL.match(lines[i])
        if m:
            labels[m.group(1)] = i
            continue
        m = INSN.match(lines[i])
        if m and BRANCH.match(m.group(1)):
            tgt = m.group(2).strip().split()[-1] if m.group(2).strip() else ""
            if tgt in labels:
                a = labels[tgt]
                nb = sum(1 for j in range(a, i) if re.match(r"^\s+s_barrier\b", lines[j]))
                found.append((nb, a, i))
    return sorted(found, reverse=True)


def mix(lines, a, b):
    """Per-interval class counts and the opcode histogram of lines [a, b]."""
    rows, cur, ops = [], collections.Counter(), collections.Counter()
    for i in range(a, b + 1):
        m = INSN.match(lines[i])
        if not m or m.group(1).startswith("."):
            continue
        op = m.group(1)
        c = classify(op)
        if c == "barrier":
            rows.append(cur)
            cur = collections.Counter()
            continue
        cur[c] += 1
        ops[op] += 1
    rows.append(cur)
    return rows, ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("kernel", nargs="?")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--loop", type=int, default=0, help="rank of the loop by barrier count (0: the most)")
    ap.add_argument("--ops", type=int, default=0, metavar="N", help="also the N most frequent opcodes of the loop")
    args = ap.parse_args()
    lines = open(args.listing).read().split("\n")
    ks = kernels(lines)
    if args.list or not args.kernel:
        for name, (lo, hi) in ks.items():
            ls = loops(lines, lo, hi)
            print("%s: %d lines, loops (barriers, lines): %s" % (name, hi - lo, [(n, b - a) for n, a, b in ls[:3]]))
        return
    names = [k for k in ks if k == args.kernel] or [k for k in ks if args.kernel in k]
    if len(names) != 1:
        sys.exit("kernel %r matches %d functions: %s" % (args.kernel, len(names), names[:8]))
    lo, hi = ks[names[0]]
    ls = loops(lines, lo, hi)
    if len(ls) <= args.loop:
        sys.exit("no such loop in %s" % names[0])
    nb, a, b = ls[args.loop]
    rows, ops = mix(lines, a, b)
    cols = ("VALU", "MFMA", "LDS", "vmem", "wait", "SALU")
    print("%s\nloop at lines %d-%d of the listing, %d barriers" % (names[0], a + 1, b + 1, nb))
    print("| interval | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    # the loop body starts after the previous tile's last barrier: the first and the
    # last piece are one interval (loop bottom + loop top)
    pieces = list(rows)
    if len(pieces) > 1:
        pieces[0] = pieces[0] + pieces[-1]
        pieces.pop()
    for i, r in enumerate(pieces):
        print("| %d | " % i + " | ".join(str(r[c]) for c in cols) + " |")
    tot = sum(rows, collections.Counter())
    print("| **loop** | " + " | ".join("**%d**" % tot[c] for c in cols) + " |")
    if args.ops:
        print("\n".join("%5d %s" % (n, op) for op, n in ops.most_common(args.ops)))


if __name__ == "__main__":
    main()
