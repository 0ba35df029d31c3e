"""pow2_scale (csrc/pow2_scale.h, the exponent-field form) against the frexpf /
ldexpf formulation it replaced, over every float bit pattern, on the host.

A stand-alone C++ program (its own main, no HIP) includes the header, walks all
2^32 patterns (both signs, zeros, subnormals, Inf, every NaN) on a few threads and
compares the bits of both results with the reference, which is the earlier device
code copied here.  Where the contract promises it (0 < M < 3.0e38f) it also checks
s * inv == 1 and, for M >= 2^-112 (above the clamp), M * s in [2^14, 2^15).
A second build with -fsanitize=undefined walks every 251st pattern (all exponents,
both signs) for the shift / subtraction arithmetic.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "pow2_scale.h"

// the formulation pow2_scale.h replaces (csrc/common.h before it): the reference
static float ref_pow2_scale(float M, float& inv) {
    if (!(M > 0.f) || !(M < 3.0e38f)) {
        inv = 1.f;
        return 1.f;
    }
    int E;
    frexpf(M, &E);
    E = E < -111 ? -111 : E;
    inv = ldexpf(1.f, E - 15);
    return ldexpf(1.f, 15 - E);
}

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float flt(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

int main(int argc, char** argv) {
    const uint64_t stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const unsigned nt = argc > 2 ? atoi(argv[2]) : 8;
    std::atomic<uint64_t> bad{0}, seen{0}, promised{0}, ranged{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            uint64_t nbad = 0, n = 0, np = 0, nr = 0;
            const uint64_t lo = (1ull << 32) * t / nt, hi = (1ull << 32) * (t + 1) / nt;
            for (uint64_t u = lo + (stride - lo % stride) % stride; u < hi; u += stride) {
                const float M = flt((uint32_t)u);
                float ri, gi;
                const float rs = ref_pow2_scale(M, ri);
                const float gs = mjrl::pow2_scale(M, gi);
                ++n;
                bool ok = bits(rs) == bits(gs) && bits(ri) == bits(gi);
                if (M > 0.f && M < 3.0e38f) {
                    ++np;
                    ok = ok && gs * gi == 1.f;
                    if (M >= 0x1p-112f) {
                        ++nr;
                        const float y = M * gs;
                        ok = ok && y >= 16384.f && y < 32768.f;
                    }
                } else {
                    ok = ok && gs == 1.f && gi == 1.f;
                }
                if (!ok && nbad++ < 4)
                    fprintf(stderr, "M bits %08x: got s %08x inv %08x, reference s %08x inv %08x\n", (unsigned)u,
                            bits(gs), bits(gi), bits(rs), bits(ri));
            }
            bad += nbad; seen += n; promised += np; ranged += nr;
        });
    for (auto& x : th) x.join();
    printf("patterns %llu promised %llu ranged %llu bad %llu\n", (unsigned long long)seen,
           (unsigned long long)promised, (unsigned long long)ranged, (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""


def _build(tmp_path, name, flags):
    src = tmp_path / "pow2_scale_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "mjrl_amd", "csrc")] + \
        flags + [str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def _counts(out):
    w = out.split()
    return {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}


def test_every_float_bit_pattern(tmp_path):
    exe = _build(tmp_path, "check", ["-O2"])
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    r = subprocess.run([exe, "1", str(threads)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    c = _counts(r.stdout)
    assert c["patterns"] == 1 << 32 and c["bad"] == 0
    # 0 < M < 3.0e38f: the positive patterns 1 .. bits(3.0e38f) - 1
    assert c["promised"] == 0x7F61B1E6 - 1
    # of them M >= 2^-112: from the pattern of 2^-112 (exponent field 15) up
    assert c["ranged"] == 0x7F61B1E6 - (15 << 23)


def test_shift_arithmetic_under_ubsan(tmp_path):
    exe = _build(tmp_path, "check_ubsan", ["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "251", "4"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    c = _counts(r.stdout)
    assert c["bad"] == 0 and c["patterns"] >= (1 << 32) // 251
