"""The extended-domain predicates (csrc/ext_plan.hpp) on the CPU: tests/native/extended_plan_check.cpp
includes only that header (and through it the NTT's plan), and over the toy field F_65537 runs the
whole coset LDE -- live indices only from a buffer of exactly n entries, dead columns, the
known-zero butterflies of the first min(e, w_0) stages -- and the whole divide / inverse / truncate
-- the 1 / t table by input index, the cut on the last pass's store into a buffer of exactly
pieces n entries -- through the plan's own index functions, against the O(n^2) definitions: every
k <= 6, e <= 4, tile log 1 .. 4, every pieces value, shifts 1 (LDE only), 3 and 3^5.  The predicates
alone are then checked at K = 26 (and at (4, 8), (2, 8)) on sampled indices in 64-bit arithmetic.
Built here with the host compiler on its own command line, under AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone program: no preload)."""
import os
import re
import shutil
import subprocess

from conftest import PKG, ROOT, sanitizer_prefix

NATIVE = os.path.join(ROOT, "tests", "native")


def test_predicate_header_has_no_hip_and_no_field_code():
    hpp = open(os.path.join(PKG, "csrc", "ext_plan.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', hpp) == ["ntt_plan.hpp"]
    assert int(re.search(r"constexpr uint32_t kExtLogMax = (\d+);", hpp).group(1)) == 8
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    assert int(re.search(r"#define SV_EXT_LOG_MAX (\d+)", h).group(1)) == 8


def test_extended_plan_runs_the_round_trip_on_the_cpu():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out_dir = os.path.join(NATIVE, "build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "extended_plan_check_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", binary,
                        os.path.join(NATIVE, "extended_plan_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(sanitizer_prefix() + [binary], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "extended_plan_check ok" in r.stdout
