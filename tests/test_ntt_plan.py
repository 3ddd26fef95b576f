"""The NTT's plan (csrc/ntt_plan.hpp) on the CPU: tests/native/ntt_plan_check.cpp includes only that
header, checks the pass widths for every k in 0..12 and tile log 1..min(k, 6) plus the default tile
log for k <= 16, runs the whole multi-pass decomposition over the toy field F_65537 through the
plan's own index and exponent functions against the O(n^2) DFT (forward and inverse, shift 1 and
shift 3), and checks the exponent functions alone for k in {20, 21, 26} on sampled indices against
i j mod 2^k in 64-bit arithmetic.  Built here with the host compiler on its own command line, under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: no preload)."""
import os
import re
import shutil
import subprocess

from conftest import PKG, ROOT, sanitizer_prefix

NATIVE = os.path.join(ROOT, "tests", "native")
T = int(re.search(r"constexpr uint32_t kNttTileLog = (\d+);", open(os.path.join(PKG, "csrc", "ntt.hpp")).read()).group(1))


def test_default_tile_log_is_in_range():
    hpp = open(os.path.join(PKG, "csrc", "ntt_plan.hpp")).read()
    block = int(re.search(r"constexpr uint32_t kNttBlockLog = (\d+);", hpp).group(1))
    assert 1 <= T <= block


def test_plan_header_runs_the_decomposition_on_the_cpu():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out_dir = os.path.join(NATIVE, "build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "ntt_plan_check_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", binary,
                        os.path.join(NATIVE, "ntt_plan_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(sanitizer_prefix() + [binary, str(T)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "ntt_plan_check ok" in r.stdout and f"default tile log {T}" in r.stdout
