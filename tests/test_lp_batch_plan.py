"""The host plan of the batched lookup permutation (csrc/lp_batch_plan.hpp) on the CPU:
tests/native/lp_batch_plan_check.cpp includes only that header and feeds it 60 000 seeded random
pointer sets -- counts 0 .. 17, aliasing tables, overlapping and abutting ranges, misaligned and null
entries, n at the caps, each array in a heap block of exactly its size -- and compares the plan with
the naive quadratic restatement written there: accept or reject and the rule that rejects, the number
of table slots, every lookup's slot, and that no two scratch regions overlap and all lie inside the
reported total.  Built here with the host compiler on its own command line, under AddressSanitizer
and UndefinedBehaviorSanitizer (a stand-alone program: no preload)."""
import os
import re
import shutil
import subprocess

from conftest import PKG, ROOT, sanitizer_prefix

NATIVE = os.path.join(ROOT, "tests", "native")


def test_plan_header_has_no_hip_and_no_field_code_and_api_calls_it_once():
    hpp = open(os.path.join(PKG, "csrc", "lp_batch_plan.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', hpp) == ["cstddef", "cstdint"]
    code = re.sub(r"//.*", "", hpp)
    assert "__device__" not in hpp and "__global__" not in hpp and "hip" not in code.lower() and "Fr" not in code
    api = open(os.path.join(PKG, "csrc", "api.cpp")).read()
    assert api.count("lp_batch_plan(") == 1                  # the entry point runs this text, once
    assert '#include "lp_batch_plan.hpp"' in api
    check = open(os.path.join(NATIVE, "lp_batch_plan_check.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', check) == ["../../snark-verifier-axiom_amd/csrc/lp_batch_plan.hpp"]
    # the numbers the plan restates are the ones of the header and of the kernels' file
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    lp = open(os.path.join(PKG, "csrc", "lookup_permute.hpp")).read()
    assert int(re.search(r"#define SV_LOOKUP_BATCH_MAX (\d+)", h).group(1)) == int(re.search(r"kLpbMax = (\d+);", hpp).group(1))
    assert int(re.search(r"SV_LOOKUP_TABLES_SORTED = (\d+)", h).group(1)) == int(re.search(r"kLpbTablesSorted = (\d+);", hpp).group(1))
    assert re.search(r"kLpTile = (\d+);", lp).group(1) == re.search(r"kLpbTile = (\d+);", hpp).group(1)


def test_plan_agrees_with_the_naive_restatement():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out_dir = os.path.join(NATIVE, "build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "lp_batch_plan_check_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", binary,
                        os.path.join(NATIVE, "lp_batch_plan_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(sanitizer_prefix() + [binary], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "lp_batch_plan_check ok" in r.stdout
