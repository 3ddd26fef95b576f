"""The walk over an expression program (csrc/expr_plan.hpp) on the CPU: tests/native/expr_plan_check.cpp
includes only that header and feeds the walk 400 000 seeded random op arrays -- raw random bytes,
programs grown op by op, arrays one op short or long of every cap, each in a heap block of exactly
its size -- and every hand-written rejection of rule 6 of sv_bn254_fr_expressions_device; the walk
must agree with the naive simulation written there on accept or reject, the deepest stack, the FOLD
count and the tables' marks.  Built here with the host compiler on its own command line, under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: no preload)."""
import os
import re
import shutil
import subprocess

from conftest import PKG, ROOT, sanitizer_prefix

NATIVE = os.path.join(ROOT, "tests", "native")


def test_walk_header_has_no_hip_and_no_field_code():
    hpp = open(os.path.join(PKG, "csrc", "expr_plan.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', hpp) == ["cstddef", "cstdint"]
    assert "__device__" not in hpp and "Fr" not in re.sub(r"//.*", "", hpp)
    api = open(os.path.join(PKG, "csrc", "api.cpp")).read()
    assert api.count("expr_walk(") == 1                      # the entry point runs this text, once
    check = open(os.path.join(NATIVE, "expr_plan_check.cpp")).read()
    assert [i for i in re.findall(r'#include\s+"([^"]+)"', check)] == ["../../snark-verifier-axiom_amd/csrc/expr_plan.hpp"]


def test_expr_walk_agrees_with_the_naive_simulation():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out_dir = os.path.join(NATIVE, "build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "expr_plan_check_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", binary,
                        os.path.join(NATIVE, "expr_plan_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(sanitizer_prefix() + [binary], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "expr_plan_check ok" in r.stdout
