"""Switches the library reads once per process, each run in a process of its own.

decider.hip keeps SVGPU_DECIDER_KC and SVGPU_DECIDER_PHASES in function-local statics, msm_plan.hpp
SVGPU_SORT_XCD and SVGPU_SORT_BM, api.cpp SVGPU_GATHER_AHEAD: by the time a test of this process
sets one with monkeypatch the value is frozen, so the other side of the switch only runs in a child
started with the variable in its environment.  The children (tests/decider_variant_child.py,
tests/msm_variant_child.py) compare with the C++ oracle themselves and exit non-zero on a mismatch.
One child at a time, each under its own timeout, no retry.

SVGPU_DECIDER_PHASES is a profiling knob: k_decide_lanes treats it as a bit mask (1: the Miller
loop, 2: the final exponentiation) and by its own comment results are only valid at 3.  So 3 is the
one value a child can be started with and compared: that pins the parse of the variable and that an
explicit 3 is the default; 1 and 2 compute no pairing and are not run."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _child(script, args, env):
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", script)] + args,
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{env}: exit {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "OK"


@pytest.mark.parametrize("env", [
    {"SVGPU_DECIDER_KC": "0", "SVGPU_DECIDER_LANES": "256"},
    {"SVGPU_DECIDER_PHASES": "3", "SVGPU_DECIDER_LANES": "48"},
    {"SVGPU_DECIDER_PHASES": "3", "SVGPU_DECIDER_LANES": "24"},
], ids=["KC=0,LANES=256", "PHASES=3,LANES=48", "PHASES=3,LANES=24"])
def test_decider_switches_read_once(gpu, env):
    """SVGPU_DECIDER_KC=0: k_decide_wg with d_kc = nullptr evaluates the lines instead of taking the
    pair products from the key's constants.  (test_decider_prologue_variants[SVGPU_DECIDER_KC=0]
    sets the variable in a process that has decided before, where it no longer takes effect.)
    SVGPU_DECIDER_PHASES=3 on both k_decide_lanes instantiations: see the module docstring."""
    _child("decider_variant_child.py", [], env)


@pytest.mark.parametrize("mode,env", [
    ("arrays", {"SVGPU_SORT_XCD": "0"}),
    ("arrays", {"SVGPU_SORT_BM": "0"}),
    ("refs", {"SVGPU_GATHER_AHEAD": "1"}),
], ids=["SORT_XCD=0", "SORT_BM=0", "GATHER_AHEAD=1"])
def test_msm_switches_read_once(gpu, mode, env):
    """One 20 000-point MSM against the C++ Pippenger: the sort passes without the XCD-aware block
    map, the key-major per-block counts (k_bin_scan_chunks), and the reference gather with a
    prefetch distance of one."""
    _child("msm_variant_child.py", [mode, "20000"], env)
