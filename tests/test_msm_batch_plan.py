"""The batched-MSM host planning (csrc/msm_batch_plan.hpp: switches, route, workspace layouts, the
small / big split, the fused-launch slot) and the host's batched affine conversion (csrc/host_ec.hpp),
run on the host through tests/native/msm_batch_plan_check.cpp: the route of every call agrees with
the table of tests/test_gpu_msm_batch_dispatch.py restated here, every buffer holds what its users
index, and the reserved total is the byte sum the driver computed before the layout was declared
once, less its two 1-byte dummy carves.  CPU only."""
import json
import os
import re
import subprocess

import pytest

from conftest import sanitizer_prefix
from oracle import bn254 as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")

COUNTS = [1, 4, 5, 64, 65, 512, 513, 4096, 4097, 65535, 65536, 2**31 - 1]
MAX_TERMS = [1, 255, 256, 257, 600, 4096]
SWITCHES = ["QUAD=0", "BUCKETS=0", "FUSE=0", "WINDOW_BITS=5", "WINDOW_BITS=8", "WINDOW_BITS=7", "HOST_MAX=0",
            "HOST_MAX=100000", "BW=0", "BW=1", "BW=26", "BW=1000", "WAIT_SPINS=0"]
XYZZ, AFF = 128, 64
QW, QB, UPW = 26, 16, 5          # windows of a 128-bit half at 5 bits, buckets per window, U_k per window
SPLIT_LENGTHS = "1 256 257 4096 4097"
AFFINE_KS = [0, 5, 0, 0, 7, 1, 123456789, 0]  # identities first, last and adjacent


def call_cases():
    """'COUNT MAX_TERMS IDS BIDX [NAME=VALUE]': the whole grid without switches, and each switch at
    every count on both sides of the 256-term limit."""
    out = ["%d %d %d %d" % (n, m, ids, bidx) for n in COUNTS for m in MAX_TERMS for ids in (0, 1) for bidx in (0, 1)]
    out += ["%d %d 0 0 SVGPU_BATCH_%s" % (n, m, sw) for sw in SWITCHES for n in COUNTS for m in (256, 257)]
    return out


OTHER_CASES = ["fixed", "slot", "affine " + " ".join(map(str, AFFINE_KS)),
               "split " + SPLIT_LENGTHS,
               "split 1 256 257 4096",                                   # 4 MSMs: SVGPU_BATCH_SEQ_MAX's default
               "split " + SPLIT_LENGTHS + " SVGPU_BATCH_MAX=256",
               "split " + SPLIT_LENGTHS + " SVGPU_BATCH_MAX=100000",
               "split " + SPLIT_LENGTHS + " SVGPU_BATCH_SEQ_MAX=5",
               "split 1 256 257 4096 SVGPU_BATCH_SEQ_MAX=0",
               "split 1 256 257 4096 SVGPU_BATCH_MAX=100"]


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("SVGPU_")}


@pytest.fixture(scope="module", params=["msm_batch_plan_check", "msm_batch_plan_check_asan"])
def plans(request):
    """{case: the harness's JSON} from the harness as built, and again under ASan + UBSan."""
    r = subprocess.run(["make", "-s", "-C", NATIVE, "build/" + request.param], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    binary = os.path.join(NATIVE, "build", request.param)
    cs = call_cases() + OTHER_CASES
    cmd = (sanitizer_prefix() if binary.endswith("_asan") else []) + [binary, "-"]
    r = subprocess.run(cmd, input="\n".join(cs) + "\n", capture_output=True, text=True, env=_clean_env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cs)
    return {c: json.loads(line) for c, line in zip(cs, lines)}


def _calls(plans):
    for case in call_cases():
        f = case.split()
        sw = dict(w[len("SVGPU_BATCH_"):].split("=") for w in f[4:])
        yield case, plans[case], int(f[0]), int(f[1]), f[2] == "1", f[3] == "1", sw


def test_case_count(plans):
    assert len(call_cases()) == 12 * 6 * 4 + 13 * 12 * 2


def test_single_case_from_arguments_and_environment(plans):
    """The harness's one-case form reads the switches from the environment, as the library does."""
    binary = os.path.join(NATIVE, "build", "msm_batch_plan_check")
    env = _clean_env()
    env["SVGPU_BATCH_BUCKETS"] = "0"
    out = subprocess.run([binary, "65", "256", "0", "0"], capture_output=True, text=True, env=env, check=True).stdout
    assert json.loads(out) == plans["65 256 0 0 SVGPU_BATCH_BUCKETS=0"]
    assert json.loads(out) != plans["65 256 0 0"]


def _expected_route(count, max_terms, ids, bidx, sw):
    """The dispatch table of tests/test_gpu_msm_batch_dispatch.py's docstring and its fallbacks, first
    match wins -> (route, window bits, Horner kind of the per-window routes)."""
    on = lambda name: int(sw.get(name, "1")) != 0
    forced = int(sw.get("WINDOW_BITS", "0"))
    c = forced if forced in (5, 8) else (5 if max_terms <= 256 else 8)
    host_max = int(sw.get("HOST_MAX", "64"))
    small = c == 5 and 1 <= max_terms <= 256                  # the quad path: window 5, kQMaxTerms
    rows = [
        (not ids and not bidx and count <= host_max and small, "HostHorner"),  # count <= 64 (kBatchHostMax)
        (not small or not on("QUAD"), "LaneWindows"),          # max_terms > 256, or SVGPU_BATCH_QUAD=0
        (count > 4096 or not on("BUCKETS"), "QuadWindows"),
        (count > 512 or not on("FUSE"), "BucketHorner"),       # (or the slot is held: the driver's downgrade)
        (True, "Fused"),                                       # count <= 512 (kFuseMax), slot free
    ]
    route = next(name for hit, name in rows if hit)
    return route, c, "quad" if on("QUAD") else "wave"


def test_route_table(plans):
    seen = set()
    for case, d, count, mt, ids, bidx, sw in _calls(plans):
        assert (d["route"], d["c"], d["horner"]) == _expected_route(count, mt, ids, bidx, sw), case
        assert d["window_bits"] == d["c"] and d["W"] == (26 if d["c"] == 5 else 16), case
        assert d["WG"] == -(-d["W"] // (256 // min(1 << (d["c"] - 1), 64))), case
        if d["route"] == "HostHorner":
            assert not ids and not bidx and mt <= 256 and d["c"] == 5, case
        bw = int(sw.get("BW", "4"))
        assert d["bw"] == min(26, max(1, bw)), case
        assert d["spin_max"] == int(sw.get("WAIT_SPINS", 2**22)), case
        seen.add((d["route"], d["c"], d["horner"]))
    assert {r for r, _, _ in seen} == {"HostHorner", "Fused", "BucketHorner", "QuadWindows", "LaneWindows"}
    assert {("LaneWindows", 5, "quad"), ("LaneWindows", 5, "wave"), ("LaneWindows", 8, "quad"),
            ("LaneWindows", 8, "wave")} <= seen
    # spot checks against the table itself
    assert plans["64 256 0 0"]["route"] == "HostHorner" and plans["65 256 0 0"]["route"] == "Fused"
    assert plans["64 256 1 0"]["route"] == "Fused" and plans["64 256 0 1"]["route"] == "Fused"
    assert plans["512 256 0 0"]["route"] == "Fused" and plans["513 256 0 0"]["route"] == "BucketHorner"
    assert plans["4096 256 0 0"]["route"] == "BucketHorner" and plans["4097 256 0 0"]["route"] == "QuadWindows"
    assert plans["1 257 0 0"]["route"] == "LaneWindows" and plans["1 257 0 0"]["c"] == 8
    assert plans["65536 256 0 0 SVGPU_BATCH_HOST_MAX=100000"]["route"] == "HostHorner"  # the known quirk


def _layouts(d):
    keys = [("buffers", "buffers_total"), ("pinned", "pinned_total")]
    if "single_buffers" in d:
        keys += [("single_buffers", "single_buffers_total"), ("single_pinned", "single_pinned_total")]
    return keys


def test_offsets(plans):
    """256-aligned, ascending without overlap, the last buffer's end rounded up is the total."""
    for case, d in plans.items():
        if "buffers" not in d:
            continue
        for key, total in _layouts(d):
            end = 0
            for name, off, nbytes in d[key]:
                assert off % 256 == 0 and off >= end and nbytes > 0, (case, name)
                end = off + nbytes
            assert d[total] == (end + 255) // 256 * 256, case
            names = [x[0] for x in d[key]]
            assert len(set(names)) == len(names), case


def _al(n):
    return (n + 255) // 256 * 256


def test_capacities_and_parent_total(plans):
    """Each buffer holds what the kernels and copies index, recomputed from the printed plan; the
    reserved total is the driver's earlier byte sum, less the 1-byte carves of its absent buffers."""
    for case, d, count, mt, ids, bidx, sw in _calls(plans):
        cap = {name: nbytes for name, _, nbytes in d["buffers"]}
        pin = {name: nbytes for name, _, nbytes in d["pinned"]}
        route = d["route"]
        if route == "HostHorner":
            back = 256 + count * QW * UPW * XYZZ
            assert d["nT"] == count * QW * UPW and d["back_bytes"] == back, case
            assert d["host_ok"] == (1 if count <= 65535 else 0), case
            assert cap["block"] >= back and pin["back"] >= back and d["pinned_total"] >= back + 16, case
            assert cap["dig"] >= count * QW * 2 * mt and cap["pts"] >= count * 2 * mt * AFF, case
            assert "off" not in cap and pin["off"] >= 16, case
            parent = 256 + _al(count * QW * UPW * XYZZ) + _al(count * QW * 2 * mt) + _al(count * 2 * mt * AFF) + 256
            assert parent - 256 <= d["buffers_total"] <= parent, case
            assert _al(back) + 16 <= d["pinned_total"] <= _al(back) + 256, case
            if count == 1:
                scap = {name: nbytes for name, _, nbytes in d["single_buffers"]}
                assert scap.pop("off") >= 16 and scap == cap, case
                assert d["single_buffers_total"] == parent and d["single_pinned"] == d["pinned"], case
            else:
                assert "single_buffers" not in d, case
            continue
        buckets, quad = route in ("Fused", "BucketHorner"), route != "LaneWindows"
        nT = count * QB * QW if buckets else count * d["W"]
        nflag = count * QW if route == "Fused" else 0
        assert d["nT"] == nT and d["nflag"] == nflag, case
        assert cap["T"] >= nT * XYZZ and cap["flags"] >= 4 * (1 + nflag), case
        if quad:
            assert d["dig_bytes"] == count * QW * 2 * mt and d["pts_bytes"] == count * 2 * mt * AFF, case
            assert cap["dig"] >= d["dig_bytes"] and cap["pts"] >= d["pts_bytes"], case
        else:
            assert d["dig_bytes"] == 0 and d["pts_bytes"] == 0 and "dig" not in cap and "pts" not in cap, case
        assert pin["back"] >= 4 and d["back_bytes"] == 4 and d["pinned_total"] == 256, case
        parent = _al(4 * (1 + nflag)) + _al(nT * XYZZ) + _al(d["dig_bytes"] or 1) + _al(d["pts_bytes"] or 1)
        assert parent - 512 <= d["buffers_total"] <= parent, case
        if route == "Fused":  # the slot is held: the same buffers without the flags
            w = d["without_slot"]
            assert (w["route"], w["nT"], w["nflag"]) == ("BucketHorner", nT, 0), case
            assert w["total"] == d["buffers_total"] - _al(4 * (1 + nflag)) + 256, case
        else:
            assert "without_slot" not in d, case
    fixed = plans["fixed"]
    assert fixed["buffers"] == [["flags", 0, 4]] and fixed["buffers_total"] == 256 and fixed["pinned_total"] == 256


def test_batch_split(plans):
    def check(case, n, small, big, max_small):
        d = plans[case]
        assert (d["small"], d["big"], d["max_small"]) == (small, big, max_small), case
        assert sorted(d["small"] + d["big"]) == list(range(n)), case
    five = "split " + SPLIT_LENGTHS                         # lengths 1, 256, 257, 4096, 4097
    check(five, 5, [0, 1, 2, 3], [4], 4096)                 # SVGPU_BATCH_MAX's default: 4096
    check("split 1 256 257 4096", 4, [0, 1], [2, 3], 256)   # at most 4 MSMs: 256 (kSmallMsmTerms)
    check(five + " SVGPU_BATCH_MAX=256", 5, [0, 1], [2, 3, 4], 256)
    check(five + " SVGPU_BATCH_MAX=100000", 5, [0, 1, 2, 3, 4], [], 4097)
    check(five + " SVGPU_BATCH_SEQ_MAX=5", 5, [0, 1], [2, 3, 4], 256)
    check("split 1 256 257 4096 SVGPU_BATCH_SEQ_MAX=0", 4, [0, 1, 2, 3], [], 4096)
    check("split 1 256 257 4096 SVGPU_BATCH_MAX=100", 4, [0], [1, 2, 3], 1)  # the lower of the two limits


def test_fuse_slot(plans):
    assert plans["slot"] == {"first": 1, "second_same_device": 0, "other_device": 1, "device_67_while_3_held": 0,
                             "after_release": 1, "scoped": 1, "after_scope": 1}


def test_batched_affine_conversion(plans):
    """x_to_affine_batch (one inversion) equals one x_to_affine per point limb for limb in both forms,
    identities are zeros, and the canonical outputs are the oracle's K G."""
    d = plans["affine " + " ".join(map(str, AFFINE_KS))]
    n = len(AFFINE_KS)
    assert d["n"] == n
    for form in ("canonical", "montgomery"):
        got = d[form]
        assert got["guard_intact"] == 1 and len(got["batch"]) == 8 * n
        assert got["batch"] == got["each"], form
    limbs = [int(v, 16) for v in d["canonical"]["batch"]]
    for i, k in enumerate(AFFINE_KS):
        x, y = (sum(limbs[8 * i + 4 * h + j] << (64 * j) for j in range(4)) for h in (0, 1))
        assert (x, y) == ((0, 0) if k == 0 else b.g1_mul(b.G1_GEN, k)), k
    rinv = pow(1 << 256, -1, b.P)
    mont = [int(v, 16) for v in d["montgomery"]["batch"]]
    for i in range(2 * n):
        assert sum(mont[4 * i + j] << (64 * j) for j in range(4)) * rinv % b.P == \
            sum(limbs[4 * i + j] << (64 * j) for j in range(4))


def test_switches_documented():
    """Every SVGPU_ name the planning header reads is in INTEGRATION.md's table."""
    with open(os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "msm_batch_plan.hpp")) as f:
        names = set(re.findall(r"SVGPU_[A-Z0-9_]+", f.read()))
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert len(names) >= 9
    missing = sorted(n for n in names if n not in doc)
    assert not missing, missing
