"""The single-MSM host planning (csrc/msm_plan.hpp: plan, switches, per-call shape, workspace layout,
event slots), run on the host through tests/native/msm_layout_check.cpp: every buffer holds what its
users index, the reserved total is the end of the last buffer, and the plan, piece bounds, per-piece
K / T and total agree with what the driver computed before the layout was declared once
(tests/golden/msm_plan.json).  CPU only."""
import json
import os
import re
import subprocess

import pytest

from conftest import sanitizer_prefix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
GOLDEN = os.path.join(ROOT, "tests", "golden", "msm_plan.json")

NS = [257, 4096, 2**14 - 1, 2**14, 40000, 2**16, 70001, 2**18, 2**20, 2**21, 2**21 + 1, 2**24, 2**26]
MODES = ["device", "split", "fed", "fed 3", "fed 16", "fed SVGPU_H2D_SPLIT=5,4,4,3", "resident", "resident_fed"]
SWITCHES = ["SVGPU_GLV=0", "SVGPU_GLV=1", "SVGPU_WINDOW_BITS=4", "SVGPU_WINDOW_BITS=10", "SVGPU_WINDOW_BITS=16",
            "SVGPU_GROUP_TREE=0", "SVGPU_GROUP_TREE=2", "SVGPU_ACC_R29=0", "SVGPU_SORT_HALVES=0"]
XYZZ, AFF, FR = 128, 64, 32


def cases():
    """'N MODE FORM [PIECES] [NAME=VALUE ...]': every size, mode and form without switches; every
    switch setting at every size in the device, host-fed and resident host-fed modes (canonical form,
    the one with the most buffers), and in the window-halves mode."""
    out = []
    for n in NS:
        for mode in MODES:
            name, *rest = mode.split()
            for form in (0, 1):
                out.append(" ".join([str(n), name, str(form), *rest]))
        for sw in SWITCHES:
            for name in ("device", "split", "fed", "resident_fed"):
                out.append(" ".join([str(n), name, "0", sw]))
    return out


@pytest.fixture(scope="module", params=["msm_layout_check", "msm_layout_check_asan"])
def layouts(request):
    """{case: the harness's JSON} from the harness as built, and again under ASan + UBSan."""
    r = subprocess.run(["make", "-s", "-C", NATIVE, "build/" + request.param], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    binary = os.path.join(NATIVE, "build", request.param)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SVGPU_")}
    cs = cases()
    cmd = (sanitizer_prefix() if binary.endswith("_asan") else []) + [binary, "-"]
    r = subprocess.run(cmd, input="\n".join(cs) + "\n", capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cs)
    return {c: json.loads(line) for c, line in zip(cs, lines)}


def test_case_count(layouts):
    assert 300 <= len(layouts) <= 1000


def test_single_case_from_arguments_and_environment(layouts):
    """The harness's one-case form reads the switches from the environment, as the library does."""
    binary = os.path.join(NATIVE, "build", "msm_layout_check")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SVGPU_")}
    env["SVGPU_WINDOW_BITS"] = "10"
    out = subprocess.run([binary, "65536", "device", "0"], capture_output=True, text=True, env=env, check=True).stdout
    assert json.loads(out) == layouts["65536 device 0 SVGPU_WINDOW_BITS=10"]


def test_offsets(layouts):
    """256-aligned, ascending without overlap, the last buffer's end rounded up is the total."""
    for case, d in layouts.items():
        for key, total in (("buffers", "total"), ("in_buffers", "in_total")):
            end = 0
            for name, off, nbytes in d[key]:
                assert off % 256 == 0 and off >= end and nbytes > 0, (case, name)
                end = off + nbytes
            assert d[total] == (end + 255) // 256 * 256, case
            names = [b[0] for b in d[key]]
            assert len(set(names)) == len(names), case


def _case(case):
    f = case.split()
    return int(f[0]), f[1], int(f[2])


def test_capacities(layouts):
    """Each buffer holds what the kernels and copies index, recomputed from the printed plan."""
    for case, d in layouts.items():
        n, mode, form = _case(case)
        fed, res = mode in ("fed", "resident_fed"), mode in ("resident", "resident_fed")
        p, s = d["plan"], d["shape"]
        cap = {name: nbytes for name, _, nbytes in d["buffers"]}
        off = {name: o for name, o, _ in d["buffers"]}
        ep = (2 if p["glv"] else 1) * p["W"]
        pieces = len(d["bounds"]) - 1
        rec = 144 if p["r29"] else XYZZ
        assert s["ep"] == ep and s["rec_bytes"] == rec, case
        assert p["r29"] == 1 or not res, case
        if s["split"]:
            assert mode == "split" and pieces == 1, case
            th = [-(-p["npts"] * w // p["K"]) for w in s["nwh"]]
            assert sum(s["nwh"]) == p["W"] and th == s["Th"], case
            tmax, tst = sum(th), sum(th) + 2
        else:
            tmax, tst = max(d["T"]), sum(t + 1 for t in d["T"])
        for k in range(pieces):  # every piece's entries are covered by its T chunks of K
            e = (d["bounds"][k + 1] - d["bounds"][k]) * ep
            assert (d["T"][k] - 1) * d["K"][k] < e <= d["T"][k] * d["K"][k], case
        assert s["Tmax"] == tmax and s["tst_total"] == tst, case
        assert cap["ent"] >= n * ep * 4, case
        assert cap["bsum"] >= p["nbt"] * rec, case
        assert cap["pfirst"] >= tmax * rec and cap["plast"] >= tmax * rec, case
        assert cap["tstart"] >= tst * 4, case
        assert cap["gst"] >= ((p["nbt"] + 1) * pieces + 1) * 4, case
        assert cap["heavy"] >= p["nbt"] * 4 and cap["multi"] >= p["nbt"] * 4, case
        # the sort scratch: the largest piece
        mp = max(b - a for a, b in zip(d["bounds"], d["bounds"][1:]))
        chunk = 256 if ep > 20 else 1024
        nblk = -(-mp // chunk)
        nbin = 1 << min(p["c"] - 1, 7 if p["glv"] else 6)
        nwb = p["W"] * nbin
        assert s["nwb"] == nwb and s["nblk"] == nblk, case
        assert cap["bcnt"] >= nwb * nblk * 4 and cap["btot"] >= nwb * 4 and cap["bstart"] >= (nwb + 1) * 4, case
        assert cap["tmp"] >= mp * ep * 8, case
        # group sums, then the error words (flag, two fixup counters per piece or half, group counters at 64)
        nfinal = p["W"] * p["NG"]
        nerr = 64 + nfinal
        assert s["nfinal"] == nfinal and s["nerr"] == nerr, case
        assert d["err_offset"] == off["ping"] + nfinal * XYZZ, case
        assert cap["ping"] >= nfinal * XYZZ + nerr * 4, case
        assert 2 * max(pieces, 2) < 64, case  # the last counter's word, below the group counters
        assert cap["racc"] >= p["J"] * p["W"] * XYZZ and cap["rtot"] >= p["J"] * p["W"] * XYZZ, case
        assert 1 <= s["gparts"] and cap["gpart"] >= nfinal * s["gparts"] * XYZZ, case
        if p["tree"]:
            assert p["J"] % 256 == 0, case
            assert cap["tree_out"] >= p["W"] * (p["J"] // 256) * 10 * XYZZ, case
        else:
            assert "tree_out" not in cap, case
        # inputs
        assert ("bases_m" in cap) == (form == 0 and not res), case
        if "bases_m" in cap:
            assert cap["bases_m"] >= n * AFF, case
        if res:
            assert "phix" not in cap, case
        elif p["r29"]:
            assert cap["phix"] >= n * (2 if p["glv"] else 1) * 72, case
            assert s["tab4"] * 16 >= (2 if p["glv"] else 1) * 72, case
        elif p["glv"]:
            assert cap["phix"] >= n * (64 if p["phi64"] else 32), case
        else:
            assert "phix" not in cap, case
        keep = not fed and not s["split"] and "SVGPU_SORT_HALVES=0" not in case
        assert ("stored" in cap) == keep, case
        if keep:
            assert cap["stored"] >= n * 32, case
        icap = {name: nbytes for name, _, nbytes in d["in_buffers"]}
        assert set(icap) == ({"in_scalars"} | (set() if res else {"in_bases"}) if fed else set()), case
        if fed:
            assert icap["in_scalars"] >= n * FR and (res or icap["in_bases"] >= n * AFF), case


def test_piece_bounds(layouts):
    for case, d in layouts.items():
        n, mode, _ = _case(case)
        b = d["bounds"]
        pieces = len(b) - 1
        assert b[0] == 0 and b[-1] == n and all(x < y for x, y in zip(b, b[1:])), case
        assert all(x % 1024 == 0 for x in b[1:-1]), case
        assert 1 <= pieces <= 16 == d["max_pieces"], case
        if pieces > 1:
            assert n >= pieces * 4096 and mode in ("fed", "resident_fed"), case
    assert len(layouts["%d fed 0 16" % 2**20]["bounds"]) == 17
    assert len(layouts["%d fed 1 3" % 2**16]["bounds"]) == 4
    assert layouts["%d fed 0 SVGPU_H2D_SPLIT=5,4,4,3" % 2**16]["bounds"] == [0, 20480, 36864, 53248, 65536]


def test_event_slots(layouts):
    """Pairwise distinct within a mode and below the workspace's 64 events, at 16 pieces too."""
    seen16 = 0
    for case, d in layouts.items():
        ev = d["events"]
        assert len(set(ev.values())) == len(ev), case
        assert all(0 <= v < 64 for v in ev.values()) and d["event_slots"] == 64, case
        if len(d["bounds"]) == 17:
            seen16 += 1
            assert "piece_sorted_15" in ev, case
    assert seen16 >= 4


def test_against_recorded_plan(layouts):
    """The plan, piece bounds and per-piece K / T equal the recorded ones; the total is the recorded
    one plus at most the three 256-B roundings the earlier byte sum left out (pfirst / plast and
    racc / rtot were summed as one buffer each, the error words apart from the group sums)."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert set(golden) == set(layouts)
    for case, d in layouts.items():
        g = golden[case]
        assert d["plan"] == g["plan"], case
        assert d["bounds"] == g["bounds"] and d["K"] == g["K"] and d["T"] == g["T"], case
        assert g["bytes"] <= d["total"] <= g["bytes"] + 768, case


def test_switches_documented():
    """Every SVGPU_ name the planning header reads is in INTEGRATION.md's table."""
    with open(os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "msm_plan.hpp")) as f:
        names = set(re.findall(r"SVGPU_[A-Z0-9_]+", f.read()))
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert len(names) >= 24
    missing = sorted(n for n in names if n not in doc)
    assert not missing, missing
