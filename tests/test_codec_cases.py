"""The tables of tests/codec_cases.py against the oracle (CPU only), so that a mistake in a table
cannot pass for a kernel result in tests/test_gpu_codec_edges.py: every case named valid decodes to
its stated point, every case named invalid raises CodecError, the facts the cases rest on hold, and
no case is skipped -- the number of cases per class is asserted against the literal counts below."""
import pytest

import codec_cases as cc
from oracle import bn254 as b

P, R = b.P, b.R

# cases per (n_limbs, bits): valid, invalid, raw
LIMB_COUNTS = {
    (3, 88): (49, 16, 2),
    (4, 68): (49, 12, 2),
    (4, 64): (49, 16, 2),
    (8, 32): (49, 12, 2),
    (2, 128): (42, 12, 2),
    (9, 29): (49, 12, 2),
    (2, 255): (42, 10, 2),
    (1, 256): (42, 6, 2),
    (256, 1): (13, 12, 2),
}


def _check_decoder(cases, decode, n_valid, n_invalid):
    seen = {"valid": 0, "invalid": 0}
    for c in cases:
        if c.want == cc.INVALID:
            with pytest.raises(b.CodecError, match=b.POINT_MSG):
                decode(c.data)
            seen["invalid"] += 1
        else:
            assert decode(c.data) == c.want, c.name
            assert c.want is None or b.g1_on_curve(c.want), c.name
            seen["valid"] += 1
    assert seen == {"valid": n_valid, "invalid": n_invalid}


def test_named_facts():
    assert b.sqrt_fp(3) is None                       # x = 0 is on no point: sign 1 is invalid
    assert cc.NON_RESIDUE_X == 4 and cc.y_of(cc.NON_RESIDUE_X) is None
    assert all(cc.y_of(x) is not None for x in range(1, cc.NON_RESIDUE_X))
    y0 = b.g1_decompress(cc._le(P - 1, 0))
    y1 = b.g1_decompress(cc._le(P - 1, 1))
    assert y0[0] == y1[0] == P - 1 and y0[1] + y1[1] == P and (y0[1] & 1, y1[1] & 1) == (0, 1)
    assert len(cc.POINTS) == cc.N_GENERATED == 64 and len(set(cc.POINTS)) == 64
    assert {p[1] & 1 for _, p in cc.VALID_POINTS if p} == {0, 1}
    assert all(x < R and y < R for x, y in cc.LIMB_POOL)
    assert cc.mont_p(1) == b.RP and cc.mont_r(1) == b.RR
    assert cc.mont_p(5) == b.to_mont(5) and b.from_mont(cc.mont_r(7), R) == 7


def test_compressed_cases():
    _check_decoder(cc.COMPRESSED_VALID + cc.COMPRESSED_INVALID, b.g1_decompress, 133, 8)
    assert all(len(c.data) == 32 for c in cc.COMPRESSED_VALID + cc.COMPRESSED_INVALID)
    # the encodings are the oracle's own, and canonical: re-encoding gives the same bytes
    assert all(b.g1_compress(c.want) == c.data for c in cc.COMPRESSED_VALID)


def test_evm_cases():
    _check_decoder(cc.EVM_VALID + cc.EVM_INVALID, b.g1_evm_decode, 133, 8)
    assert all(len(c.data) == 64 for c in cc.EVM_VALID + cc.EVM_INVALID)
    x, y = cc.POINTS[0]
    assert b.g1_on_curve((x, y)) and x + P < 1 << 256 and y + P < 1 << 256


@pytest.mark.parametrize("name", ["compressed", "evm"])
def test_layouts(name):
    valid, invalid, lays, dev = {
        "compressed": (cc.COMPRESSED_VALID, cc.COMPRESSED_INVALID, cc.COMPRESSED_LAYOUTS, cc.COMPRESSED_DEVICE_LAYOUT),
        "evm": (cc.EVM_VALID, cc.EVM_INVALID, cc.EVM_LAYOUTS, cc.EVM_DEVICE_LAYOUT)}[name]
    assert [l.name for l in lays] == [
        "1-clean", "1-first", "255-clean", "255-first", "255-last", "256-clean", "256-first", "256-last",
        "257-clean", "257-first", "257-last", "769-clean", "769-first", "769-last", "769-mixed"]
    used = set()
    for l in lays + [dev]:
        n = int(l.name.split("-")[0])
        assert len(l.rows) == n
        bad = [i for i, c in enumerate(l.rows) if c.want == cc.INVALID]
        assert l.first_invalid == (bad[0] if bad else -1)
        used |= {c.name for c in l.rows}
    assert [i for i, c in enumerate(lays[-1].rows) if c.want == cc.INVALID] == [255, 256, 700]
    assert [i for i, c in enumerate(dev.rows) if c.want == cc.INVALID] == [3, 100, 256]
    # every case of both tables is launched, and rows after an invalid one are valid points
    assert used == {c.name for c in valid + invalid} and len(used) == 141
    assert any(c.want not in (None, cc.INVALID) for c in lays[-1].rows[701:])


def test_geometries():
    assert len(cc.GEOMETRIES) == len(set(cc.GEOMETRIES)) == 9
    for n_limbs, bits in cc.GEOMETRIES:
        assert n_limbs >= 1 and 1 <= bits <= 256 and bits * (n_limbs - 1) <= 255
    assert max(bits * (n_limbs - 1) for n_limbs, bits in cc.GEOMETRIES) == 255
    for n_limbs, bits in cc.BAD_GEOMETRIES:
        assert n_limbs < 1 or bits < 1 or bits > 256 or bits * (n_limbs - 1) > 255
    # the shift arms of k_limbs_to_points (sh = bits * i, sw = sh >> 5, sb = sh & 31)
    arms = {g: {((g[1] * i) >> 5, (g[1] * i) & 31) for i in range(g[0])} for g in cc.GEOMETRIES}
    assert {(2, 0), (4, 0), (6, 0)} <= arms[(4, 64)]
    assert arms[(2, 255)] == {(0, 0), (7, 31)}
    assert len({sb for _, sb in arms[(9, 29)]}) == 9
    assert arms[(1, 256)] == {(0, 0)}


@pytest.mark.parametrize("geometry", cc.GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_limb_cases(geometry):
    n_limbs, bits = geometry
    cases = cc.LIMB_CASES[geometry]
    seen = {"valid": 0, "invalid": 0, "raw": 0}
    for c in cases:
        assert len(c.limbs) == 4 * n_limbs, c.name
        assert all(0 <= l < R for i, l in enumerate(c.limbs) if i not in c.raw), c.name
        if c.kind == "valid":
            assert c.raw == () and b.accumulator_from_limbs(c.limbs, n_limbs, bits) == c.want, c.name
        elif c.kind == "invalid":
            assert c.raw == () and c.want == cc.INVALID
            with pytest.raises(b.CodecError):
                b.accumulator_from_limbs(c.limbs, n_limbs, bits)
        else:
            # a word equal to r is no Fr element; where the geometry allows, the integers still sum
            # to an on-curve point, so the kernel's range check of the limb is all that rejects it
            assert c.want == cc.INVALID and len(c.raw) == 1 and c.limbs[c.raw[0]] == R
            if n_limbs >= 2 and bits <= 120:
                lhs, rhs = b.accumulator_from_limbs(c.limbs, n_limbs, bits)
                assert lhs is not None and rhs is not None
        seen[c.kind] += 1
    assert tuple(seen[k] for k in ("valid", "invalid", "raw")) == LIMB_COUNTS[geometry]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert sum(n.startswith("overlap") for n in names) == LIMB_COUNTS[geometry][0] - (6 if n_limbs == 256 else 42)
    for tag in ("lhs", "rhs"):
        for kind in ("off-curve", "(x,0)", "(0,y)", "raw-r"):
            assert f"{kind}-{tag}" in names
        if n_limbs > 1 and geometry != (2, 255):
            assert f"sum=p-{tag}" in names and f"sum=x+p-{tag}" in names
    if geometry in cc.PLUS_2_256:
        for c in cases:
            if c.name.startswith("sum=x+2^256"):
                # the true sum is an on-curve x plus 2^256: the low 256 bits alone are acceptable
                side = 2 * n_limbs * c.name.endswith("rhs")
                vals = [sum(l << (bits * i) for i, l in enumerate(c.limbs[side + j * n_limbs:side + (j + 1) * n_limbs]))
                        for j in (0, 1)]
                assert vals[0] >> 256 == 1 and b.g1_on_curve((vals[0] & ((1 << 256) - 1), vals[1])), c.name
        assert sum(c.name.startswith(("sum=x+2^256", "y=y+2^256")) for c in cases) == 4


def test_limb_batches():
    assert [n for n, _ in cc.LIMB_BATCHES] == [1, 1, 128, 128, 129, 129]
    for g in cc.GEOMETRIES:
        for n, bad in cc.LIMB_BATCHES:
            rows, first = cc.limb_batch(cc.LIMB_CASES[g], n, bad, turn=n)
            assert len(rows) == n and first == (min(bad) if bad else -1)
            assert [i for i, c in enumerate(rows) if c.kind != "valid"] == sorted(bad)


def test_eip197_cases(golden_decider):
    cases = cc.eip197_cases(golden_decider)
    assert len(cases) == 20 and len({c.name for c in cases}) == 20
    by_name = {c["name"]: c for c in golden_decider["cases"]}
    assert by_name["all_valid"]["first_fail"] == -1 and by_name["six_valid_one_bad_plus_identity"]["first_fail"] == 3
    n_arg = 0
    for c in cases:
        n = len(c.records) // cc.REC
        assert len(c.records) == n * cc.REC and 1 <= n <= 8, c.name
        recs = [c.records[i * cc.REC:(i + 1) * cc.REC] for i in range(n)]
        g2s = {r[64:192] for r in recs} | {r[256:384] for r in recs}
        assert len(g2s) == 2, c.name                     # one deciding key per call
        words = [int.from_bytes(recs[0][o:o + 32], "big") for o in list(range(64, 192, 32)) + list(range(256, 384, 32))]
        assert c.arg_error == any(w >= P for w in words), c.name
        n_arg += c.arg_error
        bad = []
        for i, r in enumerate(recs):
            for o in (0, 192):
                try:
                    b.g1_evm_decode(r[o:o + 64])
                except b.CodecError:
                    bad.append(i)
        assert sorted(set(bad)) == c.invalid, c.name
        if c.invalid:
            assert c.first_fail <= c.invalid[0]
    assert n_arg == 3
    want = {c.name: c.first_fail for c in cases}
    assert want == {
        "lhs-off-curve-alone": 1, "rhs-off-curve-alone-last": 3, "lhs.x+p": 2, "rhs.y+p": 0, "lhs.y=0": 3,
        "invalid-above-the-failing-check": 3, "invalid-below-the-failing-check": 1, "invalid-at-the-failing-check": 3,
        "invalid-lhs-2-rhs-1": 1, "invalid-lhs-1-rhs-3": 1, "invalid-lhs-and-rhs-of-one-check": 2,
        "identity-record-inserted": -1, "identity-record-first": -1,
        "g2-word>=p": -1, "g2-y-word>=p": -1, "minus-s_g2-word>=p": -1,
        "one-check-passing": -1, "one-check-failing": 0, "one-check-invalid": 0, "one-check-identity": -1}
    # the identity records are two identity points and the unchanged key
    ident = next(c for c in cases if c.name == "identity-record-inserted")
    lhs, _, rhs, _ = b.eip197_parse(ident.records[2 * cc.REC:3 * cc.REC])
    assert lhs is None and rhs is None and len(ident.records) == 5 * cc.REC
