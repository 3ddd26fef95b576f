"""csrc/codec.hip at its edges, through the C ABI with `form` passed (svgpu.codec always passes
SV_CANONICAL): both output forms of the two point decoders and both forms of the limb decoder,
every invalid class, what an invalid entry leaves behind (the lowest index across blocks, a zeroed
row, every other row still decoded), the limb geometries that take each shift arm of
k_limbs_to_points, the argument rule, and EIP-197 records whose G1 words are invalid.  The cases
are tests/codec_cases.py (checked against the oracle by tests/test_codec_cases.py); every
comparison is exact integer equality."""
import ctypes

import numpy as np
import pytest
import torch

import codec_cases as cc

pytestmark = pytest.mark.gpu

FORMS = [cc.CANONICAL, cc.MONTGOMERY]
PATTERN = 0x5A5A5A5A5A5A5A5A   # what the output holds before a call: every row must be written


def _rows(out):
    """An (n, 8) u64 array of affine points -> [(x, y)] integers."""
    raw = out.tobytes()
    return [(int.from_bytes(raw[64 * i:64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "little"))
            for i in range(len(raw) // 64)]


def _words(values):
    """Integers below 2^256 -> an (n, 4) u64 array, as they stand."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint64).reshape(-1, 4).copy()


def _check_decoded(layout, got, rc, first, form, msg):
    from svgpu import _lib
    want = [cc.point_row(c.want, form) for c in layout.rows]
    wrong = [(i, c.name) for i, (c, g, w) in enumerate(zip(layout.rows, got, want)) if g != w]
    assert not wrong, f"{layout.name} form {form}: rows differ from the oracle's: {wrong[:8]}"
    assert first == layout.first_invalid, layout.name
    if layout.first_invalid < 0:
        assert rc == _lib.SV_OK, (layout.name, msg)
    else:
        assert rc == _lib.SV_ERR_ARG, layout.name
        assert msg == f"Invalid elliptic curve point encoding in proof (point {layout.first_invalid})", layout.name


def _decode_host(code, form, layout):
    from svgpu import _lib
    n = len(layout.rows)
    buf = np.frombuffer(b"".join(c.data for c in layout.rows), np.uint8)
    out = np.full((n, 8), PATTERN, np.uint64)
    first = ctypes.c_int64(-7)
    rc = _lib.lib.sv_bn254_g1_decode(buf.ctypes.data, n, code, form, out.ctypes.data, ctypes.byref(first))
    _check_decoded(layout, _rows(out), rc, first.value, form, _lib.last_error())


def _decode_device(gpu, code, form, layout):
    from svgpu import _lib
    n = len(layout.rows)
    data = torch.from_numpy(np.frombuffer(b"".join(c.data for c in layout.rows), np.uint8).copy()).to(gpu)
    out = torch.full((n, 8), PATTERN, dtype=torch.int64, device=gpu)
    first = ctypes.c_int64(-7)
    rc = _lib.lib.sv_bn254_g1_decode_device(data.data_ptr(), n, code, form, gpu.index or 0,
                                            torch.cuda.current_stream(gpu).cuda_stream, out.data_ptr(),
                                            ctypes.byref(first))
    _check_decoded(layout, _rows(out.cpu().numpy().view(np.uint64)), rc, first.value, form, _lib.last_error())


@pytest.mark.parametrize("form", FORMS)
def test_compressed_layouts(gpu, form):
    """k_decode_compressed, mont_out = 0 / 1: 133 valid encodings (both parities, x = p - 1 with both
    signs, the identity) and 8 invalid ones, in 1 / 255 / 256 / 257 / 769 entries with no invalid
    entry, one at index 0, one at the last index, and three in three blocks."""
    from svgpu import _lib
    assert len(cc.COMPRESSED_LAYOUTS) == 15
    for layout in cc.COMPRESSED_LAYOUTS:
        _decode_host(_lib.SV_ENC_HALO2_COMPRESSED, form, layout)


@pytest.mark.parametrize("form", FORMS)
def test_evm_layouts(gpu, form):
    """k_decode_evm and emit(), mont_out = 0 / 1: the same points; x or y >= p (p itself, and a
    valid coordinate plus p), y off by one, (0, 1), (x, 0) and 64 bytes of ones."""
    from svgpu import _lib
    assert len(cc.EVM_LAYOUTS) == 15
    for layout in cc.EVM_LAYOUTS:
        _decode_host(_lib.SV_ENC_EVM, form, layout)


def test_device_entry_montgomery(gpu):
    """sv_bn254_g1_decode_device on torch tensors, Montgomery output: 257 entries with an invalid
    one in each block, both encodings."""
    from svgpu import _lib
    _decode_device(gpu, _lib.SV_ENC_HALO2_COMPRESSED, cc.MONTGOMERY, cc.COMPRESSED_DEVICE_LAYOUT)
    _decode_device(gpu, _lib.SV_ENC_EVM, cc.MONTGOMERY, cc.EVM_DEVICE_LAYOUT)


def _from_limbs(rows, n_limbs, bits, form, first_invalid, what):
    """One sv_bn254_kzg_accumulators_from_limbs call over `rows` (LimbCase), everything asserted."""
    from svgpu import _lib
    n = len(rows)
    vals = []
    for c in rows:
        vals += [l if (form == cc.CANONICAL or i in c.raw) else cc.mont_r(l) for i, l in enumerate(c.limbs)]
    arr = _words(vals)
    assert arr.shape == (n * 4 * n_limbs, 4)
    lhs = np.full((n, 8), PATTERN, np.uint64)
    rhs = np.full((n, 8), PATTERN, np.uint64)
    first = ctypes.c_int64(-7)
    rc = _lib.lib.sv_bn254_kzg_accumulators_from_limbs(arr.ctypes.data, n, n_limbs, bits, form, lhs.ctypes.data,
                                                       rhs.ctypes.data, ctypes.byref(first))
    got = list(zip(_rows(lhs), _rows(rhs)))
    # an invalid accumulator: the point that is wrong reads (0, 0); the other one is not specified
    wrong = []
    for i, (c, g) in enumerate(zip(rows, got)):
        if c.want == cc.INVALID:
            side = 1 if c.name.endswith("rhs") else 0
            if g[side] != (0, 0):
                wrong.append((i, c.name))
        elif g != (cc.point_row(c.want[0], form), cc.point_row(c.want[1], form)):
            wrong.append((i, c.name))
    assert not wrong, f"{what} form {form}: accumulators differ from the oracle's: {wrong[:8]}"
    assert first.value == first_invalid, what
    if first_invalid < 0:
        assert rc == _lib.SV_OK, (what, _lib.last_error())
    else:
        assert rc == _lib.SV_ERR_ARG and f"accumulator {first_invalid}:" in _lib.last_error(), what


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geometry", cc.GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_limb_geometries(gpu, geometry, form):
    """k_limbs_to_points, mont_in = mont_out = 0 / 1, per geometry: every valid case in one call
    (random accumulators, the identities, overlapping limbs that carry across words); then every
    invalid case alone between two valid accumulators (a sum of p, a coordinate plus p, plus 2^256
    through the top limb, a raw limb equal to r, off-curve, (x, 0), (0, y); in lhs and in rhs)."""
    n_limbs, bits = geometry
    cases = cc.LIMB_CASES[geometry]
    valid = [c for c in cases if c.kind == "valid"]
    _from_limbs(valid, n_limbs, bits, form, -1, f"{geometry} valid")
    for c in cases:
        if c.kind != "valid":
            _from_limbs([valid[0], c, valid[1]], n_limbs, bits, form, 1, f"{geometry} {c.name}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geometry", [g for g in cc.GEOMETRIES if g[0] != 256], ids=lambda g: f"{g[0]}x{g[1]}")
def test_limb_batches(gpu, geometry, form):
    """1, 128 (256 points: exactly one block) and 129 accumulators, clean and with invalid ones at
    several indices in both blocks: the lowest is reported, the invalid points read (0, 0), every
    other accumulator is decoded."""
    n_limbs, bits = geometry
    for turn, (n, bad) in enumerate(cc.LIMB_BATCHES):
        rows, first = cc.limb_batch(cc.LIMB_CASES[geometry], n, bad, turn=3 * turn)
        _from_limbs(rows, n_limbs, bits, form, first, f"{geometry} n={n} bad={bad}")


@pytest.mark.parametrize("form", FORMS)
def test_limb_argument_rule(gpu, form):
    """n_limbs < 1, bits < 1, bits > 256 and bits * (n_limbs - 1) > 255 are SV_ERR_ARG with nothing
    reported as an invalid accumulator; a good geometry right afterwards is exact."""
    from svgpu import _lib
    valid = [c for c in cc.LIMB_CASES[(3, 88)] if c.kind == "valid"][:5]
    arr = _words([0] * (4 * 4 * 3))   # room for 4 accumulators of any of the geometries below (n = 1 is passed)
    for n_limbs, bits in cc.BAD_GEOMETRIES:
        lhs = np.full((1, 8), PATTERN, np.uint64)
        rhs = np.full((1, 8), PATTERN, np.uint64)
        first = ctypes.c_int64(-7)
        rc = _lib.lib.sv_bn254_kzg_accumulators_from_limbs(arr.ctypes.data, 1, n_limbs, bits, form, lhs.ctypes.data,
                                                           rhs.ctypes.data, ctypes.byref(first))
        assert rc == _lib.SV_ERR_ARG and first.value == -1, (n_limbs, bits)
        _from_limbs(valid, 3, 88, form, -1, f"after ({n_limbs}, {bits})")


def test_decide_eip197_invalid_words(gpu, golden_decider):
    """sv_bn254_kzg_decide_eip197 decodes lhs and rhs with the invalid points standing as identities
    and returns the lowest of the decider's first failure and the two decoders' first invalid
    indices: invalid lhs / rhs words alone, words >= p, an invalid word above and below the case's
    own failing check, both sides in different checks, identity records, one check; a G2 word >= p
    is an argument error."""
    from svgpu import _lib
    cases = cc.eip197_cases(golden_decider)
    assert len(cases) == 20
    for c in cases:
        buf = np.frombuffer(c.records, np.uint8)
        ff = ctypes.c_int32(-2)
        rc = _lib.lib.sv_bn254_kzg_decide_eip197(buf.ctypes.data, len(c.records) // cc.REC, 0, ctypes.byref(ff))
        if c.arg_error:
            assert rc == _lib.SV_ERR_ARG and _lib.last_error() == "EIP-197 record 0: G2 word >= p", c.name
        else:
            assert rc == _lib.SV_OK, (c.name, _lib.last_error())
            assert ff.value == c.first_fail, c.name
