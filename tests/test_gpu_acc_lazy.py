"""The 29-bit bucket chain end to end over the inputs its rare paths need, at n = 2^14 + 37 (the
smallest size with GLV and the 29-bit chain, and ragged): identity bases (the table's marked
records) and zero scalars, one point 200 times under one scalar (a mid-bucket doubling and a bucket
that crosses chunks), P and -P under one scalar (a cancellation), and the scalars r - 1 and 1.  The
same input runs device-resident (dv.msm), host-fed in several pieces (the add-into accumulate over
k_vtab's table) and through a resident base set (k_resident_prepare's table); every result is the
C++ oracle's Pippenger sum."""
import numpy as np
import pytest

from oracle import bn254 as b

pytestmark = pytest.mark.gpu

N = (1 << 14) + 37


def _words(v):
    return [(v >> (64 * k)) & (2**64 - 1) for k in range(4)]


@pytest.fixture(scope="module")
def case(oracle_cpp):
    B = oracle_cpp.gen_bases(b.SEED_BASES, N, start=53).copy()
    S = oracle_cpp.gen_scalars(b.SEED_SCALARS, N, start=53).copy()
    for i in (0, 5, 3000, 9001, N - 1):  # identity bases under live scalars
        B[i] = 0
    for i in (1, 6, 3001, N - 2):  # zero scalars over live bases
        S[i] = 0
    B[4000] = 0  # and both at once
    S[4000] = 0
    B[100:300] = B[100]  # one point 200 times with one scalar
    S[100:300] = S[100]
    y = sum(int(w) << (64 * k) for k, w in enumerate(B[7000, 4:8]))
    B[7001, 0:4] = B[7000, 0:4]  # P and -P with one scalar
    B[7001, 4:8] = _words(b.P - y)
    S[7001] = S[7000]
    S[8000] = _words(b.R - 1)
    S[8001] = _words(1)
    B.setflags(write=False)
    S.setflags(write=False)
    exp = b.g1_from_bytes(oracle_cpp.msm_pippenger(B, S, 0).tobytes())
    assert exp is not None
    return B, S, exp


def test_device_msm(gpu, case):
    import torch
    import svgpu
    from svgpu import device as dv
    B, S, exp = case
    dB = torch.from_numpy(B.view(np.int64).copy()).to(gpu)
    dS = torch.from_numpy(S.view(np.int64).copy()).to(gpu)
    assert dv.msm(dB, dS, svgpu.SV_CANONICAL) == exp


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_host_fed_msm(gpu, case, monkeypatch, pieces):
    """Pieces after the first add into the buckets the earlier ones left (k_accumulate's ADD form)."""
    import svgpu
    B, S, exp = case
    monkeypatch.setenv("SVGPU_H2D_PIECES", pieces)
    assert svgpu.msm_arrays(B, S) == exp


def test_resident_set_msm(gpu, case):
    import svgpu
    B, S, exp = case
    with svgpu.ResidentBases(B) as rb:
        assert rb.msm_arrays(S) == exp
