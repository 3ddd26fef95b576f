"""SHPLONK (bdfg21) opening on a resident base set: sv_bn254_shplonk_quotient_device and
sv_bn254_shplonk_witness_device through svgpu.Bdfg21Opening / svgpu.bdfg21_open.

No expected value comes from the code under test.  The bit-for-bit tests compute c_i, h_i, h, the
linearisation L and its quotient with Python ints and take W and W' from the C++ oracle's Pippenger
over the sliced random base set; the sets are written out by hand.  The round trip commits over an
SRS s^k g, opens, builds the accumulator as Bdfg21::verify does (bdfg21.rs:47-79, with
query_set_coeffs and QuerySetCoeff::new of :169-367 restated below) in oracle group arithmetic and
hands it to the decider.  Everything is arithmetic mod r and group sums: every comparison is exact.

Sizes: the passes and divisions underneath have their own tests (test_gpu_kzg_open_batch,
test_gpu_poly_eval_points, test_gpu_poly_div_roots); here the lengths straddle kDivSpan (S) inside
and across sets, and the sets take 1, 2 and 3 points."""
import pytest

from oracle import bn254 as b
from test_gpu_kzg_open import _Open, _dev, _horner, _ints, _limbs
from test_gpu_kzg_open_batch import S, _combine
from test_gpu_resident_bases import N, _UNREDUCED

pytestmark = pytest.mark.gpu

CANONICAL, MONTGOMERY = 0, 1
FORMS = (CANONICAL, MONTGOMERY)
Z, MU, GAMMA, ZP = (b.gen_scalar(b.SEED_SCALARS, 717100 + i) for i in range(4))
W1, W2 = (b.gen_scalar(b.SEED_SCALARS, 616161 + i) for i in range(2))
inv = lambda x: pow(x, b.R - 2, b.R)


def _prod(xs):
    p = 1
    for x in xs:
        p = p * x % b.R
    return p


def _add(a, c, w):
    """a + w c over Python ints, the longer length."""
    out = list(a) + [0] * max(0, len(c) - len(a))
    for k, x in enumerate(c):
        out[k] = (out[k] + w * x) % b.R
    return out


def _reference(sets, polys, z, mu, gamma, zp):
    """sets: [([shift], [poly index])] -> (h, the quotient of L by (X - z'))."""
    cs, hs, zs = [], [], []
    for shifts, members in sets:
        c = _combine([polys[p] for p in members], mu)
        pts = [s * z % b.R for s in shifts]
        q = c
        for x in pts:
            q = _horner(q, x)[0] if len(c) > len(pts) else []
        cs.append(c), hs.append(q), zs.append(_prod((zp - x) % b.R for x in pts))
    h, L, gp = [], [], 1
    for c, q, zi in zip(cs, hs, zs):
        h = _add(h, q, gp)
        L = _add(L, c, gp * zs[0] * inv(zi) % b.R)
        gp = gp * gamma % b.R
    L = _add(L, h, (-zs[0]) % b.R)
    return h, _horner(L, zp)[0]


@pytest.fixture(scope="module")
def case(oracle_cpp):
    return _Open(oracle_cpp)


@pytest.fixture(scope="module")
def rset(gpu, case):
    import svgpu
    with svgpu.ResidentBases(case.B) as s:
        yield s


# seven polynomials in four sets of 1, 2, 3 and 2 points; the last set's polynomials have 2 and 1
# coefficients, no more than its points: h_4 = 0.  Polynomial 3 names its shifts in the other order
# and polynomial 0 is queried twice.
LENS = [S + 1, S - 1, 2 * S + 1, S, 300, 2, 1]
QUERIES = [(0, 1), (1, 1), (2, 1), (2, W1), (3, W1), (3, 1), (0, 1), (4, 1), (4, W1), (4, W2), (5, W2), (5, W1),
           (6, W1), (6, W2)]
SETS = [([1], [0, 1]), ([1, W1], [2, 3]), ([1, W1, W2], [4]), ([W2, W1], [5, 6])]


def _polys(case, lens):
    return [case.ints(j % 4)[j:j + l] for j, l in enumerate(lens)]


@pytest.mark.parametrize("mu,gamma", [(MU, GAMMA), (0, GAMMA), (MU, 0), (0, 0), (b.R - 1, 1)],
                         ids=["generated", "mu = 0", "gamma = 0", "both 0", "mu = r - 1, gamma = 1"])
def test_w_and_w_prime_against_the_oracle(gpu, case, rset, mu, gamma):
    import svgpu
    polys = _polys(case, LENS)
    off = 37
    h, q = _reference(SETS, polys, Z, mu, gamma, ZP)
    assert len(h) == 2 * S + 1 - 2 and len(q) == 2 * S
    want = ([_horner(polys[p], s * Z % b.R)[1] for p, s in QUERIES], case.witness(off, h), case.witness(off, q))
    for form in FORMS:
        T = [_dev(_limbs(a, form), gpu) for a in polys]
        assert svgpu.bdfg21_open(rset, T, QUERIES, Z, (mu, gamma, ZP), offset=off, form=form) == want, form


@pytest.mark.parametrize("lens,queries,sets", [
    # the h_i of the first set only: a later set adds nothing to W but its c_i is in L
    ([S + 1, 2, 3], [(0, 1), (1, 1), (1, W1), (2, W2), (2, 1), (2, W1)], [([1], [0]), ([1, W1], [1]), ([W2, 1, W1], [2])]),
    # the first set's h is zero, the second's is not: gamma^1 on the only row of h
    ([1, S + 2], [(0, W1), (1, 1), (1, W2)], [([W1], [0]), ([1, W2], [1])]),
    # one set, one point: the single opening's quotient, then its quotient again at z'
    ([S], [(0, W1)], [([W1], [0])]),
], ids=["only the first h", "only the second h", "one set, one point"])
def test_few_sets(gpu, case, rset, lens, queries, sets):
    import svgpu
    polys = _polys(case, lens)
    off = 5
    h, q = _reference(sets, polys, Z, MU, GAMMA, ZP)
    want = ([_horner(polys[p], s * Z % b.R)[1] for p, s in queries], case.witness(off, h), case.witness(off, q))
    for form in FORMS:
        T = [_dev(_limbs(a, form), gpu) for a in polys]
        assert svgpu.bdfg21_open(rset, T, queries, Z, (MU, GAMMA, ZP), offset=off, form=form) == want, form


def test_every_quotient_zero_and_constant_polynomials(gpu, case, rset):
    """No polynomial is longer than its set's points: h = 0, W is the identity and no MSM runs for
    it, while L (two coefficients) still has a witness.  With constants only, N = 1 and both are the
    identity."""
    import svgpu
    lens, queries = [1, 2, 2], [(0, 1), (1, 1), (1, W1), (2, W1), (2, 1)]
    sets = [([1], [0]), ([1, W1], [1, 2])]
    polys = _polys(case, lens)
    h, q = _reference(sets, polys, Z, MU, GAMMA, ZP)
    assert h == [] and len(q) == 1
    for form in FORMS:
        T = [_dev(_limbs(a, form), gpu) for a in polys]
        evals, w, wp = svgpu.bdfg21_open(rset, T, queries, Z, (MU, GAMMA, ZP), offset=N - 1, form=form)
        assert evals == [_horner(polys[p], s * Z % b.R)[1] for p, s in queries]
        assert w is None and wp == case.witness(N - 1, q)
    T = [_dev(_limbs(a[:1], CANONICAL), gpu) for a in polys]
    evals, w, wp = svgpu.bdfg21_open(rset, T, queries, Z, (MU, GAMMA, ZP), offset=N, form=CANONICAL)
    assert evals == [polys[p][0] for p, _ in queries] and w is None and wp is None


def test_rejections_ranges_and_reuse(gpu, case, rset):
    import svgpu
    polys = _polys(case, LENS)
    off = 37
    h, q = _reference(SETS, polys, Z, MU, GAMMA, ZP)
    want = (case.witness(off, h), case.witness(off, q))
    good = [_limbs(a, CANONICAL) for a in polys]
    G = [_dev(a, gpu) for a in good]
    for j, idx in ((0, S), (3, 0), (4, 299), (6, 0)):
        bad = good[j].copy()
        bad[idx] = _UNREDUCED
        with pytest.raises(svgpu.ArgumentError, match="not reduced"):
            svgpu.Bdfg21Opening(rset, G[:j] + [_dev(bad, gpu)] + G[j + 1:], QUERIES, Z, offset=off, form=CANONICAL)
    op = svgpu.Bdfg21Opening(rset, G, QUERIES, Z, offset=off, form=CANONICAL)
    with pytest.raises(svgpu.ArgumentError, match="quotient"):
        op.witness(ZP)
    with pytest.raises(svgpu.ArgumentError, match="mu 0 not reduced"):
        op.quotient(b.R, GAMMA)
    assert op.quotient(MU, GAMMA) == want[0]
    with pytest.raises(svgpu.ArgumentError, match="z_prime equals point"):
        op.witness(W1 * Z % b.R)
    assert op.witness(ZP) == want[1]
    assert (op.quotient(MU, GAMMA), op.witness(ZP)) == want   # the same object again
    # a coefficient that turns bad after the evaluations: the first call finds it on the device
    import torch
    for j, idx in ((2, 2 * S), (5, 1)):
        G[j][idx] = torch.from_numpy(_UNREDUCED.view("int64")).to(gpu)
        with pytest.raises(svgpu.ArgumentError, match="not reduced"):
            op.quotient(MU, GAMMA)
        G[j][idx] = torch.from_numpy(good[j][idx].view("int64")).to(gpu)
        assert (op.quotient(MU, GAMMA), op.witness(ZP)) == want, j
    # z = 0 makes the points of a set equal
    with pytest.raises(svgpu.ArgumentError, match="repeated point"):
        svgpu.Bdfg21Opening(rset, G, QUERIES, 0, offset=off, form=CANONICAL).quotient(MU, GAMMA)
    # the rows of the set: W takes max (N_i - K_i) = 2 S - 1 of them, W' takes N - 1 = 2 S
    tail = svgpu.Bdfg21Opening(rset, G, QUERIES, Z, offset=N - 2 * S + 1, form=CANONICAL)
    assert tail.quotient(MU, GAMMA) == case.witness(N - 2 * S + 1, h)
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        tail.witness(ZP)
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        svgpu.Bdfg21Opening(rset, G, QUERIES, Z, offset=N - 2 * S + 2, form=CANONICAL).quotient(MU, GAMMA)


def _bdfg21_accumulator(g, C, sets, evals_of, z, mu, gamma, zp, W, Wp):
    """Bdfg21::verify (bdfg21.rs:47-79) over canonical ints and oracle points.  sets: [([shift],
    [poly index])]; evals_of[(poly, shift)]; C[poly] the commitments."""
    superset = sorted({s for shifts, _ in sets for s in shifts})
    size = max([len(shifts) for shifts, _ in sets] + [2])
    powers_of_z = [pow(z, k, b.R) for k in range(size)]
    zp_minus = {s: (zp - z * s) % b.R for s in superset}
    coeffs, z_s_1 = [], None
    for shifts, _ in sets:                                      # QuerySetCoeff::new, :276-329
        ell = [_prod((sj - si) % b.R for i, si in enumerate(shifts) if i != j) for j, sj in enumerate(shifts)]
        zk = powers_of_z[len(shifts) - 1]
        bary = [inv((e * zk % b.R * zp - e * s % b.R * zk % b.R * powers_of_z[1]) % b.R) for s, e in zip(shifts, ell)]
        z_s = _prod(zp_minus[s] for s in shifts)
        commitment_coeff = None if z_s_1 is None else z_s_1 * inv(z_s) % b.R
        if z_s_1 is None:
            z_s_1 = z_s
        r_eval_coeff = (1 if commitment_coeff is None else commitment_coeff) * inv(sum(bary) % b.R) % b.R  # :341-358
        coeffs.append((z_s, bary, commitment_coeff, r_eval_coeff))
    f, gp = None, 1
    for (shifts, members), (z_s, bary, cc, rc) in zip(sets, coeffs):   # QuerySet::msm, :229-259
        msm, mp = None, 1
        for p in members:
            commitment = C[p] if cc is None else b.g1_mul(C[p], cc)
            r_eval = sum(w * evals_of[(p, s)] for w, s in zip(bary, shifts)) % b.R * rc % b.R
            term = b.g1_add(commitment, b.g1_neg(b.g1_mul(g, r_eval)))
            msm = b.g1_add(msm, b.g1_mul(term, mp))
            mp = mp * mu % b.R
        f = b.g1_add(f, b.g1_mul(msm, gp))
        gp = gp * gamma % b.R
    f = b.g1_add(f, b.g1_neg(b.g1_mul(W, coeffs[0][0])))           # - w * coeffs[0].z_s
    return b.g1_add(f, b.g1_mul(Wp, zp)), Wp                          # lhs = f + z' w', rhs = w'


def test_bdfg21_commit_open_decide(gpu, oracle_cpp):
    """commit -> bdfg21_open -> decide over an SRS s^k g: seven polynomials of 300 .. 2 coefficients,
    fourteen queries (one repeated) in four sets of 1, 2, 3 and 2 points, the last with a
    two-coefficient polynomial.  The decider accepts Bdfg21::verify's accumulator under (g, g2, s g2);
    with one evaluation replaced by e + 1 (one per set) it does not.  Driven by a transcript, the
    opening returns what the explicit challenges it squeezed return."""
    import svgpu
    from svgpu import encoding as enc
    rows = 300
    s = b.gen_scalar(b.SEED_TRAPDOOR, 1)
    srs, sp = [], 1
    for _ in range(rows):
        srs.append(b.g1_mul(b.G1_GEN, sp))
        sp = sp * s % b.R
    lens = [300, 201, 77, 256, 33, 2, 150]
    A = [oracle_cpp.gen_scalars(b.SEED_SCALARS, l, start=(70 + j) * N) for j, l in enumerate(lens)]
    ints = [_ints(a) for a in A]
    queries = [(0, 1), (1, 1), (2, 1), (2, W1), (3, W1), (3, 1), (0, 1), (4, 1), (4, W1), (4, W2), (5, W2), (5, W1),
               (6, W1), (6, W2)]
    sets = [([1], [0, 1]), ([1, W1], [2, 3]), ([1, W1, W2], [4]), ([W2, W1], [5, 6])]
    with svgpu.ResidentBases(enc.bases_array(srs)) as rs:
        C = [rs.msm_arrays(a) for a in A]
        T = [_dev(a, gpu) for a in A]
        evals, W, Wp = svgpu.bdfg21_open(rs, T, queries, Z, (MU, GAMMA, ZP), form=svgpu.SV_CANONICAL)
        t1 = svgpu.PoseidonTranscript()
        t1.common_scalar(12345)
        got_t = svgpu.bdfg21_open(rs, T, queries, Z, t1, form=svgpu.SV_CANONICAL)
        t2 = svgpu.PoseidonTranscript()
        t2.common_scalar(12345)
        mu_t, gamma_t = t2.squeeze_challenge(), t2.squeeze_challenge()
        t2.common_ec_point(got_t[1])
        zp_t = t2.squeeze_challenge()
        assert got_t == svgpu.bdfg21_open(rs, T, queries, Z, (mu_t, gamma_t, zp_t), form=svgpu.SV_CANONICAL)
        t2.common_ec_point(got_t[2])
        assert t1.squeeze_challenge() == t2.squeeze_challenge()      # W' was absorbed too
    assert evals == [_horner(ints[p], shift * Z % b.R)[1] for p, shift in queries]
    h, q = _reference(sets, ints, Z, MU, GAMMA, ZP)
    assert W == b.g1_mul(b.G1_GEN, _horner(h, s)[1]) and Wp == b.g1_mul(b.G1_GEN, _horner(q, s)[1])
    dk = svgpu.KzgDecidingKey(b.G1_GEN, b.G2_GEN, b.g2_mul(b.G2_GEN, s))

    def acc(evs):
        evals_of = {}
        for (p, shift), e in zip(queries, evs):
            evals_of.setdefault((p, shift), e)
        return svgpu.KzgAccumulator(*_bdfg21_accumulator(b.G1_GEN, C, sets, evals_of, Z, MU, GAMMA, ZP, W, Wp))

    svgpu.KzgAs.decide_all(dk, [acc(evals)])
    assert svgpu.KzgAs.first_failure(dk, [acc(evals)]) == -1
    for k in (1, 4, 9, 12):   # one query of each set
        wrong = list(evals)
        wrong[k] = (wrong[k] + 1) % b.R
        assert svgpu.KzgAs.first_failure(dk, [acc(wrong)]) == 0, k
    with pytest.raises(svgpu.AssertionFailure):
        svgpu.KzgAs.decide_all(dk, [acc(wrong)])
