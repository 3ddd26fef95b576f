"""The permutation and lookup terms of the quotient numerator on the device
(sv_bn254_fr_permutation_terms_device, sv_bn254_fr_lookup_terms_device; csrc/quotient_terms.hip)
against Python-int arithmetic, bit for bit.

Expected values.  _perm_constraints and _lookup_constraints below write the constraints of
snark-verifier/src/system/halo2.rs:533-589 and :632-651 out row by row over Python ints, and _fold is
the Horner fold of :657-668.  The formula is defined whether or not the witness is valid, so most
tests feed generated columns.  No expected value comes from the code under test.  The generated
columns are drawn once per size and shared; no test modifies them.

Sizes.  A block spans kQtSpan = 256 rows, one per thread.  (k, e) = (2, 0) is N = 4, the smallest
column in which all three rotations wrap; (8, 2) and (11, 2) are 4 and 32 blocks, where a thread's
X_j is checked against the Python power at every block and thread seam and the halo rows come from
the next (previous) block.  tests/COVERAGE_quotient_terms.md has the ledger."""
import functools

import numpy as np
import pytest

from oracle import bn254 as b
from test_gpu_extended import ZETA, ZETA2, _same
from test_gpu_kzg_open import _dev, _ints, _limbs
from test_gpu_ntt import FORMS, MONTGOMERY, _fft, _root
from test_gpu_resident_bases import _UNREDUCED

pytestmark = pytest.mark.gpu

R = b.R
SHAPES = [(2, 0, -1), (2, 1, -1), (3, 2, -2), (4, 2, -3), (8, 2, -6), (11, 2, -6)]
LAYOUTS = [(1, 1), (3, 2), (5, 2)]
WIDE = [(64, 64), (64, 1)]                   # at N = 8 only
SHIFTS = [None, ZETA, ZETA2]
BETA, GAMMA, Y = (b.gen_scalar(b.SEED_SCALARS, 777000 + i) for i in range(3))
DELTA = 7                                    # any non-residue serves the formula; halo2's is a fixed constant
CANARY = 0x0123456789ABCDEF


# ---- the reference: the reference's constraint lists over Python ints ----
def _rot(c, r, E):
    N = len(c)
    return [c[(j + r * E) % N] for j in range(N)]


def _xs(K, g):
    w, x, out = _root(K), 1 if g is None else g, []
    for _ in range(1 << K):
        out.append(x)
        x = x * w % R
    return out


def _perm_constraints(cols, sigmas, s, chunk, z, l0, l_last, l_active, beta, gamma, g, K, E, last_rotation, rot=_rot):
    """halo2.rs:533-589, self.zk: the constraint columns in the reference's order."""
    N, m, nz = 1 << K, len(cols), len(z)
    X = _xs(K, g)
    out = [[l0[j] * (1 - z[0][j]) % R for j in range(N)],
           [l_last[j] * (z[-1][j] * z[-1][j] - z[-1][j]) % R for j in range(N)]]
    for i in range(1, nz):
        prev = rot(z[i - 1], last_rotation, E)
        out.append([l0[j] * (z[i][j] - prev[j]) % R for j in range(N)])
    for i in range(nz):
        zn = rot(z[i], 1, E)
        c = []
        for j in range(N):
            left, right = zn[j], z[i][j]
            for t in range(i * chunk, min((i + 1) * chunk, m)):
                left = left * (cols[t][j] + beta * sigmas[t][j] + gamma) % R
                right = right * (cols[t][j] + s[t] * X[j] + gamma) % R
            c.append(l_active[j] * (left - right) % R)
        out.append(c)
    return out


def _lookup_constraints(lookups, l0, l_last, l_active, beta, gamma, E, rot=_rot):
    """halo2.rs:632-651, self.zk: five constraint columns per lookup."""
    out = []
    for z, pa, ps, a, s in lookups:
        N = len(z)
        zn, pam = rot(z, 1, E), rot(pa, -1, E)
        out.append([l0[j] * (1 - z[j]) % R for j in range(N)])
        out.append([l_last[j] * (z[j] * z[j] - z[j]) % R for j in range(N)])
        out.append([l_active[j] * (zn[j] * (pa[j] + beta) * (ps[j] + gamma) - z[j] * (a[j] + beta) * (s[j] + gamma)) % R
                    for j in range(N)])
        out.append([l0[j] * (pa[j] - ps[j]) % R for j in range(N)])
        out.append([l_active[j] * (pa[j] - ps[j]) * (pa[j] - pam[j]) % R for j in range(N)])
    return out


def _fold(constraints, y, acc=None):
    """halo2.rs:657-668: acc <- acc y + c per constraint."""
    acc = list(acc) if acc is not None else [0] * len(constraints[0])
    for c in constraints:
        acc = [(a * y + v) % R for a, v in zip(acc, c)]
    return acc


# ---- generated columns ----
@functools.lru_cache(maxsize=None)
def _pool(N):
    """200 generated columns of N rows (N <= 256) or 90 (above), a few edge values planted."""
    from oracle import cpu_ref
    count = 200 if N <= 256 else 90
    flat = _ints(cpu_ref.gen_scalars(b.SEED_SCALARS, count * N, start=990000))
    for i, v in enumerate((0, 1, R - 1, R - 2, 2)):
        flat[(7 * i + 3) % len(flat)] = v
    return tuple(tuple(flat[c * N:(c + 1) * N]) for c in range(count))


class _Cols:
    """Hands out the pool's columns in order; one tensor per (column, form), uploaded once."""

    def __init__(self, N, gpu):
        self.pool, self.next, self.gpu, self.dev = _pool(N), 0, gpu, {}

    def take(self, count=1):
        got = list(range(self.next, self.next + count))
        self.next += count
        assert self.next <= len(self.pool)
        return got

    def ints(self, ids):
        return [self.pool[i] for i in ids]

    def tensors(self, ids, form):
        for i in ids:
            if (i, form) not in self.dev:
                self.dev[i, form] = _dev(_limbs(list(self.pool[i]), form), self.gpu)
        return [self.dev[i, form] for i in ids]


def _s_values(m):
    return [BETA * pow(DELTA, j, R) % R for j in range(m)]


def _perm_case(gpu, k, e, last_rotation, m, chunk, shifts=SHIFTS):
    """Out of place without an accumulator, then in place on one, per shift and form."""
    from svgpu import device as dv
    K, E, nz = k + e, 1 << e, -(-m // chunk)
    cs = _Cols(1 << K, gpu)
    ids = dict(cols=cs.take(m), sigmas=cs.take(m), z=cs.take(nz), l=cs.take(3), acc=cs.take(1))
    s = _s_values(m)
    l0, l_last, l_active = cs.ints(ids["l"])
    for g in shifts:
        cons = _perm_constraints(cs.ints(ids["cols"]), cs.ints(ids["sigmas"]), s, chunk, cs.ints(ids["z"]), l0, l_last,
                                 l_active, BETA, GAMMA, g, K, E, last_rotation)
        want0, want1 = _fold(cons, Y), _fold(cons, Y, cs.ints(ids["acc"])[0])
        for form in FORMS:
            t = {key: cs.tensors(v, form) for key, v in ids.items()}
            args = (t["cols"], t["sigmas"], s, chunk, t["z"], *t["l"], BETA, GAMMA, Y, k, last_rotation)
            out = dv.permutation_terms_device(*args, shift=g, form=form)
            assert tuple(out.shape) == (1 << K, 4)
            assert _same(out, want0, form), (k, e, m, chunk, g, form, "no accumulator")
            acc = t["acc"][0].clone()
            got = dv.permutation_terms_device(*args, shift=g, form=form, acc=acc, out=acc)
            assert got.data_ptr() == acc.data_ptr()
            assert _same(acc, want1, form), (k, e, m, chunk, g, form, "in place")


def _lookup_case(gpu, k, e, n_lookups):
    from svgpu import device as dv
    K, E = k + e, 1 << e
    cs = _Cols(1 << K, gpu)
    ids = dict(l=cs.take(3), acc=cs.take(1), look=[cs.take(5) for _ in range(n_lookups)])
    l0, l_last, l_active = cs.ints(ids["l"])
    cons = _lookup_constraints([cs.ints(lk) for lk in ids["look"]], l0, l_last, l_active, BETA, GAMMA, E)
    want0, want1 = _fold(cons, Y), _fold(cons, Y, cs.ints(ids["acc"])[0])
    for form in FORMS:
        look = [cs.tensors(lk, form) for lk in ids["look"]]
        ls = cs.tensors(ids["l"], form)
        out = dv.lookup_terms_device(look, *ls, BETA, GAMMA, Y, k, form=form)
        assert _same(out, want0, form), (k, e, n_lookups, form, "no accumulator")
        acc = cs.tensors(ids["acc"], form)[0].clone()
        dv.lookup_terms_device(look, *ls, BETA, GAMMA, Y, k, form=form, acc=acc, out=acc)
        assert _same(acc, want1, form), (k, e, n_lookups, form, "in place")
        src = cs.tensors(ids["acc"], form)[0]
        out = dv.lookup_terms_device(look, *ls, BETA, GAMMA, Y, k, form=form, acc=src)
        assert _same(out, want1, form) and _same(src, cs.ints(ids["acc"])[0], form)


def test_the_reference_on_a_hand_case():
    """N = 2, E = 1, one lookup, every column constant: the five constraints by hand."""
    l0, ll, la = [1, 1], [2, 2], [3, 3]
    z, pa, ps, a, s = [2, 2], [5, 5], [4, 4], [1, 1], [1, 1]
    c = _lookup_constraints([(z, pa, ps, a, s)], l0, ll, la, 1, 1, 1)
    assert [v[0] for v in c] == [R - 1, 4, 3 * (2 * 6 * 5 - 2 * 2 * 2), 1, 0]
    assert _fold(c, 10)[0] == ((((R - 1) * 10 + 4) * 10 + 156) * 10 + 1) * 10 % R
    assert _rot([0, 1, 2, 3, 4, 5, 6, 7], -1, 2) == [6, 7, 0, 1, 2, 3, 4, 5]


# ---- bit-exact on arbitrary data ----
@pytest.mark.parametrize("m,chunk", LAYOUTS)
@pytest.mark.parametrize("k,e,last_rotation", SHAPES)
def test_permutation_terms_bit_exact(gpu, oracle_cpp, k, e, last_rotation, m, chunk):
    _perm_case(gpu, k, e, last_rotation, m, chunk)


@pytest.mark.parametrize("m,chunk", WIDE)
def test_permutation_terms_at_the_cap(gpu, oracle_cpp, m, chunk):
    """64 columns in one chunk and in 64: the whole table, at N = 8."""
    _perm_case(gpu, 2, 1, -1, m, chunk)


@pytest.mark.parametrize("n_lookups", [1, 2, 16])
@pytest.mark.parametrize("k,e,last_rotation", SHAPES)
def test_lookup_terms_bit_exact(gpu, oracle_cpp, k, e, last_rotation, n_lookups):
    _lookup_case(gpu, k, e, n_lookups)


# ---- composition ----
def test_permutation_then_lookups_is_one_fold(gpu, oracle_cpp):
    """The permutation's constraints, then two lookups', on the running accumulator (which starts as a
    stand-in for the gates): the Python fold over the whole list."""
    import svgpu
    from svgpu import device as dv
    k, e, last, m, chunk = 4, 2, -3, 3, 2
    K, E = k + e, 1 << e
    cs = _Cols(1 << K, gpu)
    ids = dict(cols=cs.take(m), sigmas=cs.take(m), z=cs.take(2), l=cs.take(3), acc=cs.take(1),
               look=[cs.take(5) for _ in range(2)])
    s = _s_values(m)
    l0, l_last, l_active = cs.ints(ids["l"])
    cons = _perm_constraints(cs.ints(ids["cols"]), cs.ints(ids["sigmas"]), s, chunk, cs.ints(ids["z"]), l0, l_last,
                             l_active, BETA, GAMMA, ZETA, K, E, last)
    cons += _lookup_constraints([cs.ints(lk) for lk in ids["look"]], l0, l_last, l_active, BETA, GAMMA, E)
    want = _fold(cons, Y, cs.ints(ids["acc"])[0])
    for form in FORMS:
        ls = cs.tensors(ids["l"], form)
        acc = cs.tensors(ids["acc"], form)[0].clone()
        # through svgpu.permutation_terms, which builds s_j = beta delta^j itself
        svgpu.permutation_terms(cs.tensors(ids["cols"], form), cs.tensors(ids["sigmas"], form),
                                cs.tensors(ids["z"], form), chunk, *ls, BETA, GAMMA, Y, DELTA, k, last, shift=ZETA,
                                form=form, acc=acc, out=acc)
        dv.lookup_terms_device([cs.tensors(lk, form) for lk in ids["look"]], *ls, BETA, GAMMA, Y, k, form=form,
                               acc=acc, out=acc)
        assert _same(acc, want, form), form


def test_four_lookups_split_two_and_two(gpu, oracle_cpp):
    from svgpu import device as dv
    k, e = 8, 2
    cs = _Cols(1 << (k + e), gpu)
    ids = dict(l=cs.take(3), look=[cs.take(5) for _ in range(4)])
    for form in FORMS:
        ls = cs.tensors(ids["l"], form)
        look = [cs.tensors(lk, form) for lk in ids["look"]]
        one = dv.lookup_terms_device(look, *ls, BETA, GAMMA, Y, k, form=form)
        half = dv.lookup_terms_device(look[:2], *ls, BETA, GAMMA, Y, k, form=form)
        both = dv.lookup_terms_device(look[2:], *ls, BETA, GAMMA, Y, k, form=form, acc=half)
        assert one.cpu().numpy().tobytes() == both.cpu().numpy().tobytes(), form


# ---- a valid witness ----
K4, BLIND, CHUNK = 4, 2, 2
N4, USABLE = 1 << K4, (1 << K4) - BLIND - 1


@functools.lru_cache(maxsize=None)
def _instance_values():
    """A small real instance on n = 16 rows, blinding 2 (13 usable rows, l_last at row 13): three
    columns tied by a permutation of the usable cells with cycles of length 1 to 4, and one lookup of a
    column into a table.  Returns (values, sigmas, lookup input, lookup table) as lists of n ints; the
    rows past the usable ones hold generated values."""
    from oracle import cpu_ref
    rnd = _ints(cpu_ref.gen_scalars(b.SEED_SCALARS, 200, start=880000))
    w = _root(K4)
    cycles = [[(0, 0), (1, 3), (2, 7), (0, 9)], [(1, 1), (2, 2), (0, 5)], [(2, 0), (1, 12)], [(0, 12), (2, 11)],
              [(1, 5), (1, 6)]]                # (column, row), usable rows only; every other cell maps to itself
    assert len({c for cyc in cycles for c in cyc}) == 13 and all(i < USABLE for cyc in cycles for _, i in cyc)
    to = {}
    values = [[rnd[20 * j + i] for i in range(N4)] for j in range(3)]
    for n_cyc, cyc in enumerate(cycles):
        for t, c in enumerate(cyc):
            to[c] = cyc[(t + 1) % len(cyc)]
            values[c[0]][c[1]] = rnd[100 + n_cyc]
    sigmas = [[0] * N4 for _ in range(3)]
    for j in range(3):
        for i in range(N4):
            tj, ti = to.get((j, i), (j, i))
            sigmas[j][i] = pow(DELTA, tj, R) * pow(w, ti, R) % R
    table = [rnd[150 + i] for i in range(N4)]
    inputs = [table[(5 * i * i + 1) % USABLE] for i in range(N4)]
    return values, sigmas, inputs, table


def _instance_witness(gpu, form):
    """z of both chunks and the lookup's a', s', z from the existing calls on the usable rows; the rows
    from the last usable one on are filled here: z[u] = the total, then generated values."""
    import svgpu
    values, sigmas, inputs, table = _instance_values()
    fill = _pool(N4)
    u, w = USABLE, _root(K4)

    def head(col):
        return _dev(_limbs(col[:u], form), gpu)

    zs, z0 = [], 1
    for i in range(0, 3, CHUNK):
        z, total = svgpu.permutation_product([head(v) for v in values[i:i + CHUNK]], [head(v) for v in sigmas[i:i + CHUNK]],
                                             BETA, GAMMA, [pow(DELTA, j, R) for j in range(i, min(i + CHUNK, 3))], w,
                                             z0=z0, form=form)
        zs.append(_from_form(z, form) + [total] + list(fill[40 + i][:N4 - u - 1]))
        z0 = total
    pa, ps, z, total = svgpu.lookup_argument(head(inputs), head(table), BETA, GAMMA, form=form)
    assert z0 == 1 and total == 1
    look = (_from_form(z, form) + [total] + list(fill[50][:N4 - u - 1]), _from_form(pa, form) + list(fill[51][:N4 - u]),
            _from_form(ps, form) + list(fill[52][:N4 - u]), inputs, table)
    return zs, look


def _from_form(t, form):
    vals = _ints(t.cpu().numpy().view(np.uint64))
    return [v * pow(1 << 256, -1, R) % R for v in vals] if form == MONTGOMERY else vals


def _selectors():
    l0 = [1 if i == 0 else 0 for i in range(N4)]
    l_last = [1 if i == USABLE else 0 for i in range(N4)]
    l_active = [1 if i < USABLE else 0 for i in range(N4)]
    return l0, l_last, l_active


@pytest.mark.parametrize("form", FORMS)
def test_valid_witness_on_the_plain_domain(gpu, oracle_cpp, form):
    """e = 0, shift NULL: the columns are the witness itself, every constraint vanishes on every row;
    one corrupted cell makes exactly the rows non-zero that the Python formula makes non-zero."""
    from svgpu import device as dv
    values, sigmas, inputs, table = _instance_values()
    zs, look = _instance_witness(gpu, form)
    sel = _selectors()
    s = _s_values(3)
    last = -(BLIND + 1)

    def up(col):
        return _dev(_limbs(list(col), form), gpu)

    def run(values, look):
        acc = dv.permutation_terms_device([up(v) for v in values], [up(v) for v in sigmas], s, CHUNK, [up(z) for z in zs],
                                          *[up(c) for c in sel], BETA, GAMMA, Y, K4, last, form=form)
        return dv.lookup_terms_device([[up(c) for c in look]], *[up(c) for c in sel], BETA, GAMMA, Y, K4, form=form,
                                      acc=acc, out=acc)

    def python(values, look):
        cons = _perm_constraints(values, sigmas, s, CHUNK, zs, *sel, BETA, GAMMA, None, K4, 1, last)
        return _fold(cons + _lookup_constraints([look], *sel, BETA, GAMMA, 1), Y)

    assert python(values, look) == [0] * N4                       # the instance is valid
    assert _same(run(values, look), [0] * N4, form)
    bad = [list(v) for v in values]
    bad[1][5] = (bad[1][5] + 1) % R                                # a cell of the second column
    want = python(bad, look)
    assert [j for j, v in enumerate(want) if v] == [5]
    assert _same(run(bad, look), want, form)
    bad_look = tuple(list(c) for c in look)
    bad_look[1][3] = (bad_look[1][3] + 1) % R                      # a cell of a'
    want = python(values, bad_look)
    assert set(j for j, v in enumerate(want) if v) >= {3} and set(j for j, v in enumerate(want) if v) <= {2, 3, 4}
    assert _same(run(values, bad_look), want, form)


def _coeffs(vals):
    """The coefficients of the polynomial of degree < n with these values on the domain."""
    n = len(vals)
    ninv = pow(n, -1, R)
    return [v * ninv % R for v in _fft(list(vals), pow(_root(n.bit_length() - 1), -1, R))]


def _eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


@pytest.mark.parametrize("form", FORMS)
def test_end_to_end_through_the_existing_calls(gpu, oracle_cpp, form):
    """The instance through lagrange_selectors_device, coset_lde_device, both terms calls and
    quotient_coeffs_device: h(x) (x^n - 1) equals the Python fold of the constraints evaluated at x
    from the coefficient forms, and h has no coefficient above its degree.
    The numerator's top term is l_active rot(z, 1) prod of `chunk` factors, degree (chunk + 2)(n - 1), so
    h has degree (chunk + 2)(n - 1) - n = 44 here: coefficients 45 .. 63 are zero.  (A bound of
    (chunk + 1)(n - 1) - n = 29 cannot hold: coefficient 44 is the product of the leading coefficients
    of l_active, z_1 and the chunk's columns, measured non-zero below.)"""
    import svgpu
    from svgpu import device as dv
    values, sigmas, inputs, table = _instance_values()
    zs, look = _instance_witness(gpu, form)
    K = svgpu.extended_k(K4, CHUNK + 2)
    e, g, w = K - K4, ZETA, _root(K4)
    l0, l_last, l_active, last = svgpu.lagrange_selectors_device(K4, e, BLIND, shift=g, form=form, device=gpu)
    assert last == -(BLIND + 1)
    s = _s_values(3)

    def ext(col):
        return dv.coset_lde_device(dv.ntt_device(_dev(_limbs(list(col), form), gpu), inverse=True, form=form), e,
                                   shift=g, form=form)

    acc = dv.permutation_terms_device([ext(v) for v in values], [ext(v) for v in sigmas], s, CHUNK, [ext(z) for z in zs],
                                      l0, l_last, l_active, BETA, GAMMA, Y, K4, last, shift=g, form=form)
    acc = dv.lookup_terms_device([[ext(c) for c in look]], l0, l_last, l_active, BETA, GAMMA, Y, K4, form=form,
                                 acc=acc, out=acc)
    h = _from_form(dv.quotient_coeffs_device(acc, K4, 1 << e, g, form=form), form)
    assert len(h) == N4 << e
    top = (CHUNK + 2) * (N4 - 1) - N4
    print("highest non-zero coefficient of h:", max(i for i, v in enumerate(h) if v), "expected", top)
    assert h[top] != 0 and not any(h[top + 1:])

    # the constraints at a random x from the coefficient forms: a column rotated by r is p(w^r x)
    x = b.gen_scalar(b.SEED_SCALARS, 424242)
    sel = [_coeffs(c) for c in _selectors()]

    def at(col):
        return _PointColumn(_coeffs(col), x)

    def rot(c, r, E):
        return [_eval(c.coeffs, x * pow(w, r, R) % R)]

    cons = _perm_constraints([at(v) for v in values], [at(v) for v in sigmas], s, CHUNK, [at(z) for z in zs],
                             *[[_eval(c, x)] for c in sel], BETA, GAMMA, x, 0, 1, last, rot=rot)
    cons += _lookup_constraints([tuple(at(c) for c in look)], *[[_eval(c, x)] for c in sel], BETA, GAMMA, 1, rot=rot)
    assert _eval(h, x) * (pow(x, N4, R) - 1) % R == _fold(cons, Y)[0]


class _PointColumn(list):
    """A one-row column, the polynomial's value at x, that keeps the coefficients: a rotation by r is
    the value at w^r x."""

    def __init__(self, coeffs, x):
        super().__init__([_eval(coeffs, x)])
        self.coeffs = coeffs


# ---- input fences ----
@pytest.mark.parametrize("k,e", [(2, 1), (8, 2)])
def test_unreduced_inputs_inputs_unchanged_and_canaries(gpu, oracle_cpp, k, e):
    """An element not below r in each input class is "not reduced" and the next call is exact; the
    inputs are only read; the rows either side of d_out keep their canary."""
    import torch
    import svgpu
    from svgpu import device as dv
    K, E, N, last, m, chunk = k + e, 1 << e, 1 << (k + e), -1, 3, 2
    cs = _Cols(N, gpu)
    ids = dict(cols=cs.take(m), sigmas=cs.take(m), z=cs.take(2), l=cs.take(3), acc=cs.take(1), look=[cs.take(5)])
    s = _s_values(m)
    l0, l_last, l_active = cs.ints(ids["l"])
    pc = _perm_constraints(cs.ints(ids["cols"]), cs.ints(ids["sigmas"]), s, chunk, cs.ints(ids["z"]), l0, l_last,
                           l_active, BETA, GAMMA, ZETA, K, E, last)
    want_p = _fold(pc, Y, cs.ints(ids["acc"])[0])
    want_l = _fold(_lookup_constraints([cs.ints(ids["look"][0])], l0, l_last, l_active, BETA, GAMMA, E), Y,
                   cs.ints(ids["acc"])[0])
    unreduced = torch.from_numpy(_UNREDUCED.view(np.int64)).to(gpu)
    for form in FORMS:
        t = {key: [x.clone() for x in cs.tensors(v, form)] for key, v in ids.items() if key != "look"}
        look = [x.clone() for x in cs.tensors(ids["look"][0], form)]
        buf = torch.full((N + 16, 4), CANARY, dtype=torch.int64, device=gpu)
        out = buf[8:8 + N]

        def perm():
            return dv.permutation_terms_device(t["cols"], t["sigmas"], s, chunk, t["z"], *t["l"], BETA, GAMMA, Y, k,
                                               last, shift=ZETA, form=form, acc=t["acc"][0], out=out)

        def lookups():
            return dv.lookup_terms_device([look], *t["l"], BETA, GAMMA, Y, k, form=form, acc=t["acc"][0], out=out)

        def fences():
            edge = buf.cpu().numpy()
            return (edge[:8] == CANARY).all() and (edge[8 + N:] == CANARY).all()

        keep = [x.clone() for key in ("cols", "sigmas", "z", "l", "acc") for x in t[key]] + [x.clone() for x in look]
        perm()
        assert _same(out, want_p, form) and fences()
        lookups()
        assert _same(out, want_l, form) and fences()
        now = [x for key in ("cols", "sigmas", "z", "l", "acc") for x in t[key]] + look
        assert all(a.cpu().numpy().tobytes() == c.cpu().numpy().tobytes() for a, c in zip(now, keep))
        # one unreduced element per input class, at a row of the last block; restored afterwards
        row = N - 3
        for call, want, victims in ((perm, want_p, [t["cols"][1], t["sigmas"][2], t["z"][0], t["z"][1], t["l"][0],
                                                    t["l"][1], t["l"][2], t["acc"][0]]),
                                    (lookups, want_l, look + [t["l"][1], t["acc"][0]])):
            for victim in victims:
                saved = victim[row].clone()
                victim[row] = unreduced
                with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                    call()
                assert fences()
                victim[row] = saved
                call()
                assert _same(out, want, form) and fences()


# ---- the selectors ----
@pytest.mark.parametrize("k,e,blinding", [(2, 1, 0), (4, 2, 2), (6, 2, 5)])
def test_lagrange_selectors(gpu, oracle_cpp, k, e, blinding):
    import svgpu
    n, K = 1 << k, k + e
    u = n - blinding - 1
    cols = ([1 if i == 0 else 0 for i in range(n)], [1 if i == u else 0 for i in range(n)],
            [1 if i < u else 0 for i in range(n)])
    for g in (None, ZETA):
        xs = _xs(K, g)
        want = [[_eval(_coeffs(c), x) for x in xs] for c in cols]
        for form in FORMS:
            l0, l_last, l_active, last = svgpu.lagrange_selectors_device(k, e, blinding, shift=g, form=form, device=gpu)
            assert last == -(blinding + 1)
            for got, w in zip((l0, l_last, l_active), want):
                assert tuple(got.shape) == (1 << K, 4) and _same(got, w, form), (k, e, blinding, g, form)
    with pytest.raises(svgpu.LengthError):
        svgpu.lagrange_selectors_device(k, e, n - 1, device=gpu)


def test_wrappers_refuse_bad_shapes(gpu, oracle_cpp):
    """The Python wrappers check shapes as the grand product's _column does, before the library."""
    import torch
    import svgpu
    from svgpu import device as dv
    cs = _Cols(8, gpu)
    c = cs.tensors(cs.take(12), MONTGOMERY)
    ls, s = c[9:12], _s_values(2)
    ok = dict(cols=c[0:2], sigmas=c[2:4], s=s, chunk=2, z=c[4:5])

    def perm(**kw):
        a = {**ok, **kw}
        return dv.permutation_terms_device(a["cols"], a["sigmas"], a["s"], a["chunk"], a["z"], *a.get("ls", ls), BETA,
                                           GAMMA, Y, a.get("log_n", 2), -1, acc=a.get("acc"), out=a.get("out"))

    short, wide = c[5][:4], torch.zeros((8, 5), dtype=torch.int64, device=gpu)
    for kw, err in ((dict(cols=[]), svgpu.EmptyError), (dict(chunk=0), svgpu.ArgumentError),
                    (dict(sigmas=c[2:3]), svgpu.LengthError), (dict(s=s[:1]), svgpu.LengthError),
                    (dict(z=c[4:6]), svgpu.LengthError), (dict(z=[short]), svgpu.LengthError),
                    (dict(cols=[c[0], wide]), svgpu.ArgumentError),
                    (dict(cols=[c[0], c[1].cpu()]), svgpu.ArgumentError),
                    (dict(cols=[c[0], c[1].to(torch.int32)]), svgpu.ArgumentError),
                    (dict(ls=[c[9], c[10], short]), svgpu.LengthError), (dict(acc=short), svgpu.LengthError),
                    (dict(out=short), svgpu.LengthError), (dict(log_n=4), svgpu.LengthError),
                    (dict(cols=[c[0][:6], c[1][:6]]), svgpu.LengthError)):
        with pytest.raises(err):
            perm(**kw)
    look = [c[4:9]]
    for args, kw, err in (([[]], {}, svgpu.EmptyError), ([[c[4:8]]], {}, svgpu.ArgumentError),
                          ([[c[4:8] + [short]]], {}, svgpu.LengthError), ([look], dict(out=short), svgpu.LengthError),
                          ([look], dict(acc=wide), svgpu.ArgumentError)):
        with pytest.raises(err):
            dv.lookup_terms_device(*args, *ls, BETA, GAMMA, Y, 2, **kw)
    assert tuple(perm().shape) == (8, 4) and tuple(dv.lookup_terms_device(look, *ls, BETA, GAMMA, Y, 2).shape) == (8, 4)
