"""Expression programs on the device (sv_bn254_fr_expressions_device; csrc/expressions.hip) against
Python-int arithmetic over the TREES (tests/expr_cases.py), bit for bit: the compiler
(svgpu.compile_expressions) and the kernel are both under test, and no expected value comes from
either.  The generated columns are drawn once per size and shared; no test modifies them.

Sizes, as (log_n, log_ext).  A block is 256 threads, one row each.  (1, 1) is N = 4, far below a
block; (8, 0) is exactly one block on the original domain; (7, 2) is two blocks, where rotations
cross the block border and the wrap; (3, 8) is E = 256, where a rotation by 7 moves 1792 of 2048
rows.  tests/COVERAGE_expressions.md has the ledger."""
import functools
import random

import numpy as np
import pytest

import expr_cases as ec
from oracle import bn254 as b
from test_gpu_extended import ZETA, _same
from test_gpu_kzg_open import _dev, _ints, _limbs
from test_gpu_ntt import FORMS, _root
from test_gpu_quotient_terms import (BETA, GAMMA, Y, _coeffs, _Cols, _eval, _fold, _from_form, _lookup_constraints,
                                     _perm_constraints, _pool, _s_values, _xs)
from test_gpu_resident_bases import _UNREDUCED

pytestmark = pytest.mark.gpu

R = b.R
SHAPES = [(1, 1), (8, 0), (7, 2), (3, 8)]
COLUMN, CONST, NEG, ADD, SUB, RSUB, MUL, FOLD, STORE = range(9)
N_COLS = 8                                   # columns of the random programs


def _run(sinks, tensors, k, form, y=Y, acc=None, out=None):
    """compile_expressions, then expressions_device with as many fresh stores as the sinks name."""
    import svgpu
    ops, consts, _ = svgpu.compile_expressions(sinks)
    n_stores = 1 + max([s[1] for s in sinks if s[0] == "store"], default=-1)
    return svgpu.expressions_device(ops, tensors, consts, stores=n_stores, y=y, acc=acc, out=out, log_n=k, form=form)


def _check(sinks, cs, ids, k, e, form, acc_id=None, want=None):
    cols = cs.ints(ids)
    acc = cs.ints([acc_id])[0] if acc_id is not None else None
    want_out, want_stores = want if want is not None else ec.program_rows(sinks, cols, 1 << e, Y, acc)
    out, stores = _run(sinks, cs.tensors(ids, form), k, form, acc=cs.tensors([acc_id], form)[0] if acc is not None else None)
    assert (out is None) == (want_out is None)
    if out is not None:
        assert _same(out, want_out, form), (k, e, form, "out")
    for i, col in want_stores.items():
        assert _same(stores[i], col, form), (k, e, form, "store", i)


# ---- each opcode alone ----
@pytest.mark.parametrize("k,e", SHAPES)
def test_each_opcode_alone(gpu, oracle_cpp, k, e):
    """Raw ops, not the compiler's: every non-sink opcode in a program of its own, ending in a FOLD or
    a STORE; COLUMN with rotations 0, +-1 and +-(n - 1)."""
    import svgpu
    n, N, E = 1 << k, 1 << (k + e), 1 << e
    cs = _Cols(N, gpu)
    ids = cs.take(2)
    a, c = cs.ints(ids)
    const = b.gen_scalar(b.SEED_SCALARS, 31337)

    def rot(col, r):
        return [col[(j + r * E) % N] for j in range(N)]

    cases = [([(COLUMN, 1, r), (FOLD, 0, 0)], rot(c, r)) for r in sorted({0, 1, -1, n - 1, -(n - 1)})]
    cases += [([(CONST, 0, 0), (FOLD, 0, 0)], [const] * N),
              ([(COLUMN, 0, 0), (NEG, 0, 0), (FOLD, 0, 0)], [-x % R for x in a]),
              ([(COLUMN, 0, 0), (COLUMN, 1, 0), (ADD, 0, 0), (FOLD, 0, 0)], [(x + z) % R for x, z in zip(a, c)]),
              ([(COLUMN, 0, 0), (COLUMN, 1, 0), (SUB, 0, 0), (FOLD, 0, 0)], [(x - z) % R for x, z in zip(a, c)]),
              ([(COLUMN, 0, 0), (COLUMN, 1, 0), (RSUB, 0, 0), (FOLD, 0, 0)], [(z - x) % R for x, z in zip(a, c)]),
              ([(COLUMN, 0, 0), (COLUMN, 1, 0), (MUL, 0, 0), (FOLD, 0, 0)], [x * z % R for x, z in zip(a, c)])]
    for form in FORMS:
        t = cs.tensors(ids, form)
        for ops, want in cases:
            out, stores = svgpu.expressions_device(ops, t, [const], y=Y, log_n=k, form=form)
            assert stores == [] and tuple(out.shape) == (N, 4)
            assert _same(out, want, form), (k, e, form, ops, "fold")
            out, stores = svgpu.expressions_device(ops[:-1] + [(STORE, 0, 0)], t, [const], stores=1, log_n=k, form=form)
            assert out is None and _same(stores[0], want, form), (k, e, form, ops, "store")
        # a sink with a value left below it (the compiler never does this): the top is refilled from LDS
        ops = [(COLUMN, 0, 0), (COLUMN, 1, 1), (CONST, 0, 0), (STORE, 0, 0), (FOLD, 0, 0), (NEG, 0, 0), (STORE, 1, 0)]
        out, stores = svgpu.expressions_device(ops, t, [const], stores=2, y=Y, log_n=k, form=form)
        assert _same(stores[0], [const] * N, form) and _same(out, rot(c, 1), form)
        assert _same(stores[1], [-x % R for x in a], form), (k, e, form, "refill")


@pytest.mark.parametrize("k,e", [(1, 1), (7, 2)])
def test_sub_and_rsub_at_zero_one_and_minus_one(gpu, oracle_cpp, k, e):
    """Operands chosen so that every row of the difference is 0, 1 and r - 1 (the pool's column holds
    0, 1 and r - 1 among its values, so the subtrahend wraps both ways)."""
    import svgpu
    N = 1 << (k + e)
    a = list(_pool(N)[0])
    a[0], a[1], a[2] = 0, 1, R - 1
    for form in FORMS:
        ta = _dev(_limbs(a, form), gpu)
        for delta, sub, rsub in ((0, 0, 0), (-1, 1, R - 1), (1, R - 1, 1)):
            tb = _dev(_limbs([(x + delta) % R for x in a], form), gpu)
            for op, want in ((SUB, sub), (RSUB, rsub)):
                ops = [(COLUMN, 0, 0), (COLUMN, 1, 0), (op, 0, 0), (STORE, 0, 0)]
                _, stores = svgpu.expressions_device(ops, [ta, tb], [], stores=1, log_n=k, form=form)
                assert _same(stores[0], [want] * N, form), (k, e, form, delta, op)


# ---- random trees ----
@functools.lru_cache(maxsize=None)
def _random_programs(k, e):
    """50 seeded trees per shape in ten programs of five sinks, two stored and three folded, with the
    values the trees give: computed once, shared by both forms."""
    N = 1 << (k + e)
    cols = _pool(N)[:N_COLS]
    acc = _pool(N)[N_COLS]
    max_rot = min((1 << k) - 1, 7)
    sizes = [1, 2, 3, 5, 8] if N > 256 else [1, 3, 6, 12, 24]
    out = []
    for p in range(10):
        sinks = ec.random_program(1000 * (k + 32 * e) + p, N_COLS, max_rot, sizes[p % 5:] + sizes[:p % 5], 2)
        out.append((sinks, ec.program_rows(sinks, cols, 1 << e, Y, acc if p % 2 else None)))
    return out


@pytest.mark.parametrize("k,e", SHAPES)
def test_random_trees_bit_exact(gpu, oracle_cpp, k, e):
    cs = _Cols(1 << (k + e), gpu)
    ids, acc_id = cs.take(N_COLS), cs.take(1)[0]
    for p, (sinks, want) in enumerate(_random_programs(k, e)):
        for form in FORMS:
            _check(sinks, cs, ids, k, e, form, acc_id=acc_id if p % 2 else None, want=want)


# ---- the caps, all at (7, 2) ----
K7, E2 = 7, 2
N7 = 1 << (K7 + E2)


def test_depth_exactly_eight(gpu, oracle_cpp):
    import svgpu
    cs = _Cols(N7, gpu)
    ids = cs.take(N_COLS)
    tree = ec.complete("mul", [("col", i % N_COLS, i % 7 - 3) for i in range(128)])
    assert svgpu.compile_expressions([("fold", tree)])[2] == 8 == svgpu._lib.SV_EXPR_STACK_MAX
    for form in FORMS:
        _check([("fold", tree), ("store", 0, ("neg", tree))], cs, ids, K7, E2, form)


def test_program_of_exactly_the_op_cap(gpu, oracle_cpp):
    import svgpu
    cs = _Cols(N7, gpu)
    ids = cs.take(N_COLS)
    tree = ec.chain("add", [("col", i % N_COLS, i % 5 - 2) for i in range(2048)], left=False)
    assert len(svgpu.compile_expressions([("fold", tree)])[0]) == svgpu._lib.SV_EXPR_OPS_MAX
    for form in FORMS:
        _check([("fold", tree)], cs, ids, K7, E2, form)


def test_256_columns_256_constants_16_stores(gpu, oracle_cpp):
    import svgpu
    flat = _ints(oracle_cpp.gen_scalars(b.SEED_SCALARS, 256 * N7, start=4400000))
    cols = [flat[c * N7:(c + 1) * N7] for c in range(256)]
    consts = [b.gen_scalar(b.SEED_SCALARS, 4500000 + i) for i in range(256)]
    every_column = ec.chain("add", [("col", i, (i % 3) - 1) for i in range(256)])
    every_const = ec.chain("add", [("scaled", ("col", i % 256, 0), consts[i]) for i in range(256)], left=False)
    stores = [("store", i, ("mul", ("col", i, 1), ("col", 255 - i, -1))) for i in range(16)]
    programs = [[("fold", every_column)], [("fold", every_const)], stores + [("fold", ("col", 0, 0))]]
    assert len(svgpu.compile_expressions(programs[1])[1]) == 256
    wants = [ec.program_rows(p, cols, 1 << E2, Y) for p in programs]
    for form in FORMS:
        whole = _dev(_limbs(flat, form), gpu)
        tensors = [whole[c * N7:(c + 1) * N7] for c in range(256)]
        for sinks, (want_out, want_stores) in zip(programs, wants):
            out, got = _run(sinks, tensors, K7, form)
            assert _same(out, want_out, form)
            assert len(got) == len(want_stores) and all(_same(got[i], want_stores[i], form) for i in want_stores)


# ---- fold continuation ----
def test_five_folds_equal_two_plus_three_and_the_corners(gpu, oracle_cpp):
    import svgpu
    cs = _Cols(N7, gpu)
    ids, acc_id = cs.take(N_COLS), cs.take(1)[0]
    rng = random.Random(55)
    pool = ec.const_pool(670000)
    trees = [ec.random_tree(rng, 6, N_COLS, 3, pool) for _ in range(5)]
    sinks = [("fold", t) for t in trees]
    cols, acc = cs.ints(ids), cs.ints([acc_id])[0]
    want, _ = ec.program_rows(sinks, cols, 1 << E2, Y, acc)
    want0, _ = ec.program_rows(sinks, cols, 1 << E2, Y)
    want_store = ec.tree_rows(trees[0], cols, 1 << E2)
    for form in FORMS:
        t, tacc = cs.tensors(ids, form), cs.tensors([acc_id], form)[0]
        one, _ = _run(sinks, t, K7, form, acc=tacc)
        assert _same(one, want, form) and _same(tacc, acc, form)           # the accumulator is only read
        half, _ = _run(sinks[:2], t, K7, form, acc=tacc)
        both, _ = _run(sinks[2:], t, K7, form, acc=half)
        assert both.cpu().numpy().tobytes() == one.cpu().numpy().tobytes()
        place = tacc.clone()                                               # d_out == d_acc_in
        got, _ = _run(sinks, t, K7, form, acc=place, out=place)
        assert got.data_ptr() == place.data_ptr() and _same(place, want, form)
        none, _ = _run(sinks, t, K7, form)                                  # d_acc_in = NULL
        assert _same(none, want0, form)
        ops, consts, _ = svgpu.compile_expressions([("store", 0, trees[0])])
        out, stores = svgpu.expressions_device(ops, t, consts, stores=1, log_n=K7, form=form)   # y, acc, out all NULL
        assert out is None and _same(stores[0], want_store, form)


# ---- agreement with the fixed-function kernels ----
def _lookup_sinks(beta, gamma):
    """One lookup's five constraints (system/halo2.rs:632-651) over columns 0 l0, 1 l_last, 2 l_active,
    3 z, 4 a', 5 s', 6 A, 7 S."""
    l0, ll, la, z, pa, ps, a, s = (("col", i, 0) for i in range(8))
    bt, gm, one = ("const", beta), ("const", gamma), ("const", 1)
    return [("fold", ("mul", l0, ("sub", one, z))),
            ("fold", ("mul", ll, ("sub", ("mul", z, z), z))),
            ("fold", ("mul", la, ("sub", ("mul", ("mul", ("col", 3, 1), ("add", pa, bt)), ("add", ps, gm)),
                                  ("mul", ("mul", z, ("add", a, bt)), ("add", s, gm))))),
            ("fold", ("mul", l0, ("sub", pa, ps))),
            ("fold", ("mul", la, ("mul", ("sub", pa, ps), ("sub", pa, ("col", 4, -1)))))]


def _perm_sinks(m, chunk, s, beta, gamma, last):
    """The permutation constraints (:533-589) over columns 0 l0, 1 l_last, 2 l_active, 3 X, then the m
    values, the m sigmas and the z columns."""
    nz = -(-m // chunk)
    l0, ll, la, X = (("col", i, 0) for i in range(4))
    v = [("col", 4 + j, 0) for j in range(m)]
    sg = [("col", 4 + m + j, 0) for j in range(m)]
    zc = [4 + 2 * m + i for i in range(nz)]
    bt, gm, one = ("const", beta), ("const", gamma), ("const", 1)
    z_last = ("col", zc[-1], 0)
    sinks = [("fold", ("mul", l0, ("sub", one, ("col", zc[0], 0)))),
             ("fold", ("mul", ll, ("sub", ("mul", z_last, z_last), z_last)))]
    for i in range(1, nz):
        sinks.append(("fold", ("mul", l0, ("sub", ("col", zc[i], 0), ("col", zc[i - 1], last)))))
    for i in range(nz):
        left, right = ("col", zc[i], 1), ("col", zc[i], 0)
        for j in range(i * chunk, min((i + 1) * chunk, m)):
            left = ("mul", left, ("add", ("add", v[j], ("mul", bt, sg[j])), gm))
            right = ("mul", right, ("add", ("add", v[j], ("scaled", X, s[j])), gm))
        sinks.append(("fold", ("mul", la, ("sub", left, right))))
    return sinks


@pytest.mark.parametrize("k,e", [(7, 2), (3, 8)])
def test_lookup_constraints_as_a_program_equal_lookup_terms(gpu, oracle_cpp, k, e):
    from svgpu import device as dv
    cs = _Cols(1 << (k + e), gpu)
    ids, acc_id = cs.take(8), cs.take(1)[0]
    c = cs.ints(ids)
    want = _fold(_lookup_constraints([tuple(c[3:8])], c[0], c[1], c[2], BETA, GAMMA, 1 << e), Y, cs.ints([acc_id])[0])
    for form in FORMS:
        t, acc = cs.tensors(ids, form), cs.tensors([acc_id], form)[0]
        fixed = dv.lookup_terms_device([t[3:8]], t[0], t[1], t[2], BETA, GAMMA, Y, k, form=form, acc=acc)
        got, _ = _run(_lookup_sinks(BETA, GAMMA), t, k, form, acc=acc)
        assert got.cpu().numpy().tobytes() == fixed.cpu().numpy().tobytes(), (k, e, form)
        assert _same(got, want, form)


@pytest.mark.parametrize("k,e", [(7, 2), (3, 8)])
def test_permutation_constraints_as_a_program_equal_permutation_terms(gpu, oracle_cpp, k, e):
    """m = 3, chunk = 2, X supplied as a column: the rotation convention and the fold order against
    the kernel that is already trusted."""
    from svgpu import device as dv
    m, chunk, last, K = 3, 2, -2, k + e
    cs = _Cols(1 << K, gpu)
    sel, vals, sigs, zs, acc_id = cs.take(3), cs.take(m), cs.take(m), cs.take(2), cs.take(1)[0]
    s, X = _s_values(m), _xs(K, ZETA)
    l0, l_last, l_active = cs.ints(sel)
    want = _fold(_perm_constraints(cs.ints(vals), cs.ints(sigs), s, chunk, cs.ints(zs), l0, l_last, l_active, BETA, GAMMA,
                                   ZETA, K, 1 << e, last), Y, cs.ints([acc_id])[0])
    sinks = _perm_sinks(m, chunk, s, BETA, GAMMA, last)
    for form in FORMS:
        acc = cs.tensors([acc_id], form)[0]
        fixed = dv.permutation_terms_device(cs.tensors(vals, form), cs.tensors(sigs, form), s, chunk, cs.tensors(zs, form),
                                            *cs.tensors(sel, form), BETA, GAMMA, Y, k, last, shift=ZETA, form=form, acc=acc)
        tensors = cs.tensors(sel, form) + [_dev(_limbs(X, form), gpu)] + cs.tensors(vals + sigs + zs, form)
        got, _ = _run(sinks, tensors, k, form, acc=acc)
        assert got.cpu().numpy().tobytes() == fixed.cpu().numpy().tobytes(), (k, e, form)
        assert _same(got, want, form)


# ---- not reduced ----
@pytest.mark.parametrize("k,e", [(1, 1), (7, 2)])
def test_unreduced_element_in_a_read_column_and_in_an_unnamed_one(gpu, oracle_cpp, k, e):
    import torch
    import svgpu
    N = 1 << (k + e)
    cs = _Cols(N, gpu)
    ids, acc_id = cs.take(4), cs.take(1)[0]
    # columns 0, 1 and 3 are named; column 2 is passed and never named
    sinks = [("fold", ("mul", ("col", 0, 1), ("col", 1, -1))), ("store", 0, ("add", ("col", 3, 0), ("col", 0, 0)))]
    cols, acc = cs.ints(ids), cs.ints([acc_id])[0]
    want = ec.program_rows(sinks, cols, 1 << e, Y, acc)
    unreduced = torch.from_numpy(_UNREDUCED.view(np.int64)).to(gpu)
    for form in FORMS:
        t = [x.clone() for x in cs.tensors(ids, form)]
        tacc = cs.tensors([acc_id], form)[0].clone()

        def call():
            out, stores = _run(sinks, t, k, form, acc=tacc)
            return _same(out, want[0], form) and _same(stores[0], want[1][0], form)

        assert call()
        row = N - 3
        for victim in (t[0], t[1], t[3], tacc):
            saved = victim[row].clone()
            victim[row] = unreduced
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                call()
            victim[row] = saved
            assert call()                                                   # the next call is exact
        t[2][row] = unreduced                                               # never named: never dereferenced
        assert call()


# ---- end to end ----
K4, E4 = 4, 2
N4 = 1 << K4


@functools.lru_cache(maxsize=None)
def _gate_instance():
    """Columns on the 16-row domain that satisfy, on every row,
         q_l a + q_r b + q_m a b - c + q_c = 0   and   q_s (d[+1] - d - e[-1]) = 0:
    ten columns 0 q_l, 1 q_r, 2 q_m, 3 q_c, 4 q_s, 5 a, 6 b, 7 c, 8 d, 9 e; the selectors random and
    non-zero, c and e defined from the others (e with wrap-around: e[j] = d[j + 2] - d[j + 1])."""
    rnd = [b.gen_scalar(b.SEED_SCALARS, 7700000 + i) for i in range(8 * N4)]
    ql, qr, qm, qc, qs, a, bb, d = (rnd[i * N4:(i + 1) * N4] for i in range(8))
    assert all(ql + qr + qm + qc + qs)
    c = [(ql[j] * a[j] + qr[j] * bb[j] + qm[j] * a[j] * bb[j] + qc[j]) % R for j in range(N4)]
    e = [(d[(j + 2) % N4] - d[(j + 1) % N4]) % R for j in range(N4)]
    return [ql, qr, qm, qc, qs, a, bb, c, d, e]


def _gate_sinks():
    ql, qr, qm, qc, qs, a, bb, c, d, e = (("col", i, 0) for i in range(10))
    one = ("sub", ("add", ("add", ("add", ("mul", ql, a), ("mul", qr, bb)), ("mul", qm, ("mul", a, bb))), qc), c)
    two = ("mul", qs, ("sub", ("sub", ("col", 8, 1), d), ("col", 9, -1)))
    return [("fold", one), ("fold", two)]


@pytest.mark.parametrize("form", FORMS)
def test_end_to_end_gates(gpu, oracle_cpp, form):
    """ntt_device (inverse) -> coset_lde_device -> expressions_device (two FOLDs under y) ->
    quotient_coeffs_device with two pieces: the numerator has degree 3 (n - 1), h degree 2 n - 3 < 2 n,
    nothing is dropped, and at three points x the folded constraints, evaluated in Python ints from
    the columns' coefficient forms at x, w x and x / w, equal h(x) (x^n - 1).  One broken witness cell
    and the identity fails."""
    from svgpu import device as dv
    w = _root(K4)
    sinks = _gate_sinks()
    points = [b.gen_scalar(b.SEED_SCALARS, 7800000 + i) for i in range(3)]

    def identity(columns):
        ext = [dv.coset_lde_device(dv.ntt_device(_dev(_limbs(list(col), form), gpu), inverse=True, form=form), E4,
                                   shift=ZETA, form=form) for col in columns]
        numer, _ = _run(sinks, ext, K4, form)
        h = _from_form(dv.quotient_coeffs_device(numer, K4, 2, ZETA, form=form), form)
        assert len(h) == 2 * N4
        coeffs = [_coeffs(col) for col in columns]
        holds = []
        for x in points:
            folded = 0
            for sink in sinks:
                v = ec.tree_value(sink[1], lambda i, rot: _eval(coeffs[i], x * pow(w, rot, R) % R))
                folded = (folded * Y + v) % R
            holds.append(_eval(h, x) * (pow(x, N4, R) - 1) % R == folded)
        return holds

    columns = _gate_instance()
    zero, _ = ec.program_rows(sinks, columns, 1, Y)
    assert zero == [0] * N4                                  # the instance satisfies both constraints
    assert identity(columns) == [True] * 3
    broken = [list(col) for col in columns]
    broken[5][3] = (broken[5][3] + 1) % R                    # a cell of a
    assert identity(broken) == [False] * 3


@pytest.mark.parametrize("form", FORMS)
def test_end_to_end_theta_compression(gpu, oracle_cpp, form):
    """(8, 0): three input expressions (one of them a product of two columns) and three table columns
    compressed under theta into A and S by one call with two STOREs, then svgpu.lookup_argument."""
    import svgpu
    k, n = 8, 256
    theta = b.gen_scalar(b.SEED_SCALARS, 7900000)
    i0, i1, i2, i3 = (list(c) for c in _pool(n)[30:34])
    for col in (i0, i1, i2, i3):                             # a few repeated rows: A has repeats
        col[10:20] = col[40:50]
    perm = [(77 * j + 5) % n for j in range(n)]              # the table is the inputs' rows, shuffled
    t0, t1, t2 = [i0[p] for p in perm], [i1[p] * i2[p] % R for p in perm], [i3[p] for p in perm]
    cols = [i0, i1, i2, i3, t0, t1, t2]
    inputs = [("col", 0, 0), ("mul", ("col", 1, 0), ("col", 2, 0)), ("col", 3, 0)]
    tables = [("col", 4, 0), ("col", 5, 0), ("col", 6, 0)]
    sinks = [("store", 0, svgpu.compress_expressions(inputs, theta)),
             ("store", 1, svgpu.compress_expressions(tables, theta))]
    A = [((x * theta + y * z) * theta + u) % R for x, y, z, u in zip(i0, i1, i2, i3)]
    S = [((x * theta + y) * theta + u) % R for x, y, u in zip(t0, t1, t2)]
    assert set(A) <= set(S)
    out, (dA, dS) = _run(sinks, [_dev(_limbs(c, form), gpu) for c in cols], k, form)
    assert out is None and _same(dA, A, form) and _same(dS, S, form)
    got = svgpu.lookup_argument(dA, dS, BETA, GAMMA, form=form)
    want = svgpu.lookup_argument(_dev(_limbs(A, form), gpu), _dev(_limbs(S, form), gpu), BETA, GAMMA, form=form)
    assert got[3] == want[3] == 1
    for x, z in zip(got[:3], want[:3]):
        assert x.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()


def test_wrapper_refuses_bad_shapes(gpu, oracle_cpp):
    import torch
    import svgpu
    cs = _Cols(8, gpu)
    c = cs.tensors(cs.take(3), 1)
    ops = [(COLUMN, 0, 0), (FOLD, 0, 0)]
    short = c[1][:4]
    for kw, err in ((dict(cols=[c[0], short]), svgpu.LengthError), (dict(cols=[c[0].cpu()]), svgpu.DeviceError),
                    (dict(acc=short), svgpu.LengthError), (dict(out=short), svgpu.LengthError),
                    (dict(stores=[short]), svgpu.LengthError), (dict(y=None), svgpu.ArgumentError),
                    (dict(log_n=None), svgpu.ArgumentError), (dict(log_n=4), svgpu.LengthError),
                    (dict(ops=[(COLUMN, 0)]), svgpu.ArgumentError), (dict(ops=[(COLUMN, 1 << 16, 0)]), svgpu.ArgumentError),
                    (dict(ops=[(COLUMN, 1, 0), (FOLD, 0, 0)]), svgpu.ArgumentError)):
        a = dict(ops=ops, cols=[c[0]], stores=(), y=Y, acc=None, out=None, log_n=2)
        a.update(kw)
        with pytest.raises(err):
            svgpu.expressions_device(a["ops"], a["cols"], [], stores=a["stores"], y=a["y"], acc=a["acc"], out=a["out"],
                                     log_n=a["log_n"])
    out, stores = svgpu.expressions_device(ops, [c[0]], [], y=Y, log_n=2)
    assert tuple(out.shape) == (8, 4) and stores == [] and out.dtype == torch.int64
