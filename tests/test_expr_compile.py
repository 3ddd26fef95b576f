"""svgpu.compile_expressions without a GPU: for seeded random trees over every variant, a postfix
interpreter over the compiled ops gives what the tree gives (tests/expr_cases.py evaluates the tree,
as the reference's Expression::evaluate walks it), the reported depth is the interpreter's deepest
stack and the tree's Sethi-Ullman label, constants are de-duplicated, and the caps raise ValueError
naming the sink."""
import random

import pytest

import expr_cases as ec
from svgpu import _lib

R = ec.R
N_COLS, MAX_ROT = 9, 3


def _column(i, rot):
    """A stand-in column value per (column, rotation)."""
    return (0x9E3779B97F4A7C15 * (i + 1) + 0x1234567 * (rot + 7)) ** 5 % R


def _check(tree, sink="fold"):
    import svgpu
    sinks = [("fold", tree)] if sink == "fold" else [("store", 3, tree)]
    ops, consts, depth = svgpu.compile_expressions(sinks)
    y, acc0 = 0xABCDEF123456789, 0x55AA55AA
    acc, stores, deepest, folds = ec.run_postfix(ops, consts, _column, y=y, acc=acc0)
    want = ec.tree_value(tree, _column)
    if sink == "fold":
        assert folds == 1 and not stores and acc == (acc0 * y + want) % R
    else:
        assert folds == 0 and acc == acc0 and stores == {3: want}
    assert depth == deepest == ec.su_label(tree), (depth, deepest, ec.su_label(tree))
    assert len(consts) == len(set(consts)) and all(0 <= c < R for c in consts)
    assert len(ops) <= _lib.SV_EXPR_OPS_MAX and depth <= _lib.SV_EXPR_STACK_MAX
    return ops, consts, depth


def test_the_tests_own_numbers_are_the_librarys():
    assert (ec.COLUMN, ec.CONST, ec.NEG, ec.ADD, ec.SUB, ec.RSUB, ec.MUL, ec.FOLD, ec.STORE) == (
        _lib.SV_EXPR_COLUMN, _lib.SV_EXPR_CONST, _lib.SV_EXPR_NEG, _lib.SV_EXPR_ADD, _lib.SV_EXPR_SUB,
        _lib.SV_EXPR_RSUB, _lib.SV_EXPR_MUL, _lib.SV_EXPR_FOLD, _lib.SV_EXPR_STORE)
    assert (ec.STACK_MAX, ec.OPS_MAX, ec.COLUMNS_MAX, ec.CONSTS_MAX, ec.STORES_MAX) == (
        _lib.SV_EXPR_STACK_MAX, _lib.SV_EXPR_OPS_MAX, _lib.SV_EXPR_COLUMNS_MAX, _lib.SV_EXPR_CONSTS_MAX,
        _lib.SV_EXPR_STORES_MAX)


def test_each_variant_by_hand():
    a, c = ("col", 0, 1), ("col", 1, -2)
    va, vc = _column(0, 1), _column(1, -2)
    for tree, want in ((a, va), (("const", 5), 5), (("const", R + 5), 5), (("neg", a), -va % R),
                       (("add", a, c), (va + vc) % R), (("sub", a, c), (va - vc) % R), (("mul", a, c), va * vc % R),
                       (("scaled", a, 7), va * 7 % R), (("powers", [a], ("const", 9)), va),
                       (("powers", [a, c, ("const", 4)], ("const", 9)), ((va * 9 + vc) * 9 + 4) % R),
                       (("sub", a, ("mul", c, ("add", a, c))), (va - vc * (va + vc)) % R)):
        assert ec.tree_value(tree, _column) == want
        _check(tree)
        _check(tree, sink="store")


def test_a_swapped_difference_is_rsub_and_commutative_operands_swap():
    import svgpu
    deep = ("mul", ("col", 0, 0), ("col", 1, 0))
    ops, _, depth = svgpu.compile_expressions([("fold", ("sub", ("col", 2, 0), deep))])
    assert [o[0] for o in ops] == [ec.COLUMN, ec.COLUMN, ec.MUL, ec.COLUMN, ec.RSUB, ec.FOLD] and depth == 2
    ops, _, depth = svgpu.compile_expressions([("fold", ("sub", deep, ("col", 2, 0)))])
    assert [o[0] for o in ops] == [ec.COLUMN, ec.COLUMN, ec.MUL, ec.COLUMN, ec.SUB, ec.FOLD] and depth == 2
    ops, _, depth = svgpu.compile_expressions([("fold", ("add", ("col", 2, 0), deep))])
    assert [o[1] for o in ops[:4]] == [0, 1, 0, 2] and depth == 2


def test_200_random_trees():
    rng = random.Random(20240)
    pool = ec.const_pool(610000)
    sizes = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89]
    for i in range(200):
        size = sizes[i % len(sizes)] if i < 190 else 400 + 80 * (i - 190)    # the last ten are large
        tree = ec.random_tree(rng, size, N_COLS, MAX_ROT, pool)
        _check(tree, sink="fold" if i % 3 else "store")


def test_chains_and_the_op_cap():
    leaves = [("col", i % N_COLS, i % 5 - 2) for i in range(64)]
    for kind in ("add", "sub", "mul"):
        _, _, d = _check(ec.chain(kind, leaves, left=True))
        assert d == 2
        _, _, d = _check(ec.chain(kind, leaves, left=False))
        assert d == 2                                    # the deeper child first: a right chain is as shallow
    # 2048 leaves and 2047 sums and the FOLD: SV_EXPR_OPS_MAX ops exactly; one leaf more is refused
    import svgpu
    many = [("col", i % N_COLS, 0) for i in range(2049)]
    ops, _, _ = _check(ec.chain("add", many[:2048], left=False))
    assert len(ops) == _lib.SV_EXPR_OPS_MAX
    with pytest.raises(ValueError, match="sink 0"):
        svgpu.compile_expressions([("fold", ec.chain("add", many, left=True))])
    with pytest.raises(ValueError, match="sink 1"):
        svgpu.compile_expressions([("fold", many[0]), ("fold", ec.chain("add", many[:2048]))])


def test_complete_trees_meet_the_stack_cap():
    import svgpu
    leaves = [("col", i % N_COLS, 0) for i in range(256)]
    _, _, depth = _check(ec.complete("mul", leaves[:128]))
    assert depth == 8 == _lib.SV_EXPR_STACK_MAX
    with pytest.raises(ValueError, match="sink 1"):
        svgpu.compile_expressions([("fold", leaves[0]), ("store", 0, ec.complete("add", leaves))])


def test_constants_are_shared_and_the_caps_raise():
    import svgpu
    tree = ("add", ("scaled", ("col", 0, 0), 7), ("mul", ("const", 7), ("powers", [("col", 1, 0), ("const", R + 7)],
                                                                        ("const", 7))))
    ops, consts, _ = svgpu.compile_expressions([("fold", tree), ("store", 0, ("const", 7)), ("fold", ("const", 8))])
    assert consts == [7, 8]
    assert [o[1] for o in ops if o[0] == ec.CONST] == [0, 0, 0, 0, 0, 1]
    ok = ec.chain("add", [("const", i) for i in range(256)])
    assert svgpu.compile_expressions([("fold", ok)])[1] == list(range(256))
    with pytest.raises(ValueError, match="sink 1"):
        svgpu.compile_expressions([("fold", ok), ("fold", ("const", 256))])
    for bad in ([("store", 16, ("const", 1))], [("store", 2, ("const", 1)), ("store", 2, ("const", 1))],
                [("fold", ("col", 256, 0))], [("fold", ("nope", 1))], [("keep", ("const", 1))],
                [("fold", ("powers", [], ("const", 2)))], [("fold", ("add", ("const", 1)))]):
        with pytest.raises(ValueError, match="sink"):
            svgpu.compile_expressions(bad)


def test_compress_expressions_is_the_horner_chain_in_theta():
    import svgpu
    exprs = [("col", 0, 0), ("mul", ("col", 1, 0), ("col", 2, 1)), ("col", 3, 0)]
    theta = 0x123456789
    tree = svgpu.compress_expressions(exprs, theta)
    v = [ec.tree_value(e, _column) for e in exprs]
    assert ec.tree_value(tree, _column) == ((v[0] * theta + v[1]) * theta + v[2]) % R
    _check(tree, sink="store")
