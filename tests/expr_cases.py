"""What the expression tests share: the oracle -- Python-int arithmetic mod r over the TREE, as the
reference's Expression::evaluate (snark-verifier/src/verifier/plonk/protocol.rs:322-370) walks it,
never over the postfix --, the Sethi-Ullman label written out a second time, a postfix interpreter
over compiled ops, and seeded builders of trees.  Nothing here imports the code under test, and
nothing recurses (a chain may be thousands of nodes long)."""
import random

from oracle import bn254 as b

R = b.R
COLUMN, CONST, NEG, ADD, SUB, RSUB, MUL, FOLD, STORE = range(9)
STACK_MAX, OPS_MAX, COLUMNS_MAX, CONSTS_MAX, STORES_MAX = 8, 4096, 256, 256, 16


def _children(e):
    kind = e[0]
    if kind in ("col", "const"):
        return []
    if kind in ("neg", "scaled"):
        return [e[1]]
    if kind == "powers":
        return list(e[1]) + [e[2]]
    return [e[1], e[2]]


def _walk(expr, leaf, join):
    """Post-order over the tree: leaf(e) for a column or a constant, join(e, values of its children)."""
    out, work = [], [(expr, False)]
    while work:
        e, done = work.pop()
        kids = _children(e)
        if not kids:
            out.append(leaf(e))
        elif not done:
            work.append((e, True))
            work += [(c, False) for c in reversed(kids)]
        else:
            vals = out[len(out) - len(kids):]
            del out[len(out) - len(kids):]
            out.append(join(e, vals))
    assert len(out) == 1
    return out[0]


def _value(expr, leaf, ap):
    """The reference's evaluate(): ap(f, operands..) applies f to scalars, or row by row to columns."""
    def join(e, v):
        kind = e[0]
        if kind == "neg":
            return ap(lambda x: -x, v[0])
        if kind == "add":
            return ap(lambda x, z: x + z, v[0], v[1])
        if kind == "sub":
            return ap(lambda x, z: x - z, v[0], v[1])
        if kind == "mul":
            return ap(lambda x, z: x * z, v[0], v[1])
        if kind == "scaled":
            return ap(lambda x: x * e[2], v[0])
        assert kind == "powers"
        acc = v[0]                                   # protocol.rs:359-368
        for x in v[1:-1]:
            acc = ap(lambda p, s, t: p * s + t, acc, v[-1], x)
        return acc
    return _walk(expr, leaf, join)


def tree_value(expr, column):
    """The tree's value where column(i, rot) is the value of Polynomial(Query(i, rot))."""
    def leaf(e):
        return column(e[1], e[2] if len(e) > 2 else 0) % R if e[0] == "col" else e[1] % R
    return _value(expr, leaf, lambda f, *a: f(*a) % R)


def tree_rows(expr, cols, E):
    """The tree at every row of the columns (lists of N ints): rot(c, r)[j] = c[(j + r E) mod N]."""
    N = len(cols[0])

    def leaf(e):
        if e[0] == "const":
            return [e[1] % R] * N
        c, shift = cols[e[1]], (e[2] if len(e) > 2 else 0) * E % N
        return list(c[shift:]) + list(c[:shift])
    return _value(expr, leaf, lambda f, *a: [f(*t) % R for t in zip(*a)])


def _su(l, r):
    return l + 1 if l == r else max(l, r)


def su_label(expr):
    """The operand stack a tree needs when every binary node evaluates its deeper child first."""
    def join(e, v):
        kind = e[0]
        if kind == "neg":
            return v[0]
        if kind == "scaled":
            return _su(v[0], 1)
        if kind == "powers":
            acc = v[0]
            for x in v[1:-1]:
                acc = _su(_su(acc, v[-1]), x)
            return acc
        return _su(v[0], v[1])
    return _walk(expr, lambda e: 1, join)


def run_postfix(ops, consts, column, y=0, acc=0):
    """The compiled ops at one row -> (acc, {store: value}, the deepest stack seen, FOLDs)."""
    stack, stores, deepest, folds = [], {}, 0, 0
    for op, index, rot in ops:
        if op == COLUMN:
            stack.append(column(index, rot) % R)
        elif op == CONST:
            assert rot == 0
            stack.append(consts[index])
        elif op == NEG:
            stack.append(-stack.pop() % R)
        elif op in (ADD, SUB, RSUB, MUL):
            top, a = stack.pop(), stack.pop()
            stack.append({ADD: a + top, SUB: a - top, RSUB: top - a, MUL: a * top}[op] % R)
        elif op == FOLD:
            acc, folds = (acc * y + stack.pop()) % R, folds + 1
        else:
            assert op == STORE and index not in stores
            stores[index] = stack.pop()
        deepest = max(deepest, len(stack))
    assert not stack
    return acc, stores, deepest, folds


# ---- builders ----
def chain(kind, leaves, left=True):
    """A left- or right-leaning chain of one binary kind over the leaves."""
    leaves = list(leaves)
    if left:
        e = leaves[0]
        for x in leaves[1:]:
            e = (kind, e, x)
    else:
        e = leaves[-1]
        for x in reversed(leaves[:-1]):
            e = (kind, x, e)
    return e


def complete(kind, leaves):
    """The complete binary tree over 2^d leaves."""
    level = list(leaves)
    while len(level) > 1:
        level = [(kind, level[i], level[i + 1]) for i in range(0, len(level), 2)]
    return level[0]


def random_leaf(rng, n_cols, max_rot, pool):
    if rng.random() < 0.7:
        return ("col", rng.randrange(n_cols), rng.randint(-max_rot, max_rot))
    return ("const", rng.choice(pool))


def random_tree(rng, size, n_cols, max_rot, pool):
    """A tree of about `size` leaves using every variant; retried until it fits the operand stack."""
    def build(size):
        if size <= 1:
            return random_leaf(rng, n_cols, max_rot, pool)
        p = rng.random()
        if p < 0.08:
            return ("neg", build(size))
        if p < 0.16:
            return ("scaled", build(size), rng.choice(pool))
        if p < 0.26 and size >= 3:
            k = rng.randint(2, min(4, size))
            cut = sorted(rng.sample(range(1, size), k - 1))
            parts = [hi - lo for lo, hi in zip([0] + cut, cut + [size])]
            return ("powers", [build(s) for s in parts], ("const", rng.choice(pool)))
        left = rng.randint(1, size - 1)
        return (rng.choice(("add", "sub", "mul", "mul")), build(left), build(size - left))
    while True:
        e = build(size)
        if su_label(e) <= STACK_MAX:
            return e


def const_pool(seed, count=12):
    """Constants for the trees: the edge values and generated scalars."""
    return [0, 1, R - 1, 2] + [b.gen_scalar(b.SEED_SCALARS, seed + i) for i in range(count - 4)]


def random_program(seed, n_cols, max_rot, sizes, n_stores):
    """Sinks for one program: a tree per size, the first n_stores of them stored, the rest folded, in
    a seeded shuffle."""
    rng = random.Random(seed)
    pool = const_pool(660000 + 16 * (seed % 1000))
    sinks = []
    for i, size in enumerate(sizes):
        tree = random_tree(rng, size, n_cols, max_rot, pool)
        sinks.append(("store", i, tree) if i < n_stores else ("fold", tree))
    rng.shuffle(sinks)
    return sinks


def program_rows(sinks, cols, E, y, acc=None):
    """What a program's sinks give over the columns: (out or None, {store: column})."""
    N = len(cols[0])
    out = list(acc) if acc is not None else [0] * N
    stores, folded = {}, False
    for sink in sinks:
        if sink[0] == "fold":
            rows = tree_rows(sink[1], cols, E)
            out = [(a * y + v) % R for a, v in zip(out, rows)]
            folded = True
        else:
            stores[sink[1]] = tree_rows(sink[2], cols, E)
    return (out if folded else None), stores
