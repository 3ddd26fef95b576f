"""Expression trees -> the postfix programs of sv_bn254_fr_expressions_device (include/svgpu.h).

A tree mirrors the reference's Expression<F> (snark-verifier/src/verifier/plonk/protocol.rs:309-370)
as nested tuples:
    ("col", i, rot)            Polynomial(Query { poly: i, rotation: rot }); a CommonPolynomial is a
                               column the caller supplies
    ("const", value)           Constant and Challenge (a canonical int)
    ("neg", a)                 Negated
    ("add", a, b)              Sum           ("sub", a, b) is Sum(a, Negated(b)) in one op
    ("mul", a, b)              Product
    ("scaled", a, value)       Scaled
    ("powers", [e0, e1, ..], base)   DistributePowers: ((e0 base + e1) base + e2) ..  (:359-368)
A sink is ("fold", expr) -- acc <- acc y + expr -- or ("store", k, expr) -- stores[k] = expr.

Every binary node evaluates its deeper child first (Sethi-Ullman labelling: a leaf needs one stack
slot, a node whose children need l and r needs max(l, r), or l + 1 when l == r), swapping the
operands of ADD and MUL and turning a swapped SUB into RSUB, so the operand stack is as shallow as
the tree allows.  Nothing here recurses: a chain may be as long as the op cap.
"""
from . import _lib
from .encoding import R

_BINARY = {"add": (_lib.SV_EXPR_ADD, _lib.SV_EXPR_ADD), "sub": (_lib.SV_EXPR_SUB, _lib.SV_EXPR_RSUB),
           "mul": (_lib.SV_EXPR_MUL, _lib.SV_EXPR_MUL)}      # kind -> (op, op with the operands swapped)


def _nodes(expr, what):
    """The tree in post-order as (kind, payload, left, right, label) rows; the root is the last."""
    nodes, made, work = [], [], [("visit", expr)]
    while work:
        tag, e = work.pop()
        if tag == "make":
            if e == "neg":
                a = made.pop()
                nodes.append(("neg", None, a, None, nodes[a][4]))
            else:
                b, a = made.pop(), made.pop()
                la, lb = nodes[a][4], nodes[b][4]
                nodes.append((e, None, a, b, la + 1 if la == lb else max(la, lb)))
            made.append(len(nodes) - 1)
            continue
        if not isinstance(e, (tuple, list)) or not e or not isinstance(e[0], str):
            raise ValueError(f"{what}: {e!r} is not an expression")
        kind = e[0]
        if kind == "col" and len(e) in (2, 3):
            nodes.append(("col", (int(e[1]), int(e[2]) if len(e) == 3 else 0), None, None, 1))
            made.append(len(nodes) - 1)
        elif kind == "const" and len(e) == 2:
            nodes.append(("const", int(e[1]) % R, None, None, 1))
            made.append(len(nodes) - 1)
        elif kind == "neg" and len(e) == 2:
            work += [("make", "neg"), ("visit", e[1])]
        elif kind in _BINARY and len(e) == 3:
            work += [("make", kind), ("visit", e[2]), ("visit", e[1])]
        elif kind == "scaled" and len(e) == 3:
            work += [("make", "mul"), ("visit", ("const", e[2])), ("visit", e[1])]
        elif kind == "powers" and len(e) == 3 and len(e[1]) >= 1:
            for x in reversed(list(e[1])[1:]):
                work += [("make", "add"), ("visit", x), ("make", "mul"), ("visit", e[2])]
            work.append(("visit", e[1][0]))
        else:
            raise ValueError(f"{what}: {kind!r} with {len(e) - 1} operands is not an expression")
    return nodes


def compile_expressions(sinks):
    """sinks: a list of ("fold", expr) and ("store", k, expr) -> (ops, consts, depth): ops a list of
    (op, index, rotation) for expressions_device, consts the de-duplicated constants (canonical
    ints) that CONST indexes, depth the deepest operand stack.  ValueError, naming the sink, when a
    tree needs more than SV_EXPR_STACK_MAX slots or the program passes a cap."""
    ops, consts, const_at, depth, stored = [], [], {}, 0, set()
    for n_sink, sink in enumerate(sinks):
        what = f"sink {n_sink}"
        if isinstance(sink, (tuple, list)) and len(sink) == 2 and sink[0] == "fold":
            last, expr = (_lib.SV_EXPR_FOLD, 0, 0), sink[1]
        elif isinstance(sink, (tuple, list)) and len(sink) == 3 and sink[0] == "store":
            k, expr = int(sink[1]), sink[2]
            if not 0 <= k < _lib.SV_EXPR_STORES_MAX or k in stored:
                raise ValueError(f"{what}: store {k} is out of range or written twice")
            stored.add(k)
            last = (_lib.SV_EXPR_STORE, k, 0)
        else:
            raise ValueError(f'{what}: a sink is ("fold", expr) or ("store", k, expr)')
        nodes = _nodes(expr, what)
        need = nodes[-1][4]
        if need > _lib.SV_EXPR_STACK_MAX:
            raise ValueError(f"{what}: the tree needs an operand stack of {need}, above SV_EXPR_STACK_MAX = "
                             f"{_lib.SV_EXPR_STACK_MAX}: store a subtree as a column first")
        depth = max(depth, need)
        work = [len(nodes) - 1]
        while work:
            item = work.pop()
            if isinstance(item, tuple):
                ops.append(item)
                continue
            kind, payload, a, b, _ = nodes[item]
            if kind == "col":
                if not 0 <= payload[0] < _lib.SV_EXPR_COLUMNS_MAX:
                    raise ValueError(f"{what}: column {payload[0]} is beyond SV_EXPR_COLUMNS_MAX")
                ops.append((_lib.SV_EXPR_COLUMN, payload[0], payload[1]))
            elif kind == "const":
                if payload not in const_at:
                    const_at[payload] = len(consts)
                    consts.append(payload)
                ops.append((_lib.SV_EXPR_CONST, const_at[payload], 0))
            elif kind == "neg":
                work += [(_lib.SV_EXPR_NEG, 0, 0), a]
            elif nodes[b][4] > nodes[a][4]:                      # the deeper child first
                work += [(_BINARY[kind][1], 0, 0), a, b]
            else:
                work += [(_BINARY[kind][0], 0, 0), b, a]
        ops.append(last)
        if len(ops) > _lib.SV_EXPR_OPS_MAX or len(consts) > _lib.SV_EXPR_CONSTS_MAX:
            raise ValueError(f"{what}: the program has grown to {len(ops)} ops and {len(consts)} constants, beyond "
                             f"SV_EXPR_OPS_MAX = {_lib.SV_EXPR_OPS_MAX} or SV_EXPR_CONSTS_MAX = "
                             f"{_lib.SV_EXPR_CONSTS_MAX}")
    return ops, consts, depth


def compress_expressions(exprs, theta):
    """The theta-compression of a lookup's input (or table) expressions (system/halo2.rs:614-619):
    DistributePowers(exprs, theta) as a tree for compile_expressions."""
    return ("powers", list(exprs), ("const", theta))
