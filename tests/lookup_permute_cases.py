"""Helpers of the lookup-permutation tests (not collected by pytest): two restatements of halo2's
permute_expression_pair (halo2_proofs/src/plonk/lookup/prover.rs) on Python ints, and the key
generators of the sort's tests.  Nothing here calls the library.

permute_direct is halo2's loop as written there: sort the input, count the table's values in an
ordered map, walk the sorted input -- a row that differs from the one before takes its own value
from the map (a missing one is the failure, reported at that row), the others are pushed on a list
of repeated rows -- then walk the map's leftovers in ascending order and pop() the repeated rows
from the BACK.  permute_sorted is the parallel formulation the device runs: both columns sorted, a
leader marks the first occurrence of its value in the sorted table (a lower bound and an equality
test), the leftovers are the unmarked positions in order, and the k-th repeat of m takes leftover
m - 1 - k.  Both return (A', S', None) or (None, None, the smallest row of A' whose value is not in
the table)."""
import bisect
import random
from collections import Counter

from oracle import bn254 as b

R = b.R


def permute_direct(a, s):
    assert len(a) == len(s)
    ap = sorted(a)
    left = Counter(s)
    sp = [None] * len(a)
    repeated = []
    for i, v in enumerate(ap):
        if i == 0 or v != ap[i - 1]:
            if left[v] == 0:
                return None, None, i
            left[v] -= 1
            sp[i] = v
        else:
            repeated.append(i)
    for v in sorted(left):                       # a BTreeMap walks its keys in ascending order
        for _ in range(left[v]):
            sp[repeated.pop()] = v
    assert not repeated
    return ap, sp, None


def permute_sorted(a, s):
    assert len(a) == len(s)
    n = len(a)
    ap, t = sorted(a), sorted(s)
    leader = [i == 0 or ap[i] != ap[i - 1] for i in range(n)]
    used = [False] * n
    missing = None
    for i in range(n):
        if leader[i]:
            p = bisect.bisect_left(t, ap[i])
            if p < n and t[p] == ap[i]:
                used[p] = True
            elif missing is None:
                missing = i
    if missing is not None:
        return None, None, missing
    left = [t[p] for p in range(n) if not used[p]]
    repeats = [i for i in range(n) if not leader[i]]
    m = len(repeats)
    assert len(left) == m
    sp = [ap[i] if leader[i] else None for i in range(n)]
    for k, i in enumerate(repeats):
        sp[i] = left[m - 1 - k]
    return ap, sp, None


def check_relations(a, s, ap, sp, beta, gamma):
    """What the verifier checks of the permuted columns (snark-verifier system/halo2.rs:593-660)."""
    assert ap[0] == sp[0]
    assert all(ap[i] == sp[i] or ap[i] == ap[i - 1] for i in range(1, len(a)))
    lhs = rhs = 1
    for x, y, xp, yp in zip(a, s, ap, sp):
        lhs = lhs * (x + beta) % R * (y + gamma) % R
        rhs = rhs * (xp + beta) % R * (yp + gamma) % R
    assert lhs == rhs


def small_case(rng, n_max=12):
    """A random small pair: few distinct values, so repeats, duplicated table entries and missing
    values all occur."""
    n = rng.randint(1, n_max)
    span = rng.randint(1, 2 * n)
    s = [rng.randrange(span) for _ in range(n)]
    if rng.random() < 0.7:
        a = [rng.choice(s) for _ in range(n)]    # every value of a is in s: the lookup holds
    else:
        a = [rng.randrange(span + 2) for _ in range(n)]
    return a, s


# ---- keys of the sort's tests -------------------------------------------------------------------

EDGES = (0, 1, R - 1)


def plant(keys):
    """0, 1 and r - 1 at the first, the middle and the last row where n allows (n >= 3)."""
    n = len(keys)
    if n >= 3:
        for i, e in zip((0, n // 2, n - 1), EDGES):
            keys[i] = e
    return keys


def full_width(n, seed):
    """Uniform in [0, r): every one of the 32 digits is live from a handful of keys on."""
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


BASE = 0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809   # below r: its top byte is 0x1a


def one_digit(n, digit, seed):
    """Keys that differ from BASE only in 8-bit digit `digit` (digit 31: values 0 .. 0x2f, so the
    key stays below r): exactly one live pass."""
    rng = random.Random(seed)
    top = 0x30 if digit == 31 else 256
    clear = BASE & ~(0xFF << (8 * digit))
    return [clear | (rng.randrange(top) << (8 * digit)) for _ in range(n)]


def two_digits(n, lo, hi, seed, values=3):
    """Keys that differ from BASE in exactly the two digits lo < hi, `values` distinct values in
    each: two live passes, and the result is sorted only if the second pass keeps the first's order."""
    rng = random.Random(seed)
    clear = BASE & ~(0xFF << (8 * lo)) & ~(0xFF << (8 * hi))
    pick = [5, 130, 250, 77, 201][:values]
    top = [1, 9, 0x2f, 4, 0x20][:values] if hi == 31 else pick
    return [clear | (rng.choice(pick) << (8 * lo)) | (rng.choice(top) << (8 * hi)) for _ in range(n)]


def three_digits(n, digits, seed):
    """Keys that differ from BASE in exactly three digits below 31, three values in each: three live
    passes, an odd parity above one."""
    rng = random.Random(seed)
    clear = BASE
    for d in digits:
        clear &= ~(0xFF << (8 * d))
    return [clear | sum(rng.choice((5, 130, 250)) << (8 * d) for d in digits) for _ in range(n)]


def few_values(n, seed):
    rng = random.Random(seed)
    vals = [rng.randrange(R) for _ in range(3)]
    return [rng.choice(vals) for _ in range(n)]
