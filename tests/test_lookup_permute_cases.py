"""The two restatements of halo2's permute_expression_pair in tests/lookup_permute_cases.py agree:
the direct one (a Counter walked in key order, pop() from the back of the repeated rows) and the
sorted one the device runs (lower bounds in the sorted table, the k-th repeat takes leftover
m - 1 - k), on a few thousand random small cases, failing ones included: the same outputs and the
same reported row.  The three relations the verifier checks hold on every output."""
import random

import lookup_permute_cases as lp

R = lp.R


def test_the_two_restatements_agree_on_random_small_cases():
    rng = random.Random(20261)
    failing = holding = with_repeats = 0
    for _ in range(5000):
        a, s = lp.small_case(rng)
        direct, sorted_ = lp.permute_direct(a, s), lp.permute_sorted(a, s)
        assert direct == sorted_, (a, s)
        ap, sp, row = direct
        if row is None:
            holding += 1
            with_repeats += len(set(a)) < len(a)
            assert sorted(sp) == sorted(s) and ap == sorted(a)
            lp.check_relations(a, s, ap, sp, rng.randrange(R), rng.randrange(R))
        else:
            failing += 1
            assert sorted(a)[row] not in s and all(v in s for v in sorted(a)[:row])
    assert failing > 500 and holding > 2000 and with_repeats > 1000


def test_hand_worked_cases():
    # the smallest leftover goes to the LAST repeated row
    a, s = [7, 7, 7, 3], [3, 7, 1, 9]
    assert lp.permute_direct(a, s) == ([3, 7, 7, 7], [3, 7, 9, 1], None)
    assert lp.permute_sorted(a, s) == ([3, 7, 7, 7], [3, 7, 9, 1], None)
    # a duplicated table entry: one copy is taken, the other is a leftover
    a, s = [5, 5, 2], [5, 5, 2]
    assert lp.permute_direct(a, s) == lp.permute_sorted(a, s) == ([2, 5, 5], [2, 5, 5], None)
    # two missing values: the smaller row; a value below min S and one above max S
    assert lp.permute_direct([9, 4, 6, 8], [4, 5, 7, 7])[2] == lp.permute_sorted([9, 4, 6, 8], [4, 5, 7, 7])[2] == 1
    assert lp.permute_sorted([1, 5], [5, 5])[2] == 0 and lp.permute_direct([1, 5], [5, 5])[2] == 0
    assert lp.permute_sorted([5, 9], [5, 5])[2] == 1 and lp.permute_direct([5, 9], [5, 5])[2] == 1
    # field-sized values
    a, s = [R - 1, 0, R - 1, 1], [1, 0, R - 1, R - 2]
    assert lp.permute_direct(a, s) == lp.permute_sorted(a, s) == ([0, 1, R - 1, R - 1], [0, 1, R - 1, R - 2], None)


def test_key_generators_have_the_live_digits_they_claim():
    def live(keys):
        return [d for d in range(32) if len({(k >> (8 * d)) & 255 for k in keys}) > 1]
    assert live(lp.full_width(300, 1)) == list(range(32))
    for d in (0, 13, 31):
        keys = lp.one_digit(300, d, d)
        assert live(keys) == [d] and max(keys) < R
    for lo, hi in ((0, 2), (3, 31), (10, 20)):
        keys = lp.two_digits(300, lo, hi, lo)
        assert live(keys) == [lo, hi] and max(keys) < R and len(set(keys)) <= 9
    assert live(lp.three_digits(300, (1, 5, 9), 2)) == [1, 5, 9]
    assert len(set(lp.few_values(300, 3))) == 3
    assert lp.plant([5] * 9)[0::4] == [0, 1, R - 1] and lp.plant([5, 5]) == [5, 5]
