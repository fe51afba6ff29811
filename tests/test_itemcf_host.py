"""ItemCF checks that need no GPU: the numpy restatements of the pair walk and
the sort-reduce (tests/itemcf_restated.py, the checkers of
tests/test_gpu_itemcf_edges.py) compose to the oracle's similarity -- the same
keys in the same first-insertion order, the same counts, values to rtol 1e-12
-- and their building blocks (key widths, run sums) are what they say."""
import math

import numpy as np
import pytest

from oracle import oracle

import itemcf_restated as rs

RTOL = 1e-12


@pytest.mark.parametrize("n_users,n_items,max_len", [(1, 3, 1), (5, 4, 6), (300, 50, 40), (400, 20000, 25),
                                                     (20, 1_100_000, 120)])
def test_pairs_then_reduce_is_the_oracle_similarity(n_users, n_items, max_len):
    rng = np.random.default_rng(n_users + n_items)
    offs, items, ts, created = rs.random_lists(rng, n_users, n_items, max_len)
    keys, slots, w, cnt = rs.pairs_ref(offs, items, ts, created, n_items, slot_base=0)
    oi, oj, ov, _, ocnt = oracle.itemcf_sim(offs, items, ts, created, n_items)
    assert np.array_equal(cnt, ocnt)
    for how in ("f64", "fsum", "longdouble"):
        i, j, v, first = rs.reduce_ref(keys, slots, w, cnt, n_items, sums=how)
        assert len(i) == len(oi)
        # ascending (i, j), no duplicates: as a set ...
        k = i.astype(np.int64) * n_items + j
        assert np.all(np.diff(k) > 0)
        assert np.array_equal(k, np.sort(oi.astype(np.int64) * n_items + oj))
        # ... and in first-insertion order
        order = np.argsort(first, kind="stable")
        assert np.array_equal(i[order], oi) and np.array_equal(j[order], oj)
        np.testing.assert_allclose(v[order], ov, rtol=RTOL, atol=0)


def test_pairs_ref_slots_sentinels_and_slot_base():
    rng = np.random.default_rng(5)
    offs, items, ts, created = rs.random_lists(rng, 40, 6, 9, repeat_p=0.3)
    L = np.diff(offs)
    k0, s0, w0, c0 = rs.pairs_ref(offs, items, ts, created, 6)
    k1, s1, w1, c1 = rs.pairs_ref(offs, items, ts, created, 6, slot_base=12345)
    assert len(k0) == int((L * L).sum())
    assert np.array_equal(s0, np.arange(len(k0))) and np.array_equal(s1, s0 + 12345)
    assert np.array_equal(k0, k1) and np.array_equal(w0, w1) and np.array_equal(c0, c1)
    sent = k0 == rs.sentinel(6)
    assert sent.any() and (w0[sent] == 0.0).all() and (w0[~sent] > 0.0).all()
    # every user has at least its L diagonal slots as sentinels
    assert int(sent.sum()) >= int(L.sum())
    assert np.array_equal(c0, np.bincount(items, minlength=6))


def test_key_widths_and_radix_passes():
    n_items = [1, 3, 15, 16, 255, 256, 4095, 4096, 65535, 65536, 2**20, 2**24, 2**28]
    assert [rs.radix_passes(n) for n in n_items] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 7, 8]
    for n in n_items:
        bj = rs.key_bits(n)
        assert (1 << bj) > n >= (1 << (bj - 1)) or n == 1
        top = int(rs.make_keys([n - 1], [n - 1], n)[0])
        assert top < rs.sentinel(n)  # the sentinel is larger than every key of the catalog
        assert (top >> bj, top & ((1 << bj) - 1)) == (n - 1, n - 1)


def test_reduce_ref_on_a_hand_built_case():
    n_items = 5
    keys = rs.make_keys([2, 0, 2, 4, 0, 2], [1, 3, 1, 4, 3, 1], n_items)
    keys[3] = rs.sentinel(n_items)
    slots = np.array([50, 7, 9, 1, 3, 8], np.int32)
    w = np.array([1.0, 2.0, 4.0, 100.0, 8.0, 16.0])
    cnt = np.array([4, 1, 9, 1, 1], np.int64)
    i, j, v, first = rs.reduce_ref(keys, slots, w, cnt, n_items)
    assert i.tolist() == [0, 2] and j.tolist() == [3, 1]
    assert first.tolist() == [7, 50]  # the slot at the smallest input position, not the smallest slot
    assert v.tolist() == [10.0 / 2.0, 21.0 / 3.0]
    assert len(rs.reduce_ref(keys[3:4], slots[3:4], w[3:4], cnt, n_items)[0]) == 0
    assert len(rs.reduce_ref(keys[:0], slots[:0], w[:0], cnt, n_items)[0]) == 0


def test_run_sums_variants_agree_with_fsum():
    rng = np.random.default_rng(9)
    x = rng.random(30000) + 0.1
    heads = np.array([0, 1, 3, 20, 10000])  # the last run: 20,000 terms
    exact = rs.run_sums(x, heads, "fsum")
    assert exact[4] == math.fsum(x[10000:].tolist())
    # 64-bit-mantissa sums rounded once: within one fp64 ulp of the exactly rounded sum
    np.testing.assert_allclose(rs.run_sums(x, heads, "longdouble"), exact, rtol=2.3e-16, atol=0)
    # a strictly sequential fp64 sum of positive terms stays far inside the 1e-12 bar
    seq = 0.0
    for t in x[10000:].tolist():
        seq += t
    assert abs(seq - exact[4]) <= 1e-13 * exact[4]
    np.testing.assert_allclose(rs.run_sums(x, heads, "f64"), exact, rtol=1e-13, atol=0)
