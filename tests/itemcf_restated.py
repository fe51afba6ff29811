"""Plain numpy restatements of the two exact seams of csrc/itemcf.hip (no
torch, no GPU): what nrk_itemcf_pairs must write per pair slot and what
nrk_itemcf_reduce must return for any (key, slot, weight) tuples.  They are
the checkers of tests/test_gpu_itemcf_edges.py; tests/test_itemcf_host.py
shows on the CPU that pairs_ref -> reduce_ref is oracle.itemcf_sim.
"""
import math

import numpy as np

LOC_ALPHA, LOC_ALPHA_REV, LOC_BETA, TIME_ALPHA, CREATED_ALPHA = 1.0, 0.7, 0.9, 0.7, 0.8

TILE = 4096  # keys per workgroup of the radix sort and the segmented sums
CHUNK = 16   # keys per thread inside a tile


def key_bits(n_items):
    """bj: the smallest b with 2^b > n_items (a key is i << bj | j, 2 bj bits)."""
    b = 1
    while (1 << b) <= n_items:
        b += 1
    return b


def sentinel(n_items):
    return (1 << (2 * key_bits(n_items))) - 1


def radix_passes(n_items):
    return -(-2 * key_bits(n_items) // 8)


def make_keys(i, j, n_items):
    bj = key_bits(n_items)
    return (np.asarray(i, np.uint64) << np.uint64(bj)) | np.asarray(j, np.uint64)


def run_sums(x, heads, how="f64"):
    """Sum of x over [heads[r], heads[r + 1]) per run r.  "f64": numpy's fp64
    sums; "fsum": exactly rounded (math.fsum per run); "longdouble": 64-bit
    mantissa sums rounded to fp64 once (vectorised, for millions of keys)."""
    if len(heads) == 0:
        return np.zeros(0, np.float64)
    if how == "f64":
        return np.add.reduceat(x, heads)
    if how == "longdouble" and np.finfo(np.longdouble).nmant >= 63:
        return np.add.reduceat(x.astype(np.longdouble), heads).astype(np.float64)
    ends = np.append(heads[1:], len(x))
    return np.array([math.fsum(x[a:b].tolist()) for a, b in zip(heads.tolist(), ends.tolist())], np.float64)


def reduce_ref(keys, slots, w, cnt, n_items, sums="f64"):
    """nrk_itemcf_reduce: one (i, j, v, first) entry per distinct key other
    than the sentinel, ascending by key.  first = slots[p0], p0 the smallest
    input position that holds the key; v = (sum of w over the key's input
    positions, ascending) / sqrt(cnt[i] * cnt[j]).  ``cnt`` is anything that
    answers cnt[ids] for an id array."""
    keys = np.asarray(keys).astype(np.uint64, copy=False)
    slots = np.asarray(slots)
    w = np.asarray(w, np.float64)
    bj = key_bits(n_items)
    order = np.argsort(keys, kind="stable")  # equal keys keep input order
    ks = keys[order]
    live = int(np.searchsorted(ks, np.uint64(sentinel(n_items)), side="left"))  # the sentinel is the largest key
    ks, order = ks[:live], order[:live]
    heads = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if live else np.zeros(0, np.int64)
    hk = ks[heads]
    i = (hk >> np.uint64(bj)).astype(np.int32)
    j = (hk & np.uint64((1 << bj) - 1)).astype(np.int32)
    s = run_sums(w[order], heads, sums)
    norm = np.sqrt((np.asarray(cnt[i], np.int64) * np.asarray(cnt[j], np.int64)).astype(np.float64))
    return i, j, s / norm, slots[order[heads]].astype(np.int64)


def pairs_ref(offsets, items, ts, created, n_items, slot_base=0):
    """nrk_itemcf_pairs: per slot p = pair_off[u] + l1 * L_u + l2 the key
    (items[l1] << bj | items[l2], the sentinel when the two are the same
    item), the global slot slot_base + p, the weight of item_cf.py:57-77
    (loc_w * click_w * created_w / log(L + 1); exactly 0.0 for a sentinel),
    and the per-item click count.  Returns (keys u64, slots i32, w f64, cnt i64)."""
    offsets = np.asarray(offsets, np.int64)
    items = np.asarray(items, np.int64)
    ts = np.asarray(ts, np.int64)
    created = np.asarray(created, np.float64)
    L = np.diff(offsets)
    pair_off = np.concatenate([[0], np.cumsum(L * L)])
    n = int(pair_off[-1])
    keys = np.full(n, sentinel(n_items), np.uint64)
    w = np.zeros(n, np.float64)
    for u in np.flatnonzero(L > 0).tolist():
        b, lu = int(offsets[u]), int(L[u])
        l1, l2 = np.divmod(np.arange(lu * lu), lu)
        i, j = items[b + l1], items[b + l2]
        m = i != j
        l1, l2, i, j = l1[m], l2[m], i[m], j[m]
        loc_w = np.where(l2 > l1, LOC_ALPHA, LOC_ALPHA_REV) * LOC_BETA ** (np.abs(l2 - l1) - 1).astype(np.float64)
        click_w = np.exp(TIME_ALPHA ** np.abs(ts[b + l1] - ts[b + l2]).astype(np.float64))
        created_w = np.exp(CREATED_ALPHA ** np.abs(created[i] - created[j]))
        p = pair_off[u] + np.flatnonzero(m)
        keys[p] = make_keys(i, j, n_items)
        w[p] = loc_w * click_w * created_w * (1.0 / math.log(lu + 1))
    slots = (slot_base + np.arange(n)).astype(np.int32)
    return keys, slots, w, np.bincount(items, minlength=n_items).astype(np.int64)


def random_lists(rng, n_users, n_items, max_len, repeat_p=0.1):
    """Random click lists as tests/test_gpu_itemcf.py draws them: lengths in
    [0, max_len], repeated clicks on the previous item, timestamps with ties
    and 1-ms gaps, equal created times."""
    L = rng.integers(0, max_len + 1, n_users)
    offs = np.zeros(n_users + 1, np.int64)
    offs[1:] = np.cumsum(L)
    items = rng.integers(0, n_items, offs[-1]).astype(np.int32)
    rep = rng.random(offs[-1]) < repeat_p
    rep[offs[:-1][L > 0]] = False
    idx = np.nonzero(rep)[0]
    items[idx] = items[idx - 1]
    ts = np.zeros(offs[-1], np.int64)
    for u in range(n_users):
        a, b = offs[u], offs[u + 1]
        ts[a:b] = 1_500_000_000_000 + np.cumsum(rng.integers(0, 4, b - a))
    created = rng.random(n_items)
    created[rng.integers(0, n_items, n_items // 10)] = 0.5
    return offs, items, ts, created
