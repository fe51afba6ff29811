"""GPU parity of the refine's half-block-wide prefilter loads (dims 16 and 32:
one wave load per contiguous KB, 2 or 4 lanes per item, the catalog row formed
only for kept items) and of the survivor sort on one u64 key (fp32 score's
ordered key, ~row) with its fallback to the exact sort when two fp32 scores
tie.

Checker = the CPU oracle, bit for bit, for every user: rows and fp32 scores,
and the exact scores where exact=True (the path that keeps the old sort).
Catalogs are 40 blocks + 13 items, so the last half-blocks are partly or wholly
past the catalog; 257 users leave a partial last workgroup.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

N_ITEMS = 40 * 32 + 13
N_USERS = 257
DIMS = [16, 32, 64, 20]  # 20: the generic path (regression)
KS = [1, 5, 31, 32, 64, 100]  # both survivor capacities, k > 64 beside the key sort


@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _hb_rows(b, h):
    """The 16 catalog rows of half-block 2 b + h, in its item order r = 0..15."""
    r = np.arange(16)
    return 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h


def _seq_dot(u, v):
    """The oracle's exact score: fp64 products summed in dimension order."""
    s = 0.0
    for a, b in zip(u.astype(np.float64), v.astype(np.float64)):
        s += a * b
    return s + 0.0


def _run(ops, users, items, k, exact=False):
    out = ops.ip_topk(_dev(users), ops.Catalog(_dev(items)), k, exact=exact)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(ops, users, items, k, exact=False):
    ref = oracle.ip_topk(users, items, k, exact=True)
    got = _run(ops, users, items, k, exact=exact)
    assert np.array_equal(got[1].astype(np.int64), ref[1])
    assert np.array_equal(got[0], ref[0])
    if exact:
        assert np.array_equal(got[2][ref[1] >= 0], ref[2][ref[1] >= 0])
    return ref


@functools.lru_cache(maxsize=None)
def _random(dim):
    rng = np.random.default_rng(100 + dim)
    users = _unit(rng.standard_normal((N_USERS, dim)))
    items = _unit(rng.standard_normal((N_ITEMS, dim)))
    users.setflags(write=False)
    items.setflags(write=False)
    return users, items


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", DIMS)
def test_random_vs_oracle(ops, dim, k):
    users, items = _random(dim)
    _check(ops, users, items, k)


@pytest.mark.parametrize("k", [31, 100])
def test_exact_scores_keep_the_exact_sort(ops, k):
    users, items = _random(32)
    _check(ops, users, items, k, exact=True)


@pytest.mark.parametrize("dim", [16, 32, 64])
def test_half_block_of_survivors(ops, dim):
    """16 users; for user j the rows of one half-block hold c_r * u_j with c
    decreasing from 1: all 16 items of one wave load (every lane group) are
    kept and survive.  The half-blocks include both halves of the last block,
    whose rows are partly past the catalog."""
    rng = np.random.default_rng(7 + dim)
    users = _unit(rng.standard_normal((N_USERS, dim)))
    items = (0.5 * _unit(rng.standard_normal((N_ITEMS, dim)))).astype(np.float32)
    spots = [(b, h) for b in (0, 1, 2, 3, 17, 38, 39, 40) for h in (0, 1)]
    planted = np.zeros(16, np.int64)
    for j, (b, h) in enumerate(spots):
        for r, row in enumerate(_hb_rows(b, h)):
            if row < N_ITEMS:
                items[row] = np.float32(1.0 - r / 64.0) * users[j]
                planted[j] += 1
    assert planted.min() >= 5 and planted.max() == 16
    _, ro = _check(ops, users, items, 31)[:2]
    for j, (b, h) in enumerate(spots):
        want = [row for row in _hb_rows(b, h) if row < N_ITEMS]
        assert ro[j, : len(want)].tolist() == want  # the fixture does what it says


@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("dim", [16, 32])
def test_exact_duplicates_lower_row_first(ops, dim, k):
    """Exact copies of a user's top item in its own half-block and in other
    blocks: equal fp64 (and fp32) scores, so the fp32-tie fallback runs and
    the lower row comes first."""
    rng = np.random.default_rng(11 + dim)
    users = _unit(rng.standard_normal((N_USERS, dim)))
    items = (0.5 * _unit(rng.standard_normal((N_ITEMS, dim)))).astype(np.float32)
    copies = {}
    for j in range(8):  # distinct blocks: no copy overwrites another user's
        b = 5 * j
        rows = [int(_hb_rows(b, j & 1)[3]), int(_hb_rows(b, j & 1)[9]), 32 * ((b + 7) % 40) + 1 + (j % 5),
                32 * ((b + 20) % 40) + 30]
        for row in rows:
            items[row] = users[j]
        copies[j] = sorted(rows)
    _, ro = _check(ops, users, items, k)[:2]
    for j, rows in copies.items():
        n = min(k, 4)
        assert ro[j, :n].tolist() == rows[:n]


def _tie_pair(u, rng):
    """Two item rows with different exact scores against u that round to the
    same fp32 score: b is a with one small coordinate moved by one fp32 ulp."""
    a = (np.float32(0.6) * u + np.float32(0.01) * rng.standard_normal(len(u)).astype(np.float32)).astype(np.float32)
    cand = [d for d in np.argsort(np.abs(a)) if a[d] != 0 and u[d] != 0]
    for d in cand:
        b = a.copy()
        b[d] = np.nextafter(a[d], np.float32(-np.inf if u[d] > 0 else np.inf), dtype=np.float32)
        sa, sb = _seq_dot(u, a), _seq_dot(u, b)
        if sa > sb and np.float32(sa) == np.float32(sb):
            return a, b, sa, sb
    raise AssertionError("no fp32-tied pair found")


@pytest.mark.parametrize("k,above", [(5, 4), (5, 1), (31, 30), (31, 7), (64, 63)])
def test_fp32_tie_with_different_exact_scores(ops, k, above):
    """The pair sits at sorted positions above, above + 1 (above = k - 1:
    straddling k, only the exactly larger one is output).  The exactly larger
    item has the HIGHER row, so the order of the u64 key (fp32 score, row asc)
    is wrong there and the exact sort has to decide."""
    dim = 32
    rng = np.random.default_rng(1000 * k + above)
    users = _unit(rng.standard_normal((N_USERS, dim)))
    items = (0.3 * _unit(rng.standard_normal((N_ITEMS, dim)))).astype(np.float32)
    pairs = {}
    n_pair_users = min(20, 1000 // (above + 2))
    # every planted row belongs to one user: the pairs that share a half-block
    # are set aside first, the rest is dealt from one permutation
    same_hb = {j: _hb_rows((7 * j) % 40, j & 1)[[2, 13]] for j in range(3, n_pair_users, 4)}
    taken = {int(x) for hb in same_hb.values() for x in hb}
    pool = [int(x) for x in rng.permutation(N_ITEMS) if int(x) not in taken]
    for j in range(n_pair_users):
        u = users[j]
        a, b, sa, sb = _tie_pair(u, rng)
        assert np.float32(sa) == np.float32(sb) and sa > sb  # fp32 tie, fp64 difference
        mine, pool = pool[: above + 2], pool[above + 2:]
        lo, hi = sorted(same_hb[j].tolist() if j in same_hb else mine[:2])
        for i, row in enumerate(mine[2:]):
            items[row] = np.float32(1.0 - 0.3 * i / above) * u  # above items, scores > 0.7
        items[hi], items[lo] = a, b
        pairs[j] = (lo, hi)
    ref = oracle.ip_topk(users, items, k, exact=True)
    for j, (lo, hi) in pairs.items():
        # the fixture does what it says: hi at position above, lo right after it (or cut off)
        assert ref[1][j, above] == hi
        if above + 1 < k:
            assert ref[1][j, above + 1] == lo and ref[0][j, above] == ref[0][j, above + 1]
            assert ref[2][j, above] > ref[2][j, above + 1]
    got = _run(ops, users, items, k)
    assert np.array_equal(got[1].astype(np.int64), ref[1])
    assert np.array_equal(got[0], ref[0])


@pytest.mark.parametrize("dim", DIMS)
def test_zero_user(ops, dim):
    users, items = _random(dim)
    users = users.copy()
    users[[0, 130, 256]] = 0.0
    s, r = _check(ops, users, items, 31)[:2]
    assert r[130].tolist() == list(range(31)) and not s[130].any()


@pytest.mark.parametrize("eu,ei", [(20, -20), (-20, 20), (20, 20), (-20, -20)])
@pytest.mark.parametrize("dim", [16, 32])
def test_power_of_two_scales(ops, dim, eu, ei):
    users, items = _random(dim)
    _check(ops, np.ldexp(users, eu).astype(np.float32), np.ldexp(items, ei).astype(np.float32), 31)


@pytest.mark.parametrize("dim", [16, 32])
def test_fp16_subnormals_in_the_packed_copy(ops, dim):
    """A third of the items have all components but one at 2^-12 of their
    largest, and half of those are 2^-16 of the catalog's scale: their small
    components are fp16 subnormals (or zero) in the packed copy."""
    rng = np.random.default_rng(31 + dim)
    users = _unit(rng.standard_normal((N_USERS, dim)))
    items = _unit(rng.standard_normal((N_ITEMS, dim)))
    idx = np.arange(0, N_ITEMS, 3)
    big = rng.integers(0, dim, len(idx))
    small = np.ldexp(rng.uniform(0.5, 2.0, (len(idx), dim)) * rng.choice([-1.0, 1.0], (len(idx), dim)), -12)
    small[np.arange(len(idx)), big] = rng.choice([-1.0, 1.0], len(idx))
    small[::2] = np.ldexp(small[::2], -16)
    items[idx] = small.astype(np.float32)
    # the catalog's scale maps max |x| into [2^13, 2^14)
    scale = np.ldexp(1.0, 14 - int(np.frexp(np.abs(items).max())[1]))
    packed = np.abs((items.astype(np.float64) * scale).astype(np.float16).astype(np.float64))
    assert np.count_nonzero((packed > 0) & (packed < 2.0 ** -14)) > 100
    _check(ops, users, items, 31)
    _check(ops, users, items, 5)
