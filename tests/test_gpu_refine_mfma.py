"""GPU parity of the dim-32 refine at every place its prefilter can put an
item: each of the 16 items of a band half-block, each of the four places a
half-block takes in a prefilter group (four half-blocks = 64 items, one lane
each), groups with one to three half-blocks missing, the catalog's last,
partly filled half-block, ties, zero and badly scaled users, the wider k
paths, the owner path and the band path.  Every case compares rows, fp32
scores and fp64 scores with oracle.ip_topk bit for bit; all of them at D = 32.

The cases were written with the matrix-pipe prefilter of round 11 (measured
and not kept) and hold for any lane mapping of a group.

A band half-block q holds the 16 catalog rows hb_row(q, r).
"""
import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

D = 32


@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _unit(x):
    n = np.linalg.norm(x, axis=1, keepdims=True)
    n[n == 0] = 1
    return (x / n).astype(np.float32)


def _hb_row(q, r):
    """catalog row of item r (0..15) of half-block q (csrc/ip_topk.hip)"""
    return (q >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (q & 1)


def _check(ops, users, items, k):
    cat = ops.Catalog(_dev(items))
    s, r, e = ops.ip_topk(_dev(users), cat, k, exact=True)
    s2, r2 = ops.ip_topk(_dev(users), cat, k)  # k <= 64: the fp32-key sort
    torch.cuda.synchronize()
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy(), eo)
    assert np.array_equal(r2.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s2.cpu().numpy(), so)
    return ro


@pytest.fixture(scope="module")
def small_catalog():
    """4,096 small random rows (norm 0.05) and 8 user directions"""
    rng = np.random.default_rng(32)
    return 0.05 * _unit(rng.standard_normal((4096, D))), _unit(rng.standard_normal((8, D)))


# The planted row is the only top item.  `place` decoys, copies of it scaled
# by 1 - 2^-13 (inside the screen's 2 eps ~ 1e-3 of the top, so their
# half-blocks stay in the band at k = 1 too, and strictly below it exactly),
# lie in earlier half-blocks of the same list (the same half of earlier
# blocks): the planted half-block comes `place` entries later in the band.
def _plant(items, user, q, r, place, scale=1.0):
    for j in range(place):
        items[_hb_row(q - 2 * (place - j), (r + 5 * j + 3) & 15)] = user * np.float32(scale * (1.0 - 2.0 ** -13))
    items[_hb_row(q, r)] = user * np.float32(scale)
    return _hb_row(q, r)


@pytest.mark.parametrize("k", [1, 31])
@pytest.mark.parametrize("place", [0, 1, 2, 3])
def test_lane_mapping_one_user(ops, small_catalog, place, k):
    base, dirs = small_catalog
    for r in range(16):
        items = base.copy()
        q = 2 * (17 + 3 * r) + (r & 1)  # both halves of a block, both lists
        row = _plant(items, dirs[0], q, r, place)
        ro = _check(ops, dirs[:1], items, k)
        assert ro[0, 0] == row


@pytest.mark.parametrize("k", [1, 31])
@pytest.mark.parametrize("place", [0, 1, 2, 3])
def test_lane_mapping_eight_users(ops, small_catalog, place, k):
    base, dirs = small_catalog
    for r0 in range(16):
        items = base.copy()
        rows = []
        for i in range(8):
            r = (r0 + 2 * i + (i >> 2)) & 15
            q = 2 * (10 + 14 * i + (r0 & 3)) + (i & 1)  # blocks 14 apart: the decoys never collide
            rows.append(_plant(items, dirs[i], q, r, place, scale=1.0 + 0.125 * i))
        ro = _check(ops, dirs, items, k)
        assert ro[:, 0].tolist() == rows


@pytest.mark.parametrize("kp", [5, 6, 7, 9])
def test_group_tails(ops, small_catalog, kp):
    """kp separated top items and k = kp: the band is their kp half-blocks,
    4 g + 1, 4 g + 2 and 4 g + 3 of them."""
    base, dirs = small_catalog
    rng = np.random.default_rng(kp)
    items = base.copy()
    users = dirs[:3]
    want = []
    for j in range(kp):
        row = _hb_row(2 * (5 + 11 * j) + (j & 1), int(rng.integers(0, 16)))
        items[row] = (users[0] + users[1] + users[2]) * np.float32(1.0 - 0.05 * j)
        want.append(row)
    ro = _check(ops, users, items, kp)
    for u in range(3):
        assert ro[u].tolist() == want


@pytest.mark.parametrize("k", [31, 10])
@pytest.mark.parametrize("n_items", [1, 15, 16, 17, 31, 33, 1000, 1039])
def test_catalog_ends(ops, n_items, k):
    """The best item is the last row, in the last, partly filled half-block;
    n_items < k pads with -1 / -FLT_MAX."""
    rng = np.random.default_rng(n_items)
    users = _unit(rng.standard_normal((5, D)))
    items = 0.05 * _unit(rng.standard_normal((n_items, D)))
    items[-1] = users.sum(0)
    ro = _check(ops, users, items, k)
    assert (ro[:, 0] == n_items - 1).all()
    if n_items < k:
        assert (ro[:, n_items:] == -1).all()


def test_duplicated_rows_lower_row_first(ops):
    rng = np.random.default_rng(7)
    users = _unit(rng.standard_normal((6, D)))
    items = _unit(rng.standard_normal((3000, D)))
    items[1500:1520] = items[40]  # ties across half-blocks and groups
    items[2999] = items[3]
    users[2] = items[40]
    users[3] = items[3]
    ro = _check(ops, users, items, 31)
    assert ro[2, :21].tolist() == [40] + list(range(1500, 1520))
    assert ro[3, :2].tolist() == [3, 2999]


def test_zero_user_beside_live_users(ops):
    rng = np.random.default_rng(8)
    users = _unit(rng.standard_normal((9, D)))
    users[0] = 0.0
    users[5] = 0.0
    ro = _check(ops, users, _unit(rng.standard_normal((3000, D))), 31)
    assert ro[0].tolist() == list(range(31)) and ro[5].tolist() == list(range(31))


def test_user_values_span_2m20_to_2p10(ops):
    """The user's power-of-two scale: users whose largest value runs from
    2^-20 to 2^10, and users whose own values span that range."""
    rng = np.random.default_rng(9)
    users = _unit(rng.standard_normal((31, D)))
    users *= (2.0 ** np.arange(-20, 11, dtype=np.float64))[:, None].astype(np.float32)
    wide = np.sign(rng.standard_normal((4, D))) * 2.0 ** rng.integers(-20, 11, size=(4, D))
    wide[:, 0], wide[:, 1] = 2.0 ** -20, 2.0 ** 10
    users = np.concatenate([users, wide.astype(np.float32)])
    _check(ops, users, _unit(rng.standard_normal((5000, D))), 31)


@pytest.mark.parametrize("k", [61, 100])
def test_wider_k(ops, k):
    """k = 61: no fp32-key sort, a wider band; k = 100: 256 survivors held."""
    rng = np.random.default_rng(k)
    users = _unit(rng.standard_normal((70, D)))
    users[3] = 0.0
    items = _unit(rng.standard_normal((20_000, D)))
    cat = ops.Catalog(_dev(items))
    s, r, e = ops.ip_topk(_dev(users), cat, k, exact=True)
    s2, r2 = ops.ip_topk(_dev(users), cat, k)
    torch.cuda.synchronize()
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy(), eo)
    assert np.array_equal(r2.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s2.cpu().numpy(), so)


def test_owner_path_two_shards(ops):
    """The owner refine (n_src > 0) runs the same prefilter and exact
    rounds: a two-shard replay, 300 users x 3,000 items."""
    from nrk.dist import HipRangeShard, owner_replay, shard_blocks

    rng = np.random.default_rng(11)
    k = 31
    users = _unit(rng.standard_normal((300, D)))
    users[7] = 0.0
    items = _unit(rng.standard_normal((3000, D)))
    items[2990] = items[10]  # a cross-shard exact tie
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    cat = ops.Catalog(_dev(items))
    tb = ops.ip_topk_tile_blocks(D)
    shards = [HipRangeShard(cat, *shard_blocks(len(items), 2, r, tb), k, len(users)) for r in range(2)]
    s, r, e = owner_replay(_dev(users), shards, k)
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy(), eo)


def test_band_path_after_bound(ops):
    """screen -> bound -> finish: the refine reads the select's band."""
    rng = np.random.default_rng(12)
    k = 31
    users = _unit(rng.standard_normal((130, D)))
    users[2] = 0.0
    items = _unit(rng.standard_normal((9000, D)))
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    u = _dev(users)
    cat = ops.Catalog(_dev(items))
    ws = ops.ip_topk_workspace(len(users), cat, k, u.device)
    s = torch.empty((len(users), k), dtype=torch.float32, device=u.device)
    r = torch.empty((len(users), k), dtype=torch.int32, device=u.device)
    e = torch.empty((len(users), k), dtype=torch.float64, device=u.device)
    ops.ip_topk_screen(u, cat, k, ws)
    ops.ip_topk_bound(u, cat, k, 4, ws)
    ops.ip_topk_finish(u, cat, k, ws, s, r, out_exact=e)
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy(), eo)
