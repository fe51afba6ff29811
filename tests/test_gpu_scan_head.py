"""GPU parity of the warp-specialized scan's step bookkeeping (D = 32, k = 31):
an MFMA wave carries a step's tile ids, ring half, body choice (masked or
not) and the source addresses of the next step's LDS-DMA pieces across the
barrier, formed one and two steps ahead.  A wrong tile in any step changes the
rows of many users, so random unit vectors suffice; the catalogs are the tile
counts at which the carried sequence changes shape.

Tiles are 128 items.  A range of n tiles has a pre-pass of n_pre = min(64,
n // 6) sampled tiles (none below 128 tiles), tile i * (n // n_pre) of the
range for i < n_pre, then the n main-pass tiles; a barrier step is two tiles of
that sequence.

Checker = the CPU oracle, bit for bit: rows, fp32 scores and exact scores.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle

D, K, TILE = 32, 31, 128
N_USERS = 1100  # one full 1,024-user workgroup + 76 users
PRE_MIN, PRE_MAX, PRE_DIV = 128, 64, 6

# name -> items
CATALOGS = {
    # the first look-ahead is the last step
    "tiles_2": 2 * TILE,
    # two steps, the second with a dummy second tile (the short last step)
    "tiles_3": 3 * TILE,
    # exactly two whole steps
    "tiles_4": 4 * TILE,
    # the longest range with no pre-pass (64 steps, the last one short)
    "tiles_127": 127 * TILE,
    # the shortest range with one: n_pre = 21, stride 6 -- odd, one step straddles the passes
    "tiles_128": 128 * TILE,
    # n_pre = 22, even; 154 sequence tiles, even; no masked tile: the unmasked body runs in every step
    "tiles_132_full": 132 * TILE,
    # A partial last tile: 129 tiles, n // n_pre = 129 // 21 = 6, sampled tiles 0, 6 .. 120: the last tile
    # (128) is NOT sampled.  150 sequence tiles: the partial tile is the second tile of the last whole step,
    # whose masked body is chosen two steps after the odd change-over step was formed.
    "partial_odd_pre": 128 * TILE + 77,
    # The other parity: 133 tiles, 133 // 22 = 6, sampled tiles 0, 6 .. 126: the last tile (132) is NOT
    # sampled either.  155 sequence tiles: the partial tile is the one tile of the short last step.
    # No range has a sampled last tile (test_last_tile_is_never_sampled): the masked choice can only ride
    # across the pre-pass -> main change-over as "unmasked" -- which every catalog of 128 tiles or more here does.
    "partial_even_pre": 132 * TILE + 77,
}
# 260 tiles, the last one partial; tile bounds of the ranges.  Two ranges: 131 + 129 tiles (both odd, both with a
# 21-tile pre-pass); three: 87 + 85 + 88 tiles (no pre-pass; two odd).  Every range but the first starts at
# tile_lo > 0; every range but the last ends before the catalog's last tile, with live tiles behind it.
SHARD_ITEMS = 259 * TILE + 77
SHARD_SPLITS = {2: (0, 131, 260), 3: (0, 87, 172, 260)}


@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _data(n_items):
    rng = np.random.default_rng(n_items)
    items = _unit(rng.standard_normal((n_items, D)))
    users = _unit(rng.standard_normal((N_USERS, D)))
    items.setflags(write=False)
    users.setflags(write=False)
    return users, items


@functools.lru_cache(maxsize=None)
def _reference(n_items):
    users, items = _data(n_items)
    return oracle.ip_topk(users, items, K, exact=True)


def _pre(n_tiles):
    n_pre = min(PRE_MAX, n_tiles // PRE_DIV) if n_tiles >= PRE_MIN else 0
    return n_pre, (n_tiles // n_pre if n_pre else 1)


def test_fixture_shapes():
    """The catalogs are what their comments say (no GPU work)."""
    tiles = {name: -(-n // TILE) for name, n in CATALOGS.items()}
    assert [tiles[f"tiles_{n}"] for n in (2, 3, 4, 127, 128)] == [2, 3, 4, 127, 128]
    assert _pre(127) == (0, 1) and _pre(128) == (21, 6) and _pre(132) == (22, 6)
    assert tiles["tiles_132_full"] == 132 and CATALOGS["tiles_132_full"] % TILE == 0
    assert (132 + 22) % 2 == 0
    assert tiles["partial_odd_pre"] == 129 and _pre(129) == (21, 6) and (129 + 21) % 2 == 0
    assert tiles["partial_even_pre"] == 133 and _pre(133) == (22, 6) and (133 + 22) % 2 == 1
    for name in ("partial_odd_pre", "partial_even_pre"):
        assert CATALOGS[name] % TILE != 0
        n_pre, stride = _pre(tiles[name])
        assert (n_pre - 1) * stride < tiles[name] - 1  # the last tile is not sampled
    assert -(-SHARD_ITEMS // TILE) == 260 and SHARD_ITEMS % TILE != 0
    for bounds in SHARD_SPLITS.values():
        counts = np.diff(bounds)
        assert bounds[0] == 0 and bounds[-1] == 260 and (counts % 2 == 1).any()
    assert [_pre(int(c))[0] for c in np.diff(SHARD_SPLITS[2])] == [21, 21]
    assert [_pre(int(c))[0] for c in np.diff(SHARD_SPLITS[3])] == [0, 0, 0]


def test_last_tile_is_never_sampled():
    """n_pre * (n // n_pre) <= n, so the largest sampled tile, (n_pre - 1) * (n // n_pre), is at most
    n - n // n_pre <= n - 6: no range -- a whole catalog or a shard's -- has its last tile in the pre-pass."""
    for n in range(PRE_MIN, 8192):
        n_pre, stride = _pre(n)
        assert stride >= PRE_DIV and (n_pre - 1) * stride <= n - PRE_DIV


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CATALOGS))
def test_scan_head_vs_oracle(ops, name):
    users, items = _data(CATALOGS[name])
    s, r, e = ops.ip_topk(_dev(users), ops.Catalog(_dev(items)), K, exact=True)
    torch.cuda.synchronize()
    so, ro, eo = _reference(CATALOGS[name])
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy()[ro >= 0], eo[ro >= 0])


@pytest.mark.gpu
@pytest.mark.parametrize("n_shards", list(SHARD_SPLITS))
def test_scan_head_shard_ranges_owner_replay(ops, n_shards):
    """The 260-tile catalog through nrk_ip_topk_shard_screen range by range (owner replay): the merged result
    equals the oracle."""
    from nrk.dist import HipRangeShard, owner_replay

    users, items = _data(SHARD_ITEMS)
    cat = ops.Catalog(_dev(items))
    tb = ops.ip_topk_tile_blocks(D)
    nblk = -(-SHARD_ITEMS // 32)
    bounds = SHARD_SPLITS[n_shards]
    shards = [HipRangeShard(cat, min(nblk, lo * tb), min(nblk, hi * tb), K, len(users))
              for lo, hi in zip(bounds[:-1], bounds[1:])]
    s, r, e = owner_replay(_dev(users), shards, K)
    torch.cuda.synchronize()
    so, ro, eo = _reference(SHARD_ITEMS)
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy()[ro >= 0], eo[ro >= 0])
