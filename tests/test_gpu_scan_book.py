"""GPU parity of the warp-specialized scan's step-level booking (D = 32,
k + 1 <= 32): the book waves book the two tiles of a barrier step as one unit
of eight blocks, and a lane that passes tau twice within a step redoes its
appends block by block.  Random data almost never makes a lane pass twice in
one step, so exact copies of a few unit vectors are planted in rows of the
same half-block side (the same lane) of consecutive tiles, and the users next
to those vectors have the copies as their top scores (exact ties: lower row
first).

Checker = the CPU oracle, bit for bit: rows, fp32 scores and exact scores.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

D, TILE, BLOCK = 32, 128, 32
N_USERS, N_PLANTED_USERS, N_VEC = 1100, 600, 8  # one full 1,024-user workgroup + 76 users
# 132 tiles, an even 22-tile pre-pass (main tiles (2a, 2a + 1) share a step), a masked partial last tile;
# 129 tiles, an odd 21-tile pre-pass (main tiles (2a + 1, 2a + 2) share a step, one step straddles the passes)
CATALOGS = {"even_pre_partial": 131 * 128 + 77, "odd_pre": 129 * 128}


@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _plant(items, vecs, t):
    """Copies of the 8 vectors around tile t, all in rows 0-3 of a 32-item
    block (one half-block side, so one lane sees them all): two blocks of
    tile t, one block of tile t + 1, one of tile t + 2 -- whichever way tiles
    pair into steps, one pair holds two copies -- and one copy in rows 4-7
    (the other side).  Tiles past the catalog get nothing; tile t + 1's
    copies sit in its first two blocks, which a 77-item partial tile still
    has."""
    n_tiles = (len(items) + TILE - 1) // TILE
    # (tile offset, block of vectors 0-3, block of vectors 4-7, first row within the block)
    for dt, b_lo, b_hi, row0 in ((0, 0, 1, 0), (0, 2, 3, 0), (1, 1, 0, 0), (2, 3, 0, 0), (1, 0, 1, 4)):
        if t + dt >= n_tiles:
            continue
        for i in range(N_VEC):
            row = (t + dt) * TILE + (b_lo if i < 4 else b_hi) * BLOCK + row0 + i % 4
            assert row < len(items)
            items[row] = vecs[i]


@functools.lru_cache(maxsize=None)
def _data(name):
    n_items = CATALOGS[name]
    rng = np.random.default_rng(n_items)
    items = _unit(rng.standard_normal((n_items, D)))
    vecs = _unit(rng.standard_normal((N_VEC, D)))
    n_tiles = (n_items + TILE - 1) // TILE
    last_full = n_items // TILE - 1
    # t = 5: tile 6 is a sampled tile (stride 6) and shares a step with an
    # ordinary one; t = 20: no sampled tile in reach of a pair with two
    # copies ... the last full tile and what follows it (the partial tile of
    # the 132-tile catalog; with 129 full tiles the last two)
    for t in (5, 20, last_full if last_full + 1 < n_tiles else last_full - 1):
        _plant(items, vecs, t)
    users = _unit(rng.standard_normal((N_USERS, D)))
    noisy = vecs[np.arange(N_PLANTED_USERS) % N_VEC] + 1e-3 * rng.standard_normal((N_PLANTED_USERS, D))
    users[:N_PLANTED_USERS] = _unit(noisy)
    items.setflags(write=False)
    users.setflags(write=False)
    return users, items


@functools.lru_cache(maxsize=None)
def _reference(name, k):
    users, items = _data(name)
    return oracle.ip_topk(users, items, k, exact=True)


def _single(ops, name, k):
    users, items = _data(name)
    s, r, e = ops.ip_topk(_dev(users), ops.Catalog(_dev(items)), k, exact=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy().astype(np.int64), e.cpu().numpy()


def test_planted_copies_are_the_top_scores():
    """The fixture does what it says (no GPU work): a planted user's best rows
    are copies of its vector, several of them in one tile pair."""
    for name in CATALOGS:
        users, items = _data(name)
        so, ro, _ = _reference(name, 11)
        for u in (0, 7, N_PLANTED_USERS - 1):
            assert np.all(ro[u] % BLOCK < 8) and np.all(np.diff(so[u]) <= 0)
            assert np.array_equal(items[ro[u, 0]], items[ro[u, 1]])
            tiles = ro[u] // TILE
            assert len(tiles) - len(set(tiles.tolist())) >= 2  # two copies in one tile, at two positions at least


@pytest.mark.parametrize("k", [11, 31, 32])
@pytest.mark.parametrize("name", list(CATALOGS))
def test_scan_step_booking_planted_vs_oracle(ops, name, k):
    s, r, e = _single(ops, name, k)
    so, ro, eo = _reference(name, k)
    assert np.array_equal(r, ro)
    assert np.array_equal(s, so)
    assert np.array_equal(e[ro >= 0], eo[ro >= 0])


@pytest.mark.parametrize("n_shards", [2, 3])
def test_scan_step_booking_planted_owner_replay(ops, n_shards):
    """The planted 132-tile catalog through the owner replay (shard scans:
    insert period 4, list bounds): rows and scores identical to one GPU."""
    from nrk.dist import HipRangeShard, owner_replay, shard_blocks

    name, k = "even_pre_partial", 31
    users, items = _data(name)
    s1, r1, _ = _single(ops, name, k)
    cat = ops.Catalog(_dev(items))
    tb = ops.ip_topk_tile_blocks(D)
    shards = [HipRangeShard(cat, *shard_blocks(len(items), n_shards, r, tb), k, len(users)) for r in range(n_shards)]
    s, r, _ = owner_replay(_dev(users), shards, k)
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy().astype(np.int64), r1)
    assert np.array_equal(s.cpu().numpy(), s1)
    so, ro, _ = _reference(name, k)
    assert np.array_equal(r1, ro)
    assert np.array_equal(s1, so)
