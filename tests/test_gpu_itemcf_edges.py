"""GPU parity at the boundaries of csrc/itemcf.hip that random click logs do
not reach, through the two exact seams of the C ABI (nrk_itemcf_reduce,
nrk_itemcf_pairs) and the public ops:

* the radix sort and the three-level segmented sums on hand-built keys: runs
  that end on, just before and just after tile edges (tile 4,096, chunk 16),
  whole tiles without a head, sentinel tails, the second level of every scan
  (> 256 and > 1,024 tiles) and every pass count of the key width (1..8);
* the flat pair walk on crafted logs (long blocks of users without pairs,
  users ending on chunk edges), the LDS count hash at its wrap-around, the
  one-workgroup scans on both sides of their 8,192-value tile;
* every candidate-count rung of rc_query_kernel on both sides of 64 distinct
  candidates;
* the wide top-n / top-k paths at their 2,048 cap.

Checkers: tests/itemcf_restated.py (shown equal to the oracle on the CPU by
tests/test_itemcf_host.py) and the oracle.  Structure is exact everywhere.
Values: with integer weights and unit counts every association of the sums
is exact, so they are compared bit for bit; with real weights they are held
to rtol 1e-12 (the ItemCF bar) against 64-bit-mantissa sums -- all terms are
positive, so any summation order is within depth * 2^-53 of the true sum --
and two runs of the same call must agree bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import oracle

import itemcf_restated as rs

pytestmark = pytest.mark.gpu
RTOL = 1e-12
T = rs.TILE
MIXED = [1, 2, 15, 16, 17, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5]


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------ 2. sort-reduce --
def _run_keys(rng, runs, n_items, n_sentinel=0):
    """len(runs) distinct keys in ascending order, key r repeated runs[r]
    times, then n_sentinel sentinels: the sorted layout.  Returned with a
    random permutation applied, so input order differs from key order."""
    R = len(runs)
    ids = np.unique(rng.integers(0, n_items * n_items, 2 * R + 64))
    assert len(ids) >= R
    ids = np.sort(rng.permutation(ids)[:R])
    keys = np.repeat(rs.make_keys(ids // n_items, ids % n_items, n_items), runs)
    keys = np.concatenate([keys, np.full(n_sentinel, rs.sentinel(n_items), np.uint64)])
    return keys[rng.permutation(len(keys))]


def _slots(rng, n):
    """n distinct int32 values over the whole positive range, in random order."""
    step = max(1, (2**31 - 1) // max(n, 1) - 1)
    return (rng.permutation(n).astype(np.int64) * step + 5).astype(np.int32)


class _SparseCount:
    """cnt[ids] of a count array that is 1 except at ``ids`` (a 2^28-item
    catalog's counts are not held on the host)."""

    def __init__(self, ids, vals):
        self.ids, self.vals = ids, vals

    def __getitem__(self, x):
        if len(self.ids) == 0:
            return np.ones(len(x), np.int64)
        p = np.minimum(np.searchsorted(self.ids, x), len(self.ids) - 1)
        return np.where(self.ids[p] == x, self.vals[p], 1)


def _check_reduce(rng, keys, n_items, cnt_dev=None):
    """Both weight regimes of one key layout against reduce_ref."""
    from nrk import ops

    n = len(keys)
    bj = rs.key_bits(n_items)
    slots = _slots(rng, n)
    if cnt_dev is None:
        cnt_dev = torch.ones(n_items, dtype=torch.int64, device="cuda")
    assert bool((cnt_dev == 1).all()) or n_items > 2**26
    dk, ds = _d(keys.view(np.int64)), _d(slots)
    # exact: integer weights, unit counts -> every association of the sums is exact
    w = rng.integers(1, 1000, n).astype(np.float64)
    got = ops.itemcf_reduce(dk, ds, _d(w), n_items, cnt_dev)
    ri, rj, rv, rf = rs.reduce_ref(keys, slots, w, _SparseCount(np.zeros(0, np.int64), None), n_items)
    assert rv.size == 0 or float(np.max(rv)) < 2.0**53
    assert got.i.numel() == len(ri)
    assert np.array_equal(got.i.cpu().numpy(), ri) and np.array_equal(got.j.cpu().numpy(), rj)
    assert np.array_equal(got.first.cpu().numpy(), rf)
    assert np.array_equal(got.v.cpu().numpy(), rv)
    # real: positive weights, counts in [1, 50] at the ids in use
    w = rng.random(n) + 0.1
    live = keys[keys != np.uint64(rs.sentinel(n_items))]
    used = np.unique(np.concatenate([live >> np.uint64(bj), live & np.uint64((1 << bj) - 1)]).astype(np.int64))
    cvals = rng.integers(1, 51, len(used))
    if len(used):
        cnt_dev[_d(used)] = _d(cvals)
    dw = _d(w)
    got = ops.itemcf_reduce(dk, ds, dw, n_items, cnt_dev)
    again = ops.itemcf_reduce(dk, ds, dw, n_items, cnt_dev)
    if len(used):
        cnt_dev[_d(used)] = 1
    ri, rj, rv, rf = rs.reduce_ref(keys, slots, w, _SparseCount(used, cvals), n_items, sums="longdouble")
    assert got.i.numel() == len(ri)
    assert np.array_equal(got.i.cpu().numpy(), ri) and np.array_equal(got.j.cpu().numpy(), rj)
    assert np.array_equal(got.first.cpu().numpy(), rf)
    gv = got.v.cpu().numpy()
    if len(rv):
        print(f"reduce n={n} entries={len(rv)} max rel err {np.max(np.abs(gv - rv) / rv):.3e}")
    np.testing.assert_allclose(gv, rv, rtol=RTOL, atol=0)
    for a, b in ((got.i, again.i), (got.j, again.j), (got.first, again.first)):
        assert torch.equal(a, b)
    assert np.array_equal(gv.view(np.int64), again.v.cpu().numpy().view(np.int64))  # the association is fixed
    return len(ri)


@pytest.fixture(scope="module")
def ones3000():
    return torch.ones(3000, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193])
def test_reduce_all_keys_distinct(n, ones3000):
    rng = np.random.default_rng(n)
    assert _check_reduce(rng, _run_keys(rng, [1] * n, 3000), 3000, ones3000) == n


@pytest.mark.parametrize("n", [1, 4096, 4097, 3 * T, 3 * T + 1, 5 * T + 17])
def test_reduce_one_key_only(n, ones3000):
    rng = np.random.default_rng(n + 1)
    assert _check_reduce(rng, _run_keys(rng, [n], 3000), 3000, ones3000) == 1


@pytest.mark.parametrize("runs", [[T, T], [T - 1, 1, T], [1, 2 * T - 1, 1], [T + 1, T - 1], [17, 3 * T, 5]],
                         ids=lambda r: "-".join(map(str, r)))
def test_reduce_runs_on_tile_edges(runs, ones3000):
    """Run ends and starts on, just before and just after tile edges; whole
    tiles without a head (their sum is written from a later tile)."""
    rng = np.random.default_rng(sum(runs) + len(runs))
    assert _check_reduce(rng, _run_keys(rng, runs, 3000), 3000, ones3000) == len(runs)


def _mixed_runs(rng, total):
    runs, s = [], 0
    while s < total:
        r = min(int(rng.choice(MIXED)), total - s)
        runs.append(r)
        s += r
    return runs


def test_reduce_mixed_run_lengths(ones3000):
    """About 60k keys: every length of the mixed set twice, a few more drawn, in random order."""
    rng = np.random.default_rng(60)
    runs = MIXED * 2
    while sum(runs) < 60_000:
        runs = runs + [int(rng.choice(MIXED))]
    runs = rng.permutation(runs).tolist()
    assert set(runs) == set(MIXED) and 60_000 <= sum(runs) < 60_000 + 3 * T + 5
    ends = np.cumsum(runs)
    assert ((ends // T) - ((ends - runs) // T) >= 2).any()  # a run covers a whole tile
    assert _check_reduce(rng, _run_keys(rng, runs, 3000), 3000, ones3000) == len(runs)


@pytest.mark.parametrize("live,on_edge", [([100, 2 * T - 100], True), ([100, 2 * T - 93], False)],
                         ids=["tile_edge", "mid_chunk"])
@pytest.mark.parametrize("tail", [1, 17, T, T + 904])
def test_reduce_sentinel_tail(tail, live, on_edge, ones3000):
    """Sentinels after a run that ends exactly on a tile edge, and beginning
    in the middle of a thread's chunk; tail T and T + 904 leave whole tiles
    of sentinels."""
    start = sum(live)
    assert start % T == 0 if on_edge else start % rs.CHUNK != 0
    rng = np.random.default_rng(tail + start)
    assert _check_reduce(rng, _run_keys(rng, live, 3000, n_sentinel=tail), 3000, ones3000) == 2


def test_reduce_all_sentinel_and_empty(ones3000):
    from nrk import ops

    rng = np.random.default_rng(3)
    assert _check_reduce(rng, _run_keys(rng, [], 3000, n_sentinel=T + 5), 3000, ones3000) == 0
    e = lambda dt: torch.empty(0, dtype=dt, device="cuda")  # noqa: E731
    got = ops.itemcf_reduce(e(torch.int64), e(torch.int32), e(torch.float64), 3000, ones3000)
    assert got.i.numel() == 0 and got.v.numel() == 0 and got.first.numel() == 0


@pytest.mark.parametrize("tiles,cross", [(257, 256), (1025, 1024)])
def test_reduce_two_level_scans(tiles, cross, ones3000):
    """More than 256 tiles (rs_scan_rows walks chunks of tiles) and more than
    1,024 (cf_carry_scan / cf_head_scan do); a 3T + 5 run lies across tiles
    cross - 1 / cross, the edge between two scan chunks."""
    n = tiles * T + 3
    rng = np.random.default_rng(tiles)
    start = (cross - 3) * T + 50
    runs = _mixed_runs(rng, start) + [3 * T + 5]
    runs += _mixed_runs(rng, n - sum(runs))
    ends = np.cumsum(runs)
    assert sum(runs) == n and -(-n // T) > cross
    k = int(np.searchsorted(ends, cross * T, side="right"))  # the run that holds key cross * T
    assert runs[k] == 3 * T + 5 and ends[k] - runs[k] < (cross - 1) * T and ends[k] > cross * T
    assert _check_reduce(rng, _run_keys(rng, runs, 3000), 3000, ones3000) == len(runs)


@pytest.mark.parametrize("n_items,passes", list(zip(
    [1, 3, 15, 16, 255, 256, 4095, 4096, 65535, 65536, 2**20, 2**24, 2**28],
    [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 7, 8])))
def test_reduce_key_width(n_items, passes):
    """Every radix pass count: about 10,000 tuples with repeats over random
    ids that include 0 and n_items - 1, so the top digit is populated."""
    assert rs.radix_passes(n_items) == passes
    rng = np.random.default_rng(passes * 131 + n_items % 97)
    pi, pj = rng.integers(0, n_items, 2000), rng.integers(0, n_items, 2000)
    pi[:2], pj[:2] = [0, n_items - 1], [n_items - 1, 0]
    pick = rng.integers(0, 2000, 10_000)
    pick[:2] = [0, 1]
    keys = rs.make_keys(pi[pick], pj[pick], n_items)
    assert int(keys.max()) >> (8 * (passes - 1)) != 0 or n_items == 1
    assert len(np.unique(keys)) < len(keys)
    cnt = torch.ones(n_items, dtype=torch.int64, device="cuda")
    assert _check_reduce(rng, keys, n_items, cnt) == len(np.unique(keys))


# ------------------------------------- 3. pair walk, count hash, scans --
GAPS = np.array([0, 1, 5, 3000])


def _log(rng, lens, n_items, gaps=GAPS):
    lens = np.asarray(lens, np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = rng.integers(0, n_items, offs[-1]).astype(np.int32)
    ts = np.zeros(offs[-1], np.int64)
    for u in np.flatnonzero(lens).tolist():
        ts[offs[u]:offs[u + 1]] = 1_500_000_000_000 + np.cumsum(rng.choice(gaps, lens[u]))
    return offs, items, ts, rng.random(n_items)


def _blocks(mask):
    """Lengths of the blocks of consecutive True."""
    out, cur = [], 0
    for m in list(mask) + [False]:
        if m:
            cur += 1
        elif cur:
            out.append(cur)
            cur = 0
    return out


def _pair_cases():
    c = {}
    # (a) blocks of users without pairs between users with pairs, at the start and at the end too
    c["empty_blocks"] = ([0] * 70 + [5] + [0] * 130 + [3, 9] + [0] * 200 + [7, 2] + [0] * 70, 50)
    # (b) 64, 65 and 200 consecutive one-click users (one sentinel slot each)
    c["one_click_blocks"] = ([4] + [1] * 64 + [6] + [1] * 65 + [5] + [1] * 200 + [3], 50)
    # (c) users that end exactly on 64-slot / 512-slot boundaries
    c["len8_only"] = ([8] * 40, 50)
    c["len16_only"] = ([16] * 40, 50)
    # (d) a 10,000-slot user after a block of empty users
    c["len100_after_empty"] = ([0] * 150 + [100], 500)
    # (e) position gaps >= 64, both alphas, dt on both sides of the pow shortcut
    c["len70_ts_gaps"] = ([70, 70], 500)
    # (f) the same item at several positions
    c["repeated_items"] = ([12, 3, 30, 7, 1, 9], 4)
    # (g) a total that is not a multiple of 64
    c["odd_total"] = ([3, 5, 7], 10)
    return c


PAIR_CASES = _pair_cases()


@pytest.mark.parametrize("slot_base", [0, 12345])
@pytest.mark.parametrize("case", list(PAIR_CASES))
def test_pairs_vs_restated(case, slot_base):
    from nrk import ops

    lens, n_items = PAIR_CASES[case]
    rng = np.random.default_rng(len(lens) * 31 + n_items)
    offs, items, ts, created = _log(rng, lens, n_items)
    L = np.asarray(lens)
    total = int((L * L).sum())
    # the preconditions of each crafted log, from the host data
    if case == "empty_blocks":
        assert L[0] == 0 and L[-1] == 0 and _blocks(L == 0) == [70, 130, 200, 70]
    if case == "one_click_blocks":
        assert _blocks(L == 1) == [64, 65, 200]
    if case in ("len8_only", "len16_only"):
        assert total % 512 == 0 and (np.cumsum(L * L) % 64 == 0).all()
    if case == "len100_after_empty":
        assert total == 10_000 and _blocks(L == 0) == [150]
    if case == "len70_ts_gaps":
        dt = np.abs(ts[:70, None] - ts[None, :70])
        assert L.max() - 2 >= 64 and (dt == 0).any() and ((dt > 0) & (dt < 100)).any() and (dt > 5000).any()
    if case == "repeated_items":
        assert max(np.bincount(items[offs[u]:offs[u + 1]]).max() for u in range(len(lens)) if L[u]) >= 3
    if case == "odd_total":
        assert total % 64 != 0
    gk, gs, gw, gc = ops.itemcf_pairs(_d(offs), _d(items), _d(ts), _d(created), n_items, slot_base=slot_base)
    rk, rsl, rw, rc = rs.pairs_ref(offs, items, ts, created, n_items, slot_base=slot_base)
    assert gk.numel() == total
    assert np.array_equal(gk.cpu().numpy().view(np.uint64), rk)
    assert np.array_equal(gs.cpu().numpy(), rsl)
    assert np.array_equal(gc.cpu().numpy(), rc)
    gw = gw.cpu().numpy()
    sent = rk == np.uint64(rs.sentinel(n_items))
    assert sent.any() and (gw[sent] == 0.0).all() and not np.signbit(gw[sent]).any()
    np.testing.assert_allclose(gw[~sent], rw[~sent], rtol=RTOL, atol=0)


@pytest.mark.parametrize("case", list(PAIR_CASES))
def test_sim_on_crafted_logs_vs_oracle(case):
    """The same logs through nrk_itemcf_sim (its own launch of the pair walk) against the oracle."""
    from nrk import ops

    lens, n_items = PAIR_CASES[case]
    rng = np.random.default_rng(len(lens) * 31 + n_items)
    offs, items, ts, created = _log(rng, lens, n_items)
    sim = ops.itemcf_sim(_d(offs), _d(items), _d(ts), _d(created), n_items)
    oi, oj, ov, _, cnt = oracle.itemcf_sim(offs, items, ts, created, n_items)
    order = np.argsort(sim.first.cpu().numpy(), kind="stable")
    assert sim.i.numel() == len(oi)
    assert np.array_equal(sim.i.cpu().numpy()[order], oi) and np.array_equal(sim.j.cpu().numpy()[order], oj)
    np.testing.assert_allclose(sim.v.cpu().numpy()[order], ov, rtol=RTOL, atol=0)
    assert np.array_equal(sim.cnt.cpu().numpy(), cnt)


@pytest.mark.parametrize("chunks", [1, 2, 12])
def test_item_count_hash_wraps(chunks):
    """300 item ids that all hash to slot 8190 of the 8,192-slot LDS table:
    the probes wrap past its end.  Inside one 4,096-click chunk and across
    two the ids take cycling click counts (300 different counts do not fit
    8,192 clicks); over twelve chunks id k is clicked k + 1 times."""
    from nrk import ops

    n_items = 1 << 22
    ids = np.arange(n_items, dtype=np.uint64)
    ids = np.flatnonzero(((ids * np.uint64(2654435761)) % np.uint64(1 << 32)) >> np.uint64(19) == 8190)[:300]
    assert len(ids) == 300
    times = np.arange(300) % {1: 25, 2: 39, 12: 300}[chunks] + 1
    rng = np.random.default_rng(8190)
    items = rng.permutation(np.repeat(ids, times)).astype(np.int32)
    n = len(items)
    assert -(-n // 4096) == chunks
    if chunks == 2:  # ids with clicks in both chunks
        assert len(np.intersect1d(items[:4096], items[4096:])) > 100
    offs = np.arange(n + 1, dtype=np.int64)  # one click per user: one (sentinel) slot each
    ts = np.full(n, 1_500_000_000_000, np.int64)
    created = torch.zeros(n_items, dtype=torch.float64, device="cuda")
    _, _, _, gc = ops.itemcf_pairs(_d(offs), _d(items), _d(ts), created, n_items)
    assert np.array_equal(gc.cpu().numpy(), np.bincount(items, minlength=n_items))


SCAN_N = [0, 1, 1023, 1024, 8191, 8192, 8193, 16384, 16385, 3 * 8192 + 5]


@pytest.mark.parametrize("n", SCAN_N)
def test_pair_offsets_scan(n):
    from nrk import _lib, ops

    rng = np.random.default_rng(n)
    L = rng.integers(0, 300, n)
    offs = _d(np.concatenate([[0], np.cumsum(L)]).astype(np.int64))
    out = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    _lib.call("nrk_itemcf_pair_offsets", ops._ptr(offs), n, ops._ptr(out), ops._stream())
    assert np.array_equal(out.cpu().numpy(), np.concatenate([[0], np.cumsum(L * L)]))


@pytest.mark.parametrize("n", SCAN_N)
def test_recall_offsets_scan_in_place(n):
    """One-click histories: query q's candidate count is nbr_cnt[q], scanned
    in place (the counts and the offsets share one buffer)."""
    from nrk import _lib, ops

    rng = np.random.default_rng(n + 1)
    cnt = rng.integers(0, 2**31 - 1, n).astype(np.int32)  # totals far past 2^32
    q = _d(np.arange(n, dtype=np.int64))
    offs = _d(np.arange(n + 1, dtype=np.int64))
    items = _d(np.arange(n, dtype=np.int32))
    out = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    _lib.call("nrk_itemcf_recall_offsets", ops._ptr(q), n, ops._ptr(offs), ops._ptr(items), ops._ptr(_d(cnt)),
              ops._ptr(out), ops._stream())
    assert np.array_equal(out.cpu().numpy(), np.concatenate([[0], np.cumsum(cnt.astype(np.int64))]))


# ------------------------------------------------------ 4. recall rungs --
RUNG_C = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024]
RUNG_ITEMS, RUNG_TOPN, RUNG_POOL = 2000, 8, 40


def _rung(c):
    return 0 if c <= 64 else 1 if c <= 128 else 2 if c <= 256 else 3 if c <= 512 else 4


def _build_rung_case():
    """Neighbour tables built directly: rows [0, 1000) draw their neighbours
    from a 40-item pool (at most 40 distinct candidates), rows [1000, 2000)
    from the whole catalog; 40% of the rows have 8 neighbours, 25% none, the
    rest 1..7.  One history per (c, side, length): c // 8 rows of 8, one row
    of c % 8 and rows without neighbours up to the length, shuffled.  On the
    catalog side the draw is repeated until the candidates are all distinct
    (c <= 65) or more than 64 are (c > 65)."""
    rng = np.random.default_rng(4)
    n_items, topn = RUNG_ITEMS, RUNG_TOPN
    share = [0.25] + [0.05] * 7 + [0.40]
    nbr_cnt = np.zeros(n_items, np.int32)
    for lo in (0, 1000):
        nbr_cnt[lo:lo + 1000] = rng.permutation(np.repeat(np.arange(9), (np.array(share) * 1000).astype(int)))
    nbr_cols = np.full((n_items, topn), -1, np.int32)
    nbr_vals = np.zeros((n_items, topn))
    for i in range(n_items):
        pool = np.arange(RUNG_POOL) if i < 1000 else np.arange(n_items)
        nbr_cols[i, :nbr_cnt[i]] = rng.permutation(pool[pool != i])[:nbr_cnt[i]]
        nbr_vals[i, :nbr_cnt[i]] = rng.random(nbr_cnt[i]) + 0.05
    assert ((nbr_cols >= 0).sum(1) == nbr_cnt).all() and not (nbr_cols == np.arange(n_items)[:, None]).any()
    created = rng.random(n_items)
    hists, meta = [], []
    for c in RUNG_C:
        need = -(-c // 8)
        for side in (0, 1):
            rows = np.arange(1000) + 1000 * side
            for hl in sorted({max(need, 1), 64, 65, 130}):
                if hl < need:
                    continue
                for _ in range(500):
                    h = list(rng.permutation(rows[nbr_cnt[rows] == 8])[:c // 8])
                    if c % 8:
                        h.append(rng.permutation(rows[nbr_cnt[rows] == c % 8])[0])
                    cand = np.concatenate([nbr_cols[i, :nbr_cnt[i]] for i in h]) if c else np.zeros(0, np.int32)
                    fill = rows[nbr_cnt[rows] == 0]
                    if side == 1:  # the rows without neighbours are not among the candidates
                        fill = np.setdiff1d(fill, cand)
                    h += list(rng.permutation(fill)[:hl - len(h)])
                    h = rng.permutation(np.array(h, np.int32))
                    cand = np.concatenate([nbr_cols[i, :nbr_cnt[i]] for i in h]) if c else np.zeros(0, np.int32)
                    nd = len(np.setdiff1d(cand, h))
                    if side == 0 or (nd == c if c <= 65 else nd > 64):
                        break
                assert len(h) == hl and len(set(h.tolist())) == hl and int(nbr_cnt[h].sum()) == c == len(cand)
                hists.append(h)
                meta.append((c, nd, hl, int(np.isin(cand, h).sum())))  # (c, distinct, length, in-history candidates)
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    q = []
    for u in range(len(hists)):  # a cold query after every third user
        q.append(u)
        if u % 3 == 2:
            q.append(-1)
    return dict(nbr_cols=nbr_cols, nbr_vals=nbr_vals, nbr_cnt=nbr_cnt, created=created, offs=offs,
                items=np.concatenate(hists), q=np.array(q, np.int64), meta=meta,
                hot=rng.permutation(n_items)[:100].astype(np.int32))


@pytest.fixture(scope="module")
def rung_case():
    return _build_rung_case()


def test_recall_rung_preconditions(rung_case):
    """Which (candidate-count rung, distinct side of 64, distinct side of
    topk) combinations the crafted histories hit -- from the host data."""
    meta = rung_case["meta"]
    assert sorted(set(m[0] for m in meta)) == RUNG_C
    # every rung (c <= 64 / 128 / 256 / 512 / listed) with at most and with more than 64 distinct candidates
    hit = set((_rung(c), nd > 64) for c, nd, _, _ in meta)
    assert hit == {(0, False)} | {(r, s) for r in (1, 2, 3, 4) for s in (False, True)}
    for c in RUNG_C:  # and every c on both sides where c allows
        assert {nd > 64 for cc, nd, _, _ in meta if cc == c} == ({False, True} if c > 64 else {False})
    # history lengths around the 64-lane chunks (a listed query has at least 65 clicks: 513 = 64 * 8 + 1)
    assert {hl for _, _, hl, _ in meta} >= {1, 64, 65, 130}
    assert {_rung(c) for c, _, h, _ in meta if h == 64} == {0, 1, 2, 3}
    for hl in (65, 130):
        assert {_rung(c) for c, _, h, _ in meta if h == hl} == {0, 1, 2, 3, 4}
    assert any(inh > 0 for c, _, _, inh in meta if _rung(c) < 4)  # neighbours inside the history: dropped candidates
    # distinct candidates against topk: which rungs have a query with fewer than topk, and with at least topk
    below = {k: {_rung(c) for c, nd, _, _ in meta if nd < k} for k in (10, 64, 65)}
    reach = {k: {_rung(c) for c, nd, _, _ in meta if nd >= k} for k in (10, 64, 65)}
    every = {0, 1, 2, 3, 4}
    assert reach == {10: every, 64: every, 65: every - {0}}  # 64 candidates cannot give 65 distinct
    assert below[64] == every and below[65] == every
    assert below[10] == {0}  # the 40-item pool still leaves 10 or more once c > 64


@pytest.mark.parametrize("n_hot", [0, 100])
@pytest.mark.parametrize("topk", [10, 64, 65])
def test_recall_rungs_vs_oracle(rung_case, topk, n_hot):
    from nrk import ops

    g = rung_case
    hot = g["hot"][:n_hot]
    gi, gs, gsrc, gn = ops.itemcf_recall(_d(g["q"]), _d(g["offs"]), _d(g["items"]), _d(g["nbr_cols"]),
                                         _d(g["nbr_vals"]), _d(g["nbr_cnt"]), _d(g["created"]), _d(hot), topk)
    oi, os_, on = oracle.itemcf_recall(g["q"], g["offs"], g["items"], g["nbr_cols"], g["nbr_vals"], g["nbr_cnt"],
                                       g["created"], hot, topk, RUNG_ITEMS)
    gi, gs, gsrc, gn = (t.cpu().numpy() for t in (gi, gs, gsrc, gn))
    assert np.array_equal(gn, on)
    for r, u in enumerate(g["q"].tolist()):
        m = on[r]
        assert np.array_equal(gi[r, :m], oi[r, :m]), (r, g["meta"][u] if u >= 0 else "cold")
        np.testing.assert_allclose(gs[r, :m], os_[r, :m], rtol=RTOL, atol=0)
        assert (gsrc[r, :m] == 2).all() if u < 0 else (gsrc[r, :m] < 2).all()
        if u >= 0:  # the number of candidates kept, the rest hot fills
            nd = g["meta"][u][1]
            assert int((gsrc[r, :m] == 0).sum()) == min(nd, topk)


# ------------------------------------------------- 5. the wide paths' caps --
@pytest.mark.parametrize("topn", [128, 129, 1024, 1025, 2048])
def test_topn_wide_at_every_width(topn):
    """cf_topn_wide_kernel at K = 128, 256, 1024, 2048 (the LDS cap: 96 KB of
    dynamic LDS), rows around K and 2K, many exact ties."""
    from nrk import ops

    K = 64
    while K < topn:
        K <<= 1
    rng = np.random.default_rng(topn)
    lens = np.array([0, 1, K - 1, K, K + 1, 2 * K, 2 * K + 1, 5000])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    vals = np.round(rng.random(n) * 50) / 50
    cols = rng.integers(0, 10**6, n).astype(np.int32)
    first = np.arange(n, dtype=np.int64)
    gc, gv, gn = ops.itemcf_topn(_d(off), _d(cols), _d(vals), _d(first), topn)
    oc, ov, on = oracle.itemcf_topn(off, cols, vals, topn)
    assert np.array_equal(gn.cpu().numpy(), on) and on.tolist() == np.minimum(lens, topn).tolist()
    assert np.array_equal(gc.cpu().numpy(), oc)
    assert np.array_equal(gv.cpu().numpy(), ov)


def test_topn_above_the_cap_is_refused():
    from nrk import _lib, ops

    off, e = _d(np.array([0, 0], np.int64)), torch.empty(0, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.itemcf_topn(off, e, e.double(), e.long(), 2049)
    oc = torch.empty((1, 2049), dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):  # the C entry point itself, before any launch
        _lib.call("nrk_itemcf_topn", ops._ptr(off), 1, None, None, None, 2049, ops._ptr(oc), ops._ptr(oc.double()),
                  ops._ptr(oc), ops._stream())


def _sim_recall_case(rng, n_users, n_items, max_len, topn, n_hot):
    from nrk import ops

    offs, items, ts, created = rs.random_lists(rng, n_users, n_items, max_len)
    sim = ops.itemcf_sim(_d(offs), _d(items), _d(ts), _d(created), n_items)
    nc, nv, nn = ops.itemcf_topn(sim.row_offsets(), sim.j, sim.v, sim.first, topn)
    hot = rng.permutation(n_items)[:n_hot].astype(np.int32)
    return offs, items, created, nc, nv, nn, hot


@pytest.fixture(scope="module", params=[(60, 5000, 250, 64, 300), (50, 60, 8, 20, 30)], ids=["many_cands", "hot_runs_out"])
def wide_recall_case(request):
    n_users, n_items, max_len, topn, n_hot = request.param
    rng = np.random.default_rng(n_users * 7 + n_hot)
    offs, items, created, nc, nv, nn, hot = _sim_recall_case(rng, n_users, n_items, max_len, topn, n_hot)
    nc_h, nn_h = nc.cpu().numpy(), nn.cpu().numpy()
    nd = []
    for u in range(n_users):
        h = items[offs[u]:offs[u + 1]]
        cand = np.concatenate([nc_h[i, :nn_h[i]] for i in h]) if len(h) else np.zeros(0, np.int32)
        nd.append(len(np.setdiff1d(cand, h)))
    return request.param, offs, items, created, nc, nv, nn, hot, np.array(nd)


@pytest.mark.parametrize("topk", [1024, 2048])
def test_recall_wide_at_the_cap(wide_recall_case, topk):
    """rc_topk_wide_kernel at K = 1024 and 2048 (96 KB of dynamic LDS):
    queries with more than 2,048 distinct candidates, and a catalog so small
    that the hot list runs out."""
    from nrk import ops

    (n_users, n_items, _, _, n_hot), offs, items, created, nc, nv, nn, hot, nd = wide_recall_case
    if n_items == 5000:
        assert (nd > 2048).any() and (nd < 1024).any()
    q = np.concatenate([np.arange(n_users), [-1, -1]]).astype(np.int64)
    gi, gs, gsrc, gn = ops.itemcf_recall(_d(q), _d(offs), _d(items), nc, nv, nn, _d(created), _d(hot), topk)
    oi, os_, on = oracle.itemcf_recall(q, offs, items, nc.cpu().numpy(), nv.cpu().numpy(), nn.cpu().numpy(),
                                       created, hot, topk, n_items)
    gi, gs, gsrc, gn = (t.cpu().numpy() for t in (gi, gs, gsrc, gn))
    assert np.array_equal(gn, on)
    if n_items == 60:
        assert (on[:n_users] < topk).all() and (on[-2:] == n_hot).all()  # the hot list ran out
        assert any((gsrc[r, :on[r]] == 1).any() for r in range(n_users))
    for r in range(len(q)):
        m = on[r]
        assert np.array_equal(gi[r, :m], oi[r, :m]), r
        np.testing.assert_allclose(gs[r, :m], os_[r, :m], rtol=RTOL, atol=0)
        assert (gsrc[r, :m] == 2).all() if q[r] < 0 else (gsrc[r, :m] < 2).all()
        assert (gi[r, m:] == -1).all()


def test_recall_above_the_cap_is_refused(wide_recall_case):
    from nrk import ops

    (n_users, *_), offs, items, created, nc, nv, nn, hot, _ = wide_recall_case
    with pytest.raises(NotImplementedError):
        ops.itemcf_recall(_d(np.arange(n_users, dtype=np.int64)), _d(offs), _d(items), nc, nv, nn, _d(created),
                          _d(hot), 2049)
