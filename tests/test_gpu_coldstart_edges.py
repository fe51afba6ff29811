"""nrk_coldstart_filter / nrk_coldstart_recall against the numpy restatement
(coldstart_restated.py) on hand-built arrays, at the smallest shapes where the
kernels can go wrong: list lengths around the 64-entry chunk and the 2,048
survivor cap, keep patterns, survivor counts around topk, score ties, the two
thresholds to the last bit, category sets around the chunk size, and the -1
rows."""
import numpy as np
import pytest
import torch

from nrk import _lib, ops

import coldstart_restated as rs

pytestmark = pytest.mark.gpu

# item rows of the default tables: 0 passes every rule of profile 0; 1 has the
# wrong category, 2 is clicked, 3 is 201 words off, 4 is 0.26 away in time
KEEP, DROPS = 0, (1, 2, 3, 4, -1)
TABLES = dict(cat_off=[0, 1], cat=[7], mean_words=[500.0], last_created=[0.5], item_type=[7, 8, 7, 7, 7],
              item_words=[500.0, 500.0, 500.0, 701.0, 500.0], item_created=[0.5, 0.5, 0.5, 0.5, 0.76],
              item_clicked=[0, 0, 1, 0, 0])
DTYPES = dict(cat_off=np.int64, cat=np.int32, mean_words=np.float64, last_created=np.float64, item_type=np.int32,
              item_words=np.float64, item_created=np.float64, item_clicked=np.uint8)


def _tables(**over):
    return tuple(np.asarray(over.get(k, TABLES[k]), dt) for k, dt in DTYPES.items())


def _items(mask, rng):
    """Item rows for a keep pattern: row 0 where kept, some failing row elsewhere."""
    mask = np.asarray(mask, bool)
    return np.where(mask, KEEP, rng.choice(DROPS, size=len(mask))).astype(np.int32)


def _run(lists, scores, topk, prof=None, q=None, tables=None, want_keep=None):
    """Both kernels over ``lists`` (item rows per list) against the
    restatement.  Queries whose survivors pass 2,048 must raise; the others are
    compared list by list.  Returns the restated kept counts."""
    tables = _tables() if tables is None else tables
    list_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    item = np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)])
    score = np.concatenate([np.asarray(x, np.float64) for x in scores] + [np.zeros(0)])
    prof = np.zeros(len(lists), np.int32) if prof is None else np.asarray(prof, np.int32)
    q = np.arange(len(lists), dtype=np.int64) if q is None else np.asarray(q, np.int64)
    args = (list_off, item, prof) + tables
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = [d(a) for a in args]
    keep, kept = rs.keep_mask(*args)
    if want_keep is not None:
        assert keep.tolist() == list(want_keep)
    keep_d, kept_d = ops.coldstart_filter(*dev)
    assert np.array_equal(keep_d.cpu().numpy(), keep)
    assert np.array_equal(kept_d.cpu().numpy(), kept)
    over = np.array([l >= 0 and kept[l] > ops.CS_MAX for l in q.tolist()], bool)
    if over.any():
        with pytest.raises(NotImplementedError):
            ops.coldstart_recall(d(q[over][:1]), dev[0], dev[1], d(score), *dev[2:], topk)
        # the entry point itself: out_cnt = -1 and padded rows for those users, the others as usual
        nq = len(q)
        o = (torch.empty((nq, topk), dtype=torch.int32, device="cuda"),
             torch.empty((nq, topk), dtype=torch.float64, device="cuda"),
             torch.empty(nq, dtype=torch.int32, device="cuda"))
        p, dq, ds = ops._ptr, d(q), d(score)
        _lib.call("nrk_coldstart_recall", p(dq), nq, p(dev[0]), len(lists), p(dev[1]), p(ds), len(item),
                  p(dev[2]), p(dev[3]), p(dev[4]), len(tables[1]), p(dev[5]), p(dev[6]), len(tables[2]), p(dev[7]),
                  p(dev[8]), p(dev[9]), p(dev[10]), len(tables[4]), 200.0, 0.25, ops.CS_MAX, topk, p(o[0]), p(o[1]),
                  p(o[2]), ops._stream())
        raw_pos, raw_sc, raw_cnt = (x.cpu().numpy() for x in o)
        assert (raw_cnt[over] == -1).all() and (raw_pos[over] == -1).all() and (raw_sc[over] == 0.0).all()
        assert (raw_cnt[~over] >= 0).all()
    q = q[~over]
    pos, sc, cnt = ops.coldstart_recall(d(q), dev[0], dev[1], d(score), *dev[2:], topk)
    assert pos.shape == (len(q), topk) and sc.shape == (len(q), topk) and cnt.shape == (len(q),)
    rs.check_recall(rs.recall(q, list_off, score, keep, topk), pos.cpu().numpy(), sc.cpu().numpy(),
                    cnt.cpu().numpy(), topk)
    return kept


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 5000])
def test_list_lengths_and_keep_patterns(n):
    rng = np.random.default_rng(n)
    i = np.arange(n)
    masks = [np.ones(n, bool), np.zeros(n, bool), i == 0, i == n - 1, i % 2 == 0, (i == 63) | (i == 64),
             rng.random(n) < 0.3]
    lists = [_items(m, rng) for m in masks]
    scores = [np.round(rng.random(n) * 2, 1) for _ in masks]  # 21 values: ties in every longer list
    kept = _run(lists, scores, 30)
    assert kept.tolist() == [int(m.sum()) for m in masks]
    if n == 5000:  # all kept and alternating pass the cap (refused), the random third does not
        assert kept[0] > kept[4] > ops.CS_MAX > kept[6] > 1000
    _run(lists[::-1], scores[::-1], 1)


@pytest.mark.parametrize("topk", [1, 5, 64, 65, 256, 2048])
def test_survivor_counts_around_topk(topk):
    rng = np.random.default_rng(topk)
    lists, scores = [], []
    for c in (topk - 1, topk, topk + 1):
        n = c + int(rng.integers(0, 70))
        mask = np.zeros(n, bool)
        mask[rng.permutation(n)[:c]] = True
        lists.append(_items(mask, rng))
        scores.append(np.round(rng.standard_normal(n), 1))
    kept = _run(lists, scores, topk)
    assert kept.tolist() == [topk - 1, topk, topk + 1]


def test_ties_fall_to_position():
    rng = np.random.default_rng(3)
    n = 300
    lists = [_items(rng.random(n) < 0.8, rng) for _ in range(5)]
    scores = [np.full(n, 0.25),                                               # all equal
              rng.choice([0.1, 0.2, 0.3, 0.4], n),                            # four distinct values
              rng.choice([-0.0, 0.0], n),                                     # the two zeros are one tie
              rng.choice([-0.0, 0.0, -1.5, 2.0], n),
              rng.choice([-np.inf, np.inf, -3.0, -0.5, 0.0, 1e300, -1e-300], n)]  # negative and infinite
    for topk in (7, 64, 300):
        _run(lists, scores, topk)
    # the zeros spelled out: both kept, the first position first, its own sign of zero returned
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    t = [d(a) for a in (np.array([0, 3], np.int64), np.zeros(3, np.int32), np.zeros(1, np.int32)) + _tables()]
    pos, sc, cnt = ops.coldstart_recall(d(np.zeros(1, np.int64)), t[0], t[1], d(np.array([-0.0, 0.0, -0.0])),
                                        *t[2:], 3)
    assert pos.cpu().tolist() == [[0, 1, 2]] and cnt.item() == 3
    assert np.signbit(sc.cpu().numpy()).tolist() == [[True, False, True]]


def test_thresholds_to_the_last_bit():
    up, down = np.inf, -np.inf
    words = [700.0, np.nextafter(700.0, up), 300.0, np.nextafter(300.0, down), 500.0, 500.0, 500.0, 500.0]
    # 0.5 - nextafter(0.25, down) rounds back to 0.25, so the lower side steps two ulps of 0.25 down
    created = [0.5, 0.5, 0.5, 0.5, 0.75, np.nextafter(0.75, up), 0.25, 0.25 - 2.0**-53]
    n = len(words)
    tables = _tables(cat_off=[0, 1, 2, 3, 4], cat=[7, 7, 7, 7], mean_words=[500.0, np.nan, 500.0, np.nan],
                     last_created=[0.5, 0.5, np.nan, np.nan], item_type=[7] * n, item_words=words,
                     item_created=created, item_clicked=[0] * n)
    lists = [np.arange(n)] * 4
    scores = [np.arange(n) * 0.5] * 4
    # |delta| exactly at the tolerance is kept, one ulp past it dropped; a NaN mean or time keeps the pair
    want = ([1, 0, 1, 0, 1, 0, 1, 0] + [1, 1, 1, 1, 1, 0, 1, 0] + [1, 0, 1, 0, 1, 1, 1, 1] + [1] * 8)
    _run(lists, scores, 8, prof=[0, 1, 2, 3], tables=tables, want_keep=want)
    # word counts just under 2^53, where consecutive integers are still distinct doubles
    big = float(2**53)
    tables = _tables(cat_off=[0, 1, 2], cat=[7, 7], mean_words=[big - 201.0, big - 202.0], last_created=[0.5, 0.5],
                     item_type=[7, 7], item_words=[big - 1.0, big - 401.0], item_created=[0.5, 0.5],
                     item_clicked=[0, 0])
    _run([[0, 1]] * 2, [[1.0, 2.0]] * 2, 2, prof=[0, 1], tables=tables, want_keep=[1, 1, 0, 1])


def test_category_sets_of_every_size():
    """A user with n categories = the even codes below 2n; item row t has
    category t: the matching code is first, last, inside, or absent (odd, or
    past the end)."""
    sizes = [0, 1, 63, 64, 65, 300]
    n_items = 2 * max(sizes) + 2
    cats = [np.arange(0, 2 * n, 2) for n in sizes]
    tables = _tables(cat_off=np.concatenate([[0], np.cumsum(sizes)]), cat=np.concatenate(cats),
                     mean_words=[500.0] * len(sizes), last_created=[0.5] * len(sizes), item_type=np.arange(n_items),
                     item_words=[500.0] * n_items, item_created=[0.5] * n_items, item_clicked=[0] * n_items)
    rng = np.random.default_rng(11)
    lists = [np.arange(n_items)] * len(sizes)
    scores = [np.round(rng.random(n_items), 2) for _ in sizes]
    kept = _run(lists, scores, 300, prof=np.arange(len(sizes)), tables=tables)
    assert kept.tolist() == sizes
    want = np.concatenate([(np.arange(n_items) % 2 == 0) & (np.arange(n_items) < 2 * n) for n in sizes])
    _run(lists, scores, 1, prof=np.arange(len(sizes)), tables=tables, want_keep=want.astype(int).tolist())


def test_missing_rows_and_queries():
    rng = np.random.default_rng(13)
    lists = [np.zeros(70, np.int32), np.zeros(70, np.int32), np.full(70, -1, np.int32),
             np.where(np.arange(70) % 3 == 0, -1, 0).astype(np.int32)]
    scores = [rng.random(70) for _ in lists]
    # list 1 has no profile; list 2 only missing items; -1 and repeated queries
    kept = _run(lists, scores, 10, prof=[0, -1, 0, 0], q=[3, -1, 0, 0, 1, 2, -1, 3])
    assert kept.tolist() == [70, 0, 0, 46]
    _run(lists, scores, 10, prof=[-1] * 4, q=[-1, -1])
    _run(lists, scores, 10, prof=[0, -1, 0, 0], q=[])  # Q = 0
    _run([], [], 5)  # no list at all
    _run([[], []], [[], []], 5, q=[1, 0, -1])  # only empty lists
