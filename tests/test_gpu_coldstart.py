"""ColdStartRecaller on the GPU (csrc/coldstart.hip) against the
reference-executed fixture: filtered_results, every recall list, the
statistics and the error cases; then ip_topk's [U, K] rows fed straight into
ops.coldstart_recall against the numpy restatement (coldstart_restated.py,
pinned to the fixture by test_coldstart_host.py)."""
import numpy as np
import pytest
import torch

from nrk import ops
from nrk.config import RecallConfig
from nrk.recall import ColdStartRecaller

import coldstart_restated as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden("coldstart_small")


@pytest.fixture(scope="module")
def rec(fx):
    return ColdStartRecaller(RecallConfig(), *rs.recaller_args(fx))


def _same(got, want):
    """Equal tuples, and an int score still an int."""
    assert got == want
    assert [type(s) for _, s in got] == [type(s) for _, s in want]


def test_filtered_results_equal_the_reference(fx, rec):
    want = rs.lists_of(fx, "filtered", rs.as_score)
    assert list(rec.filtered_results) == list(want)  # the same users, in the base dict's order
    for u, lst in want.items():
        _same(rec.filtered_results[u], lst)
    assert any(isinstance(s, int) for lst in rec.filtered_results.values() for _, s in lst)


@pytest.mark.parametrize("topk", [1, 5, 30])
def test_recall_equals_the_reference(fx, rec, topk):
    want = rs.lists_of(fx, f"recall{topk}", rs.as_score)
    queries = fx["queries"].tolist()
    batch = rec.batch_recall(queries, topk=topk)
    assert list(batch) == queries
    for u in queries:
        _same(batch[u], want[u])
    for u in queries[:40] + queries[-2:]:  # one call per user; the last two are unknown
        _same(rec.recall(u, topk=topk), want[u])
    assert batch[queries[-1]] == [] and batch[queries[-2]] == []
    assert rec.batch_recall([], topk=topk) == {}


def test_statistics_equal_the_reference(fx, rec):
    got = rec.get_statistics()
    assert list(got) == fx["stats_keys"].tolist()
    assert [float(v) for v in got.values()] == fx["stats_values"].tolist()


def test_constructor_errors(fx):
    args = list(rs.recaller_args(fx))
    u = next(iter(args[1]))
    words = dict(args[2])
    del words[u]
    with pytest.raises(KeyError):  # in the types dict, not in the words dict (coldstart_recaller.py:81)
        ColdStartRecaller(RecallConfig(), args[0], args[1], words, *args[3:])
    last = dict(args[3])
    del last[u]
    with pytest.raises(KeyError):
        ColdStartRecaller(RecallConfig(), *args[:3], last, *args[4:])
    base = dict(args[0])
    v = next(k for k, lst in base.items() if lst)
    base[v] = [(base[v][0][0], float("nan"))] + base[v][1:]
    with pytest.raises(ValueError):
        ColdStartRecaller(RecallConfig(), base, *args[1:])


def test_ops_refuse_bad_inputs(rec):
    t, sc = rec._tables, rec._score
    q = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.coldstart_recall(q, t[0], t[1], torch.full_like(sc, float("nan")), *t[2:], 5)
    with pytest.raises(ValueError):
        ops.coldstart_recall(q + len(t[2]), t[0], t[1], sc, *t[2:], 5)  # q past the lists
    with pytest.raises(NotImplementedError):
        ops.coldstart_recall(q, t[0], t[1], sc, *t[2:], 2049)
    with pytest.raises(ValueError):
        ops.coldstart_filter(t[0], t[1] + len(t[7]), *t[2:])  # item row past the tables
    with pytest.raises(ValueError):
        ops.coldstart_filter(t[0], t[1], t[2] + len(t[5]), *t[3:])  # profile row past the tables
    with pytest.raises(ValueError):
        ops.coldstart_filter(*t[:4], torch.flip(t[4], [0]), *t[5:])  # categories not ascending
    with pytest.raises(ValueError):
        ops.coldstart_filter(t[0] + 1, *t[1:])  # offsets not from 0
    with pytest.raises(ValueError):
        ops.coldstart_filter(*t[:5], t[5].float(), *t[6:])  # dtype


def test_ip_topk_rows_feed_coldstart_recall():
    """300 users over 4,000 items: the [U, 128] rows and fp32 scores of
    ops.ip_topk go into ops.coldstart_recall as they are (list_off = arange *
    K; no list is built on the host)."""
    rng = np.random.default_rng(5)
    U, I, D, K, topk = 300, 4000, 32, 128, 3
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    users = d((rng.standard_normal((U, D)) * 0.1).astype(np.float32))
    cat = ops.Catalog(d((rng.standard_normal((I, D)) * 0.1).astype(np.float32)))
    s, r = ops.ip_topk(users, cat, K)
    n_cat = 12
    sets = [np.sort(rng.choice(n_cat, size=rng.integers(0, 7), replace=False)) for _ in range(U)]
    cat_off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.int64)
    tables = (np.arange(U + 1, dtype=np.int64) * K, None, np.arange(U, dtype=np.int32), cat_off,
              np.concatenate(sets).astype(np.int32), rng.integers(100, 900, U).astype(np.float64), rng.random(U),
              rng.integers(0, n_cat, I).astype(np.int32), rng.integers(100, 900, I).astype(np.float64),
              rng.random(I), (rng.random(I) < 0.5).astype(np.uint8))
    dev = [d(a) if a is not None else r for a in tables]
    q = d(np.arange(U, dtype=np.int64))
    pos, sc, cnt = ops.coldstart_recall(q, dev[0], r, s, *dev[2:], topk)
    keep_d, kept_d = ops.coldstart_filter(dev[0], r, *dev[2:])
    rows, s64 = r.cpu().numpy(), s.cpu().numpy().astype(np.float64)
    keep, kept = rs.keep_mask(tables[0], rows, *tables[2:])
    assert (kept > topk).any() and (kept == topk).any() and (kept < topk).any() and (kept == 0).any()
    assert np.array_equal(keep_d.cpu().numpy(), keep) and np.array_equal(kept_d.cpu().numpy(), kept)
    rs.check_recall(rs.recall(np.arange(U), tables[0], s64, keep, topk), pos.cpu(), sc.cpu(), cnt.cpu(), topk)
