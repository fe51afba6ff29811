"""Cold-start and ensemble checks that need no GPU: the numpy restatement (the
checker of the GPU tests) over the plugin's own dense arrays equals
reference-executed data, the two host extractors equal the reference's dicts,
the ensemble restatement equals the reference's RecallEnsemble, and the new C
entry points refuse bad arguments before touching a pointer."""
import numpy as np
import pytest

from nrk import _lib
from nrk.data import extractors
from nrk.recall.coldstart_recaller import dense_inputs

import coldstart_restated as rs


@pytest.fixture(scope="module")
def fx(golden):
    return golden("coldstart_small")


@pytest.fixture(scope="module")
def dense(fx):
    args = rs.recaller_args(fx)
    users, score, tables = dense_inputs(*args)
    keep, kept = rs.keep_mask(*tables)
    return args[0], users, score, tables, keep, kept


def test_fixture_cannot_hide_a_failure(fx):
    """The conditions the generator asserts, visible from the stored data."""
    base, filt = rs.lists_of(fx, "base", rs.as_score), rs.lists_of(fx, "filtered", rs.as_score)
    assert sum(1 for u in base if u not in filt) >= 20
    assert sum(1 for lst in filt.values() if len(lst) > 5) >= 20
    assert sum(1 for lst in filt.values() if len({s for _, s in lst}) < len(lst)) >= 10
    known = set(fx["item_ids"].tolist())
    assert sum(1 for lst in base.values() for i, _ in lst if i not in known) >= 20
    assert any(isinstance(s, int) for lst in filt.values() for _, s in lst)
    assert len(set(base) - set(fx["prof_users"].tolist())) == 2


def test_restated_filter_equals_the_reference(fx, dense):
    base, users, _, tables, keep, kept = dense
    want = rs.lists_of(fx, "filtered", rs.as_score)
    off = tables[0]
    got = {}
    for n, u in enumerate(users):
        lst = [base[u][p] for p in np.flatnonzero(keep[off[n]:off[n + 1]]).tolist()]
        assert len(lst) == kept[n]
        if lst:
            got[u] = lst
    assert list(got) == list(want)  # the same users in the same order
    assert got == want
    stats = dict(zip(fx["stats_keys"].tolist(), fx["stats_values"].tolist()))
    assert stats["cold_start_users"] == len(got) and stats["total_items_after_filtering"] == int(kept.sum())
    assert stats["total_items_before_filtering"] == len(keep) and stats["total_users"] == len(users)


@pytest.mark.parametrize("topk", [1, 5, 30])
def test_restated_recall_equals_the_reference(fx, dense, topk):
    base, users, score, tables, keep, _ = dense
    assert topk in fx["topks"].tolist()
    want = rs.lists_of(fx, f"recall{topk}", rs.as_score)
    queries = fx["queries"].tolist()
    assert list(want) == queries
    row = {u: n for n, u in enumerate(users)}
    q = [row.get(u, -1) for u in queries]
    assert q.count(-1) == 2
    for u, (pos, sc) in zip(queries, rs.recall(q, tables[0], score, keep, topk)):
        assert [base[u][p] for p in pos] == want[u], u
        assert sc == [float(s) for _, s in want[u]], u


def test_dense_inputs_contract(dense):
    _, users, score, t, _, _ = dense
    list_off, item, prof, cat_off, cat, mean_words, last_created, item_type, words, created, clicked = t
    assert list_off[-1] == len(item) == len(score) and len(prof) == len(users)
    assert item.dtype == np.int32 and prof.dtype == np.int32 and cat.dtype == np.int32 and clicked.dtype == np.uint8
    assert item.min() == -1 and (prof == -1).sum() == 2 and cat_off[-1] == len(cat)
    for p in range(len(cat_off) - 1):
        assert (np.diff(cat[cat_off[p]:cat_off[p + 1]]) > 0).all()
    for a in (mean_words, last_created, words, created, score):
        assert a.dtype == np.float64
    with pytest.raises(ValueError):
        dense_inputs({1: [(2, 2**53)]}, {}, {}, {}, {2: 0}, {2: 10}, {2: 0.5}, set())
    with pytest.raises(ValueError):
        dense_inputs({1: [(2, 0.5)]}, {}, {}, {}, {2: 0}, {2: 2**53}, {2: 0.5}, set())
    with pytest.raises(ValueError):
        dense_inputs({1: [(2, float("nan"))]}, {}, {}, {}, {2: 0}, {2: 10}, {2: 0.5}, set())
    with pytest.raises(KeyError):  # a profile without a mean word count (coldstart_recaller.py:81)
        dense_inputs({1: [(2, 0.5)]}, {1: {0}}, {}, {1: 0.5}, {2: 0}, {2: 10}, {2: 0.5}, set())
    # Python's == across types: category 3.0 of the user matches the item's 3; ids of any hashable type
    a, b = ("a", 1), ("b", 2)
    _, _, t2 = dense_inputs({"u": [(a, 1), (b, 2.5)]}, {"u": {3.0}}, {"u": 10.0}, {"u": 0.5},
                            {a: 3, b: 4}, {a: 10, b: 10}, {a: 0.5, b: 0.5}, {b})
    assert t2[1].tolist() == [0, 1] and t2[7][0] == t2[4][0] != t2[7][1] and t2[10].tolist() == [0, 1]
    assert rs.keep_mask(*t2)[0].tolist() == [1, 0]


def _frames(fx):
    import pandas as pd

    merged = pd.DataFrame({"user_id": fx["click_user"], "click_article_id": fx["click_item"],
                           "click_timestamp": fx["click_ts"], "category_id": fx["click_category"],
                           "words_count": fx["click_words"], "created_at_ts": fx["click_created"]})
    arts = pd.DataFrame({"click_article_id": fx["art_id"], "category_id": fx["art_category"],
                         "words_count": fx["art_words"], "created_at_ts": fx["art_created"]})
    return merged, arts


def test_user_hist_item_info_equals_the_reference(fx):
    merged, _ = _frames(fx)
    types, ids, words, last = extractors.user_hist_item_info(merged)
    assert types == rs.sets_of(fx, "types") and list(types) == fx["types_users"].tolist()
    assert ids == rs.sets_of(fx, "hist") and list(ids) == fx["hist_users"].tolist()
    assert list(words) == fx["words_users"].tolist() and list(last) == fx["last_users"].tolist()
    assert np.array(list(words.values()), np.float64).tobytes() == fx["words_values"].tobytes()
    assert np.array(list(last.values()), np.float64).tobytes() == fx["last_values"].tobytes()


def test_item_info_equals_the_reference(fx):
    _, arts = _frames(fx)
    item_type, item_words, item_created = extractors.item_info(arts)
    ids = fx["item_ids"].tolist()
    assert list(item_type) == ids and list(item_words) == ids and list(item_created) == ids
    assert list(item_type.values()) == fx["item_type"].tolist()
    assert list(item_words.values()) == fx["item_words"].tolist()
    assert np.array(list(item_created.values()), np.float64).tobytes() == fx["item_created"].tobytes()


@pytest.mark.parametrize("strategy", ["weighted_avg", "weighted_sum", "max_score"])
def test_restated_ensemble_equals_the_reference(fx, strategy):
    chans = [rs.lists_of(fx, "base", rs.as_score), rs.lists_of(fx, "stub_a"), rs.lists_of(fx, "stub_b")]
    bad = set(fx["ens_bad_b"].tolist())
    assert bad and bad <= set(chans[2])
    want = rs.lists_of(fx, "ens_" + strategy)
    topk, weights = int(fx["ens_topk"]), fx["ens_weights"].tolist()
    for u in fx["queries"].tolist():
        lists = [c.get(u, [])[:2 * topk] for c in chans]
        keep = [n for n in range(3) if not (n == 2 and u in bad)]
        got = rs.ensemble([lists[n] for n in keep], [weights[n] for n in keep], strategy, topk)
        assert [i for i, _ in got] == [i for i, _ in want[u]], u
        assert np.array([s for _, s in got]).tobytes() == np.array([s for _, s in want[u]]).tobytes(), u


def test_argument_errors():
    L = _lib.lib()
    err = lambda: L.nrk_last_error()  # noqa: E731

    def filt(n_lists=4, n_entries=10, n_cat=3, n_prof=2, n_items=5):
        return L.nrk_coldstart_filter(None, n_lists, None, n_entries, None, None, None, n_cat, None, None, n_prof,
                                      None, None, None, None, n_items, 200.0, 0.25, None, None, None)

    def rec(topk=30, cap=150, n_query=3, n_lists=4, n_entries=10, n_cat=3, n_prof=2, n_items=5):
        return L.nrk_coldstart_recall(None, n_query, None, n_lists, None, None, n_entries, None, None, None, n_cat,
                                      None, None, n_prof, None, None, None, None, n_items, 200.0, 0.25, cap, topk,
                                      None, None, None, None)

    assert filt() == _lib.NRK_EINVAL and b"nrk_coldstart_filter: null pointer" in err()
    for kw in ("n_lists", "n_entries", "n_cat", "n_prof", "n_items"):
        assert filt(**{kw: -1}) == _lib.NRK_EINVAL and b"negative size" in err(), kw
        assert rec(**{kw: -1}) == _lib.NRK_EINVAL and b"negative size" in err(), kw
    assert filt(n_entries=2**31) == _lib.NRK_EINVAL and b"2^31" in err()
    assert rec() == _lib.NRK_EINVAL and b"nrk_coldstart_recall: null pointer" in err()
    assert rec(n_query=-1) == _lib.NRK_EINVAL and b"negative size" in err()
    for topk in (0, -1, 2049):
        assert rec(topk=topk) == _lib.NRK_EINVAL and b"topk must be in [1, 2048]" in err()
    for cap in (0, 2049):
        assert rec(cap=cap) == _lib.NRK_EINVAL and b"cap must be in [1, 2048]" in err()
    with pytest.raises(ValueError):
        _lib.check(rec(topk=0), "nrk_coldstart_recall")
    assert L.nrk_abi_version() == 3
