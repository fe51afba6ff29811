"""RecallEnsemble on the GPU (nrk_fuse / nrk_fuse_wide) against the
reference-executed fixture -- lists and scores bit for bit for its three
strategies, a recaller that fails for some users, users without any list --
and an ensemble of the real ColdStartRecaller and ItemCFRecaller against the
host restatement of the merge (coldstart_restated.ensemble, pinned to the
fixture by test_coldstart_host.py) over those recallers' own lists."""
import numpy as np
import pandas as pd
import pytest

from nrk.config import RecallConfig
from nrk.data import extractors
from nrk.recall import ColdStartRecaller, ItemCFRecaller, RecallEnsemble
from nrk.similarity.item_cf import ItemCFSimilarity

import coldstart_restated as rs

pytestmark = pytest.mark.gpu

STRATEGIES = ["weighted_avg", "weighted_sum", "max_score"]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("coldstart_small")


class Stub:
    """A recaller over stored lists without a batch call; raises for the users of ``bad``."""

    def __init__(self, lists, bad=()):
        self.lists, self.bad, self.calls = lists, set(bad), 0

    def recall(self, user_id, topk=10):
        self.calls += 1
        if user_id in self.bad:
            raise RuntimeError("stub failure")
        return self.lists.get(user_id, [])[:topk]


class BatchStub(Stub):
    """The same with a batch call, which fails as a whole when one of its users does."""

    def batch_recall(self, user_ids, topk=10):
        return {u: self.recall(u, topk) for u in user_ids}


def _same(got, want):
    assert [i for i, _ in got] == [i for i, _ in want]
    assert np.array([s for _, s in got], np.float64).tobytes() == np.array([s for _, s in want]).tobytes()
    assert all(type(s) is float for _, s in got)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("stub", [Stub, BatchStub])
def test_ensemble_equals_the_reference(fx, strategy, stub):
    chans = [stub(rs.lists_of(fx, "base", rs.as_score)), stub(rs.lists_of(fx, "stub_a")),
             stub(rs.lists_of(fx, "stub_b"), fx["ens_bad_b"].tolist())]
    ens = RecallEnsemble(RecallConfig(), fusion_strategy=strategy)
    for name, c, w in zip(("base", "a", "b"), chans, fx["ens_weights"].tolist()):
        ens.add_recaller(name, c, w)
    want = rs.lists_of(fx, "ens_" + strategy)
    queries, topk = fx["queries"].tolist(), int(fx["ens_topk"])
    got = ens.batch_recall(queries, topk=topk)
    assert list(got) == queries
    for u in queries:
        _same(got[u], want[u])
    # the failing recaller is swallowed user by user: its other users still count
    bad = set(fx["ens_bad_b"].tolist())
    assert any(u not in bad and chans[2].lists.get(u) for u in queries)
    assert sum(1 for u in queries if got[u] == []) >= 2  # users whose every list is empty
    for u in queries[:25] + queries[-2:]:
        _same(ens.recall(u, topk=topk), want[u])


def test_ensemble_edges():
    lists = {1: [(10, 0.5), (11, 0.25)], 2: []}
    with pytest.raises(ValueError):
        RecallEnsemble(RecallConfig(), fusion_strategy="rrf")
    ens = RecallEnsemble(RecallConfig())
    assert ens.batch_recall([1, 2], topk=5) == {1: [], 2: []}  # no recaller at all
    ens.add_recaller("a", Stub(lists), 1.0)
    ens.add_recaller("b", Stub(lists), -1.0)
    with pytest.raises(ZeroDivisionError):  # weighted_avg over a zero weight sum (fusion.py:526-529)
        ens.recall(1, topk=5)
    assert ens.recall(2, topk=5) == [] and ens.recall(99, topk=5) == []
    assert ens.batch_recall([], topk=5) == {}
    ws = RecallEnsemble(RecallConfig(), fusion_strategy="weighted_sum")
    ws.add_recaller("a", Stub(lists), 1.0)
    ws.add_recaller("b", Stub(lists), -1.0)
    assert ws.recall(1, topk=5) == [(10, 0.0), (11, 0.0)]
    # more than 256 entries for one user take nrk_fuse_wide; more than 2,048 are refused
    wide = {1: [(i, float(i % 7)) for i in range(300)]}
    ens = RecallEnsemble(RecallConfig(), fusion_strategy="max_score")
    ens.add_recaller("w", Stub(wide), 2.0)
    _same(ens.recall(1, topk=150), rs.ensemble([wide[1]], [2.0], "max_score", 150))
    big = {1: [(i, float(i)) for i in range(2049)]}
    ens.add_recaller("x", Stub(big), 1.0)
    with pytest.raises(NotImplementedError):
        ens.recall(1, topk=1025)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_ensemble_of_real_recallers(fx, strategy):
    """ColdStartRecaller and ItemCFRecaller built from the fixture as the
    channels; the merge of their own outputs restated on the host."""
    cfg = RecallConfig()
    cold = ColdStartRecaller(cfg, *rs.recaller_args(fx))
    df = pd.DataFrame({"user_id": fx["click_user"], "click_article_id": fx["click_item"],
                       "click_timestamp": fx["click_ts"]})
    created = dict(zip(fx["item_ids"].tolist(), fx["item_created"].tolist()))
    sim = ItemCFSimilarity(cfg).calculate(df, created)
    uit = extractors.csr_to_dict(*extractors.user_item_time_csr(df))
    itemcf = ItemCFRecaller(cfg, sim, created, uit, extractors.item_topk_click(df))
    ens = RecallEnsemble(cfg, fusion_strategy=strategy)
    ens.add_recaller("coldstart", cold, 0.6)
    ens.add_recaller("itemcf", itemcf, 1.0)
    queries, topk = fx["queries"].tolist()[::3] + fx["queries"].tolist()[-2:], 10
    got = ens.batch_recall(queries, topk=topk)
    a, b = cold.batch_recall(queries, 2 * topk), itemcf.batch_recall(queries, 2 * topk)
    assert sum(1 for u in queries if a[u] and b[u]) > 20
    for u in queries:
        _same(got[u], rs.ensemble([a[u], b[u]], [0.6, 1.0], strategy, topk))
