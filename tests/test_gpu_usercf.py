"""UserCF on the GPU (csrc/usercf.hip): similarity bit-identical to the
reference-executed fixture (values, row order, entry order), the direct
top-n, and the recaller; then the numpy restatement (usercf_restated.py,
pinned to the fixture by test_usercf_host.py) at the smallest shapes where
each mechanism of the kernels can fail."""
import numpy as np
import pandas as pd
import pytest
import torch

from nrk import ops
from nrk.config import RecallConfig
from nrk.data import extractors
from nrk.recall.usercf_recaller import UserCFRecaller
from nrk.similarity.user_cf import UserCFSimilarity

import usercf_restated as rs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ fixture --
@pytest.fixture(scope="module")
def fx(golden):
    return golden("usercf_small")


def _df(user, item, ts=None):
    ts = np.arange(len(user), dtype=np.int64) * 7 + 1_500_000_000_000 if ts is None else ts
    return pd.DataFrame({"user_id": np.asarray(user, np.int64), "click_article_id": np.asarray(item, np.int64),
                         "click_timestamp": np.asarray(ts, np.int64)})


@pytest.fixture(scope="module")
def fx_run(fx):
    """The fixture's log through UserCFSimilarity.calculate, once."""
    df = _df(fx["click_user"], fx["click_item"], fx["click_ts"])
    act = dict(zip(fx["act_ids"].tolist(), fx["act_vals"].tolist()))
    calc = UserCFSimilarity(RecallConfig())
    sim = calc.calculate(df, act)
    return calc, sim


def _fx_rows(fx):
    rows = {u: ([], []) for u in fx["sim_rows"].tolist()}
    for a, b, v in zip(fx["sim_i"].tolist(), fx["sim_j"].tolist(), fx["sim_v"].tolist()):
        rows[a][0].append(b)
        rows[a][1].append(v)
    return rows


def test_calculate_equals_the_reference_bit_for_bit(fx, fx_run):
    _, sim = fx_run
    assert list(sim) == fx["sim_rows"].tolist()  # row keys and their order
    want = _fx_rows(fx)
    for u, d in sim.items():
        assert list(d) == want[u][0], u  # entry keys and their order
        assert np.array_equal(np.array(list(d.values())), np.array(want[u][1])), u  # no tolerance


def test_compute_top20_and_nnz_equal_the_reference(fx, fx_run):
    calc, _ = fx_run
    r = calc.result
    cols, vals = (x.cpu().numpy() for x in r.top(20))
    nnz, cnt = r.nnz.cpu().numpy(), r.cnt.cpu().numpy()
    want = _fx_rows(fx)
    clicks = dict(zip(*np.unique(fx["click_user"], return_counts=True)))
    split = 0
    for row, u in enumerate(r.user_ids.tolist()):
        v, w = np.array(want[u][0], np.int64), np.array(want[u][1])
        assert nnz[row] == len(v) and cnt[row] == clicks[u]
        top = rs.stable_top(w, 20)
        m = len(top)
        assert np.array_equal(r.user_ids[cols[row, :m]], v[top]), u
        assert np.array_equal(vals[row, :m], w[top]), u
        assert (cols[row, m:] == -1).all()
        split += len(w) > 20 and np.sort(w)[::-1][19] == np.sort(w)[::-1][20]
    assert split > 0  # the cut does fall inside tie groups in this fixture


def test_get_similar_users(fx, fx_run):
    calc, sim = fx_run
    u = int(fx["sim_rows"][3])
    assert calc.get_similar_users(u, 7) == sorted(sim[u].items(), key=lambda x: x[1], reverse=True)[:7]
    assert calc.get_similar_users(-12345) == []
    with pytest.raises(ValueError, match="not calculated"):
        UserCFSimilarity(RecallConfig()).get_similar_users(u)


def _fx_dicts(fx):
    uo, ui, ut = fx["uit_offsets"], fx["uit_items"].tolist(), fx["uit_ts"].tolist()
    uit = {u: list(zip(ui[uo[n]:uo[n + 1]], ut[uo[n]:uo[n + 1]])) for n, u in enumerate(fx["uit_users"].tolist())}
    created = dict(zip(fx["created_ids"].tolist(), fx["created_vals"].tolist()))
    emb = {}
    for a, b, v in zip(fx["emb_i"].tolist(), fx["emb_j"].tolist(), fx["emb_v"].tolist()):
        emb.setdefault(a, {})[b] = v
    return uit, created, emb


def _check_lists(res, users, off, items, scores, cold):
    for n, u in enumerate(users):
        got = res[u]
        assert [i for i, _ in got] == items[off[n]:off[n + 1]].tolist(), u
        want = scores[off[n]:off[n + 1]]
        assert np.allclose([s for _, s in got], want, rtol=1e-12, atol=0), u
        # hot-fill (-i - 100) and cold-start (-i) scores are Python ints, a candidate's sum (>= 0) a float
        for (_, s), w in zip(got, want):
            assert isinstance(s, int) == (u in cold or w <= -100), (u, s)


@pytest.mark.parametrize("with_emb", [False, True])
@pytest.mark.parametrize("source", ["result", "dict"])
def test_recaller_equals_the_reference(fx, fx_run, source, with_emb):
    calc, sim = fx_run
    uit, created, emb = _fx_dicts(fx)
    hot = fx["hot"].tolist()
    e = emb if with_emb else None
    if source == "result":
        rec = UserCFRecaller.from_result(RecallConfig(), calc.result, uit, created, hot, e)
    else:
        rec = UserCFRecaller(RecallConfig(), sim, uit, created, hot, e)
    users = fx["recall_users"].tolist()
    res = rec.batch_recall(users, topk=int(fx["topk"]))
    p = "emb_" if with_emb else ""
    _check_lists(res, users, fx[p + "recall_offsets"], fx[p + "recall_items"], fx[p + "recall_scores"], {-5, 10**9})
    # unknown users: the cold-start list
    for u in (-5, 10**9):
        assert res[u] == [(it, -i) for i, it in enumerate(hot[:int(fx["topk"])])]
    one = users[7]
    assert rec.recall(one, topk=int(fx["topk"])) == res[one]


def test_recaller_missing_created_time_is_a_keyerror(fx, fx_run):
    calc, _ = fx_run
    uit, created, _ = _fx_dicts(fx)
    gone = int(fx["uit_items"][0])
    created = {k: v for k, v in created.items() if k != gone}
    with pytest.raises(KeyError):
        UserCFRecaller.from_result(RecallConfig(), calc.result, uit, created, fx["hot"].tolist())


# -------------------------------------------------------------- restatement --
def _dense(df):
    """The device inputs of a log, as UserCFSimilarity.compute forms them, and the restated similarity."""
    act = extractors.user_activate_degree(df)
    calc = UserCFSimilarity(RecallConfig())
    r = calc.compute(df, act)
    _, i_off, users_raw, _ = extractors.item_user_time_csr(df)
    user_ids, i_users = np.unique(users_raw, return_inverse=True)
    a = np.array([act[u] for u in user_ids.tolist()])
    acc, first, cnt = rs.similarity(i_off, i_users, a)
    return r, acc, first, cnt


def _check_sim(r, acc, first, cnt, topns=(20,)):
    n = len(acc)
    assert np.array_equal(r.cnt.cpu().numpy(), cnt)
    assert np.array_equal(r.nnz.cpu().numpy(), (first >= 0).sum(1))
    row_off, v, s, f = (x.cpu().numpy() for x in ops.usercf_sim(*r._inputs, r.nnz))
    rows = np.repeat(np.arange(n), np.diff(row_off))
    got_acc = np.zeros_like(acc)
    got_first = np.full_like(first, -1)
    got_acc[rows, v] = s
    got_first[rows, v] = f
    assert np.array_equal(got_first, first)
    assert np.array_equal(got_acc, acc)  # bit for bit
    for topn in topns:
        cols, vals = (x.cpu().numpy() for x in r.top(topn))
        assert cols.shape == (n, topn)
        for u in range(n):
            vs = np.nonzero(first[u] >= 0)[0]
            vs = vs[np.argsort(first[u, vs], kind="stable")]
            top = vs[rs.stable_top(acc[u, vs], topn)]
            m = len(top)
            assert np.array_equal(cols[u, :m], top), (topn, u)
            assert np.array_equal(vals[u, :m], acc[u, top]), (topn, u)
            assert (cols[u, m:] == -1).all(), (topn, u)


def test_one_user_one_item_is_an_empty_row():
    r, acc, first, cnt = _dense(_df([5], [9]))
    _check_sim(r, acc, first, cnt)
    calc = UserCFSimilarity(RecallConfig())
    assert calc.calculate(_df([5], [9]), {5: 0.0}) == {5: {}}


def test_dense_log_sums_many_terms_in_order():
    # 5 users x 40 items, ~30 clicks each with different activity: every pair sums ~25 differently
    # weighted terms, so a reordered or FMA-contracted sum shows in the last bits
    rng = np.random.default_rng(3)
    user, item = [], []
    for u in range(5):
        its = rng.choice(40, 26 + 2 * u, replace=False)
        user += [u * 11 + 2] * len(its)
        item += its.tolist()
    perm = rng.permutation(len(user))
    _check_sim(*_dense(_df(np.array(user)[perm], np.array(item)[perm])))


def test_everything_ties_and_only_the_first_slot_decides():
    # every user clicks the same single item: all values of a row are equal
    rng = np.random.default_rng(4)
    users = rng.permutation(330) * 2 + 1
    r, acc, first, cnt = _dense(_df(users, np.full(330, 77)))
    assert len(np.unique(acc[first >= 0])) == 1
    _check_sim(r, acc, first, cnt, topns=(1, 20, 64, 65, 300))


def test_repeat_clicks_on_both_sides_of_a_pair():
    # u = 0 and v = 1 both click item 3 twice (and item 5 once / three times); w = 2 clicks each once
    user = [0, 1, 0, 2, 1, 0, 1, 1, 2, 1, 3]
    item = [3, 3, 3, 3, 3, 5, 5, 5, 5, 5, 8]
    r, acc, first, cnt = _dense(_df(user, item))
    assert first[0, 1] >= 0 and first[3].max() == -1
    _check_sim(r, acc, first, cnt, topns=(1, 2, 20))


@pytest.fixture(scope="module")
def wide_log():
    # 3,000 users: one item clicked by all of them (wider than a workgroup's 256 lanes; every row
    # holds 2,999 neighbours, past the selection's 256-entry chunks), 40 of them twice, plus random clicks
    rng = np.random.default_rng(5)
    n = 3000
    user = np.concatenate([np.arange(n), rng.choice(n, 40, replace=False), rng.integers(0, n, 6000)])
    item = np.concatenate([np.full(n + 40, 1), rng.integers(2, 900, 6000)])
    perm = rng.permutation(len(user))
    return _dense(_df(user[perm], item[perm]))


def test_item_wider_than_a_workgroup(wide_log):
    r, acc, first, cnt = wide_log
    assert ((first >= 0).sum(1) == 2999).all()
    _check_sim(r, acc, first, cnt, topns=(20, 300))


def test_ops_refuse_bad_ids():
    d = "cuda"
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=d)  # noqa: E731
    i_off, u_off = t([0, 2], torch.int64), t([0, 1, 2], torch.int64)
    act, pen = t([0.0, 1.0], torch.float64), t([0.5], torch.float64)
    good = (i_off, t([0, 1], torch.int32), u_off, t([0, 0], torch.int32), act, pen)
    ops.usercf_topn(*good, topn=3)
    with pytest.raises(ValueError, match="out of"):
        ops.usercf_topn(i_off, t([0, 2], torch.int32), u_off, t([0, 0], torch.int32), act, pen)
    with pytest.raises(ValueError, match="out of"):
        ops.usercf_topn(i_off, t([0, 1], torch.int32), u_off, t([0, 1], torch.int32), act, pen)
    with pytest.raises(ValueError, match="finite"):
        ops.usercf_topn(i_off, t([0, 1], torch.int32), u_off, t([0, 0], torch.int32),
                        t([0.0, float("nan")], torch.float64), pen)
    with pytest.raises(NotImplementedError):
        ops.usercf_topn(*good, topn=1025)


# ------------------------------------------------------------------- recall --
@pytest.fixture(scope="module")
def recall_log():
    """60 users x 300 items; user 0 has a 200-click history (with repeats), user
    1's history lies wholly inside it, and so does user 59's inside user 58's."""
    rng = np.random.default_rng(6)
    user, item = [0] * 200, rng.integers(0, 150, 200).tolist()
    user += [1] * 6
    item += item[10:16]
    for u in range(2, 58):
        L = int(rng.integers(1, 16))
        user += [u] * L
        item += rng.integers(0, 300, L).tolist()
    # users 58 and 59 are each other's only neighbour, and 59's history lies wholly inside 58's
    user += [58, 58, 58, 59, 59]
    item += [400, 401, 402, 400, 401]
    perm = rng.permutation(len(user))
    df = _df(np.array(user)[perm] * 5 + 3, np.array(item)[perm] * 2 + 10)
    act = extractors.user_activate_degree(df)
    calc = UserCFSimilarity(RecallConfig())
    sim = calc.calculate(df, act)
    users, off, items, ts = extractors.user_item_time_csr(df)
    uit = extractors.csr_to_dict(users, off, items, ts)
    ids = np.unique(df["click_article_id"].to_numpy())
    created = dict(zip(ids.tolist(), rng.random(len(ids)).tolist()))
    hot = extractors.item_topk_click(df, k=50)
    emb = {}
    for a in ids[::3].tolist():
        emb[a] = {int(b): float(rng.random()) for b in rng.choice(ids, 12, replace=False)}
    return calc, sim, uit, created, hot, emb


@pytest.mark.parametrize("sim_topk", [1, 5, 20])
@pytest.mark.parametrize("topk", [10, 30, 100])
def test_recall_equals_the_restatement(recall_log, sim_topk, topk):
    calc, sim, uit, created, hot, emb = recall_log
    assert set(i for i, _ in uit[8]) <= set(i for i, _ in uit[3]) and len(uit[3]) == 200
    assert list(sim[58 * 5 + 3]) == [59 * 5 + 3]  # its one neighbour adds no candidate: hot fill only
    cfg = RecallConfig()
    cfg.usercf_sim_user_topk = sim_topk
    users = list(uit) + [-1]
    for e in (None, emb):
        rec = UserCFRecaller.from_result(cfg, calc.result, uit, created, hot, e)
        res = rec.batch_recall(users, topk=topk)
        for u in users:
            want = rs.recall(u, topk, sim, uit, created, hot, e or {}, sim_topk, cfg.loc_beta)
            assert [i for i, _ in res[u]] == [i for i, _ in want], (u, e is not None)
            assert np.allclose([s for _, s in res[u]], [s for _, s in want], rtol=1e-12, atol=0), u
            assert all(isinstance(s, int) == isinstance(w, int) for (_, s), (_, w) in zip(res[u], want)), u
