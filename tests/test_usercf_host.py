"""UserCF checks that need no GPU: the numpy restatement (the checker of the
GPU tests) equals reference-executed data, the host-side extractors equal the
reference's dicts, and the new C entry points answer their host queries and
refuse bad arguments before touching a pointer."""
import numpy as np
import pytest

from nrk import _lib
from nrk.config import RecallConfig
from nrk.data import extractors

import usercf_restated as rs


@pytest.fixture(scope="module")
def fx(golden):
    return golden("usercf_small")


@pytest.fixture(scope="module")
def dense(fx):
    """The fixture's item -> user CSR over dense user ids."""
    user_ids, i_users = np.unique(fx["iut_users"], return_inverse=True)
    act = dict(zip(fx["act_ids"].tolist(), fx["act_vals"].tolist()))
    return user_ids, i_users, np.array([act[u] for u in user_ids.tolist()])


def _dicts(fx):
    uo, ui, ut = fx["uit_offsets"], fx["uit_items"].tolist(), fx["uit_ts"].tolist()
    uit = {u: list(zip(ui[uo[n]:uo[n + 1]], ut[uo[n]:uo[n + 1]])) for n, u in enumerate(fx["uit_users"].tolist())}
    u2u = {u: {} for u in fx["sim_rows"].tolist()}
    for a, b, v in zip(fx["sim_i"].tolist(), fx["sim_j"].tolist(), fx["sim_v"].tolist()):
        u2u[a][b] = v
    created = dict(zip(fx["created_ids"].tolist(), fx["created_vals"].tolist()))
    emb = {}
    for a, b, v in zip(fx["emb_i"].tolist(), fx["emb_j"].tolist(), fx["emb_v"].tolist()):
        emb.setdefault(a, {})[b] = v
    return uit, u2u, created, emb


def test_restated_similarity_equals_the_reference(fx, dense):
    user_ids, i_users, act = dense
    acc, first, _ = rs.similarity(fx["iut_offsets"], i_users, act)
    rows = rs.rows_in_order(acc, first)
    # row order: first encounter of u in the item walk
    _, pos = np.unique(i_users, return_index=True)
    assert np.array_equal(user_ids[np.argsort(pos, kind="stable")], fx["sim_rows"])
    gi, gj, gv = [], [], []
    for r in np.argsort(pos, kind="stable").tolist():
        v, w = rows[r]
        gi += [int(user_ids[r])] * len(v)
        gj += user_ids[v].tolist()
        gv += w.tolist()
    assert np.array_equal(gi, fx["sim_i"]) and np.array_equal(gj, fx["sim_j"])
    assert np.array_equal(np.array(gv), fx["sim_v"])  # bit for bit: the top-n cut falls inside ties


@pytest.mark.parametrize("with_emb", [False, True])
def test_restated_recall_equals_the_reference(fx, with_emb):
    uit, u2u, created, emb = _dicts(fx)
    p = "emb_" if with_emb else ""
    off, items, scores = fx[p + "recall_offsets"], fx[p + "recall_items"], fx[p + "recall_scores"]
    hot = fx["hot"].tolist()
    for n, u in enumerate(fx["recall_users"].tolist()):
        got = rs.recall(u, int(fx["topk"]), u2u, uit, created, hot, emb if with_emb else {},
                        int(fx["sim_user_topk"]), float(fx["loc_beta"]))
        assert [i for i, _ in got] == items[off[n]:off[n + 1]].tolist(), u
        assert np.allclose([s for _, s in got], scores[off[n]:off[n + 1]], rtol=1e-12, atol=0), u


def test_item_user_time_csr_equals_the_reference(fx):
    import pandas as pd

    df = pd.DataFrame({"user_id": fx["click_user"], "click_article_id": fx["click_item"],
                       "click_timestamp": fx["click_ts"]})
    items, off, users, ts = extractors.item_user_time_csr(df)
    assert np.array_equal(items, fx["iut_items"]) and np.array_equal(off, fx["iut_offsets"])
    assert np.array_equal(users, fx["iut_users"]) and np.array_equal(ts, fx["iut_ts"])


def test_user_activate_degree_equals_the_reference(fx):
    import pandas as pd

    df = pd.DataFrame({"user_id": fx["click_user"], "click_article_id": fx["click_item"],
                       "click_timestamp": fx["click_ts"]})
    act = extractors.user_activate_degree(df)
    assert list(act) == fx["act_ids"].tolist()
    assert np.array_equal(np.array(list(act.values())), fx["act_vals"])


def test_config_defaults():
    c = RecallConfig()
    assert c.usercf_sim_user_topk == 20 and c.usercf_recall_num == 10


def test_workspace_is_bounded_by_rows_not_pairs():
    L = _lib.lib()
    # a 4 MB dense row (fp64 sum + int64 first slot per user) and a 1 MB touched
    # list per resident workgroup, 2 per CU on 256 CUs: ~2.6 GB at 250k users;
    # the u2u matrix itself (sum n_i^2 = 3.6e10 terms) would be hundreds of GB
    ws = L.nrk_usercf_workspace_bytes(250000, 1630832, 20)
    assert 0 < ws < 4 << 30
    assert L.nrk_usercf_workspace_bytes(250000, 1630832, 0) == 0
    assert L.nrk_usercf_workspace_bytes(-1, 10, 20) == 0
    assert L.nrk_usercf_recall_workspace_bytes(1000) == L.nrk_itemcf_recall_workspace_bytes(1000) > 0
    assert L.nrk_usercf_recall_workspace_bytes(-1) == 0


def test_argument_errors():
    L = _lib.lib()
    err = lambda: L.nrk_last_error()  # noqa: E731
    # nrk_usercf_topn: topn, sizes, null pointers -- all before any launch
    a = (None, 10, None, None, 10, None, 20, None, None)
    assert L.nrk_usercf_topn(*a, 0, None, None, None, None, None, 0, None) == _lib.NRK_EINVAL
    assert b"topn must be >= 1" in err()
    assert L.nrk_usercf_topn(*a, 1025, None, None, None, None, None, 0, None) == _lib.NRK_EUNSUPPORTED
    assert L.nrk_usercf_topn(*a, 20, None, None, None, None, None, 0, None) == _lib.NRK_EINVAL
    assert b"null pointer" in err()
    assert L.nrk_usercf_topn(None, 10, None, None, -1, None, 20, None, None, 20, None, None, None, None, None, 0,
                             None) == _lib.NRK_EINVAL
    assert b"negative size" in err()
    with pytest.raises(ValueError):
        _lib.check(_lib.NRK_EINVAL, "nrk_usercf_topn")
    # nrk_usercf_sim
    assert L.nrk_usercf_sim(*a, None, 5, None, None, None, None, 0, None) == _lib.NRK_EINVAL
    assert b"null pointer" in err()
    assert L.nrk_usercf_sim(None, 10, None, None, 10, None, -3, None, None, None, 5, None, None, None, None, 0,
                            None) == _lib.NRK_EINVAL
    assert b"negative size" in err()
    # nrk_usercf_recall_offsets
    assert L.nrk_usercf_recall_offsets(None, -1, None, None, None, 20, None, None) == _lib.NRK_EINVAL
    assert L.nrk_usercf_recall_offsets(None, 5, None, None, None, 0, None, None) == _lib.NRK_EINVAL
    assert b"topn must be >= 1" in err()
    assert L.nrk_usercf_recall_offsets(None, 5, None, None, None, 20, None, None) == _lib.NRK_EINVAL
    assert b"null pointer" in err()
    # nrk_usercf_recall
    r = lambda topn, topk, n_cand=10: L.nrk_usercf_recall(  # noqa: E731
        None, 5, None, None, None, None, None, topn, None, None, 100, None, 0, None, None, None, 0, 0.8, None,
        n_cand, topk, None, None, None, None, None, 0, None)
    assert r(20, 0) == _lib.NRK_EINVAL and b"topk must be >= 1" in err()
    assert r(20, 2049) == _lib.NRK_EUNSUPPORTED
    assert r(0, 10) == _lib.NRK_EINVAL
    assert r(20, 10, -1) == _lib.NRK_EINVAL and b"negative size" in err()
    assert r(20, 10, 2**31) == _lib.NRK_EINVAL and b"2^31" in err()
    assert r(20, 10) == _lib.NRK_EINVAL and b"null pointer" in err()
