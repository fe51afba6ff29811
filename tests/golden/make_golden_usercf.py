"""Generate tests/golden/usercf_small*.npz by executing the REFERENCE's
UserCFSimilarity.calculate and UserCFRecaller.batch_recall (user_cf.py,
usercf_recaller.py), imported through make_golden.import_reference.  Runs
only where make_golden.py runs.

Usage:  python tests/golden/make_golden_usercf.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

TOPK = 30
EMB_TOPK = 64  # the default 20 of 1,500 items leaves the content weight without a visible effect


def _csr(d):
    keys, off, a, b = [], [0], [], []
    for k, lst in d.items():
        keys.append(k)
        for x, y in lst:
            a.append(x)
            b.append(y)
        off.append(len(a))
    return (np.array(keys, np.int64), np.array(off, np.int64), np.array(a, np.int64), np.array(b, np.int64))


def _lists(res, users):
    it, sc, off = [], [], [0]
    for u in users:
        for i, s in res[u]:
            it.append(i)
            sc.append(s)
        off.append(len(it))
    return np.array(off, np.int64), np.array(it, np.int64), np.array(sc, np.float64)


def gen_usercf(tmp):
    import pandas as pd
    from nrk.data import synth
    from src.data.extractors import InteractionFeatureExtractor, ItemFeatureExtractor, UserFeatureExtractor
    from src.recall.usercf_recaller import UserCFRecaller
    from src.similarity.embedding import EmbeddingSimilarity
    from src.similarity.user_cf import UserCFSimilarity
    from src.utils.config import RecallConfig

    n_users, n_items = 400, 1500
    log = synth.make_click_log(n_users=n_users, n_items=n_items, seed=7, max_len=30)
    art = synth.make_articles(n_items, seed=7)
    click_df = pd.DataFrame({"user_id": log.user_id * 3 + 100, "click_article_id": log.click_article_id * 7 + 11,
                             "click_timestamp": log.click_timestamp})
    articles_df = pd.DataFrame({"click_article_id": art.article_id * 7 + 11, "category_id": art.category_id,
                                "words_count": art.words_count, "created_at_ts": art.created_at_ts})
    _, _, created = ItemFeatureExtractor.get_item_info_dict(articles_df)
    hot = ItemFeatureExtractor.get_item_topk_click(click_df, k=50)
    uit = UserFeatureExtractor.get_user_item_time_dict(click_df)
    iut = InteractionFeatureExtractor.get_item_user_time_dict(click_df)
    act = UserFeatureExtractor.get_user_activate_degree_dict(click_df)

    cfg = RecallConfig(_project_root=tmp)
    sim = UserCFSimilarity(cfg).calculate(click_df, act)
    rows, si, sj, sv = [], [], [], []
    for u, d in sim.items():
        rows.append(u)
        for v, w in d.items():
            si.append(u)
            sj.append(v)
            sv.append(w)
    users = list(uit.keys()) + [-5, 10**9]
    rec = UserCFRecaller(cfg, sim, uit, created, hot, emb_similarity_matrix={})
    res = rec.batch_recall(users, topk=TOPK)

    erng = np.random.default_rng(17)
    art_ids = articles_df["click_article_id"].to_numpy(np.int64)
    eemb = erng.standard_normal((len(art_ids), 16)).astype(np.float32)
    edf = pd.DataFrame(eemb, columns=[f"emb_{n}" for n in range(16)])
    edf.insert(0, "article_id", art_ids)
    ecfg = RecallConfig(_project_root=tmp)
    ecfg.embedding_topk = EMB_TOPK
    esim_all = EmbeddingSimilarity(ecfg).calculate(edf)
    clicked = set(click_df["click_article_id"].tolist())  # only clicked items can meet in a walk
    esim = {a: {b: v for b, v in dd.items() if b in clicked} for a, dd in esim_all.items() if a in clicked}
    esim = {a: dd for a, dd in esim.items() if dd}
    ei, ej, ev = [], [], []
    for a, dd in esim.items():
        for b, v in dd.items():
            ei.append(a)
            ej.append(b)
            ev.append(v)
    eres = UserCFRecaller(cfg, sim, uit, created, hot, emb_similarity_matrix=esim).batch_recall(users, topk=TOPK)

    # the conditions that let the tests demand exact order
    for r in (res, eres):
        for u in users:
            sc = [s for _, s in r[u] if s > 0]
            for a, b in zip(sc, sc[1:]):
                assert a > b and (a - b) > 1e-9 * a, (u, a, b)
    assert any([i for i, _ in res[u]] != [i for i, _ in eres[u]] for u in users), "content weight changes no list"

    roff, ri, rs = _lists(res, users)
    eroff, eri, ers = _lists(eres, users)
    iut_items, iut_off, iut_users, iut_ts = _csr(iut)
    uit_users, uit_off, uit_items, uit_ts = _csr(uit)
    aids = np.array(sorted(act.keys()), np.int64)
    cids = np.array(sorted(created.keys()), np.int64)
    out = mg.save_parts(
        os.path.join(HERE, "usercf_small.npz"),
        click_user=click_df["user_id"].to_numpy(np.int64),
        click_item=click_df["click_article_id"].to_numpy(np.int64),
        click_ts=click_df["click_timestamp"].to_numpy(np.int64),
        iut_items=iut_items, iut_offsets=iut_off, iut_users=iut_users, iut_ts=iut_ts,
        uit_users=uit_users, uit_offsets=uit_off, uit_items=uit_items, uit_ts=uit_ts,
        act_ids=aids, act_vals=np.array([act[a] for a in aids], np.float64),
        created_ids=cids, created_vals=np.array([created[c] for c in cids], np.float64),
        hot=np.array(hot, np.int64),
        sim_rows=np.array(rows, np.int64), sim_i=np.array(si, np.int64), sim_j=np.array(sj, np.int64),
        sim_v=np.array(sv, np.float64),
        recall_users=np.array(users, np.int64), recall_offsets=roff, recall_items=ri, recall_scores=rs,
        topk=np.int64(TOPK), sim_user_topk=np.int64(cfg.usercf_sim_user_topk), loc_beta=np.float64(cfg.loc_beta),
        emb_i=np.array(ei, np.int64), emb_j=np.array(ej, np.int64), emb_v=np.array(ev, np.float64),
        emb_recall_offsets=eroff, emb_recall_items=eri, emb_recall_scores=ers,
    )
    lens = [len(d) for d in sim.values()]
    print(f"usercf_small: {len(click_df)} clicks, {len(si)} pairs, {lens.count(0)} empty rows, max row {max(lens)}, "
          f"hottest item {max(len(v) for v in iut.values())} clickers, {len(ei)} emb entries, "
          f"{sum(1 for u in users if [i for i, _ in res[u]] != [i for i, _ in eres[u]])} lists changed by the "
          f"content weight -> {[os.path.basename(p) for p in out]}")


def main():
    mg.import_reference()
    mg.seed_all()
    with tempfile.TemporaryDirectory() as tmp:
        gen_usercf(tmp)


if __name__ == "__main__":
    main()
