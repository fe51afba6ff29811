"""Generate tests/golden/coldstart_small*.npz by executing the REFERENCE's
ColdStartRecaller (coldstart_recaller.py), its two extractors
(get_user_hist_item_info_dict, get_item_info_dict) and RecallEnsemble
(fusion.py:419-556), imported through make_golden.import_reference.  Runs
only where make_golden.py runs.

The default synthetic article table (461 categories, word counts up to
6,690) lets almost no pair through the four rules, so the fixture builds its
own: 12 categories and word counts of 100-899.

Usage:  python tests/golden/make_golden_coldstart.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

TOPKS = (1, 5, 30)
ENS_TOPK = 10
ENS_WEIGHTS = (1.0, 0.7, 0.5)
STRATEGIES = ("weighted_avg", "weighted_sum", "max_score")
MAX_LIST = 200  # base lists of 0 .. MAX_LIST - 1 distinct items


def _csr(d, key_dtype=np.int64, a_dtype=np.int64):
    """{key: [(a, b), ...]} -> keys, offsets, a, b (b as f64)."""
    keys, off, a, b = [], [0], [], []
    for k, lst in d.items():
        keys.append(k)
        for x, y in lst:
            a.append(x)
            b.append(y)
        off.append(len(a))
    return np.array(keys, key_dtype), np.array(off, np.int64), np.array(a, a_dtype), np.array(b, np.float64)


def _sets(d):
    """{key: set} -> keys, offsets, members (each set ascending)."""
    keys, off, v = [], [0], []
    for k, s in d.items():
        keys.append(k)
        v += sorted(s)
        off.append(len(v))
    return np.array(keys, np.int64), np.array(off, np.int64), np.array(v, np.int64)


def as_score(x):
    """The base lists' scores: an integral value is a Python int (the plugin
    must hand it back as one), every other a float."""
    x = float(x)
    return int(x) if x.is_integer() else x


class Stub:
    """A recaller over stored lists; raises for the users of ``bad``."""

    def __init__(self, lists, bad=()):
        self.lists, self.bad = lists, set(bad)

    def recall(self, user_id, topk=10):
        if user_id in self.bad:
            raise RuntimeError("stub failure")
        return self.lists.get(user_id, [])[:topk]


def gen_coldstart(tmp):
    import pandas as pd
    from nrk.data import synth
    from src.data.extractors import ItemFeatureExtractor, UserFeatureExtractor
    from src.recall.coldstart_recaller import ColdStartRecaller
    from src.recall.fusion import RecallEnsemble
    from src.utils.config import RecallConfig

    n_users, n_items = 400, 1500
    rng = np.random.default_rng(29)
    log = synth.make_click_log(n_users=n_users, n_items=n_items, seed=7, max_len=30)
    art = synth.make_articles(n_items, seed=7)
    click_df = pd.DataFrame({"user_id": log.user_id * 3 + 100, "click_article_id": log.click_article_id * 7 + 11,
                             "click_timestamp": log.click_timestamp})
    articles_df = pd.DataFrame({"click_article_id": art.article_id * 7 + 11,
                                "category_id": rng.integers(0, 12, n_items),
                                "words_count": rng.integers(100, 900, n_items),
                                "created_at_ts": art.created_at_ts})
    merged = click_df.merge(articles_df, on="click_article_id")
    types, hist_ids, words, last = UserFeatureExtractor.get_user_hist_item_info_dict(merged)
    item_type, item_words, item_created = ItemFeatureExtractor.get_item_info_dict(articles_df)
    clicked = set(click_df["click_article_id"].tolist())

    # base lists: 0 .. MAX_LIST - 1 distinct items per user, scores with two decimals (ties, and integral
    # values as ints); ids 5 and 6 are in no article table; the last two users have no profile
    users = sorted(types)
    art_ids = articles_df["click_article_id"].to_numpy()
    pool = np.concatenate([art_ids, [5, 6]])
    base = {}
    for u in users:
        n = int(rng.integers(0, MAX_LIST))
        its = rng.choice(pool, size=n, replace=False).tolist()
        base[u] = [(int(i), as_score(s)) for i, s in zip(its, np.round(rng.random(n) * 3, 2).tolist())]
    no_profile = users[-2:]
    p_types, p_words, p_last = ({u: v for u, v in d.items() if u not in no_profile} for d in (types, words, last))

    cfg = RecallConfig(_project_root=tmp)
    rec = ColdStartRecaller(cfg, base, p_types, p_words, p_last, item_type, item_words, item_created, clicked)
    filtered = rec.filtered_results
    stats = rec.get_statistics()
    queries = users + [-5, 10**9]
    recalls = {k: {u: rec.recall(u, topk=k) for u in queries} for k in TOPKS}

    # what each rule does to the pairs that reach it (the reference's order, :74-115)
    reach = {r: 0 for r in ("item", "type", "clicked", "words", "time")}
    drop = dict(reach)
    for u, lst in base.items():
        if u not in p_types:
            continue
        for it, _ in lst:
            for rule, bad in (("item", lambda: it not in item_type),
                              ("type", lambda: item_type[it] not in p_types[u]),
                              ("clicked", lambda: it in clicked),
                              ("words", lambda: abs(item_words[it] - p_words[u]) > 200),
                              ("time", lambda: abs(item_created[it] - p_last[u]) > 0.25)):
                reach[rule] += 1
                if bad():
                    drop[rule] += 1
                    break
    for rule in ("type", "clicked", "words", "time"):
        share = drop[rule] / reach[rule]
        assert 0.1 <= share <= 0.9, (rule, share)
    assert drop["item"] >= 20, drop
    surv = {u: len(filtered.get(u, ())) for u in base}
    assert sum(1 for u in base if surv[u] == 0) >= 20
    assert sum(1 for u in base if surv[u] > 5) >= 20
    tied = sum(1 for lst in filtered.values() if len({s for _, s in lst}) < len(lst))
    assert tied >= 10, tied
    assert any(isinstance(s, int) for lst in filtered.values() for _, s in lst), "no int score survives"

    # Part 2: the base lists and two more stored recalls as stub recallers; stub b fails for a few users
    def more(seed, frac):
        r = np.random.default_rng(seed)
        out = {}
        for u in users:
            if r.random() > frac:
                continue
            own = [i for i, _ in base[u]][:40]
            n = int(r.integers(0, 26))
            its = list(dict.fromkeys(r.choice(np.concatenate([own, art_ids[:60]]).astype(np.int64), size=n).tolist()))
            out[u] = [(int(i), float(s)) for i, s in zip(its, np.round(r.random(len(its)) * 5, 1).tolist())]
        return out

    stub_a, stub_b = more(31, 0.9), more(37, 0.7)
    bad_b = [u for u in users if u in stub_b][3:40:6]
    ens = {}
    for strat in STRATEGIES:
        e = RecallEnsemble(cfg, fusion_strategy=strat)
        for name, r, w in zip(("base", "a", "b"), (Stub(base), Stub(stub_a), Stub(stub_b, bad_b)), ENS_WEIGHTS):
            e.add_recaller(name, r, w)
        ens[strat] = e.batch_recall(queries, topk=ENS_TOPK)
    assert sum(1 for u in queries if not ens["weighted_avg"][u]) >= 2
    assert any([i for i, _ in ens["weighted_avg"][u]] != [i for i, _ in ens["max_score"][u]] for u in queries)

    arrays = {}

    def put(prefix, d, order=None):
        d = d if order is None else {u: d[u] for u in order}
        k, off, a, b = _csr(d)
        arrays.update({f"{prefix}_users": k, f"{prefix}_offsets": off, f"{prefix}_items": a, f"{prefix}_scores": b})

    put("base", base)
    put("filtered", filtered)
    for k in TOPKS:
        put(f"recall{k}", recalls[k], queries)
    put("stub_a", stub_a)
    put("stub_b", stub_b)
    for strat in STRATEGIES:
        put(f"ens_{strat}", ens[strat], queries)
    tk, toff, tv = _sets(p_types)
    hk, hoff, hv = _sets(hist_ids)
    fk, foff, fv = _sets(types)
    iid = np.array(list(item_type), np.int64)
    out = mg.save_parts(
        os.path.join(HERE, "coldstart_small.npz"),
        click_user=merged["user_id"].to_numpy(np.int64), click_item=merged["click_article_id"].to_numpy(np.int64),
        click_ts=merged["click_timestamp"].to_numpy(np.int64),
        click_category=merged["category_id"].to_numpy(np.int64), click_words=merged["words_count"].to_numpy(np.int64),
        click_created=merged["created_at_ts"].to_numpy(np.int64),
        art_id=art_ids.astype(np.int64), art_category=articles_df["category_id"].to_numpy(np.int64),
        art_words=articles_df["words_count"].to_numpy(np.int64),
        art_created=articles_df["created_at_ts"].to_numpy(np.int64),
        # the extractors' dicts over every user, then the profile dicts the recaller got (two users left out)
        types_users=fk, types_offsets=foff, types_values=fv,
        hist_users=hk, hist_offsets=hoff, hist_values=hv,
        words_users=np.array(list(words), np.int64), words_values=np.array(list(words.values()), np.float64),
        last_users=np.array(list(last), np.int64), last_values=np.array(list(last.values()), np.float64),
        prof_users=tk, prof_offsets=toff, prof_values=tv,
        item_ids=iid, item_type=np.array([item_type[i] for i in iid.tolist()], np.int64),
        item_words=np.array([item_words[i] for i in iid.tolist()], np.int64),
        item_created=np.array([item_created[i] for i in iid.tolist()], np.float64),
        clicked=np.array(sorted(clicked), np.int64),
        stats_keys=np.array(list(stats)), stats_values=np.array([float(v) for v in stats.values()], np.float64),
        queries=np.array(queries, np.int64), topks=np.array(TOPKS, np.int64),
        ens_topk=np.int64(ENS_TOPK), ens_weights=np.array(ENS_WEIGHTS, np.float64), ens_bad_b=np.array(bad_b, np.int64),
        **arrays,
    )
    print(f"coldstart_small: {sum(len(x) for x in base.values())} pairs, dropped/reached {drop} / {reach}, "
          f"{sum(len(x) for x in filtered.values())} kept for {len(filtered)} users (max {max(surv.values())}, "
          f"{sum(1 for v in surv.values() if v > 5)} with more than 5), {tied} users with tied survivors "
          f"-> {[os.path.basename(p) for p in out]}")


def main():
    mg.import_reference()
    mg.seed_all()
    with tempfile.TemporaryDirectory() as tmp:
        gen_coldstart(tmp)


if __name__ == "__main__":
    main()
