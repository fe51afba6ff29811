"""Generate tests/golden/profile_small*.npz by executing the REFERENCE's
FeatureExtractor._extract_user_profile_features, _extract_item_features and
_add_labels (src/features/feature_extractor.py:296-438, :752-836) and
DINRanker._prepare_vocab_dicts (src/rank/DIN.py:560-619), imported through
make_golden.import_reference.  Runs only where make_golden.py runs.

The three methods run twice: as shipped, where load_data's str re-keying of
article_words_dict (:110-112, repeated here because load_data reads files)
makes every integer lookup of :353 miss, and with the dict re-keyed by int
("repaired": arrays with the prefix ``fix_``).

Usage:  python tests/golden/make_golden_profile.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

N_USERS, N_ARTICLES = 300, 400
DEVICES = np.arange(1, 15)  # 14 device groups: "10.0" sorts before "2.0"


def make_log():
    """About 3,000 clicks in shuffled frame order: a one-click and a two-click user, repeated articles,
    last-click timestamp ties, device-group mode ties, unclicked articles, two clicked articles that
    the article table lacks."""
    rng = np.random.default_rng(41)
    lens = np.minimum(1 + rng.geometric(1 / 9.0, N_USERS), 70)
    lens[0], lens[1] = 1, 2
    user = np.repeat(np.arange(N_USERS) * 3 + 100, lens)
    n = len(user)
    item = ((rng.zipf(1.3, n) - 1) % 330) * 7 + 11          # articles 330.. stay unclicked
    item[rng.choice(n, 5, replace=False)] = [9, 9, 10, 9, 10]  # not in the article table
    ts = 1_507_029_570_190 + rng.integers(0, 16 * 86_400_000, n)
    home = rng.choice(DEVICES, N_USERS)
    device = np.where(rng.random(n) < 0.6, np.repeat(home, lens), rng.choice(DEVICES, n))
    off = np.concatenate([[0], np.cumsum(lens)])
    for u in range(2, N_USERS, 7):  # the maximal timestamp twice, on different articles
        a, b = off[u], off[u + 1]
        if b - a >= 3:
            ts[a + 1] = ts[a:b].max()
            item[a + 1] = 11 + 7 * (300 + u % 30)
    device[off[1]:off[2]] = [9, 4]  # the two-click user: a mode tie, the smaller value second
    order = rng.permutation(n)
    return user[order], item[order], ts[order], device[order]


def run(fe_cls, cfg, clicks, arts, words_dict, main):
    fe = fe_cls(cfg)
    fe.train_click_df, fe.article_info_df = clicks, arts
    fe.article_words_dict = words_dict
    fe.main_df = main.copy()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        fe._extract_user_profile_features()
        fe._extract_item_features()
        fe._add_labels()
    return fe


def gen(tmp):
    import types

    import pandas as pd
    from nrk.rank.encode import DinEncoder

    # gensim is not installed: a stand-in satisfies feature_extractor.py's import, as in
    # make_golden.gen_ctxfeat; Word2Vec is never called here
    gm, gmm = types.ModuleType("gensim"), types.ModuleType("gensim.models")
    gmm.Word2Vec = None
    gm.models = gmm
    sys.modules.setdefault("gensim", gm)
    sys.modules.setdefault("gensim.models", gmm)
    from src.data.extractors import InteractionFeatureExtractor, ItemFeatureExtractor
    from src.features.feature_extractor import FeatureExtractor
    from src.rank.DIN import DINRanker
    from src.utils.config import RankConfig, RecallConfig

    user, item, ts, device = make_log()
    rng = np.random.default_rng(43)
    clicks = pd.DataFrame({"user_id": user, "click_article_id": item, "click_timestamp": ts,
                           "click_deviceGroup": device})
    art_id = np.arange(N_ARTICLES) * 7 + 11
    arts = pd.DataFrame({"click_article_id": art_id, "category_id": rng.integers(0, 40, N_ARTICLES),
                         "created_at_ts": 1_506_600_000_000 - rng.integers(0, 5 * 10**10, N_ARTICLES),
                         "words_count": rng.integers(0, 3000, N_ARTICLES)})

    # what the fixture must contain
    n_clicks = clicks.groupby("user_id").size()
    assert (n_clicks == 1).any() and (n_clicks == 2).any()
    assert clicks.duplicated(["user_id", "click_article_id"]).sum() >= 50
    top = clicks[clicks["click_timestamp"] == clicks.groupby("user_id")["click_timestamp"].transform("max")]
    tied = top.groupby("user_id")["click_article_id"].nunique()
    assert (tied > 1).sum() >= 10, "no last-click tie between different articles"
    sizes = clicks.groupby(["user_id", "click_deviceGroup"]).size()
    best = sizes.groupby("user_id").transform("max")
    assert ((sizes == best).groupby("user_id").sum() > 1).sum() >= 20, "no mode ties"
    assert len(set(art_id) - set(item)) >= 50 and len(set(item) - set(art_id)) == 2

    # the pairs to label: every user's last click, random articles, unknown users and articles
    _, last = InteractionFeatureExtractor.get_hist_and_last_click(clicks, offline=True)
    pu = np.concatenate([last["user_id"].to_numpy(), rng.choice(user, 1500), [1, 2, 5]])
    pi = np.concatenate([last["click_article_id"].to_numpy(), rng.choice(art_id, 1500), [11, 18, 25]])
    pi[5:300:9] = 12  # an unknown article for known users
    keep = rng.permutation(len(pu))
    pu, pi = pu[keep], pi[keep]
    main = pd.DataFrame({"user_id": [str(x) for x in pu], "item_id": [str(x) for x in pi]})

    _, words, _ = ItemFeatureExtractor.get_item_info_dict(arts)
    shipped = {str(int(k)): v for k, v in words.items()}      # feature_extractor.py:110-112
    repaired = {int(k): v for k, v in shipped.items()}

    arrays = dict(click_user=user, click_item=item, click_ts=ts, click_device=device, art_id=art_id,
                  art_category=arts["category_id"].to_numpy(), art_created=arts["created_at_ts"].to_numpy(),
                  art_words=arts["words_count"].to_numpy(), pair_user=pu, pair_item=pi)
    arrays = {k: np.asarray(v, np.int64) for k, v in arrays.items()}
    for prefix, wd in (("", shipped), ("fix_", repaired)):
        fe = run(FeatureExtractor, RecallConfig(_project_root=tmp), clicks, arts, wd, main)
        upd, ifd = fe.user_profile_dict, fe.item_features_dict
        assert all(type(p[f]) is (str if f == "device_group" else float) for p in upd.values() for f in p)
        assert all(type(p[f]) is (float if f == "article_popularity" else int) for p in ifd.values() for f in p)
        ranker = DINRanker(RankConfig(_project_root=tmp))
        ranker.user_profile_dict, ranker.item_features_dict = upd, ifd
        ranker.user_profile_features, ranker.item_features = fe.user_profile_features, fe.item_features
        ranker.context_features, ranker.main_df = [], pd.DataFrame(index=range(3))
        with contextlib.redirect_stdout(io.StringIO()):
            uv, iv, _ = ranker._prepare_vocab_dicts()
        enc = DinEncoder(upd, ifd, {}, fe.user_profile_features, fe.item_features, [], ranker.label_encoders, 1)
        out = {"user_keys": np.array(list(upd)), "user_features": np.array(fe.user_profile_features),
               "item_keys": np.array(list(ifd)), "item_features": np.array(fe.item_features),
               "device_group": np.array([p["device_group"] for p in upd.values()]),
               "device_classes": np.array(list(ranker.label_encoders["device_group"].classes_)),
               "user_table": enc.user_table, "item_table": enc.item_table,
               "user_vocab": np.array([uv[f] for f in fe.user_profile_features], np.int64),
               "item_vocab": np.array([iv[f] for f in fe.item_features], np.int64),
               "labels": fe.main_df["label"].to_numpy(np.int64)}
        for f in fe.user_profile_features:
            if f != "device_group":
                out["u_" + f] = np.array([p[f] for p in upd.values()], np.float64)
        for f in fe.item_features:
            out["i_" + f] = np.array([p[f] for p in ifd.values()], np.float64 if f == "article_popularity"
                                     else np.int64)
        assert fe.main_df["user_id"].tolist() == main["user_id"].tolist()
        arrays.update({prefix + k: v for k, v in out.items()})
    assert not arrays["u_avg_word_count"].any() and (arrays["fix_u_avg_word_count"] > 0).sum() > 250
    assert 10 <= arrays["labels"].sum() and np.array_equal(arrays["labels"], arrays["fix_labels"])
    classes = arrays["device_classes"].tolist()
    assert len(classes) >= 12 and classes.index("10.0") < classes.index("2.0")

    cfg = RecallConfig(_project_root=tmp)
    cfg.offline = False
    arrays["labels_online"] = run(FeatureExtractor, cfg, clicks, arts, shipped, main).main_df["label"].to_numpy(np.int64)
    out = mg.save_parts(os.path.join(HERE, "profile_small.npz"), **arrays)
    print(f"profile_small: {len(user)} clicks, {N_USERS} users, {N_ARTICLES} articles, {len(pu)} pairs with "
          f"{int(arrays['labels'].sum())} positives, {len(classes)} device classes, vocab "
          f"{arrays['user_vocab'].tolist()} / {arrays['item_vocab'].tolist()} -> "
          f"{[os.path.basename(p) for p in out]}")


def main():
    mg.import_reference()
    mg.seed_all()
    with tempfile.TemporaryDirectory() as tmp:
        gen(tmp)


if __name__ == "__main__":
    main()
