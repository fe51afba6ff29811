"""Host restatement of three FeatureExtractor methods with vectorised pandas /
sklearn calls (feature_extractor.py:296-438, :752-836) and of the encoders of
DINRanker._prepare_vocab_dicts (DIN.py:579-603): the checker of the GPU tests.
tests/test_profile_host.py holds it to reference-executed data bit for bit.

Frames as the reference's: clicks (user_id, click_article_id,
click_timestamp, click_deviceGroup), articles (click_article_id, category_id,
created_at_ts, words_count), all integer columns."""
import numpy as np
import pandas as pd
from sklearn.preprocessing import LabelEncoder, MinMaxScaler

USER_FEATURES = ["user_click_count", "user_avg_time_gap", "device_group", "avg_click_time", "avg_word_count"]
ITEM_FEATURES = ["category_id", "article_popularity", "created_at_ts", "words_count"]


def _scaled(col):
    return MinMaxScaler().fit_transform(np.asarray(col).reshape(-1, 1))[:, 0]


def frames(fx):
    clicks = pd.DataFrame({"user_id": fx["click_user"], "click_article_id": fx["click_item"],
                           "click_timestamp": fx["click_ts"], "click_deviceGroup": fx["click_device"]})
    arts = pd.DataFrame({"click_article_id": fx["art_id"], "category_id": fx["art_category"],
                         "created_at_ts": fx["art_created"], "words_count": fx["art_words"]})
    return clicks, arts


def last_clicks(clicks):
    """get_hist_and_last_click's last click per user (extractors.py:253-258): a stable two-key sort, so
    timestamp ties go to the later frame row.  A Series user_id -> article."""
    last = clicks.sort_values(by=["user_id", "click_timestamp"]).groupby("user_id").tail(1)
    return pd.Series(last["click_article_id"].to_numpy(), index=last["user_id"].to_numpy())


def user_columns(clicks, arts, repair_word_lookup=False):
    """One row per user, ascending user_id: the raw and the scaled columns."""
    g = clicks.groupby("user_id")
    n = g["click_article_id"].count()
    tmax, tmin = g["click_timestamp"].max(), g["click_timestamp"].min()
    many = (n > 1).to_numpy()
    gap = np.zeros(len(n), np.float64)
    gap[many] = (tmax - tmin).to_numpy()[many] / (n.to_numpy()[many] - 1)
    # mode()[0]: the most frequent value, the smallest among ties
    sizes = clicks.groupby(["user_id", "click_deviceGroup"]).size().reset_index(name="k")
    mode = sizes.sort_values(["user_id", "k", "click_deviceGroup"], ascending=[True, False, True],
                             kind="stable").groupby("user_id").head(1)
    assert mode["user_id"].to_numpy().tolist() == n.index.tolist()
    mean_ts = g["click_timestamp"].mean()
    # mean words of the distinct articles; the shipped lookup (str keys, int ids) finds none
    dist = clicks.drop_duplicates(["user_id", "click_article_id"])
    if repair_word_lookup:
        table = pd.Series(arts["words_count"].to_numpy(), index=arts["click_article_id"].to_numpy())
        w = dist["click_article_id"].map(table).fillna(0).astype(np.int64)
    else:
        w = pd.Series(0, index=dist.index, dtype=np.int64)
    dg = w.groupby(dist["user_id"])
    words = dg.sum().to_numpy().astype(np.float64) / dg.count().to_numpy()
    return pd.DataFrame({
        "user_id": n.index.to_numpy(), "click_count": n.to_numpy(), "avg_time_gap": gap,
        "mean_click_time": mean_ts.to_numpy(), "device_group": mode["click_deviceGroup"].to_numpy(),
        "user_click_count": _scaled(n.to_numpy()), "user_avg_time_gap": _scaled(gap),
        "avg_click_time": _scaled(mean_ts.to_numpy()), "avg_word_count": words,
        "last_item": last_clicks(clicks).reindex(n.index).to_numpy()})


def item_columns(clicks, arts):
    """One row per article row: popularity fitted over the clicked articles, 0.0 for an unclicked one."""
    vc = clicks["click_article_id"].value_counts()
    scaled = pd.Series(_scaled(vc.to_numpy()), index=vc.index)
    out = arts[["click_article_id", "category_id", "created_at_ts", "words_count"]].copy()
    out["click_count"] = out["click_article_id"].map(vc).fillna(0).astype(np.int64).to_numpy()
    out["article_popularity"] = out["click_article_id"].map(scaled).fillna(0.0).to_numpy()
    return out


def dicts(ucols, icols):
    """user_profile_dict / item_features_dict with the reference's keys, order and value types."""
    user = {}
    for u, c, g, d, t, w in zip(ucols["user_id"].tolist(), ucols["user_click_count"].tolist(),
                                ucols["user_avg_time_gap"].tolist(), ucols["device_group"].tolist(),
                                ucols["avg_click_time"].tolist(), ucols["avg_word_count"].tolist()):
        user[str(int(u))] = {"user_click_count": c, "user_avg_time_gap": g, "device_group": str(np.float64(d)),
                             "avg_click_time": t, "avg_word_count": w}
    items = {}
    for i, c, p, t, w in zip(icols["click_article_id"].tolist(), icols["category_id"].tolist(),
                             icols["article_popularity"].tolist(), icols["created_at_ts"].tolist(),
                             icols["words_count"].tolist()):
        items[str(i)] = {"category_id": c, "article_popularity": p, "created_at_ts": t, "words_count": w}
    return user, items


def check_dicts(fx, prefix, user, items):
    """The two dicts equal the reference's stored ones: keys, key order, feature order, value types, bits."""
    assert list(user) == fx[prefix + "user_keys"].tolist() and list(items) == fx[prefix + "item_keys"].tolist()
    assert fx[prefix + "user_features"].tolist() == USER_FEATURES
    assert fx[prefix + "item_features"].tolist() == ITEM_FEATURES
    for p in user.values():
        assert list(p) == USER_FEATURES
        assert all(type(p[f]) is (str if f == "device_group" else float) for f in p)
    for p in items.values():
        assert list(p) == ITEM_FEATURES
        assert all(type(p[f]) is (float if f == "article_popularity" else int) for f in p)
    for f in USER_FEATURES:
        if f == "device_group":
            assert [p[f] for p in user.values()] == fx[prefix + "device_group"].tolist()
        else:
            assert np.array([p[f] for p in user.values()], np.float64).tobytes() == fx[prefix + "u_" + f].tobytes(), f
    for f in ITEM_FEATURES:
        want = fx[prefix + "i_" + f]
        assert np.array([p[f] for p in items.values()], want.dtype).tobytes() == want.tobytes(), f


def encoders(user, items):
    """_prepare_vocab_dicts for the two dicts: {feature: LabelEncoder} and the vocabulary sizes."""
    enc, uvoc, ivoc = {}, [], []
    for feats, d, voc in ((USER_FEATURES, user, uvoc), (ITEM_FEATURES, items, ivoc)):
        for f in feats:
            values = {p[f] for p in d.values() if f in p}
            if values:
                enc[f] = LabelEncoder().fit(list(values))
                voc.append(len(enc[f].classes_) + 1)
    return enc, uvoc, ivoc


def encoded(user, items):
    """(user_table, item_table, user vocabularies, item vocabularies) through DinEncoder."""
    from nrk.rank.encode import DinEncoder

    enc, uvoc, ivoc = encoders(user, items)
    e = DinEncoder(user, items, {}, USER_FEATURES, ITEM_FEATURES, [], enc, 1)
    return e.user_table, e.item_table, uvoc, ivoc


def labels(clicks, pair_user, pair_item, offline=True):
    """_add_labels: 1 where (user, item) is the user's last click; -1 everywhere online."""
    if not offline:
        return np.full(len(pair_user), -1, np.int64)
    last = last_clicks(clicks)
    want = pd.Series(np.asarray(pair_user)).map(last)
    return (want.to_numpy() == np.asarray(pair_item)).astype(np.int64)
