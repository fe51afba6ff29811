"""nrk.profile.ProfileFeatures on the GPU: user profiles, item features,
encoded tables and labels equal reference-executed data exactly (the
profile_small fixture, as shipped and with the word lookup repaired), and the
host restatement (tests/profile_restated.py, itself held to the fixture in
tests/test_profile_host.py) at the shapes where the kernels take another
path: the 64-click chunk boundaries, a repeat across two chunks, the Kahan
path of the mean timestamp, a constant column, no users, unknown rows, online
mode, too many device groups, one long user."""
import numpy as np
import pandas as pd
import pytest
import torch

import profile_restated as rs

pytestmark = pytest.mark.gpu

BASE_TS = 1_507_029_570_190


@pytest.fixture(scope="module")
def fx(golden):
    return golden("profile_small")


def _articles(n, rng):
    return pd.DataFrame({"click_article_id": np.arange(n) * 5 + 3, "category_id": rng.integers(0, 9, n),
                         "created_at_ts": 1_506_000_000_000 + rng.integers(0, 10**9, n),
                         "words_count": rng.integers(1, 4000, n)})


def _clicks(user, item, ts, device, rng=None):
    df = pd.DataFrame({"user_id": np.asarray(user, np.int64), "click_article_id": np.asarray(item, np.int64),
                       "click_timestamp": np.asarray(ts, np.int64), "click_deviceGroup": np.asarray(device, np.int64)})
    return df if rng is None else df.iloc[rng.permutation(len(df))].reset_index(drop=True)


def _bits(t):
    return t.cpu().numpy().tobytes()


def check_against_restatement(clicks, arts, repair=True):
    from nrk.profile import ProfileFeatures

    pf = ProfileFeatures.from_frames(clicks, arts, repair_word_lookup=repair)
    ucols, icols = rs.user_columns(clicks, arts, repair_word_lookup=repair), rs.item_columns(clicks, arts)
    ur, ir = pf.user_raw, pf.item_raw
    assert pf.user_ids.tolist() == ucols["user_id"].tolist()
    assert ur["click_count"].cpu().tolist() == ucols["click_count"].tolist()
    for f in ("avg_time_gap", "mean_click_time", "user_click_count", "user_avg_time_gap", "avg_click_time",
              "avg_word_count"):
        assert _bits(ur[f]) == ucols[f].to_numpy(np.float64).tobytes(), f
    assert pf.dev_values[ur["device_code"].cpu().numpy()].tolist() == ucols["device_group"].tolist()
    assert pf.row_ids[pf.last_item.cpu().numpy()].tolist() == ucols["last_item"].tolist()
    assert ir["click_count"].cpu().tolist() == icols["click_count"].tolist()
    assert _bits(ir["article_popularity"]) == icols["article_popularity"].to_numpy(np.float64).tobytes()
    user, items, uf, itf = pf.dicts()
    assert (user, items) == rs.dicts(ucols, icols) and uf == rs.USER_FEATURES and itf == rs.ITEM_FEATURES
    ut, it, uvoc, ivoc = pf.encoded()
    wu, wi, wuv, wiv = rs.encoded(user, items)
    assert ut.dtype == torch.int32 and it.dtype == torch.int32
    assert np.array_equal(ut.cpu().numpy(), wu) and np.array_equal(it.cpu().numpy(), wi)
    assert uvoc == wuv and ivoc == wiv
    return pf, ucols, icols


@pytest.mark.parametrize("prefix", ["", "fix_"])
def test_fixture_through_from_frames(fx, prefix):
    from nrk.profile import ProfileFeatures

    clicks, arts = rs.frames(fx)
    pf = ProfileFeatures.from_frames(clicks, arts, repair_word_lookup=bool(prefix))
    for f in ("user_click_count", "user_avg_time_gap", "avg_click_time", "avg_word_count"):
        assert _bits(pf.user_raw[f]) == fx[prefix + "u_" + f].tobytes(), f
    assert _bits(pf.item_raw["article_popularity"]) == fx[prefix + "i_article_popularity"].tobytes()
    for f in ("category_id", "created_at_ts", "words_count"):
        assert _bits(pf.item_raw[f]) == fx[prefix + "i_" + f].tobytes(), f
    user, items, uf, itf = pf.dicts()
    assert uf == rs.USER_FEATURES and itf == rs.ITEM_FEATURES
    rs.check_dicts(fx, prefix, user, items)
    ut, it, uvoc, ivoc = pf.encoded()
    assert np.array_equal(ut.cpu().numpy(), fx[prefix + "user_table"])
    assert np.array_equal(it.cpu().numpy(), fx[prefix + "item_table"])
    assert uvoc == fx[prefix + "user_vocab"].tolist() and ivoc == fx[prefix + "item_vocab"].tolist()
    # the pairs as rows; -1 = a user / article the frames do not hold (row_ids: a clicked article without
    # an article row has an item row all the same, and can be a last click)
    urow = pd.Index(pf.user_ids).get_indexer(fx["pair_user"])
    irow = pd.Index(pf.row_ids).get_indexer(fx["pair_item"])
    assert (urow < 0).sum() == 3 and (irow < 0).sum() >= 10
    d = lambda a: torch.from_numpy(a.astype(np.int32)).cuda()  # noqa: E731
    assert pf.labels(d(urow), d(irow)).cpu().tolist() == fx[prefix + "labels"].tolist()
    assert pf.labels(d(urow), d(irow), offline=False).cpu().tolist() == fx["labels_online"].tolist()


def test_chunk_boundaries_and_a_repeat_across_chunks():
    """Users of 1, 2, 63, 64, 65, 128 and 129 clicks over 40 articles (every long user repeats some), and a
    100-click user whose one repeated article holds positions 60-69 of the ascending item order."""
    rng = np.random.default_rng(5)
    arts = _articles(200, rng)
    ids = arts["click_article_id"].to_numpy()
    user, item = [], []
    for u, n in enumerate((1, 2, 63, 64, 65, 128, 129)):
        user += [10 + 2 * u] * n
        item += rng.choice(ids[:40], n).tolist()
    user += [7] * 100
    item += ids[:60].tolist() + [ids[60]] * 10 + ids[61:91].tolist()
    n = len(user)
    ts = BASE_TS + rng.integers(0, 10**6, n)   # a narrow window: timestamp ties
    clicks = _clicks(user, item, ts, rng.integers(1, 5, n), rng)
    pf, ucols, _ = check_against_restatement(clicks, arts)
    assert ucols["click_count"].tolist() == [100, 1, 2, 63, 64, 65, 128, 129]
    words = arts["words_count"].to_numpy()
    assert pf.user_raw["avg_word_count"][0].item() == float(words[:91].sum()) / 91
    check_against_restatement(clicks, arts, repair=False)


def test_kahan_path_of_the_mean_timestamp():
    """Five timestamps near 4e15: their sum is past 2^53, so the kernel repeats pandas' compensated loop."""
    rng = np.random.default_rng(6)
    arts = _articles(10, rng)
    ids = arts["click_article_id"].to_numpy()
    big = 4 * 10**15 + np.array([1, 333, 77_777, 5, 999_999_999])
    assert int(big.sum()) > 2**53
    clicks = _clicks([1] * 5 + [2] * 3, ids[:8], np.concatenate([big, BASE_TS + np.arange(3)]), [1] * 8)
    pf, ucols, _ = check_against_restatement(clicks, arts)
    want = clicks.groupby("user_id")["click_timestamp"].mean().to_numpy()
    assert _bits(pf.user_raw["mean_click_time"]) == want.tobytes()


def test_constant_columns_scale_to_zero():
    """Every user with two clicks one second apart on one device: range 0 -> scale 1, every scaled value 0.0;
    every article clicked once: the popularity range is 0 too."""
    rng = np.random.default_rng(7)
    arts = _articles(12, rng)
    ids = arts["click_article_id"].to_numpy()
    user = np.repeat(np.arange(6), 2)
    ts = BASE_TS + np.tile([0, 1000], 6)
    pf, ucols, icols = check_against_restatement(_clicks(user, ids, ts, [3] * 12), arts)
    assert not pf.user_raw["user_click_count"].any() and not pf.user_raw["user_avg_time_gap"].any()
    assert not pf.item_raw["article_popularity"].any() and pf.item_raw["click_count"].cpu().tolist() == [1] * 12


def test_zero_users_and_unknown_rows():
    from nrk.profile import ProfileFeatures

    rng = np.random.default_rng(8)
    arts = _articles(7, rng)
    pf = ProfileFeatures.from_frames(_clicks([], [], [], []), arts, repair_word_lookup=True)
    assert pf.n_users == 0 and all(v.numel() == 0 for v in pf.user_raw.values())
    assert pf.item_raw["article_popularity"].cpu().tolist() == [0.0] * 7
    ut, it, uvoc, ivoc = pf.encoded()
    assert tuple(ut.shape) == (0, 5) and tuple(it.shape) == (7, 4) and uvoc == [1] * 5
    user, items, _, _ = pf.dicts()
    assert user == {} and list(items) == [str(i) for i in arts["click_article_id"].tolist()]
    d = lambda a: torch.tensor(a, dtype=torch.int32).cuda()  # noqa: E731
    assert pf.labels(d([-1, -1]), d([0, -1])).cpu().tolist() == [0, 0]
    assert pf.labels(d([]), d([])).numel() == 0

    # two users; pairs with a -1 user, a -1 item, both, the last click and another article
    ids = arts["click_article_id"].to_numpy()
    clicks = _clicks([5, 5, 9], [ids[1], ids[2], ids[3]], [BASE_TS, BASE_TS + 1, BASE_TS], [1, 1, 2])
    pf, _, _ = check_against_restatement(clicks, arts)
    assert pf.labels(d([0, 0, 1, -1, 0, -1]), d([2, 1, 3, 2, -1, -1])).cpu().tolist() == [1, 0, 1, 0, 0, 0]
    assert pf.labels(d([0, -1, 1]), d([2, 2, -1]), offline=False).cpu().tolist() == [-1, -1, -1]


def test_too_many_device_groups():
    from nrk.profile import ProfileFeatures

    rng = np.random.default_rng(9)
    arts = _articles(5, rng)
    ids = arts["click_article_id"].to_numpy()
    for n, ok in ((64, True), (65, False)):
        clicks = _clicks(np.arange(n) // 2, rng.choice(ids, n), BASE_TS + np.arange(n), np.arange(n) * 3)
        if ok:
            check_against_restatement(clicks, arts)
        else:
            with pytest.raises(NotImplementedError):
                ProfileFeatures.from_frames(clicks, arts)


def test_one_long_user():
    """5,000 clicks over 50 articles: a dedup quadratic in a user's clicks would not finish in the suite's time."""
    rng = np.random.default_rng(10)
    arts = _articles(80, rng)
    ids = arts["click_article_id"].to_numpy()
    item = np.concatenate([ids[:50], rng.choice(ids[:50], 4950)])
    clicks = _clicks([3] * 5000, item, BASE_TS + rng.integers(0, 10**9, 5000), rng.integers(1, 4, 5000), rng)
    pf, _, _ = check_against_restatement(clicks, arts)
    words = arts["words_count"].to_numpy()
    assert pf.user_raw["avg_word_count"].cpu().tolist() == [float(words[:50].sum()) / 50]


def test_encoded_tables_pass_fused_validation(fx):
    from nrk import ops
    from nrk.pipeline import FusedRecallRank
    from nrk.profile import ProfileFeatures
    from test_gpu_din import synth_model

    clicks, arts = rs.frames(fx)
    pf = ProfileFeatures.from_frames(clicks, arts, repair_word_lookup=True)
    ut, it, uvoc, ivoc = pf.encoded()
    rng = np.random.default_rng(11)
    I, T = it.shape[0], 8
    sd, feats = synth_model(rng, uvoc, ivoc, [11] * 16)
    p = ops.DinParams(sd, *feats, table_dtype="bf16")
    cat = ops.Catalog(torch.from_numpy((rng.standard_normal((I, 32)) * 0.1).astype(np.float32)).cuda())
    hist = torch.zeros((ut.shape[0], T), dtype=torch.int32, device="cuda")
    hlen = torch.zeros(ut.shape[0], dtype=torch.int32, device="cuda")
    FusedRecallRank(cat, p, ut, it, hist, hlen, k=30, batch_size=64, chunk_users=64)
    with pytest.raises(ValueError):  # one vocabulary too small: the check does look at these tables
        small = list(uvoc)
        small[1] -= 1
        sd2, feats2 = synth_model(rng, small, ivoc, [11] * 16)
        FusedRecallRank(cat, ops.DinParams(sd2, *feats2, table_dtype="bf16"), ut, it, hist, hlen, k=30,
                        batch_size=64, chunk_users=64)
