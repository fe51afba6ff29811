"""GPU: nrk_ctx_features (csrc/ctxfeat.hip) at every shape the host wrapper
accepts, against oracle.ctx_features on the same dicts.

test_gpu_ctxfeat.py and test_gpu_fused.py run the kernel at one shape
(dc = 250, dw = dy = 64, last_n = 3, groups of at most 30 rows, at most 12
categories).  Here: every pairwise-plan shape and leaf kind of the float64
word_diff (content widths 1..256), last_n 1..4, the scalar and the float4
float32 dots, groups of several 64-row chunks, users with up to 150 history
categories, empty histories, absent users, tables without YouTubeDNN
vectors, pre-grouped calls, and the codes (bin edges, lut zeros, unseen
values, codes-only output).

Bars (every case):
  * score, time_diff_*, word_diff_*, recall_in_user_cat identical to the
    oracle (word_diff: numpy's float64 pairwise norm, which
    test_ctxfeat_host.py pins to the kernel's plan bit for bit).  word_diff
    is returned as a float32, which hides the order of the float64 sum on
    ordinary rows, so the worlds carry tie rows (tie_history_row) whose sum
    sits an ulp or two from a float32 rounding boundary: there another
    order of summation gives the other float32;
  * sim_i and item_user_sim against the float64 dot of the same float32
    vectors: |got - exact| <= (n + 1) * 2^-24 * sum_i |a_i b_i| with n the
    vector width -- a length-n chain of fmas rounds n times, each by at most
    2^-24 of a partial sum that sum|ab| bounds (to first order), and the
    extra 2^-24 sum|ab| covers the second-order terms.  The bound is 0 where
    a vector is absent, so those sims are exactly 0; NaN exactly where the
    oracle has NaN;
  * sim_max / mean / min / std identical to numpy's nan-statistics of the
    kernel's own float32 sims, and within 1e-5 of the oracle's.
"""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle
from test_ctxfeat_host import tie_history_row
from test_ctxfeat_oracle import apply_spec_host

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
F32, F64 = np.float32, np.float64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)


# --- the world ---------------------------------------------------------------

def make_world(dc, dw, dy, last_n, yt=True, n_items=300, n_users=40, n_cat=12, seed=0):
    """The reference's dicts (str ids) with gaps on purpose: items without a
    w2v vector / content row / created time / category / yt vector, all-zero
    content rows, table items with no data at all ("bare*"), item ids outside
    the item table ("zz*", row -1), users absent from the history dict, users
    with an empty history list, users with 1 .. last_n + 2 history items,
    users without a yt vector, user ids outside the user table ("ghost*",
    row -1).  Content components span orders of magnitude; the float32 that
    word_diff is returned as hides the order of its float64 sum on such rows,
    so every world with dc >= 2 also has tie rows, where it does not."""
    rng = np.random.default_rng([seed, dc, dw, dy, last_n])
    ids = [f"a{i * 7 + 3}" for i in range(n_items)]
    keep = lambda frac: [i for i in ids if rng.random() < frac]  # noqa: E731
    w = SimpleNamespace(dc=dc, dw=dw, dy=dy, last_n=last_n, rng=rng, ids=ids)
    w.w2v = {i: (rng.standard_normal(dw) * 0.3).astype(F32) for i in keep(0.9)}
    w.content = {i: rng.standard_normal(dc) * np.exp(rng.standard_normal(dc)) for i in keep(0.9)}
    w.zero_items = list(w.content)[:12]
    for i in w.zero_items:
        w.content[i] = np.zeros(dc)
    w.created = {i: F64(rng.random()) for i in keep(0.9)}
    w.ctype = {i: int(rng.integers(0, n_cat)) for i in keep(0.95)}
    w.art_yt = {i: rng.standard_normal(dy).astype(F32) for i in keep(0.9)} if yt else None
    w.bare = [f"bare{k}" for k in range(5)]
    w.unknown = [f"zz{k}" for k in range(20)]
    w.pool = ids + w.bare + w.unknown
    w.users = [f"u{k}" for k in range(n_users)]
    w.ghosts = ["ghost0", "ghost1"]
    w.hist = {}
    for k, u in enumerate(w.users):
        if k < 2:
            continue  # no history entry
        L = 0 if k < 4 else k - 3 if k < 4 + last_n + 2 else int(rng.integers(1, 10))
        w.hist[u] = [w.pool[j] for j in rng.integers(0, len(w.pool), L)]
    # tie rows (test_ctxfeat_host.tie_history_row): the item "unit" against
    # history rows placed so that the order of the float64 sum decides the
    # float32 word_diff; the large square at the first, an early, the middle
    # and the last element, the sum just above and just below the boundary
    w.extra, w.tie_users, w.tie_wd = [], [], {}
    if dc >= 2:
        w.content["unit"] = np.eye(1, dc)[0]
        for p in sorted({0, min(3, dc - 1), dc // 2, dc - 1}):
            for side in (1, -1):
                h, wd = tie_history_row(dc, p, side, rng)
                w.content[f"tie{len(w.tie_wd)}"] = h
                w.tie_wd[f"tie{len(w.tie_wd)}"] = wd
        ties = list(w.tie_wd)
        w.extra = ["unit"] + ties
        for n in range(len(ties)):
            w.tie_users.append(f"t{n}")
            w.hist[f"t{n}"] = [ties[(n + i) % len(ties)] for i in range(last_n)]
        w.users += w.tie_users
    w.user_yt = {u: rng.standard_normal(dy).astype(F32) for u in w.users if rng.random() < 0.85} if yt else None
    return w


def tables(w):
    from nrk.features import CtxTables

    return CtxTables(w.ids + w.bare + w.extra, w.users, w.w2v, w.content, w.created, w.ctype, w.hist, user_yt=w.user_yt,
                     item_yt=w.art_yt, last_n=w.last_n, device=DEVICE)


def main_rows(w, users, lo=5, hi=31):
    """(user ids, item ids, scores) of a shuffled recall frame."""
    rng = w.rng
    mu, mi = [], []
    for u in users:
        n = int(rng.integers(lo, hi))
        mu += [u] * n
        mi += [w.pool[j] for j in rng.integers(0, len(w.pool), n)]
        if u in w.tie_users:
            mu, mi = mu + [u], mi + ["unit"]
    p = rng.permutation(len(mu))
    return [mu[j] for j in p], [mi[j] for j in p], np.round(rng.random(len(mu)), 3)


def rows_of(tb, users, items):
    urow = tb.user_index.get_indexer(np.array(users, dtype=object)).astype(np.int32)
    irow = tb.item_index.get_indexer(np.array(items, dtype=object)).astype(np.int32)
    return urow, irow


def kernel(tb, users, items, scores, spec=None, **kw):
    from nrk.features import ctx_features

    urow, irow = rows_of(tb, users, items)
    raw, codes = ctx_features(tb, _dev(urow), _dev(irow), _dev(np.asarray(scores, F64)), spec, **kw)
    return (raw.cpu().numpy() if raw is not None else None, codes.cpu().numpy() if codes is not None else None)


# --- the checker -------------------------------------------------------------

def reference(w, users, items, scores):
    return oracle.ctx_features(users, items, np.asarray(scores, F64), w.hist, w.w2v, w.content, w.created, w.ctype,
                               w.user_yt, w.art_yt, last_n=w.last_n, emb_dim=w.dy, content_dim=w.dc, w2v_dim=w.dw)


def dot_terms(a, b):
    """the products a_i b_i of float32 vectors, exact in float64 (rows of a
    against the one vector b)."""
    return a.astype(F64) * b.astype(F64)[None]


def exact_dots(w, users, items):
    """float64 dots of the float32 vectors behind sim_i [n, N] and
    item_user_sim [n], with the derived bounds (0 where the reference defines
    the value as 0)."""
    n, N = len(items), w.last_n
    ex, bd = np.zeros((n, N)), np.zeros((n, N))
    exy, bdy = np.zeros(n), np.zeros(n)
    zw, zy = np.zeros(w.dw, F32), np.zeros(w.dy, F32)
    iv = np.array([w.w2v.get(i, zw) for i in items], F32)
    ua = np.array(users, dtype=object)
    for u in dict.fromkeys(users):
        if u not in w.hist:
            continue
        rows = np.flatnonzero(ua == u)
        for k, h in enumerate(w.hist[u][-N:]):
            hv = w.w2v.get(h)
            if hv is not None:
                p = dot_terms(iv[rows], hv)
                ex[rows, k] = p.sum(1)
                bd[rows, k] = (w.dw + 1) * 2.0 ** -24 * np.abs(p).sum(1)
        if w.user_yt is not None and u in w.user_yt:
            p = dot_terms(np.array([w.art_yt.get(items[r], zy) for r in rows], F32), w.user_yt[u])
            exy[rows] = p.sum(1)
            bdy[rows] = (w.dy + 1) * 2.0 ** -24 * np.abs(p).sum(1)
    return ex, bd, exy, bdy


def check_raw(w, users, items, scores, raw, exp=None):
    from nrk.features import ctx_feature_names

    names = ctx_feature_names(w.last_n)
    N = w.last_n
    assert raw.shape == (len(items), len(names)) and raw.dtype == F64
    exp = reference(w, users, items, scores) if exp is None else exp
    col = lambda f: raw[:, names.index(f)]  # noqa: E731
    exact = ["score", "recall_in_user_cat"] + [f"{p}_{i}" for i in range(1, N + 1) for p in ("time_diff", "word_diff")]
    for f in exact:
        got, e = col(f), exp[f].astype(F64)
        bad = np.flatnonzero(~((got == e) | (np.isnan(got) & np.isnan(e))))
        assert bad.size == 0, (f, bad.size, bad[:4].tolist(), got[bad][:4].tolist(), e[bad][:4].tolist())
    ex, bd, exy, bdy = exact_dots(w, users, items)
    for i in range(N):
        got, e = col(f"sim_{i + 1}"), exp[f"sim_{i + 1}"]
        assert np.array_equal(np.isnan(got), np.isnan(e)), f"sim_{i + 1}: NaN rows"
        m = ~np.isnan(e)
        bad = np.flatnonzero(m & ~(np.abs(got - ex[:, i]) <= bd[:, i]))
        assert bad.size == 0, (f"sim_{i + 1}", bad.size, got[bad][:4].tolist(), ex[bad, i][:4].tolist(),
                               bd[bad, i][:4].tolist())
        # the bound holds for any order of summation, the oracle's sgemv included
        assert (np.abs(e[m] - ex[m, i]) <= bd[m, i]).all(), f"sim_{i + 1}: the oracle misses the bound"
    got, e = col("item_user_sim"), exp["item_user_sim"]
    bad = np.flatnonzero(~(np.abs(got - exy) <= bdy))
    assert bad.size == 0, ("item_user_sim", bad.size, got[bad][:4].tolist(), exy[bad][:4].tolist())
    assert (np.abs(e - exy) <= bdy).all(), "item_user_sim: the oracle misses the bound"
    if w.user_yt is None:
        assert (got == 0).all()
    sims = np.stack([col(f"sim_{i + 1}") for i in range(N)], 1)
    assert np.array_equal(sims.astype(F32).astype(F64), sims, equal_nan=True)  # the sims are float32 values
    sims = sims.astype(F32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = [np.nanmax(sims, 1), np.nanmean(sims, 1), np.nanmin(sims, 1), np.nanstd(sims, 1)]
    for j, f in enumerate(("sim_max", "sim_mean", "sim_min", "sim_std")):
        got = col(f)
        assert st[j].dtype == F32
        bad = np.flatnonzero(~((got == st[j]) | (np.isnan(got) & np.isnan(st[j]))))
        assert bad.size == 0, (f, sims[bad][:4].tolist(), got[bad][:4].tolist(), st[j][bad][:4].tolist())
        np.testing.assert_allclose(got, exp[f], rtol=1e-5, atol=1e-5, equal_nan=True, err_msg=f)
    return exp


def run_world(dc, dw, dy, last_n, yt=True):
    w = make_world(dc, dw, dy, last_n, yt=yt)
    tb = tables(w)
    assert (tb.dc, tb.dw, tb.dy, tb.last_n) == (dc, dw, dy if yt else 0, last_n)
    users, items, scores = main_rows(w, w.users + w.ghosts)
    raw, codes = kernel(tb, users, items, scores)
    assert codes is None
    exp = check_raw(w, users, items, scores, raw)
    # the case has what it is for: live word_diffs and sims, NaN sims, users
    # with fewer history items than last_n (when last_n > 1), unknown items
    assert (exp["word_diff_1"] > 0).sum() > 100 and (np.nan_to_num(exp["sim_1"]) != 0).sum() > 100
    assert np.isnan(exp[f"sim_{last_n}"]).any() and not np.isnan(exp[f"sim_{last_n}"]).all()
    assert (rows_of(tb, users, items)[1] < 0).any() and (rows_of(tb, users, items)[0] < 0).any()
    # the tie rows are there, and the oracle gives them what the restated plan gives
    ties = [r for r, (u, i) in enumerate(zip(users, items)) if i == "unit" and u in w.tie_users]
    assert len(ties) == len(w.tie_users) and (dc < 2) == (not ties)
    for r in ties:
        for k, h in enumerate(w.hist[users[r]]):
            assert exp[f"word_diff_{k + 1}"][r] == w.tie_wd[h]
    return w, raw


# --- cases -------------------------------------------------------------------

# 1, 5, 7: a tail-only leaf; 8, 16: no tail; 9, 15: a leaf and its tail; 128:
# the largest single leaf; 129: the first split (64, 65); 136 / 137: (64, 72) /
# (64, 73); 248: the last two-leaf width (120, 128); 249: the first
# three-leaf width (120, 64, 65); 250: (120, 64, 66); 255: (120, 64, 71); 256:
# (128, 128)
@pytest.mark.parametrize("dc", [1, 5, 7, 8, 9, 15, 16, 63, 64, 127, 128, 129, 136, 137, 200, 248, 249, 250, 255, 256])
def test_content_widths(dc):
    run_world(dc, 64, 64, 3)


@pytest.mark.parametrize("dc", [40, 250, 256])
@pytest.mark.parametrize("last_n", [1, 2, 4])
def test_last_n(last_n, dc):
    w, raw = run_world(dc, 64, 64, last_n)
    assert raw.shape[1] == 1 + 3 * last_n + 6
    # history lengths below, at and above last_n
    lens = {len(h) for h in w.hist.values()}
    assert 0 in lens and last_n in lens and last_n + 2 in lens and (last_n == 1 or last_n - 1 in lens)


@pytest.mark.parametrize("dw, dy", [(1, 1), (3, 6), (4, 16), (30, 33), (50, 1), (100, 6), (127, 16), (128, 33)])
def test_dot_widths(dw, dy):
    run_world(40, dw, dy, 3)


def test_no_yt_tables():
    w, raw = run_world(40, 30, 64, 3, yt=False)
    assert (raw[:, -2] == 0).all()  # item_user_sim


GROUP_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200]


@pytest.mark.parametrize("dc", [250, 9])
def test_group_sizes(dc):
    """Groups of one to four 64-row chunks, 9 groups (not a multiple of the
    4 a workgroup takes), once through the default stable sort (pair_pos set,
    rows interleaved) and once pre-grouped (pair_pos null); an all-zero
    content row and an unknown item at chunk positions 0, 63, 64 and in the
    last row (alone in its chunk for 65 and 129, the odd row of a half-wave
    pair for 1, 63, 65, 127, 129)."""
    w = make_world(dc, 64, 64, 3)
    rng = w.rng
    gu = [f"g{k}" for k in range(len(GROUP_SIZES))]
    live = [i for i in w.ids if i in w.w2v and i in w.content and i not in w.zero_items]
    for k, u in enumerate(gu):
        w.users.append(u)
        w.hist[u] = [live[j] for j in rng.integers(0, len(live), k % 5)] + [f"tie{k % len(w.tie_wd)}"]
        w.user_yt[u] = rng.standard_normal(w.dy).astype(F32)
    tb = tables(w)
    users, items = [], []
    for k, (u, n) in enumerate(zip(gu, GROUP_SIZES)):
        its = [w.pool[j] for j in rng.integers(0, len(w.pool), n)]
        special = [w.zero_items[k], w.unknown[k]]
        for t, pos in enumerate((0, 63, 64, n - 1)):
            if pos < n:
                its[pos] = special[(k + t) % 2]
        for pos in (1, 62, 66, n - 2):  # tie rows: both rows of a half-wave pair, either side of a chunk edge
            if 0 < pos < n - 1 and pos not in (63, 64):
                its[pos] = "unit"
        users += [u] * n
        items += its
    scores = np.round(rng.random(len(items)), 3)
    # every (special, position) pair occurs
    off = np.concatenate([[0], np.cumsum(GROUP_SIZES)])
    for kind in (w.zero_items, w.unknown):
        for pos in (0, 63, 64, -1):
            assert any(items[off[k] + (pos if pos >= 0 else n - 1)] in kind
                       for k, n in enumerate(GROUP_SIZES) if pos < n)
    from nrk.features import ctx_features

    urow, irow = rows_of(tb, users, items)
    # pre-grouped, groups in a user order that is not sorted
    order = rng.permutation(len(gu))
    go = np.concatenate([[0], np.cumsum(np.array(GROUP_SIZES)[order])]).astype(np.int64)
    idx = np.concatenate([np.arange(off[k], off[k + 1]) for k in order])
    assert np.array_equal(urow[idx], np.repeat(urow[off[:-1]][order], np.array(GROUP_SIZES)[order]))
    raw, _ = ctx_features(tb, _dev(urow[idx]), _dev(irow[idx]), _dev(scores[idx]),
                          groups=(_dev(go), _dev(urow[off[:-1]][order].astype(np.int32)), None))
    exp = check_raw(w, [users[j] for j in idx], [items[j] for j in idx], scores[idx], raw.cpu().numpy())
    assert (exp["word_diff_1"] > 0).sum() > 500
    ties = [r for r, j in enumerate(idx) if items[j] == "unit"]
    assert len(ties) == 22
    for r in ties:
        h = w.hist[users[idx[r]]][-3:]
        assert exp[f"word_diff_{len(h)}"][r] == w.tie_wd[h[-1]]
    # ungrouped: the users interleaved, each user's rows in their order
    lab = rng.permutation(np.repeat(np.arange(len(gu)), GROUP_SIZES))
    sh = np.empty(len(items), np.int64)
    for k in range(len(gu)):
        sh[lab == k] = np.arange(off[k], off[k + 1])
    inv = np.empty(len(idx), np.int64)
    inv[idx] = np.arange(len(idx))  # grouped-layout row of each original row
    raw2, _ = ctx_features(tb, _dev(urow[sh]), _dev(irow[sh]), _dev(scores[sh]))
    raw2 = raw2.cpu().numpy()
    check_raw(w, [users[j] for j in sh], [items[j] for j in sh], scores[sh], raw2,
              exp={f: v[inv[sh]] for f, v in exp.items()})
    # the same rows give the same bits in both layouts
    assert np.array_equal(raw2, raw.cpu().numpy()[inv[sh]], equal_nan=True)


def user_cats(hist, ctype):
    """the distinct categories of a history, in first-seen order (:497-506)."""
    return list(dict.fromkeys(ctype[i] for i in hist if i in ctype))


N_CATS = [0, 1, 63, 64, 65, 150]


def test_category_counts():
    """Users with 0, 1, 63, 64, 65 and 150 distinct history categories (up to
    64 are held one per lane, more are read from memory per row); recalled
    items in the user's first, 64th, 65th and last category, in an absent
    one, and without a category."""
    w = make_world(40, 64, 64, 3, n_items=400, n_cat=200)
    rng = w.rng
    w.ctype = {i: k % 200 for k, i in enumerate(w.ids) if k < 200 or rng.random() < 0.8}
    by_cat = {}
    for i, c in w.ctype.items():
        by_cat.setdefault(c, []).append(i)
    nocat = [i for i in w.ids if i not in w.ctype] + w.bare
    cu = [f"c{k}" for k in N_CATS]
    want = {}
    for u, k in zip(cu, N_CATS):
        cats = rng.permutation(200)[:k].tolist()
        h = []
        for c in cats:
            h.append(by_cat[c][int(rng.integers(len(by_cat[c])))])
            if rng.random() < 0.2:
                h.append(nocat[int(rng.integers(len(nocat)))])
        h += [h[j] for j in rng.integers(0, len(h), 3)] if h else [nocat[0], nocat[1]]
        w.users.append(u)
        w.hist[u] = h
        w.user_yt[u] = rng.standard_normal(w.dy).astype(F32)
        want[u] = cats
        assert user_cats(h, w.ctype) == cats
    tb = tables(w)
    users, items, hit = [], [], []
    for u, k in zip(cu, N_CATS):
        cats = user_cats(w.hist[u], w.ctype)
        its = [(by_cat[cats[j]][-1], 1) for j in (0, 63, 64, k - 1) if 0 <= j < k]
        absent = next(c for c in range(200) if c not in want[u])
        its += [(by_cat[absent][0], 0), (nocat[-1], 0), (nocat[0], 0), (w.unknown[0], 0)]
        for j in rng.integers(0, len(w.ids), 40):
            its.append((w.ids[j], int(w.ctype.get(w.ids[j], -1) in cats)))
        its = [its[j] for j in rng.permutation(len(its))]
        users += [u] * len(its)
        items += [i for i, _ in its]
        hit += [h for _, h in its]
    scores = np.round(rng.random(len(items)), 3)
    raw, _ = kernel(tb, users, items, scores)
    exp = check_raw(w, users, items, scores, raw)
    hit = np.array(hit, F64)
    assert np.array_equal(raw[:, -1], hit)
    assert np.array_equal(exp["recall_in_user_cat"].astype(F64), hit)
    ua = np.array(users)
    for u, k in zip(cu, N_CATS):
        assert hit[ua == u].sum() >= min(k, 1) and (hit[ua == u] == 0).sum() >= 4
    ncat = np.diff(tb.t["ucat_off"].cpu().numpy())
    assert ncat[-len(cu):].tolist() == N_CATS


def test_absent_users():
    """A block of rows whose user is outside the user table (row -1) and one
    whose user has no history entry: NaN sims and statistics, zeros
    elsewhere, the score passed through."""
    from nrk.features import ctx_feature_names

    w = make_world(250, 64, 64, 3)
    tb = tables(w)
    users, items, scores = main_rows(w, ["ghost0"] * 4 + w.users[:2] * 3 + w.users[4:8], lo=40, hi=90)
    urow, _ = rows_of(tb, users, items)
    raw, _ = kernel(tb, users, items, scores)
    check_raw(w, users, items, scores, raw)
    names = ctx_feature_names(3)
    gone = np.array([u not in w.hist for u in users])
    assert (urow[gone] < 0).sum() > 64 and (urow[gone] >= 0).sum() > 64 and (~gone).sum() > 64
    nan_cols = [k for k, f in enumerate(names) if f.startswith("sim_")]
    zero_cols = [k for k, f in enumerate(names) if not f.startswith("sim_") and f != "score"]
    assert np.isnan(raw[gone][:, nan_cols]).all()
    assert (raw[gone][:, zero_cols] == 0).all()
    assert np.array_equal(raw[:, 0], scores)
    assert not np.isnan(raw[~gone][:, names.index("sim_1")]).any()


def hand_spec(names, raw, left_out):
    """A CtxSpec filled by hand from the kernel's own raw columns: binned
    features whose inner edges are values of the column (rows sit exactly on
    an edge), the NaN fill on an edge, a lut with a 0 entry; score (rounded
    to one decimal) and recall_in_user_cat by exact value, with ``left_out``
    values missing from the table (unseen -> 0)."""
    from nrk.features import CtxSpec, CtxSpecC

    specs = []
    for k, f in enumerate(names):
        sp = CtxSpecC()
        v = raw[:, k]
        if f in ("score", "recall_in_user_cat"):
            vals = [x for x in np.unique(v).tolist() if x not in left_out[f]]
            sp.kind, sp.n_vals = 1, len(vals)
            for j, x in enumerate(vals):
                sp.vals[j], sp.codes[j] = x, 3 + 2 * j
        else:
            u = np.unique(v[~np.isnan(v)])
            edges = u[np.unique(np.linspace(0, len(u) - 1, min(len(u), 9)).astype(int))] if len(u) else u
            sp.kind, sp.n_edges, sp.n_lut = 0, len(edges), len(edges) + 1
            sp.edges[:len(edges)] = edges.tolist()
            sp.fill = float(edges[len(edges) // 2]) if len(edges) else 0.0
            for b in range(sp.n_lut):
                sp.lut[b] = 0 if b == 2 else 5 + b
        specs.append(sp)
    return CtxSpec(specs, names)


@pytest.mark.parametrize("last_n", [3, 1])
def test_codes(last_n):
    from nrk.features import CtxSpec, ctx_feature_names

    w = make_world(40, 64, 64, last_n)
    tb = tables(w)
    names = ctx_feature_names(last_n)
    F = len(names)
    users, items, scores = main_rows(w, w.users + w.ghosts)
    scores = np.round(scores, 1)
    raw0, _ = kernel(tb, users, items, scores)
    check_raw(w, users, items, scores, raw0)
    left_out = {"score": [0.3], "recall_in_user_cat": [0.0]}
    hand = hand_spec(names, raw0, left_out)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fitted = CtxSpec.fit({f: (raw0[:, j].astype(F32) if f != "score" else raw0[:, j])
                              for j, f in enumerate(names)}, names)
    assert {sp.kind for sp in fitted.specs} == {0, 1}
    for spec in (hand, fitted):
        raw, codes = kernel(tb, users, items, scores, spec)
        assert np.array_equal(raw, raw0, equal_nan=True)
        assert codes.shape == (len(items), F) and codes.dtype == np.int32
        for k, f in enumerate(names):
            assert np.array_equal(codes[:, k], apply_spec_host(spec.specs[k], raw[:, k])), f
        # codes only, into the caller's tensor (the fused pipeline's call)
        out = torch.full((len(items), F), -7, dtype=torch.int32, device=DEVICE)
        r2, c2 = kernel(tb, users, items, scores, spec, raw=False, out_codes=out)
        assert r2 is None and np.array_equal(c2, codes) and np.array_equal(out.cpu().numpy(), codes)
    # the hand-built spec, spelled out (codes holds the hand spec's last)
    raw, codes = kernel(tb, users, items, scores, hand)
    on_edge = nan_rows = 0
    for k, f in enumerate(names):
        sp, v, c = hand.specs[k], raw[:, k], codes[:, k]
        if sp.kind == 1:
            for x in left_out[f]:
                assert (v == x).any() and (c[v == x] == 0).all(), f  # an unseen value codes 0
            for j in range(sp.n_vals):
                assert (c[v == sp.vals[j]] == sp.codes[j]).all(), f
            continue
        for j in range(sp.n_edges):  # a row on an edge lands in the upper bin
            m = v == sp.edges[j]
            assert m.any() and (c[m] == sp.lut[j + 1]).all(), (f, j)
            on_edge += int(m.sum())
        if sp.n_edges:
            below = v < sp.edges[0]
            assert (c[below] == sp.lut[0]).all(), f
            m = np.isnan(v)  # NaN takes the fill, which sits on edge n_edges // 2
            assert (c[m] == sp.lut[sp.n_edges // 2 + 1]).all(), f
            nan_rows += int(m.sum())
        if sp.n_lut > 2:
            assert (c == 0).any(), f  # the lut's 0 entry is hit
    assert on_edge > 100 and nan_rows > 50
