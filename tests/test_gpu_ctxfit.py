"""GPU: CtxSpec.fit_device (nrk_ctx_fit_stats / nrk_ctx_fit_count_below,
csrc/ctxfit.hip) against the numpy restatement (tests/ctxfit_restated.py), the
host fit (CtxSpec.fit) and the reference's own run (tests/golden/ctxfeat_small).

Bar everywhere: equal.  The device does integer comparison and selection only,
plus one add-and-halve whose contraction is off; the host finish is numpy's own
arithmetic.  Floats are compared with ==."""
import warnings

import numpy as np
import pytest
import torch

import ctxfit_restated as R

pytestmark = pytest.mark.gpu

F64_BITS = lambda b: np.asarray(b, np.uint64).view(np.float64)  # noqa: E731


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host_fit(raw, names, kinds, **kw):
    from nrk.features import CtxSpec

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CtxSpec.fit(R.typed_columns(raw, names, kinds), names, **kw)


# ---------------------------------------------------------------- fixture --
def test_fit_device_on_the_reference_fixture(golden):
    from nrk.features import CtxSpec, CtxTables, ctx_features
    from test_ctxfeat_oracle import ctx_inputs

    g = golden("ctxfeat_small")
    names = g["ctx_feats"].tolist()
    raw = np.stack([g[f"raw::{f}"].astype(np.float64) for f in names], 1)
    assert raw.shape == (4643, 16)
    spec = CtxSpec.fit_device(_dev(raw), names)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = CtxSpec.fit({f: g[f"raw::{f}"] for f in names}, names)
    R.assert_specs_equal(spec, exp)
    R.assert_specs_equal(spec, R.restated_spec(raw, names))
    for k, f in enumerate(names):
        sp = spec.specs[k]
        if f"edges::{f}" in g.files:
            assert sp.kind == 0 and list(sp.edges[:sp.n_edges]) == g[f"edges::{f}"][1:-1].tolist(), f
        # the spec applied to the reference's raw values gives the reference's codes
        assert np.array_equal(R.apply_spec_host(sp, raw[:, k]), g["codes"][:, k]), f
    # ... and so does nrk_ctx_features with it, on every row whose own raw values are the
    # reference's (the float32 dots differ in the last ulp on a few: tests/test_gpu_ctxfeat.py)
    d = ctx_inputs(g)
    mu, mi = g["in::main::user_id"].tolist(), g["in::main::item_id"].tolist()
    item_ids = list(dict.fromkeys(list(d["w2v"]) + list(d["content"]) + list(d["created"]) + list(d["ctype"])
                                  + list(d["art_yt"]) + mi))
    user_ids = list(dict.fromkeys(mu + list(d["hist"])))
    tb = CtxTables(item_ids, user_ids, d["w2v"], d["content"], d["created"], d["ctype"], d["hist"],
                   user_yt=d["user_yt"], item_yt=d["art_yt"])
    urow = tb.user_index.get_indexer(np.array(mu, dtype=object)).astype(np.int32)
    irow = tb.item_index.get_indexer(np.array(mi, dtype=object)).astype(np.int32)
    raw_d, codes = ctx_features(tb, _dev(urow), _dev(irow), _dev(g["in::main::score"]), spec)
    raw_d, codes = raw_d.cpu().numpy(), codes.cpu().numpy()
    same = ((raw_d == raw) | (np.isnan(raw_d) & np.isnan(raw))).all(1)
    assert same.sum() > 500
    assert np.array_equal(codes[same], g["codes"][same])
    for k, f in enumerate(names):
        assert np.array_equal(codes[:, k], R.apply_spec_host(exp.specs[k], raw_d[:, k])), f


# ------------------------------------------------- stats at the boundaries --
KINDS = [0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 2, 0]


def _recipe(r, n, rng):
    """column recipe r (kind KINDS[r]) over n rows."""
    if r == 0:  # values that differ in the low mantissa byte only
        return F64_BITS(np.uint64(0x3FF8000000000000) | rng.integers(0, 256, n).astype(np.uint64))
    if r == 1:  # every digit, both signs
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)
        idx = np.arange(0, n - 1, 5)
        v[idx] = -v[idx + 1]  # pairs that differ in the sign only
        return v
    if r == 2:  # one value on 90 % of the rows
        return np.where(rng.random(n) < 0.9, 0.25, rng.standard_normal(n))
    if r in (3, 4):  # exactly 20 / 21 distinct values (when n allows): the bin / no-bin switch
        m = 20 + (r - 3)
        v = rng.integers(0, m, n).astype(np.float64)
        v[:min(n, m)] = np.arange(min(n, m))
        return rng.permutation(v).astype(np.float32).astype(np.float64) / 4
    if r == 5:
        return np.full(n, np.nan)
    if r == 6:  # one NaN
        v = rng.standard_normal(n)
        v[n // 2] = np.nan
        return v
    if r == 7:  # -0.0 beside 0.0
        return rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, -1.0, 1.0, 5e-324, -5e-324]), n)
    if r == 8:  # float32 column: an even-count median is (a + b) / 2 rounded to float32, no column value
        return rng.standard_normal(n).astype(np.float32).astype(np.float64)
    if r == 9:  # float32, half NaN
        v = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        v[rng.permutation(n)[:n // 2]] = np.nan
        return v
    if r == 10:  # integers
        return rng.integers(-3, 40, n).astype(np.float64)
    v = rng.standard_normal(n)  # +inf among the values
    v[::4] = np.inf
    return v


@pytest.mark.parametrize("F", [1, 16, 17])
@pytest.mark.parametrize("n_off", [("1", 1), ("2", 2), ("21", 21), ("T-1", -1), ("T", 0), ("T+1", 1), ("3T+5", 5)],
                         ids=lambda p: p[0])
def test_stats_at_the_sort_boundaries(n_off, F):
    from nrk import _lib
    from nrk.features import FIT_COL_DTYPE, _finish_edges, ctx_fit_count_below, ctx_fit_stats, fit_stats_host

    T = _lib.lib().nrk_ctx_fit_tile()
    label, off = n_off
    n = off if label in ("1", "2", "21") else (3 * T + off if label == "3T+5" else T + off)
    rng = np.random.default_rng(n * 31 + F)
    rec = [(c + (1 if F == 1 else 0)) % 12 for c in range(F)]
    ld = F + 3
    store = np.full((n, ld), 777.0)  # the padding columns are never read as data
    for c, r in enumerate(rec):
        store[:, c] = _recipe(r, n, rng)
    raw = store[:, :F]
    cols = list(rng.permutation(F)) if F == 1 else [int(c) for c in rng.permutation(F)[:F - 2]]
    kinds = [KINDS[rec[c]] for c in cols]
    ranks = np.arange(n) if n <= 64 else _finish_edges(None, n, 17, 0)
    store_d = _dev(store)
    raw_d = store_d[:, :F]
    assert raw_d.stride(0) == ld or n == 1
    need = _lib.lib().nrk_ctx_fit_workspace_bytes(n, len(cols))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stats, picks = ctx_fit_stats(raw_d if n > 1 else raw_d.contiguous(), cols, kinds, ranks, workspace=ws)
    stats, picks = fit_stats_host(stats), picks.cpu().numpy()
    exp_stats, exp_picks = R.restated_stats(raw, cols, kinds, ranks)
    assert set(FIT_COL_DTYPE.names) == set(R.FIELDS)
    for j, c in enumerate(cols):
        for f in R.FIELDS:
            got, exp = stats[j][f], exp_stats[j][f]
            assert not np.isnan(exp_stats[j]["fill"])
            assert np.array_equal(np.asarray(got), np.asarray(exp)), (label, F, c, rec[c], f, got, exp)
        assert np.array_equal(picks[j], exp_picks[j]), (label, F, c, rec[c], picks[j], exp_picks[j])
    assert np.array_equal(store_d.cpu().numpy(), store, equal_nan=True)  # the input is not written
    # counts below a few probes per column, on the workspace the sort left
    probes = np.stack([np.concatenate([exp_picks[j][:3], [np.nan, -np.inf, np.inf, 0.0, 0.3]]) for j in range(len(cols))])
    below = ctx_fit_count_below(n, len(cols), _dev(probes), ws).cpu().numpy()
    for j, c in enumerate(cols):
        v = raw[:, c]
        valid = np.sort(v[~np.isnan(v)])
        exp = [0 if np.isnan(p) else int(np.searchsorted(valid, p, "left")) for p in probes[j]]
        assert below[j].tolist() == exp, (label, F, c, rec[c])


# ------------------------------------------------------- the fitted specs --
def test_unbinned_columns():
    from nrk.features import CtxSpec

    rng = np.random.default_rng(3)
    n = 3001
    ints = rng.integers(0, 2, n).astype(np.float64)
    five = rng.choice(np.array([0.1, 0.5, 2.0, -1.25, 3.0], np.float32), n).astype(np.float64)
    five[rng.permutation(n)[:300]] = np.nan
    five0 = rng.choice(np.array([0.0, 0.5, 2.0], np.float32), n).astype(np.float64)  # the fillna(0) class is a value
    five0[::9] = np.nan
    allnan = np.full(n, np.nan)
    f64 = rng.choice(np.array([0.1, 1 / 3, 7.0]), n)
    raw = np.stack([ints, five, allnan, five0, f64], 1)
    names, kinds = ["ints", "five", "allnan", "five0", "f64"], [2, 1, 1, 1, 0]
    got = CtxSpec.fit_device(_dev(raw), names, kinds=kinds)
    exp = _host_fit(raw, names, kinds)
    assert [sp.kind for sp in got.specs] == [1] * 5
    R.assert_specs_equal(got, exp, probe=[0.1, np.float32(0.1), 1.0, 2.0, 1 / 3])
    for c in range(5):
        assert np.array_equal(R.apply_spec_host(got.specs[c], raw[:, c]), R.apply_spec_host(exp.specs[c], raw[:, c]))


def test_refusals():
    from nrk.features import CtxSpec

    rng = np.random.default_rng(4)
    n = 500
    raw = rng.standard_normal((n, 2)).astype(np.float32).astype(np.float64)
    names = ["a", "b"]
    d = _dev(raw)
    with pytest.raises(NotImplementedError, match="CtxSpec.fit"):
        CtxSpec.fit_device(d, names, kinds=[1, 1], n_bins=18)
    with pytest.raises(NotImplementedError, match="CtxSpec.fit"):
        CtxSpec.fit_device(d, names, kinds=[1, 1], strategy="kmeans")
    bad = raw.copy()
    bad[7, 1] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        CtxSpec.fit_device(_dev(bad), names, kinds=[1, 1])
    bad = raw.copy()
    bad[7, 0] = 0.1  # the float64 0.1 is no float32
    with pytest.raises(ValueError, match="float32"):
        CtxSpec.fit_device(_dev(bad), names, kinds=[1, 1])
    CtxSpec.fit_device(_dev(bad), names, kinds=[0, 1])  # as a float64 column it is fine
    ints = np.stack([rng.integers(0, 50, n), rng.integers(0, 3, n)], 1).astype(np.float64)
    with pytest.raises(NotImplementedError, match="CtxSpec.fit"):
        CtxSpec.fit_device(_dev(ints), names, kinds=[2, 2])  # 50 values: binned in the integer dtype
    CtxSpec.fit_device(_dev(ints), names, kinds=[0, 2])
    with pytest.raises(ValueError, match="int64"):
        CtxSpec.fit_device(d, names, kinds=[2, 1])
    with pytest.raises(ValueError):
        CtxSpec.fit_device(d, names + ["c"])
    with pytest.raises(ValueError, match="workspace_bytes"):
        CtxSpec.fit_device(d, names, workspace_bytes=100)


@pytest.mark.parametrize("n_bins", [10, 5])
def test_uniform_strategy(n_bins):
    from nrk.features import CtxSpec

    rng = np.random.default_rng(6)
    n = 5000
    raw = np.stack([rng.standard_normal(n), rng.standard_normal(n).astype(np.float32).astype(np.float64),
                    np.concatenate([rng.random(n - 2), [50.0, 100.0]])], 1)  # the last one leaves bins empty
    raw[::11, 1] = np.nan
    names, kinds = ["a", "b", "skew"], [0, 1, 0]
    got = CtxSpec.fit_device(_dev(raw), names, kinds=kinds, n_bins=n_bins, strategy="uniform")
    exp = _host_fit(raw, names, kinds, n_bins=n_bins, strategy="uniform")
    R.assert_specs_equal(got, exp)
    assert [sp.kind for sp in got.specs] == [0, 0, 0]
    assert 0 in list(got.specs[2].lut[:got.specs[2].n_lut])


def test_quantile_bins_without_rows():
    from nrk.features import CtxSpec

    rng = np.random.default_rng(8)
    ties = np.concatenate([np.zeros(160), np.ones(210), 1 + rng.random(30) * 2]).astype(np.float32)
    raw = rng.permutation(ties).astype(np.float64)[:, None]
    got = CtxSpec.fit_device(_dev(raw), ["ties"], kinds=[1])
    R.assert_specs_equal(got, _host_fit(raw, ["ties"], [1]))
    assert 0 in list(got.specs[0].lut[:got.specs[0].n_lut])


def test_column_groups(golden):
    from nrk import _lib
    from nrk.features import CtxSpec

    g = golden("ctxfeat_small")
    names = g["ctx_feats"].tolist()
    raw = _dev(np.stack([g[f"raw::{f}"].astype(np.float64) for f in names], 1))
    n = raw.shape[0]
    L = _lib.lib()
    one = CtxSpec.fit_device(raw, names)
    for per in (1, 5):
        ws = L.nrk_ctx_fit_workspace_bytes(n, per)
        assert ws < L.nrk_ctx_fit_workspace_bytes(n, per + 1)
        spec = CtxSpec.fit_device(raw, names, workspace_bytes=ws)
        assert bytes(spec._host) == bytes(one._host), per
    # a row stride is allowed
    wide = torch.full((n, 20), 5.0, dtype=torch.float64, device="cuda")
    wide[:, :16] = raw
    assert bytes(CtxSpec.fit_device(wide[:, :16], names)._host) == bytes(one._host)


# ----------------------------------------------------------------- fused --
def _world(rng, U, I, D, T, vu, vi):
    users = rng.standard_normal((U, D)).astype(np.float32)
    users /= np.linalg.norm(users, axis=1, keepdims=True)
    items = rng.standard_normal((I, D)).astype(np.float32)
    items /= np.linalg.norm(items, axis=1, keepdims=True)
    user_feat = np.stack([rng.integers(0, v, U) for v in vu], 1).astype(np.int32)
    item_feat = np.stack([rng.integers(0, v, I) for v in vi], 1).astype(np.int32)
    user_hist = rng.integers(0, I, (U, T)).astype(np.int32)
    hist_len = rng.integers(0, T + 1, U).astype(np.int32)
    return users, items, user_feat, item_feat, user_hist, hist_len


def _ctx_world(rng, users, items, user_hist, hist_len, n_cat=12):
    I, U = len(items), len(users)
    w2v = {str(i): (rng.standard_normal(64) * 0.3).astype(np.float32) for i in range(I) if rng.random() < 0.9}
    content = {str(i): rng.standard_normal(250) for i in range(I) if rng.random() < 0.9}
    for key in list(content)[:20]:
        content[key] = np.zeros(250)
    created = {str(i): np.float64(rng.random()) for i in range(I) if rng.random() < 0.9}
    ctype = {str(i): int(rng.integers(0, n_cat)) for i in range(I)}
    hist = {str(u): [str(x) for x in user_hist[u, :hist_len[u]]] for u in range(U) if hist_len[u] > 0}
    user_yt = {str(u): users[u] for u in range(U)}
    art_yt = {str(i): items[i] for i in range(I)}
    return w2v, content, created, ctype, hist, user_yt, art_yt


def test_fused_fit_ctx():
    """FusedRecallRank.fit_ctx over the recalled pairs equals CtxSpec.fit of
    the same raw rows on the host (21,000 rows: the host fit does not
    subsample), whatever the chunking; max_users fits on the first users."""
    from nrk import ops
    from nrk.features import CtxTables, ctx_feature_names, ctx_features, default_ctx_kinds
    from nrk.pipeline import FusedRecallRank
    from test_gpu_din import synth_model

    rng = np.random.default_rng(41)
    U, I, D, T, k = 700, 1500, 64, 50, 30
    vu, vi, vc = [50, 300, 7, 2000, 90], [60, 900, 5000, 70], [24] * 16
    users, items, user_feat, item_feat, user_hist, hist_len = _world(rng, U, I, D, T, vu, vi)
    w2v, content, created, ctype, hist, user_yt, art_yt = _ctx_world(rng, users, items, user_hist, hist_len)
    tables = CtxTables([str(i) for i in range(I)], [str(u) for u in range(U)], w2v, content, created, ctype, hist,
                       user_yt=user_yt, item_yt=art_yt)
    sd, feats = synth_model(rng, vu, vi, vc)
    p = ops.DinParams(sd, *feats, table_dtype="bf16")
    names = ctx_feature_names()
    kinds = default_ctx_kinds(names)
    specs = {}
    for chunk, bs in ((2048, 4096), (128, 3840)):  # one chunk; five full chunks and a partial one
        fused = FusedRecallRank(ops.Catalog(_dev(items)), p, _dev(user_feat), _dev(item_feat), _dev(user_hist),
                                _dev(hist_len), k=k, chunk_users=chunk, batch_size=bs)
        s, r = fused.recall(_dev(users))
        specs[chunk] = fused.fit_ctx(tables, s, r)
        part = fused.fit_ctx(tables, s, r, n_bins=7, max_users=300)
    pu = np.repeat(np.arange(U), k).astype(np.int32)
    pi = r[:, 1:k + 1].reshape(-1).to(torch.int32).contiguous()
    ps = s[:, 1:k + 1].reshape(-1).to(torch.float64).contiguous()
    raw, _ = ctx_features(tables, _dev(pu), pi, ps)
    raw = raw.cpu().numpy()
    assert raw.shape == (U * k, 16)
    exp = _host_fit(raw, names, kinds)
    R.assert_specs_equal(specs[2048], exp)
    assert bytes(specs[128]._host) == bytes(specs[2048]._host)
    assert sum(sp.kind == 0 for sp in exp.specs) >= 10
    R.assert_specs_equal(part, _host_fit(raw[:300 * k], names, kinds, n_bins=7))
    # the spec is usable: the fused pipeline accepts it
    FusedRecallRank(ops.Catalog(_dev(items)), p, _dev(user_feat), _dev(item_feat), _dev(user_hist), _dev(hist_len),
                    k=k, chunk_users=2048, ctx=(tables, specs[2048]))
