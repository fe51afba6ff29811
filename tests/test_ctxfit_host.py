"""CPU: the host half of CtxSpec.fit_device (nrk/features.py) and the argument
checks of the nrk_ctx_fit_* entries.

* _finish_edges against np.percentile itself, bit for bit (the same
  arithmetic on the same picked values);
* the filled-rank rule and the median against pandas;
* the whole decision logic, driven by the numpy restatement of the device
  statistics (tests/ctxfit_restated.py), against the reference's own fitted
  edges and codes on tests/golden/ctxfeat_small and against CtxSpec.fit;
* every argument check of the entries (none launches)."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

import ctxfit_restated as R
from nrk import _lib
from nrk.features import CtxSpec, _finish_edges, default_ctx_kinds

DT = {0: np.float64, 1: np.float32}


def _columns(rng, n, kind):
    dt = DT[kind]
    a = rng.standard_normal(n).astype(dt)
    ties = np.round(rng.standard_normal(n), 1).astype(dt)  # many ties
    zeros = rng.standard_normal(n).astype(dt)
    zeros[::3] = -0.0
    zeros[1::3] = 0.0
    wide = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(dt)
    return {"normal": a, "ties": ties, "zeros": zeros, "wide": wide}


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [21, 22, 101, 2999])
def test_finish_edges_is_np_percentile(n, kind):
    rng = np.random.default_rng(1000 * kind + n)
    for n_bins in (2, 3, 7, 10, 17):
        ranks = _finish_edges(None, n, n_bins, kind)
        assert ranks.dtype == np.int64 and (np.diff(ranks) > 0).all() and 0 <= ranks[0] and ranks[-1] < n
        assert len(ranks) <= 2 * (n_bins + 1)
        for name, col in _columns(rng, n, kind).items():
            exp = np.asarray(np.percentile(col, np.linspace(0, 100, n_bins + 1)), dtype=np.float64)
            got = _finish_edges(np.sort(col)[ranks].astype(np.float64), n, n_bins, kind, mask=False)
            assert got.dtype == np.float64
            masked = _finish_edges(np.sort(col)[ranks].astype(np.float64), n, n_bins, kind)
            exp_masked = exp[np.ediff1d(exp, to_begin=np.inf) > 1e-8]
            if name == "zeros":
                # -0.0 == 0.0: which of the two a rank holds is np.partition's choice inside
                # np.percentile and np.sort's here, not a property of the column (the device
                # writes +0.0 for both).  Every other bit is compared.
                got, exp, masked, exp_masked = got + 0.0, exp + 0.0, masked + 0.0, exp_masked + 0.0
            assert got.tobytes() == exp.tobytes(), (name, n_bins, got, exp)
            assert masked.tobytes() == exp_masked.tobytes(), (name, n_bins)


def test_finish_edges_equals_kbins_discretizer():
    from sklearn.preprocessing import KBinsDiscretizer

    rng = np.random.default_rng(7)
    for kind in (0, 1):
        col = np.round(rng.standard_normal(500), 1).astype(DT[kind])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            disc = KBinsDiscretizer(n_bins=10, encode="ordinal", strategy="quantile").fit(col[:, None])
        ranks = _finish_edges(None, 500, 10, kind)
        got = _finish_edges(np.sort(col)[ranks].astype(np.float64), 500, 10, kind)
        assert got.tobytes() == np.asarray(disc.bin_edges_[0], np.float64).tobytes()


def test_finish_edges_refuses_integer_columns():
    with pytest.raises(NotImplementedError):
        _finish_edges(np.arange(22.0), 100, 10, 2)


def _nan_cases(rng, kind):
    dt = DT[kind]
    for n, n_nan in ((30, 0), (31, 0), (30, 1), (31, 1), (40, 20), (41, 20), (41, 21), (5, 4), (3, 0)):
        v = rng.standard_normal(n).astype(dt)
        v[rng.permutation(n)[:n_nan]] = np.nan
        yield f"random n={n} nan={n_nan}", v
        t = np.round(v, 0)  # ties: an even-count median that is (or is not) a column value
        yield f"ties n={n} nan={n_nan}", t
    v = np.array([1, 2, 2, 3, np.nan, np.nan], dt)  # fill 2 is a value, twice
    yield "fill is a value", v
    v = np.array([1, 2, 4, 3, np.nan], dt)  # fill 2.5 is not
    yield "fill is no value", v
    yield "float32 median is no column value", np.array([0.1, 0.2, 0.7, 0.3, np.nan, np.nan], dt)


@pytest.mark.parametrize("kind", [0, 1])
def test_filled_rank_rule_and_median_are_pandas(kind):
    rng = np.random.default_rng(11 + kind)
    for name, v in _nan_cases(rng, kind):
        s = pd.Series(v)
        n = len(v)
        st, picks, valid = R.column_stats(v.astype(np.float64), kind, np.arange(n))
        med = s.median()
        assert med.dtype == v.dtype, name
        assert st["fill"] == float(med), name
        exp = np.sort(s.fillna(med).to_numpy()).astype(np.float64)
        assert np.array_equal(picks, exp), name  # the restatement's filled column is pandas'
        # the device's rule: the filled column from (sorted valid, fill, n_lt, n_eq, n_nan)
        n_nan, lt, eq = n - st["n_valid"], st["n_lt_fill"], st["n_eq_fill"]
        rule = np.array([valid[r] if r < lt else st["fill"] if r < lt + eq + n_nan else valid[r - n_nan]
                         for r in range(n)])
        assert np.array_equal(rule, exp), name
        assert st["n_distinct"] == s.nunique(), name


def _fixture_raw(g):
    names = g["ctx_feats"].tolist()
    return names, np.stack([g[f"raw::{f}"].astype(np.float64) for f in names], 1)


def test_fixture_dtypes_are_the_default_kinds(golden):
    g = golden("ctxfeat_small")
    names = g["ctx_feats"].tolist()
    kind_of = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}
    got = [kind_of.get(g[f"raw::{f}"].dtype, 2) for f in names]
    assert got == default_ctx_kinds(names)


def test_restated_fit_matches_reference(golden):
    g = golden("ctxfeat_small")
    names, raw = _fixture_raw(g)
    spec = R.restated_spec(raw, names)
    n_binned = 0
    for k, f in enumerate(names):
        sp = spec.specs[k]
        if f"edges::{f}" in g.files:
            n_binned += 1
            assert sp.kind == 0, f
            assert np.asarray(sp.edges[:sp.n_edges]).tobytes() == g[f"edges::{f}"][1:-1].tobytes(), f
        codes = R.apply_spec_host(sp, raw[:, k])
        assert np.array_equal(codes, g["codes"][:, k]), f
    assert n_binned == 15


def test_restated_fit_matches_host_fit(golden):
    g = golden("ctxfeat_small")
    names, raw = _fixture_raw(g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = CtxSpec.fit({f: g[f"raw::{f}"] for f in names}, names)
        R.assert_specs_equal(R.restated_spec(raw, names), exp)
        for n_bins, strategy in ((4, "quantile"), (17, "quantile"), (10, "uniform"), (5, "uniform")):
            exp = CtxSpec.fit({f: g[f"raw::{f}"] for f in names}, names, n_bins=n_bins, strategy=strategy)
            R.assert_specs_equal(R.restated_spec(raw, names, n_bins=n_bins, strategy=strategy), exp)


def test_restated_fit_with_empty_bins_and_unbinned_columns():
    """Heavy ties leave quantile bins without a row, a skewed column leaves
    uniform bins without one: the LabelEncoder sees fewer classes, and the
    codes follow CtxSpec.fit."""
    rng = np.random.default_rng(5)
    n = 400
    # the 40th percentile lies at rank 159.6, between the last 0 and the first 1: edges 0.6 and 1.0, no row between
    ties = np.concatenate([np.zeros(160), np.ones(210), 1 + rng.random(30) * 2]).astype(np.float32)
    skew = np.concatenate([rng.random(n - 2), [50.0, 100.0]])
    small = rng.integers(0, 5, n).astype(np.float32)
    small[::7] = np.nan
    ints = rng.integers(0, 2, n).astype(np.float64)
    allnan = np.full(n, np.nan)
    raw = np.stack([skew, ties, small, allnan, ints], 1).astype(np.float64)
    names, kinds = ["skew", "ties", "small", "allnan", "ints"], [0, 1, 1, 1, 2]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for strategy in ("quantile", "uniform"):
            exp = CtxSpec.fit(R.typed_columns(raw, names, kinds), names, strategy=strategy)
            got = R.restated_spec(raw, names, kinds, strategy=strategy)
            R.assert_specs_equal(got, exp)
            sp = got.specs[0 if strategy == "uniform" else 1]
            lut = list(sp.lut[:sp.n_lut])
            assert 0 in lut, (strategy, lut)  # the case is what it says: some bin is empty


def test_fit_device_refusals_need_no_device():
    with pytest.raises(NotImplementedError, match="CtxSpec.fit"):
        CtxSpec.fit_device(None, ["a"], strategy="kmeans")
    with pytest.raises(NotImplementedError, match="CtxSpec.fit"):
        CtxSpec.fit_device(None, ["a"], n_bins=18)
    with pytest.raises(ValueError):
        CtxSpec.fit_device(None, ["a"], n_bins=1)
    with pytest.raises(ValueError):
        CtxSpec.fit_device(np.zeros((3, 1)), ["a"])  # not a device tensor


# ------------------------------------------------------------ the entries --
FAKE = ctypes.c_void_p(4096)  # non-null, never dereferenced: every case returns before a launch


def _stats(raw=FAKE, n_rows=10, ld=16, cols=(0, 1), kinds=(0, 1), n_cols=None, ranks=(0, 9), n_ranks=None,
           out_stats=FAKE, out_picks=FAKE, ws=FAKE, ws_bytes=None):
    L = _lib.lib()
    c = (ctypes.c_int32 * max(len(cols), 1))(*cols)
    k = (ctypes.c_int32 * max(len(kinds), 1))(*kinds)
    r = (ctypes.c_int64 * max(len(ranks), 1))(*ranks)
    n_cols = len(cols) if n_cols is None else n_cols
    if ws_bytes is None:
        ws_bytes = L.nrk_ctx_fit_workspace_bytes(n_rows, max(1, min(n_cols, 64)))
    return L.nrk_ctx_fit_stats(raw, n_rows, ld, ctypes.cast(c, ctypes.c_void_p) if cols is not None else None,
                               ctypes.cast(k, ctypes.c_void_p), n_cols, ctypes.cast(r, ctypes.c_void_p),
                               len(ranks) if n_ranks is None else n_ranks, out_stats, out_picks, ws, ws_bytes, None)


def test_ctx_fit_stats_argument_checks():
    L = _lib.lib()
    E = _lib.NRK_EINVAL
    assert _stats(raw=None) == E and b"null pointer" in L.nrk_last_error()
    assert _stats(out_stats=None) == E and b"null pointer" in L.nrk_last_error()
    assert _stats(out_picks=None) == E and b"null pointer" in L.nrk_last_error()
    assert _stats(ws=None) == E and b"null pointer" in L.nrk_last_error()
    assert L.nrk_ctx_fit_stats(FAKE, 10, 16, None, None, 2, None, 0, FAKE, None, FAKE, 1 << 20, None) == E
    assert b"null pointer" in L.nrk_last_error()
    assert _stats(cols=(), kinds=(), n_cols=0) == E and b"n_cols" in L.nrk_last_error()
    assert _stats(cols=tuple(range(65)), kinds=(0,) * 65, ld=80) == E and b"n_cols" in L.nrk_last_error()
    assert _stats(cols=(0, 16)) == E and b"ld" in L.nrk_last_error()
    assert _stats(cols=(0, -1)) == E and b"ld" in L.nrk_last_error()
    assert _stats(kinds=(0, 3)) == E and b"col_kind" in L.nrk_last_error()
    assert _stats(n_ranks=65) == E and b"n_ranks" in L.nrk_last_error()
    assert _stats(ranks=(0, 10)) == E and b"rank" in L.nrk_last_error()
    assert _stats(ranks=(5, 4)) == E and b"ascend" in L.nrk_last_error()
    assert _stats(n_rows=-1) == E
    assert _stats(ws_bytes=L.nrk_ctx_fit_workspace_bytes(10, 2) - 1) == E and b"workspace" in L.nrk_last_error()
    with pytest.raises(ValueError):
        _lib.check(E, "nrk_ctx_fit_stats")
    # nothing to do / too large: decided before any pointer is used
    assert _stats(n_rows=0, ranks=(), ws_bytes=0) == _lib.NRK_OK
    rc = _stats(n_rows=1 << 31, ranks=(0,), ws_bytes=0)
    assert rc == _lib.NRK_EUNSUPPORTED and b"2^31" in L.nrk_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, "nrk_ctx_fit_stats")


def test_ctx_fit_count_below_argument_checks():
    L = _lib.lib()
    E = _lib.NRK_EINVAL
    ws = L.nrk_ctx_fit_workspace_bytes(10, 2)
    assert L.nrk_ctx_fit_count_below(10, 2, None, 4, FAKE, FAKE, ws, None) == E and b"null" in L.nrk_last_error()
    assert L.nrk_ctx_fit_count_below(10, 2, FAKE, 4, None, FAKE, ws, None) == E
    assert L.nrk_ctx_fit_count_below(10, 2, FAKE, 4, FAKE, None, ws, None) == E
    assert L.nrk_ctx_fit_count_below(10, 0, FAKE, 4, FAKE, FAKE, ws, None) == E and b"n_cols" in L.nrk_last_error()
    assert L.nrk_ctx_fit_count_below(10, 65, FAKE, 4, FAKE, FAKE, ws, None) == E
    assert L.nrk_ctx_fit_count_below(10, 2, FAKE, 65, FAKE, FAKE, ws, None) == E
    assert L.nrk_ctx_fit_count_below(10, 2, FAKE, 4, FAKE, FAKE, ws - 1, None) == E
    assert b"workspace" in L.nrk_last_error()
    assert L.nrk_ctx_fit_count_below(0, 2, None, 4, None, None, 0, None) == _lib.NRK_OK
    assert L.nrk_ctx_fit_count_below(10, 2, None, 0, None, None, 0, None) == _lib.NRK_OK
    assert L.nrk_ctx_fit_count_below(1 << 31, 2, FAKE, 4, FAKE, FAKE, 0, None) == _lib.NRK_EUNSUPPORTED


def test_ctx_fit_host_queries():
    L = _lib.lib()
    assert L.nrk_abi_version() == 3
    T = L.nrk_ctx_fit_tile()
    assert T > 0
    sizes = [[L.nrk_ctx_fit_workspace_bytes(n, c) for c in (1, 2, 5, 16, 64)]
             for n in (0, 1, T - 1, T, T + 1, 100_000, 7_500_000)]
    for row in sizes:
        assert all(b > 0 for b in row) and row == sorted(row), sizes
    for col in zip(*sizes):
        assert list(col) == sorted(col), sizes
    # two planes of keys per column dominate
    assert sizes[-1][3] >= 2 * 7_500_000 * 16 * 8
    assert sizes[-1][3] < 2.1 * 7_500_000 * 16 * 8
    # out of range: no size
    assert L.nrk_ctx_fit_workspace_bytes(10, 0) == 0 and L.nrk_ctx_fit_workspace_bytes(10, 65) == 0
    assert L.nrk_ctx_fit_workspace_bytes(-1, 1) == 0 and L.nrk_ctx_fit_workspace_bytes(1 << 31, 1) == 0
