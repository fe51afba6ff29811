"""numpy / pandas restatement of what nrk_ctx_fit_stats and
nrk_ctx_fit_count_below return (csrc/ctxfit.hip), for the tests of
CtxSpec.fit_device.  No GPU work and no nrk kernels: the statistics come from
np.sort / np.unique of each column, and the picks from the sorted FILLED
column itself (not from the device's rank rule), so the rank rule is checked
too.  ``restated_spec`` drives nrk.features' host-side decisions with them."""
import numpy as np

FIELDS = ("n_valid", "n_distinct", "vmin", "vmax", "mid_lo", "mid_hi", "fill", "n_lt_fill", "n_eq_fill", "small",
          "inexact")


def median_in_kind(a, b, kind):
    """(a + b) / 2 in the column's dtype, as Series.median() forms it."""
    if kind == 1:
        return float((np.float32(a) + np.float32(b)) / np.float32(2))
    return float((np.float64(a) + np.float64(b)) / np.float64(2))


def column_stats(v, kind, ranks):
    """(stats dict, picks) of one raw float64 column."""
    v = np.asarray(v, np.float64)
    n = len(v)
    valid = np.sort(v[~np.isnan(v)] + 0.0)  # + 0.0: -0.0 -> +0.0
    nv = len(valid)
    uniq = np.unique(valid)
    st = dict(n_valid=nv, n_distinct=len(uniq), vmin=0.0, vmax=0.0, mid_lo=0.0, mid_hi=0.0, fill=0.0, n_lt_fill=0,
              n_eq_fill=0, small=np.zeros(21), inexact=0)
    if nv:
        st["vmin"], st["vmax"] = float(valid[0]), float(valid[-1])
        st["mid_lo"], st["mid_hi"] = float(valid[(nv - 1) // 2]), float(valid[nv // 2])
        st["fill"] = st["mid_lo"] if nv % 2 else median_in_kind(st["mid_lo"], st["mid_hi"], kind)
        st["n_lt_fill"] = int(np.searchsorted(valid, st["fill"], "left"))
        st["n_eq_fill"] = int(np.searchsorted(valid, st["fill"], "right")) - st["n_lt_fill"]
        st["small"][:min(len(uniq), 21)] = uniq[:21]
        with np.errstate(over="ignore", invalid="ignore"):
            if kind == 1:
                st["inexact"] = int((valid.astype(np.float32).astype(np.float64) != valid).any())
            elif kind == 2:
                st["inexact"] = int(((valid != np.rint(valid)) | ~(np.abs(valid) <= 2.0 ** 53)).any())
    filled = np.sort(np.where(np.isnan(v), st["fill"], v) + 0.0)
    picks = filled[np.asarray(ranks, np.int64)] if n else np.zeros(len(ranks))
    return st, picks, valid


def restated_stats(raw, cols, kinds, ranks):
    """stats (list of dicts) and picks [len(cols), len(ranks)] of columns ``cols`` of raw [n, F]."""
    out = [column_stats(raw[:, c], k, ranks)[:2] for c, k in zip(cols, kinds)]
    return [o[0] for o in out], np.stack([o[1] for o in out]) if out else np.zeros((0, len(ranks)))


def restated_spec(raw, names, kinds=None, n_bins=10, strategy="quantile"):
    """CtxSpec.fit_device without a device: the same host decisions
    (nrk.features._fit_decide / _fit_spec) on the restated statistics."""
    from nrk.features import CtxSpec, _finish_edges, _fit_decide, _fit_spec, default_ctx_kinds

    raw = np.asarray(raw, np.float64)
    n = raw.shape[0]
    kinds = default_ctx_kinds(names) if kinds is None else kinds
    ranks = _finish_edges(None, n, n_bins, 0) if strategy == "quantile" else np.zeros(0, np.int64)
    specs = []
    for c, f in enumerate(names):
        st, picks, valid = column_stats(raw[:, c], kinds[c], ranks)
        inner = _fit_decide(st, kinds[c], picks, n, n_bins, strategy, f)
        below = np.searchsorted(valid, inner, "left") if inner is not None else None
        specs.append(_fit_spec(st, kinds[c], inner, below, n))
    return CtxSpec(specs, names)


def apply_spec_host(spec, v):
    """ctx_code of csrc/ctxfeat.hip on the host: one fitted feature applied to raw values."""
    v = np.asarray(v, np.float64)
    if spec.kind == 0:
        v = np.where(np.isnan(v), spec.fill, v)
        b = (np.asarray(spec.edges[:spec.n_edges])[None, :] <= v[:, None]).sum(1)
        lut = np.asarray(spec.lut[:spec.n_lut])
        return np.where(b < spec.n_lut, lut[np.minimum(b, spec.n_lut - 1)], 0)
    vals = np.asarray(spec.vals[:spec.n_vals])
    codes = np.asarray(spec.codes[:spec.n_vals])
    m = v[:, None] == vals[None, :]
    return np.where(m.any(1), codes[np.argmax(m, 1)], 0)


def spec_fields(sp):
    """the fields of a CtxSpecC that the kernel reads."""
    return dict(kind=sp.kind, fill=sp.fill, n_edges=sp.n_edges, edges=list(sp.edges[:sp.n_edges]), n_lut=sp.n_lut,
                lut=list(sp.lut[:sp.n_lut]), n_vals=sp.n_vals)


def assert_specs_equal(got, exp, probe=None):
    """``got`` equals ``exp`` feature by feature: the binned fields one by
    one; an unbinned feature through the codes of its own values and of
    ``probe`` (the order of vals[] is free)."""
    assert got.names == exp.names
    for f, a, b in zip(got.names, got.specs, exp.specs):
        assert spec_fields(a) == spec_fields(b), (f, spec_fields(a), spec_fields(b))
        if a.kind == 1:
            assert sorted(a.vals[:a.n_vals]) == sorted(b.vals[:b.n_vals]), f
            v = np.concatenate([np.asarray(b.vals[:b.n_vals]), [np.nan, 0.0, 12345.5],
                                np.zeros(0) if probe is None else np.asarray(probe, np.float64)])
            assert np.array_equal(apply_spec_host(a, v), apply_spec_host(b, v)), f


def typed_columns(raw, names, kinds):
    """the main_df-typed columns CtxSpec.fit wants, from raw float64 [n, F]."""
    dt = {0: np.float64, 1: np.float32, 2: np.int64}
    # an integer column has no NaN; one that has is float64 in a frame
    return {f: raw[:, c].astype(np.float64 if kinds[c] == 2 and np.isnan(raw[:, c]).any() else dt[kinds[c]])
            for c, f in enumerate(names)}
