"""Ranker context features on the GPU.

Restates the context part of the reference's feature pipeline for the rows
the ranker scores:
  * FeatureExtractor._extract_context_features
    (src/features/feature_extractor.py:440-723) -- computed on the device by
    ``nrk_ctx_features`` (csrc/ctxfeat.hip) from resident tables;
  * FeatureExtractor._apply_binning (:838-898) + the context LabelEncoders of
    DINRanker._prepare_vocab_dicts (src/rank/DIN.py:603-613) -- FITTED on the
    host (``CtxSpec.fit``, sklearn's KBinsDiscretizer exactly as the reference
    calls it) or from device-resident raw features (``CtxSpec.fit_device``:
    the columns are sorted and summarised by ``nrk_ctx_fit_stats``,
    csrc/ctxfit.hip, and the bin edges finished in numpy's own arithmetic;
    the same spec, every row used) and APPLIED on the device in the same
    kernel, giving the int codes DINDataset feeds the model (DIN.py:330-353).

``CtxTables`` holds the lookup tables in HBM, built from the dicts the
reference keeps (str item / user ids): article-id Word2Vec vectors,
250-d content embeddings (float64), MinMax created times, categories,
YouTubeDNN user / item vectors, and each user's history (last N items, the
distinct categories of the whole history).
"""
from __future__ import annotations

import ctypes
from itertools import chain

import numpy as np
import pandas as pd
import torch

from . import _lib, ops

P = ctypes.c_void_p


def ctx_feature_names(last_n=3):
    """feature_extractor.py:470-481 (the feature_lists.pkl order)."""
    names = ["score"]
    for i in range(1, last_n + 1):
        names += [f"sim_{i}", f"time_diff_{i}", f"word_diff_{i}"]
    return names + ["sim_max", "sim_mean", "sim_min", "sim_std", "item_user_sim", "recall_in_user_cat"]


class CtxTablesC(ctypes.Structure):
    """include/nrk.h nrk_ctx_tables."""
    _fields_ = [("n_groups", ctypes.c_int64), ("group_off", P), ("group_user", P), ("pair_pos", P),
                ("pair_item", P), ("pair_score", P), ("last_n", ctypes.c_int32), ("code_stride", ctypes.c_int32),
                ("hist_last", P), ("hist_n", P), ("ucat_off", P), ("ucat", P), ("user_yt", P), ("user_yt_ok", P),
                ("n_items", ctypes.c_int64), ("w2v", P), ("w2v_ok", P), ("dw", ctypes.c_int32), ("content", P),
                ("content_flags", P), ("dc", ctypes.c_int32), ("created", P), ("category", P), ("item_yt", P),
                ("item_yt_ok", P), ("dy", ctypes.c_int32)]


class CtxSpecC(ctypes.Structure):
    """include/nrk.h nrk_ctx_spec."""
    _fields_ = [("kind", ctypes.c_int32), ("n_edges", ctypes.c_int32), ("n_lut", ctypes.c_int32),
                ("n_vals", ctypes.c_int32), ("fill", ctypes.c_double), ("edges", ctypes.c_double * 16),
                ("vals", ctypes.c_double * 32), ("lut", ctypes.c_int32 * 32), ("codes", ctypes.c_int32 * 32)]


def _stack(d, keys, dim, dtype):
    """rows of dict ``d`` for ``keys`` (zeros + ok=0 when absent)."""
    out = np.zeros((len(keys), dim), dtype)
    ok = np.zeros(len(keys), np.uint8)
    for n, k in enumerate(keys):
        v = d.get(k)
        if v is not None:
            out[n] = v
            ok[n] = 1
    return out, ok


class CtxTables:
    """Device tables for nrk_ctx_features.  ``item_ids`` / ``user_ids`` fix
    the dense rows (str ids, as the reference's dicts key them)."""

    def __init__(self, item_ids, user_ids, w2v, content, created, category, user_history, user_yt=None,
                 item_yt=None, last_n=3, device="cuda"):
        self.device = torch.device(device)
        self.last_n = int(last_n)
        self.item_ids = list(item_ids)
        self.user_ids = list(user_ids)
        self.item_index = pd.Index(_obj(self.item_ids), dtype=object)
        self.user_index = pd.Index(_obj(self.user_ids), dtype=object)
        I = len(self.item_ids)
        dw = len(next(iter(w2v.values()))) if w2v else 1
        dc = len(next(iter(content.values()))) if content else 1
        w, w_ok = _stack(w2v, self.item_ids, dw, np.float32)
        c, c_ok = _stack(content, self.item_ids, dc, np.float64)
        flags = c_ok | ((c.astype(np.float32) != 0).any(1).astype(np.uint8) << 1)  # :641-643 on the f32 rows
        cre = np.array([created.get(i, np.nan) for i in self.item_ids], np.float64)
        cat = np.array([category.get(i, -1) if category.get(i) is not None else -1 for i in self.item_ids], np.int32)
        # per user: the last N history items (:519) and the categories of the
        # whole history (:497-506); history item ids not in the item table
        # (no vector, no content, no created time, no category) -> -1
        N = self.last_n
        hl = np.full((len(self.user_ids), N), -1, np.int32)
        hn = np.full(len(self.user_ids), -1, np.int32)
        cats = []
        for n, u in enumerate(self.user_ids):
            h = user_history.get(u)
            if h is None:
                cats.append([])
                continue
            last = h[-N:]
            r = self.item_index.get_indexer(_obj(last)) if len(last) else np.zeros(0, np.int64)
            hl[n, :len(last)] = r
            hn[n] = len(last)
            seen = []
            for it in h:
                cc = category.get(it)
                if cc is not None and cc not in seen:
                    seen.append(cc)
            cats.append(seen)
        co = np.concatenate([[0], np.cumsum([len(x) for x in cats])]).astype(np.int64)
        cv = np.array(list(chain.from_iterable(cats)), np.int32) if co[-1] else np.zeros(1, np.int32)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self.t = {"w2v": d(w), "w2v_ok": d(w_ok), "content": d(c), "flags": d(flags), "created": d(cre),
                  "category": d(cat), "hist_last": d(hl), "hist_n": d(hn), "ucat_off": d(co), "ucat": d(cv)}
        self.dw, self.dc, self.dy = dw, dc, 0
        if user_yt is not None and item_yt is not None and len(item_yt):
            dy = len(next(iter(item_yt.values())))
            uy, uy_ok = _stack(user_yt, self.user_ids, dy, np.float32)
            iy, iy_ok = _stack(item_yt, self.item_ids, dy, np.float32)
            self.t.update(user_yt=d(uy), user_yt_ok=d(uy_ok), item_yt=d(iy), item_yt_ok=d(iy_ok))
            self.dy = dy
        self.n_items = I

    @classmethod
    def from_device(cls, tensors, last_n=3):
        """Wrap device tensors laid out as in __init__ (the fused pipeline
        builds them on the GPU directly)."""
        self = cls.__new__(cls)
        self.device = tensors["w2v"].device
        self.last_n = int(last_n)
        self.t = dict(tensors)
        self.dw = tensors["w2v"].shape[1]
        self.dc = tensors["content"].shape[1]
        self.dy = tensors["item_yt"].shape[1] if "item_yt" in tensors else 0
        self.n_items = tensors["w2v"].shape[0]
        return self

    def struct(self, group_off, group_user, pair_item, pair_score, pair_pos=None, code_stride=None):
        t = self.t
        p = lambda x: P(x.data_ptr()) if x is not None else None  # noqa: E731
        F = 1 + 3 * self.last_n + 6
        return CtxTablesC(group_user.numel(), p(group_off), p(group_user), p(pair_pos), p(pair_item),
                          p(pair_score), self.last_n, code_stride or F, p(t["hist_last"]), p(t["hist_n"]),
                          p(t["ucat_off"]), p(t["ucat"]), p(t.get("user_yt")), p(t.get("user_yt_ok")),
                          self.n_items, p(t["w2v"]), p(t["w2v_ok"]), self.dw, p(t["content"]), p(t["flags"]),
                          self.dc, p(t["created"]), p(t["category"]), p(t.get("item_yt")), p(t.get("item_yt_ok")),
                          self.dy)


class CtxSpec:
    """The fitted binning + label encoding of every context feature."""

    def __init__(self, specs, names):
        self.names = list(names)
        self.specs = specs
        arr = (CtxSpecC * len(specs))(*specs)
        raw = np.frombuffer(bytes(arr), dtype=np.uint8)
        self._host = raw
        self._dev = {}

    def device(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self._host.copy()).to(device)
        return self._dev[key]

    @classmethod
    def fit(cls, columns, names, n_bins=10, strategy="quantile"):
        """``columns``: feature -> raw column (numpy, the main_df dtype) over
        the rows the reference fits on.  _apply_binning (:838-898): numeric
        columns with > 20 distinct values are NaN-filled with their median and
        KBins-binned (n_bins = min(10, distinct)); then one LabelEncoder per
        feature over str(column.fillna(0)) (DIN.py:603-613)."""
        from sklearn.preprocessing import KBinsDiscretizer, LabelEncoder

        specs = []
        for f in names:
            col = pd.Series(columns[f])
            sp = CtxSpecC()
            binned = None
            if pd.api.types.is_numeric_dtype(col) and col.nunique() > 20 and not col.isna().all():
                med = col.median()
                fill = 0 if pd.isna(med) else med
                col = col.fillna(fill)
                nb = min(n_bins, col.nunique())
                if nb >= 2:
                    disc = KBinsDiscretizer(n_bins=nb, encode="ordinal", strategy=strategy)
                    binned = np.asarray(disc.fit_transform(col.to_frame())).astype(int).flatten()
                    edges = np.asarray(disc.bin_edges_[0], np.float64)[1:-1]
                    if len(edges) > 16:
                        raise NotImplementedError("more than 17 bins")
                    sp.kind = 0
                    sp.fill = float(np.asarray(fill, dtype=col.dtype))  # fillna casts to the column dtype
                    sp.n_edges = len(edges)
                    sp.edges[:len(edges)] = edges.tolist()
            elif pd.api.types.is_numeric_dtype(col) and col.isna().all():
                col = pd.Series(np.zeros(len(col), np.int64))  # all-NaN column -> 0 (:860-864)
            if binned is not None:
                le = LabelEncoder().fit(pd.Series(binned).astype(str))
                classes = list(le.classes_)
                sp.n_lut = len(edges) + 1
                for b in range(sp.n_lut):
                    sp.lut[b] = classes.index(str(b)) + 1 if str(b) in classes else 0
            else:
                le = LabelEncoder().fit(col.fillna(0).astype(str))
                classes = list(le.classes_)
                vals = pd.unique(col.dropna())
                if len(vals) > 32:
                    raise NotImplementedError(f"{f}: more than 32 distinct unbinned values")
                sp.kind = 1
                sp.n_vals = len(vals)
                for k, v in enumerate(vals):
                    sp.vals[k] = float(v)
                    sp.codes[k] = classes.index(str(v)) + 1 if str(v) in classes else 0
            specs.append(sp)
        return cls(specs, names)

    @classmethod
    def fit_device(cls, raw, names, kinds=None, n_bins=10, strategy="quantile", workspace_bytes=1 << 30):
        """``fit`` from device-resident data: ``raw`` is the float64 [n, F]
        device tensor ``ctx_features(..., raw=True)`` returns (a row stride is
        allowed), ``names`` its F columns, ``kinds`` the main_df dtype of each
        (0 float64, 1 float32, 2 integer; default ``default_ctx_kinds``).  The
        columns are sorted and summarised on the GPU (nrk_ctx_fit_stats) in
        groups that fit ``workspace_bytes``; only the per-column summary and
        the <= 2 * (n_bins + 1) values np.percentile interpolates between come
        to the host, where ``_finish_edges`` repeats numpy's arithmetic.

        The decisions are ``fit``'s and the spec is identical to ``fit`` of the
        same rows up to 200,000 rows.  Above that ``fit`` and the reference take
        their quantiles from a random resample (KBinsDiscretizer's default
        subsample=200000, random_state=None); this fit always uses every row,
        which is what subsample=None means, and is deterministic.

        Refused, with ``fit`` as the way out: strategy "kmeans", n_bins > 17, a
        binned integer-kind column (numpy interpolates those in the integer
        dtype).  +-inf in a binned column is a ValueError, as in sklearn, and so
        is a value its column's kind cannot hold."""
        names = list(names)
        if strategy == "kmeans":
            raise NotImplementedError("fit_device has no kmeans strategy; use CtxSpec.fit")
        if strategy not in ("quantile", "uniform"):
            raise ValueError(f"unknown strategy {strategy!r}")
        if n_bins > 17:
            raise NotImplementedError("fit_device holds at most 17 bins (16 inner edges); use CtxSpec.fit")
        if n_bins < 2:
            raise ValueError("n_bins must be >= 2")
        n, F, _ = _fit_raw(raw)
        if F != len(names):
            raise ValueError(f"raw has {F} columns for {len(names)} names")
        if n == 0:
            raise ValueError("fit_device needs at least one row")
        kinds = default_ctx_kinds(names) if kinds is None else [int(k) for k in kinds]
        if len(kinds) != F or any(k not in (0, 1, 2) for k in kinds):
            raise ValueError("kinds must hold 0 (float64), 1 (float32) or 2 (integer) per column")
        L = _lib.lib()
        per = 0
        for g in range(1, min(F, 64) + 1):
            b = L.nrk_ctx_fit_workspace_bytes(n, g)
            if b == 0 or b > workspace_bytes:
                break
            per = g
        if per == 0:
            raise ValueError(f"workspace_bytes = {workspace_bytes} is too small for one column of {n} rows "
                             f"({L.nrk_ctx_fit_workspace_bytes(n, 1)} bytes)")
        ws = torch.empty(L.nrk_ctx_fit_workspace_bytes(n, per), dtype=torch.uint8, device=raw.device)
        ranks = _finish_edges(None, n, n_bins, 0) if strategy == "quantile" else np.zeros(0, np.int64)
        specs = [None] * F
        for c0 in range(0, F, per):
            cols = list(range(c0, min(c0 + per, F)))
            ck = [kinds[c] for c in cols]
            stats, picks = ctx_fit_stats(raw, cols, ck, ranks, workspace=ws)
            stats, picks = fit_stats_host(stats), picks.cpu().numpy()
            plans = [_fit_decide(stats[j], ck[j], picks[j], n, n_bins, strategy, names[c]) for j, c in enumerate(cols)]
            probes = np.full((len(cols), 16), np.nan)
            for j, inner in enumerate(plans):
                if inner is not None:
                    probes[j, :len(inner)] = inner
            below = None
            if any(p is not None for p in plans):
                below = ctx_fit_count_below(n, len(cols), torch.from_numpy(probes).to(raw.device), ws).cpu().numpy()
            for j, c in enumerate(cols):
                specs[c] = _fit_spec(stats[j], ck[j], plans[j], None if below is None else below[j], n)
        return cls(specs, names)


# include/nrk.h nrk_ctx_fit_col
FIT_COL_DTYPE = np.dtype([("n_valid", "<i8"), ("n_distinct", "<i8"), ("vmin", "<f8"), ("vmax", "<f8"),
                          ("mid_lo", "<f8"), ("mid_hi", "<f8"), ("fill", "<f8"), ("n_lt_fill", "<i8"),
                          ("n_eq_fill", "<i8"), ("small", "<f8", (21,)), ("inexact", "<i8")])
_KIND_DTYPE = {0: np.float64, 1: np.float32, 2: np.int64}


def default_ctx_kinds(names):
    """The reference's main_df dtypes of the context columns: score float64,
    recall_in_user_cat integer, every other feature float32."""
    return [0 if f == "score" else 2 if f == "recall_in_user_cat" else 1 for f in names]


def _edge_plan(n_rows, n_bins):
    """np.percentile(column, np.linspace(0, 100, n_bins + 1)) up to the values
    (numpy/lib/_function_base_impl.py percentile, _quantile, _get_indexes,
    _get_gamma; method 'linear'): the neighbouring ranks of every percentile
    and its weight.  Depends on the row count only."""
    q = np.true_divide(np.linspace(0, 100, n_bins + 1), np.float64(100))
    virtual = (n_rows - 1) * q
    prev = np.floor(virtual)
    nxt = prev + 1
    above = virtual >= n_rows - 1
    prev[above] = -1  # numpy takes the last element for both ...
    nxt[above] = -1
    gamma = virtual - prev  # ... and forms gamma after that; the two values are equal there
    lo = prev.astype(np.intp) % n_rows
    hi = nxt.astype(np.intp) % n_rows
    ranks = np.unique(np.concatenate([lo, hi])).astype(np.int64)
    return ranks, np.searchsorted(ranks, lo), np.searchsorted(ranks, hi), gamma


def _finish_edges(picks, n_rows, n_bins, kind, mask=True):
    """The bin edges KBinsDiscretizer(strategy="quantile") fits on a column of
    ``n_rows`` values whose sorted values at the ranks ``_finish_edges(None,
    n_rows, n_bins, kind)`` returns are ``picks``: numpy's _lerp on the two
    neighbours of every percentile -- the difference in the column's dtype
    (float32 for kind 1), everything else in float64 -- then sklearn's removal
    of bins no wider than 1e-8 (``mask=False``: np.percentile's values)."""
    ranks, ia, ib, gamma = _edge_plan(n_rows, n_bins)
    if picks is None:
        return ranks
    if kind not in (0, 1):
        raise NotImplementedError("quantiles of an integer column are interpolated in the integer dtype")
    v = np.asarray(picks).astype(_KIND_DTYPE[kind])
    a, b = v[ia], v[ib]
    diff = np.subtract(b, a)
    edges = np.asanyarray(np.add(a, diff * gamma))
    np.subtract(b, diff * (1 - gamma), out=edges, where=gamma >= 0.5, casting="unsafe", dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    if mask:
        edges = edges[np.ediff1d(edges, to_begin=np.inf) > 1e-8]
    return edges


def _fit_decide(st, kind, picks, n_rows, n_bins, strategy, name):
    """CtxSpec.fit's binning decision for one column from its device summary:
    the inner bin edges, or None for an unbinned column."""
    if st["inexact"]:
        raise ValueError(f"{name}: a value is not a {np.dtype(_KIND_DTYPE[kind]).name} (kinds[] names the column's dtype)")
    if not (st["n_distinct"] > 20 and st["n_valid"] > 0):
        return None
    if kind == 2:
        raise NotImplementedError(f"{name}: an integer column with more than 20 values is binned in the integer "
                                  "dtype; use CtxSpec.fit")
    if not (np.isfinite(st["vmin"]) and np.isfinite(st["vmax"])):
        raise ValueError(f"{name}: infinity in a binned column")
    dt = _KIND_DTYPE[kind]
    if strategy == "uniform":  # sklearn: np.linspace(col_min, col_max, n_bins + 1) in the column dtype
        edges = np.asarray(np.linspace(dt(st["vmin"]), dt(st["vmax"]), n_bins + 1), np.float64)
    else:
        edges = _finish_edges(picks, n_rows, n_bins, kind)
    return edges[1:-1]


def _fit_spec(st, kind, inner, below, n_rows):
    """One column's CtxSpecC as CtxSpec.fit builds it.  ``below[k]``: valid
    values below inner edge k."""
    from sklearn.preprocessing import LabelEncoder

    sp = CtxSpecC()
    n_nan = n_rows - int(st["n_valid"])
    if inner is not None:
        fill = float(st["fill"])
        m = len(inner)
        # rows per bin of the filled column: bin b = [edge b - 1, edge b)
        cum = np.concatenate([[0], below[:m] + n_nan * (fill < inner), [n_rows]])
        seen = [str(b) for b in range(m + 1) if cum[b + 1] > cum[b]]
        classes = list(LabelEncoder().fit(seen).classes_)
        sp.kind = 0
        sp.fill = fill
        sp.n_edges = m
        sp.edges[:m] = inner.tolist()
        sp.n_lut = m + 1
        for b in range(m + 1):
            sp.lut[b] = classes.index(str(b)) + 1 if str(b) in classes else 0
        return sp
    nd = int(st["n_distinct"])
    if nd == 0:  # all NaN: the reference's int64 zeros
        vals = np.zeros(1, np.int64)
        col = pd.Series(vals)
    else:
        # an integer column has no NaN; one that has is float64 in a frame
        dt = np.float64 if (kind == 2 and n_nan) else _KIND_DTYPE[kind]
        vals = np.asarray(st["small"][:nd]).astype(dt)
        col = pd.Series(np.concatenate([vals, np.zeros(1 if n_nan else 0, dt)]))
    classes = list(LabelEncoder().fit(col.astype(str)).classes_)
    sp.kind = 1
    sp.n_vals = len(vals)
    for k, v in enumerate(vals):
        sp.vals[k] = float(v)
        sp.codes[k] = classes.index(str(v)) + 1 if str(v) in classes else 0
    return sp


def fit_stats_host(stats):
    """nrk_ctx_fit_col records (device uint8 tensor) as a numpy record array."""
    return np.frombuffer(stats.cpu().numpy().tobytes(), dtype=FIT_COL_DTYPE)


def _fit_raw(raw):
    if not (torch.is_tensor(raw) and raw.is_cuda and raw.dtype == torch.float64 and raw.dim() == 2):
        raise ValueError("raw must be a float64 [n, F] device tensor")
    n, F = raw.shape
    if n > 1 and ((F > 1 and raw.stride(1) != 1) or raw.stride(0) < F):
        raise ValueError("raw must be row-major (a row stride >= F is allowed)")
    if n <= 1 and not raw.is_contiguous():
        raise ValueError("raw must be row-major")
    return n, F, (raw.stride(0) if n > 1 else F)


def ctx_fit_stats(raw, cols, kinds, ranks, workspace=None):
    """nrk_ctx_fit_stats: the summary (uint8 tensor of nrk_ctx_fit_col records,
    see ``fit_stats_host``) and the picks (f64 [len(cols), len(ranks)]) of the
    columns ``cols`` of ``raw`` (f64 [n, F] device tensor, row stride >= F)."""
    n, F, ld = _fit_raw(raw)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    if cols.ndim != 1 or kinds.shape != cols.shape or not 1 <= len(cols) <= 64:
        raise ValueError("cols / kinds: 1 to 64 columns, one kind each")
    if len(cols) and (cols.min() < 0 or cols.max() >= F):
        raise ValueError("column index out of [0, F)")
    if len(ranks) > 64 or (len(ranks) and (ranks.min() < 0 or ranks.max() >= max(n, 1) or (np.diff(ranks) < 0).any())):
        raise ValueError("ranks must ascend within [0, n_rows), at most 64")
    dev = raw.device
    L = _lib.lib()
    need = L.nrk_ctx_fit_workspace_bytes(n, len(cols))
    if n >= 1 << 31:
        raise NotImplementedError("n_rows must be < 2^31")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    stats = torch.zeros(len(cols) * FIT_COL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    picks = torch.zeros((len(cols), len(ranks)), dtype=torch.float64, device=dev)
    _lib.call("nrk_ctx_fit_stats", P(raw.data_ptr()), n, ld, P(cols.ctypes.data), P(kinds.ctypes.data), len(cols),
              P(ranks.ctypes.data) if len(ranks) else None, len(ranks), P(stats.data_ptr()),
              P(picks.data_ptr()) if len(ranks) else None, P(workspace.data_ptr()), workspace.numel(),
              ops._stream())
    return stats, picks


def ctx_fit_count_below(n_rows, n_cols, probes, workspace):
    """nrk_ctx_fit_count_below on the workspace the last ``ctx_fit_stats`` of
    the same shape used: int64 [n_cols, n_probes] valid values below each
    probe (f64 [n_cols, n_probes] device tensor)."""
    ops._dev(probes, workspace)
    if probes.dtype != torch.float64 or probes.dim() != 2 or probes.shape[0] != n_cols:
        raise ValueError(f"probes must be float64 [{n_cols}, n_probes]")
    out = torch.zeros(probes.shape, dtype=torch.int64, device=probes.device)
    _lib.call("nrk_ctx_fit_count_below", n_rows, n_cols, P(probes.data_ptr()), probes.shape[1], P(out.data_ptr()),
              P(workspace.data_ptr()), workspace.numel(), ops._stream())
    return out


def ctx_features(tables: CtxTables, user_rows, item_rows, scores, spec: CtxSpec | None = None, raw=True,
                 groups=None, out_codes=None, out_raw=None):
    """Context features of n rows (device tensors: user_rows int32 [n] dense
    user row, item_rows int32 [n] (-1 unknown), scores f64 [n]).  Rows are
    grouped by user here (stable), or pass ``groups`` = (group_off int64,
    group_user int32, pair_pos int64 | None).  Returns (raw f64 [n, F] | None,
    codes int32 [n, F] | None); ``out_raw`` (contiguous f64 [n, F]) is written
    in place of a new tensor."""
    ops._dev(item_rows, scores, out_raw)
    n = item_rows.numel()
    F = 1 + 3 * tables.last_n + 6
    dev = item_rows.device
    if out_raw is not None and (tuple(out_raw.shape) != (n, F) or out_raw.dtype != torch.float64):
        raise ValueError(f"out_raw must be float64 [{n}, {F}]")
    if groups is None:
        order = torch.sort(user_rows.long(), stable=True).indices
        us = user_rows.long()[order]
        uniq, counts = torch.unique_consecutive(us, return_counts=True)
        group_off = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=dev)
        group_off[1:] = torch.cumsum(counts, 0)
        groups = (group_off, uniq.to(torch.int32).contiguous(), order.contiguous())
    group_off, group_user, pair_pos = groups
    if out_raw is None and raw:
        out_raw = torch.empty((n, F), dtype=torch.float64, device=dev)
    if spec is not None and out_codes is None:
        out_codes = torch.empty((n, F), dtype=torch.int32, device=dev)
    if out_codes is not None and (tuple(out_codes.shape) != (n, F) or out_codes.dtype != torch.int32):
        raise ValueError(f"out_codes must be int32 [{n}, {F}]")
    st = tables.struct(group_off, group_user, item_rows, scores, pair_pos)
    sp = spec.device(dev) if spec is not None else None
    _lib.call("nrk_ctx_features", P(ctypes.addressof(st)), P(sp.data_ptr()) if sp is not None else None,
              P(out_raw.data_ptr()) if out_raw is not None else None,
              P(out_codes.data_ptr()) if out_codes is not None else None, ops._stream())
    return out_raw, out_codes


def _obj(seq):
    a = np.empty(len(seq), dtype=object)
    a[:] = list(seq)
    return a
