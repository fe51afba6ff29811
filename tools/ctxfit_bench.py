"""The context fit at the Tianchi shape (dev tool): raw context features of
--users (250,000) x --pairs-per-user (30) pairs over the click log and
articles of nrk.data.synth (random candidates; random vectors where the data
set has learned ones), written into one device buffer by nrk_ctx_features.
Times, with HIP events (3 warm-up calls, then the median of --iters calls in
one process), nrk_ctx_fit_stats over all 16 columns in one group and
nrk_ctx_fit_count_below, and CtxSpec.fit_device end to end (host clock around
a device synchronise: both entries, the two read-backs and the host finish);
the split of one nrk_ctx_fit_stats call into its keys / sort / summary kernels
comes from torch.profiler's kernel records (null when it gives none).  Beside
them raw.cpu() + CtxSpec.fit on the same rows, once.  Above 200,000 rows the
host fit takes its quantiles from a random resample, so the two specs are
compared on the first 200,000 rows, where both are deterministic.  Reports ms
and GB/s against the algorithmic bytes of the device path: the row read, then
8 passes that read and write n * F * 8 B of keys.  Prints one JSON line.
DESIGN §4.14."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "news-recommendation-tc_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctxfit_restated as rs  # noqa: E402
from nrk import _lib  # noqa: E402
from nrk.data import synth  # noqa: E402
from nrk.features import (CtxSpec, CtxTables, _finish_edges, ctx_feature_names, ctx_features,  # noqa: E402
                          ctx_fit_count_below, ctx_fit_stats, default_ctx_kinds)

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=synth.N_USERS)
ap.add_argument("--items", type=int, default=synth.N_ITEMS)
ap.add_argument("--pairs-per-user", type=int, default=30)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--skip-host", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "ctxfit_bench needs a GPU"
dev = torch.device("cuda")
warnings.simplefilter("ignore")

# ------------------------------------------------------------- the rows --
U, I, k, N = a.users, a.items, a.pairs_per_user, 3
log = synth.make_click_log(n_users=U, n_items=I)
art = synth.make_articles(I)
uid, off, hist_items, _ = synth.user_lists(log)
assert len(uid) == U
lens = np.diff(off)
hl = np.full((U, N), -1, np.int32)
for t in range(N):  # the last min(len, N) clicks, oldest first
    pos = off[1:] - np.minimum(lens, N) + t
    ok = t < np.minimum(lens, N)
    hl[ok, t] = hist_items[pos[ok]]
cat = art.category_id.astype(np.int64)
pairs = np.unique(np.repeat(np.arange(U), lens) * 1024 + cat[hist_items])  # distinct (user, category)
ucat_off = np.concatenate([[0], np.cumsum(np.bincount(pairs // 1024, minlength=U))]).astype(np.int64)
g = torch.Generator(device=dev).manual_seed(23)
unit = lambda n, d: torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=g), dim=1).contiguous()  # noqa: E731
d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)  # noqa: E731
content = torch.randn(I, 250, device=dev, dtype=torch.float64, generator=g)
present = torch.rand(I, device=dev, generator=g) >= 0.05
content[~present] = 0.0
created = d(synth.minmax_created(art), np.float64)
created[torch.rand(I, device=dev, generator=g) < 0.05] = float("nan")
ones = lambda n: torch.ones(n, dtype=torch.uint8, device=dev)  # noqa: E731
tables = CtxTables.from_device({
    "w2v": (torch.randn(I, 64, device=dev, generator=g) * 0.3).contiguous(), "w2v_ok": ones(I), "content": content,
    "flags": (present.to(torch.uint8) * 3).contiguous(), "created": created, "category": d(cat, np.int32),
    "hist_last": d(hl, np.int32), "hist_n": d(np.minimum(lens, N), np.int32), "ucat_off": d(ucat_off, np.int64),
    "ucat": d(pairs % 1024, np.int32), "user_yt": unit(U, 32), "user_yt_ok": ones(U), "item_yt": unit(I, 32),
    "item_yt_ok": ones(I)}, last_n=N)
names = ctx_feature_names(N)
kinds = default_ctx_kinds(names)
F = len(names)
n = U * k
raw = torch.empty((n, F), dtype=torch.float64, device=dev)
cand = torch.randint(0, I, (U, k), device=dev, generator=g, dtype=torch.int32)
score = torch.sort(torch.rand(U, k, device=dev, dtype=torch.float64, generator=g), 1, descending=True).values
CH = 4096
for u0 in range(0, U, CH):
    nu = min(CH, U - u0)
    goff = torch.arange(0, (nu + 1) * k, k, dtype=torch.int64, device=dev)
    gus = torch.arange(u0, u0 + nu, dtype=torch.int32, device=dev)
    ctx_features(tables, None, cand[u0:u0 + nu].reshape(-1).contiguous(), score[u0:u0 + nu].reshape(-1).contiguous(),
                 None, groups=(goff, gus, None), out_raw=raw[u0 * k:(u0 + nu) * k])
torch.cuda.synchronize()
del tables, content


# ------------------------------------------------------------ the times --
def timed(fn):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def wall(fn, reps=5):
    fn()
    s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(s), min(s), max(s)


L = _lib.lib()
ws = torch.empty(L.nrk_ctx_fit_workspace_bytes(n, F), dtype=torch.uint8, device=dev)
ranks = _finish_edges(None, n, 10, 0)
cols = list(range(F))
probes = torch.rand(F, 16, device=dev, dtype=torch.float64, generator=g)
res = {"users": U, "pairs_per_user": k, "rows": n, "features": F, "iters": a.iters, "tile": L.nrk_ctx_fit_tile(),
       "workspace_bytes": ws.numel()}
row_bytes, pass_bytes = n * F * 8, 2 * n * F * 8
res["algorithmic_bytes"] = {"keys": row_bytes + n * F * 8, "sort": 8 * pass_bytes, "summary": n * F * 8,
                            "stats_total": row_bytes + n * F * 8 + 8 * pass_bytes + n * F * 8}
for name, fn in (("fit_stats", lambda: ctx_fit_stats(raw, cols, kinds, ranks, workspace=ws)),
                 ("count_below", lambda: ctx_fit_count_below(n, F, probes, ws))):
    med, lo, hi = timed(fn)
    res[name + "_ms_median"] = round(med, 4)
    res[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
res["fit_stats_gbps"] = round(res["algorithmic_bytes"]["stats_total"] / res["fit_stats_ms_median"] / 1e6, 1)

split = None
try:  # one call's kernels by stage
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ctx_fit_stats(raw, cols, kinds, ranks, workspace=ws)
        torch.cuda.synchronize()
    stage = {"ctxfit_keys": "keys", "ctxfit_hist": "sort", "ctxfit_scan": "sort", "ctxfit_scatter": "sort",
             "ctxfit_distinct": "summary", "ctxfit_summary": "summary"}
    us = {"keys": 0.0, "sort": 0.0, "summary": 0.0}
    for ev in prof.events():
        for kn, st in stage.items():
            if kn in ev.name:
                us[st] += getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0)
    if all(v > 0 for v in us.values()):
        split = {st: round(v / 1e3, 4) for st, v in us.items()}
        split["gbps"] = {st: round(res["algorithmic_bytes"][st] / split[st] / 1e6, 1) for st in us}
except Exception as e:  # noqa: BLE001 -- the split is an extra; the timed numbers above stand without it
    res["kernel_split_error"] = repr(e)[:200]
res["kernel_split_ms"] = split

med, lo, hi = wall(lambda: CtxSpec.fit_device(raw, names, workspace_bytes=ws.numel()))
res["fit_device_wall_ms_median"] = round(med, 3)
res["fit_device_wall_ms_min_max"] = [round(lo, 3), round(hi, 3)]

if not a.skip_host:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = raw.cpu().numpy()
    t1 = time.perf_counter()
    typed = rs.typed_columns(host, names, kinds)
    CtxSpec.fit(typed, names)
    t2 = time.perf_counter()
    res["host_copy_s"] = round(t1 - t0, 3)
    res["host_fit_s"] = round(t2 - t1, 3)
    res["host_rows_fitted"] = "200,000 resampled (KBinsDiscretizer subsample)" if n > 200_000 else n
    # both deterministic on 200,000 rows: the specs are equal
    m = min(n, 200_000)
    rs.assert_specs_equal(CtxSpec.fit_device(raw[:m], names), CtxSpec.fit(rs.typed_columns(host[:m], names, kinds), names))
    res["specs_equal_on_rows"] = m
print(json.dumps(res))
