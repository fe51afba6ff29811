"""Cold-start filter and recall at the config-2 shape (dev tool): 250,000 users
x 150 candidates over a 364,047-item table, about 6 of 24 categories per
user, topk 30.  Times nrk_coldstart_filter and nrk_coldstart_recall with HIP
events (warm-up, then the median of --iters launches in one process) and
reports ms and GB/s against the algorithmic bytes -- the lists read once
(item rows, offsets, profile rows; the scores too for the recall) plus the
outputs written -- beside the reference's per-pair dict loop
(coldstart_recaller.py:71-120, restated below) on a --cpu-users sample.
Prints one JSON line.  DESIGN §4.12."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "news-recommendation-tc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nrk import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=250_000)
ap.add_argument("--cands", type=int, default=150)
ap.add_argument("--items", type=int, default=364_047)
ap.add_argument("--cats", type=int, default=24)
ap.add_argument("--topk", type=int, default=30)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--cpu-users", type=int, default=2000)
a = ap.parse_args()

rng = np.random.default_rng(23)
U, K, I = a.users, a.cands, a.items
item = rng.integers(0, I, (U, K), dtype=np.int64).astype(np.int32)
item[rng.random((U, K)) < 0.002] = -1  # a few ids outside the article table
score = np.round(rng.random((U, K)), 2)
n_cat = rng.integers(1, 12, U)  # about 6 categories per user
cat_off = np.concatenate([[0], np.cumsum(n_cat)]).astype(np.int64)
owner = np.repeat(np.arange(U), n_cat)
draw = rng.random((U, a.cats)).argsort(1)  # a random subset per user, then ascending
cat = np.sort(np.where(np.arange(a.cats)[None, :] < n_cat[:, None], draw, a.cats), 1)
cat = cat[cat < a.cats].astype(np.int32)
assert len(cat) == cat_off[-1] and len(owner) == len(cat)
host = (np.arange(U + 1, dtype=np.int64) * K, item.reshape(-1), np.arange(U, dtype=np.int32), cat_off, cat,
        rng.uniform(100, 900, U), rng.random(U), rng.integers(0, a.cats, I).astype(np.int32),
        rng.integers(100, 900, I).astype(np.float64), rng.random(I), (rng.random(I) < 0.1).astype(np.uint8))
t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host]
d_score = torch.from_numpy(score.reshape(-1)).cuda()
q = torch.arange(U, dtype=torch.int64, device="cuda")
keep, kept = ops.coldstart_filter(*t)  # validates the tables once (and warms up)
pos, sc, cnt = ops.coldstart_recall(q, t[0], t[1], d_score, *t[2:], a.topk)
N = U * K
p = ops._ptr
tail = (p(t[2]), p(t[3]), p(t[4]), t[4].numel(), p(t[5]), p(t[6]), U, p(t[7]), p(t[8]), p(t[9]), p(t[10]), I,
        ops.CS_WORDS_TOL, ops.CS_TIME_TOL)
cap = min(K, ops.CS_MAX)


def filt():
    _lib.call("nrk_coldstart_filter", p(t[0]), U, p(t[1]), N, *tail, p(keep), p(kept), ops._stream())


def recall():
    _lib.call("nrk_coldstart_recall", p(q), U, p(t[0]), U, p(t[1]), p(d_score), N, *tail, cap, a.topk, p(pos), p(sc),
              p(cnt), ops._stream())


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


f_ms, r_ms = timed(filt), timed(recall)
f_bytes = N * 4 + (U + 1) * 8 + U * 4 + N + U * 4
r_bytes = N * 12 + (U + 1) * 8 + U * 4 + U * 8 + U * a.topk * 12 + U * 4

# the reference's loop over a sample of users: six dict / set lookups per pair
S = min(a.cpu_users, U)
ids = list(range(I))
item_type_d = dict(zip(ids, host[7].tolist()))
item_words_d = dict(zip(ids, host[8].tolist()))
item_created_d = dict(zip(ids, host[9].tolist()))
clicked_s = set(np.flatnonzero(host[10]).tolist())
types_d = {u: set(cat[cat_off[u]:cat_off[u + 1]].tolist()) for u in range(S)}
words_d, last_d = dict(enumerate(host[5][:S].tolist())), dict(enumerate(host[6][:S].tolist()))
base = {u: list(zip(item[u].tolist(), score[u].tolist())) for u in range(S)}
t0 = time.perf_counter()
n_kept = 0
for u, lst in base.items():
    if u not in types_d:
        continue
    ts_, mw, lc = types_d[u], words_d[u], last_d[u]
    out = []
    for it, s in lst:
        if it not in item_type_d or it not in item_words_d or it not in item_created_d:
            continue
        if item_type_d[it] not in ts_ or it in clicked_s:
            continue
        if abs(item_words_d[it] - mw) > 200 or abs(item_created_d[it] - lc) > 0.25:
            continue
        out.append((it, s))
    n_kept += len(out)
cpu_s = time.perf_counter() - t0
assert n_kept == int(kept[:S].sum().item()), "the host loop and the kernel disagree"

kc = kept.cpu().numpy()
print(json.dumps({
    "users": U, "cands": K, "items": I, "cats": a.cats, "topk": a.topk, "iters": a.iters,
    "survivors_per_user_mean": round(float(kc.mean()), 3), "survivors_per_user_max": int(kc.max()),
    "filter_ms_median": round(f_ms[0], 4), "filter_ms_min_max": [round(f_ms[1], 4), round(f_ms[2], 4)],
    "filter_gbps": round(f_bytes / f_ms[0] / 1e6, 1), "filter_bytes": f_bytes,
    "recall_ms_median": round(r_ms[0], 4), "recall_ms_min_max": [round(r_ms[1], 4), round(r_ms[2], 4)],
    "recall_gbps": round(r_bytes / r_ms[0] / 1e6, 1), "recall_bytes": r_bytes,
    "cpu_loop_users": S, "cpu_loop_s": round(cpu_s, 4),
    "cpu_loop_s_scaled_to_all_users": round(cpu_s * U / S, 1),
}))
