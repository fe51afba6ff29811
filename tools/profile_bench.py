"""Profile features at the Tianchi shape (dev tool): the click log of
nrk.data.synth (250,000 users, 364,047 articles) with five device groups.
Times, with HIP events (warm-up, then the median of --iters launches in one
process), the four entry points of csrc/profile.hip on resident data -- the
user kernel, the item count, one MinMax column (nrk_fuse_minmax +
nrk_profile_scale), the labels of 30 pairs per user -- the wrapper's key sort,
and ProfileFeatures.from_device + encoded() end to end (host clock around a
device synchronise); reports ms and GB/s against the algorithmic bytes.
Beside them the vectorised host restatement (tests/profile_restated.py) on
the same data, once: the only host comparison there is -- the reference's own
loops (a groupby loop per user, a frame filter per article) are far slower.
Prints one JSON line.  DESIGN §4.13."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "news-recommendation-tc_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

import profile_restated as rs  # noqa: E402
from nrk import _lib, ops  # noqa: E402
from nrk.data import synth  # noqa: E402
from nrk.profile import ProfileFeatures  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=synth.N_USERS)
ap.add_argument("--items", type=int, default=synth.N_ITEMS)
ap.add_argument("--pairs-per-user", type=int, default=30)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--skip-host", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "profile_bench needs a GPU"

rng = np.random.default_rng(23)
log = synth.make_click_log(n_users=a.users, n_items=a.items)
art = synth.make_articles(a.items)
U, I, N = a.users, a.items, len(log)
device = rng.choice(np.array([1, 2, 3, 4, 5]), N, p=[0.55, 0.02, 0.35, 0.06, 0.02])
clicks = pd.DataFrame({"user_id": log.user_id, "click_article_id": log.click_article_id,
                       "click_timestamp": log.click_timestamp, "click_deviceGroup": device})
arts = pd.DataFrame({"click_article_id": art.article_id, "category_id": art.category_id,
                     "created_at_ts": art.created_at_ts, "words_count": art.words_count})

d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()  # noqa: E731
u_off = d(np.concatenate([[0], np.cumsum(np.bincount(log.user_id, minlength=U))]), np.int64)
item, ts, code = d(log.click_article_id, np.int32), d(log.click_timestamp, np.int64), d(device - 1, np.int32)
cat, created, words = d(art.category_id, np.int64), d(art.created_at_ts, np.int64), d(art.words_count, np.int64)
dev_values = np.arange(1, 6)
p = ops._ptr


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


def wall(fn, n=5):
    fn()
    s = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(s), min(s), max(s)


row = torch.repeat_interleave(torch.arange(U, dtype=torch.int64, device="cuda"), u_off[1:] - u_off[:-1])


def key_sort():
    key, _ = torch.sort(row * I + item)
    return (key - row * I).to(torch.int32)


sorted_item = key_sort()
out = [torch.empty(U, dtype=dt, device="cuda") for dt in (torch.int64, torch.float64, torch.float64, torch.int32,
                                                         torch.float64, torch.int32)]
cnt = torch.empty(I, dtype=torch.int64, device="cuda")
mm = torch.zeros(2, dtype=torch.float64, device="cuda")
P = U * a.pairs_per_user
pu = d(np.repeat(np.arange(U), a.pairs_per_user), np.int32)
pi = d(rng.integers(-1, I, P), np.int32)
lab = torch.empty(P, dtype=torch.int32, device="cuda")


def user_kernel():
    _lib.call("nrk_profile_user", p(u_off), U, p(item), p(ts), p(code), N, 5, p(sorted_item), p(words), I,
              *(p(o) for o in out), ops._stream())


def item_count():
    _lib.call("nrk_profile_item_count", p(item), N, I, p(cnt), ops._stream())


def scale_column():
    _lib.call("nrk_fuse_minmax", p(out[1]), U, p(mm), ops._stream())
    _lib.call("nrk_profile_scale", p(out[1]), U, p(mm), 0, p(out[4]), ops._stream())


def labels():
    _lib.call("nrk_profile_labels", p(pu), p(pi), P, p(out[5]), U, 1, p(lab), ops._stream())


def end_to_end():
    pf = ProfileFeatures.from_device(u_off, item, ts, code, dev_values, cat, created, words,
                                     repair_word_lookup=True, validate=False)
    return pf.encoded()


user_kernel()
res = {"users": U, "items": I, "clicks": N, "pairs": P, "iters": a.iters}
# algorithmic bytes: every input read once, every output written once
nbytes = {"user_kernel": N * (8 + 4 + 4) + (U + 1) * 8 + U * (8 + 8 + 8 + 4 + 8 + 4 + 4),
          "item_count": N * 4 + I * 8, "scale_column": U * 8 * 3, "labels": P * 12 + U * 4}
for name, fn in (("key_sort", key_sort), ("user_kernel", user_kernel), ("item_count", item_count),
                 ("scale_column", scale_column), ("labels", labels)):
    med, lo, hi = timed(fn)
    res[name + "_ms_median"] = round(med, 4)
    res[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
    if name in nbytes:
        res[name + "_gbps"] = round(nbytes[name] / med / 1e6, 1)
med, lo, hi = wall(end_to_end)
res["from_device_encoded_wall_ms_median"] = round(med, 3)
res["from_device_encoded_wall_ms_min_max"] = [round(lo, 3), round(hi, 3)]

if not a.skip_host:
    t0 = time.perf_counter()
    ucols = rs.user_columns(clicks, arts, repair_word_lookup=True)
    icols = rs.item_columns(clicks, arts)
    res["host_restatement_s"] = round(time.perf_counter() - t0, 3)
    # the two agree on this data (bit for bit), so the times compare like with like
    pf = ProfileFeatures.from_device(u_off, item, ts, code, dev_values, cat, created, words, repair_word_lookup=True)
    for f in ("user_click_count", "user_avg_time_gap", "avg_click_time", "avg_word_count"):
        assert pf.user_raw[f].cpu().numpy().tobytes() == ucols[f].to_numpy(np.float64).tobytes(), f
    assert pf.item_raw["article_popularity"].cpu().numpy().tobytes() == \
        icols["article_popularity"].to_numpy(np.float64).tobytes()
    assert pf.last_item.cpu().tolist() == ucols["last_item"].tolist()
print(json.dumps(res))
