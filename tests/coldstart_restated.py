"""Plain Python / numpy restatement of the cold-start filter and recall over
the dense arrays of include/nrk.h (coldstart_recaller.py:54-147), and of
RecallEnsemble's merge (fusion.py:488-538).  test_coldstart_host.py checks
both against reference-executed data; the GPU tests use them as the checker.
"""
import math

import numpy as np


def as_score(x):
    """make_golden_coldstart.as_score: the base lists hold an integral score as a Python int."""
    x = float(x)
    return int(x) if x.is_integer() else x


def lists_of(fx, prefix, score=float):
    """The {user: [(item, score), ...]} dict stored under ``prefix``."""
    off, it, sc = fx[prefix + "_offsets"], fx[prefix + "_items"].tolist(), fx[prefix + "_scores"].tolist()
    return {u: [(i, score(s)) for i, s in zip(it[off[n]:off[n + 1]], sc[off[n]:off[n + 1]])]
            for n, u in enumerate(fx[prefix + "_users"].tolist())}


def sets_of(fx, prefix):
    off, v = fx[prefix + "_offsets"], fx[prefix + "_values"].tolist()
    return {u: set(v[off[n]:off[n + 1]]) for n, u in enumerate(fx[prefix + "_users"].tolist())}


def recaller_args(fx):
    """The eight dict / set arguments the fixture's reference ColdStartRecaller got, in order."""
    prof = sets_of(fx, "prof")
    words = {u: w for u, w in zip(fx["words_users"].tolist(), fx["words_values"].tolist()) if u in prof}
    last = {u: w for u, w in zip(fx["last_users"].tolist(), fx["last_values"].tolist()) if u in prof}
    ids = fx["item_ids"].tolist()
    return (lists_of(fx, "base", as_score), prof, words, last, dict(zip(ids, fx["item_type"].tolist())),
            dict(zip(ids, fx["item_words"].tolist())), dict(zip(ids, fx["item_created"].tolist())),
            set(fx["clicked"].tolist()))


def keep_mask(list_off, item, prof, cat_off, cat, mean_words, last_created, item_type, item_words, item_created,
              item_clicked, words_tol=200.0, time_tol=0.25):
    """keep [N] uint8, kept [L] int32: the four rules pair by pair, in f64."""
    item = np.asarray(item).reshape(-1)
    keep = np.zeros(len(item), np.uint8)
    n_lists = len(list_off) - 1
    for l in range(n_lists):
        p = int(prof[l])
        if p < 0:
            continue
        cats = set(cat[cat_off[p]:cat_off[p + 1]].tolist())
        mw, lc = float(mean_words[p]), float(last_created[p])
        for e in range(int(list_off[l]), int(list_off[l + 1])):
            it = int(item[e])
            if it < 0:
                continue
            if int(item_type[it]) not in cats:
                continue
            if item_clicked[it]:
                continue
            if abs(float(item_words[it]) - mw) > words_tol:
                continue
            if abs(float(item_created[it]) - lc) > time_tol:
                continue
            keep[e] = 1
    kept = np.array([int(keep[list_off[l]:list_off[l + 1]].sum()) for l in range(n_lists)], np.int32)
    return keep, kept


def recall(q, list_off, score, keep, topk):
    """Per query: (positions, scores) of the stable descending top-k of the
    kept entries -- Python's sorted(..., reverse=True)[:topk] on float scores,
    so -0.0 ties with 0.0 and ties keep list order."""
    score = np.asarray(score, np.float64).reshape(-1)
    out = []
    for l in np.asarray(q).tolist():
        if l < 0:
            out.append(([], []))
            continue
        b, e = int(list_off[l]), int(list_off[l + 1])
        surv = [(i - b, float(score[i])) for i in range(b, e) if keep[i]]
        top = sorted(surv, key=lambda x: x[1], reverse=True)[:topk]
        out.append(([p for p, _ in top], [s for _, s in top]))
    return out


def check_recall(want, pos, sc, cnt, topk):
    """Compare restated lists with the kernel's padded [Q, topk] outputs."""
    pos, sc, cnt = np.asarray(pos), np.asarray(sc), np.asarray(cnt)
    for n, (wp, ws) in enumerate(want):
        m = int(cnt[n])
        assert m == len(wp), (n, m, len(wp))
        assert pos[n, :m].tolist() == wp, n
        assert sc[n, :m].tobytes() == np.array(ws, np.float64).tobytes(), n  # bit for bit, the sign of zero included
        assert (pos[n, m:] == -1).all() and (sc[n, m:] == 0.0).all(), n


def ensemble(lists, weights, strategy, topk):
    """One user's RecallEnsemble merge: ``lists`` in recaller order (a failed
    recaller's list left out), every list min-max normalised on its own, then
    the strategy per item and a stable descending sort."""
    sources = {}
    for lst, w in zip(lists, weights):
        if len(lst) == 0:
            continue
        scores = [s for _, s in lst]
        hi, lo = max(scores), min(scores)
        for it, s in lst:
            sources.setdefault(it, []).append((w, (s - lo) / (hi - lo) if hi > lo else 1.0))
    merged = {}
    for it, src in sources.items():
        if strategy == "weighted_sum":
            merged[it] = sum(w * s for w, s in src)
        elif strategy == "weighted_avg":
            merged[it] = sum(w * s for w, s in src) / sum(w for w, _ in src)
        elif strategy == "max_score":
            merged[it] = max(w * s for w, s in src)
        else:
            raise ValueError(strategy)
    assert not any(math.isnan(v) for v in merged.values())
    return sorted(merged.items(), key=lambda x: x[1], reverse=True)[:topk]
