"""UserCF restated in numpy / plain Python: the checker of the GPU path on
random inputs (test_usercf_host.py pins it to reference-executed data).

Similarity (user_cf.py:31-66): items in ascending order, one sequential
``np.add.at`` per (item, entry of u) -- so every pair's terms are summed in
the reference's order with its association -- then the normalisation.
Recall (usercf_recaller.py:37-118): the reference's loops.
"""
import math

import numpy as np


def similarity(i_off, i_users, act):
    """Dense ids.  -> (acc [U, U] f64 normalised values, first [U, U] int64
    first slot or -1, cnt [U]).  Small inputs only (dense U x U)."""
    n_users = len(act)
    acc = np.zeros((n_users, n_users), np.float64)
    first = np.full((n_users, n_users), -1, np.int64)
    cnt = np.bincount(i_users, minlength=n_users).astype(np.int64)
    for i in range(len(i_off) - 1):
        a, b = int(i_off[i]), int(i_off[i + 1])
        lst = i_users[a:b]
        if not len(lst):
            continue
        pen = 1.0 / math.log(len(lst) + 1)
        slots = np.arange(a, b)
        for u in lst.tolist():
            keep = lst != u
            v = lst[keep]
            np.add.at(acc[u], v, (50.0 * (act[u] + act[v])) * pen)  # unbuffered: duplicates of v add twice
            new = first[u, v] < 0
            # the smallest slot of a duplicated v: walk them in reverse so the first one lands last
            first[u, v[new][::-1]] = slots[keep][new][::-1]
    nz = first >= 0
    den = np.sqrt((cnt[:, None] * cnt[None, :]).astype(np.float64))
    acc[nz] = acc[nz] / den[nz]
    return acc, first, cnt


def rows_in_order(acc, first):
    """-> per user the (v, value) list in the reference's dict order."""
    out = []
    for u in range(len(acc)):
        v = np.nonzero(first[u] >= 0)[0]
        v = v[np.argsort(first[u, v], kind="stable")]
        out.append((v, acc[u, v]))
    return out


def stable_top(vals, n):
    """Positions of sorted(..., key=value, reverse=True)[:n] (stable)."""
    return np.argsort(-np.asarray(vals), kind="stable")[:n]


def recall(user_id, topk, u2u, uit, created, hot, emb, sim_user_topk, loc_beta):
    """usercf_recaller.py:37-118, line for line (u2u: {u: {v: w}})."""
    if user_id not in uit or user_id not in u2u:
        return [(item, -i) for i, item in enumerate(hot[:topk])]
    hist = uit[user_id]
    hist_items = set(i for i, _ in hist)
    similar = sorted(u2u[user_id].items(), key=lambda x: x[1], reverse=True)[:sim_user_topk]
    rank = {}
    for sim_u, wuv in similar:
        if sim_u not in uit:
            continue
        for i, _ in uit[sim_u]:
            if i in hist_items:
                continue
            rank.setdefault(i, 0)
            loc_w, content_w, created_w = 1.0, 1.0, 1.0
            for loc, (j, _) in enumerate(hist):
                loc_w += loc_beta ** (len(hist) - loc)
                if emb:
                    if i in emb and j in emb[i]:
                        content_w += emb[i][j]
                    if j in emb and i in emb[j]:
                        content_w += emb[j][i]
                created_w += np.exp(0.8 ** np.abs(created[i] - created[j]))
            rank[i] += loc_w * content_w * created_w * wuv
    if len(rank) < topk:
        for i, item in enumerate(hot):
            if item in rank or item in hist_items:
                continue
            rank[item] = -i - 100
            if len(rank) == topk:
                break
    return sorted(rank.items(), key=lambda x: x[1], reverse=True)[:topk]
