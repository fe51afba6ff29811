"""CPU oracle for the nrk hot path -- TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg may import this module, and only as the checker (or the
timed CPU baseline).  The product path (``nrk``) never imports it and fails
loudly when its HIP library is missing.

Each function restates the reference (file:line cited) in numpy / C:

* ``ip_topk``            -- faiss.IndexFlatIP contract, youtubednn_recaller.py:493-494, :520
* ``youtubednn_recall``  -- YoutubeDNNRecaller.recall, youtubednn_recaller.py:497-535
* ``embedding_similarity`` / ``embedding_sim_dict``
                         -- EmbeddingSimilarity.calculate, similarity/embedding.py:35-62
* ``tower_user``         -- YoutubeDNN.forward + _extract_embeddings re-norm, :129-178, :467-470
* ``tower_item``         -- get_item_embedding + re-norm, :184-188, :485-489
* ``tower_user_layers_f64`` / ``tower_item_f64``
                         -- the same two expressions in float64 (the yardstick of
                            tests/test_tower_host.py and tests/test_gpu_tower_shapes.py)
* ``itemcf_sim``         -- ItemCFSimilarity.calculate, item_cf.py:17-89
* ``itemcf_topn``        -- ItemCFRecaller._precompute_topk_similar_items, itemcf_recaller.py:41-54
* ``itemcf_recall``      -- ItemCFRecaller.recall, itemcf_recaller.py:56-129
* ``din_forward``        -- Dice / ActivationUnit / DINModel.forward, DIN.py:29-286
* ``din_forward_f64``    -- the same in float64, per Dice batch (the yardstick of
                            tests/test_din_host.py and tests/test_gpu_din_shapes.py)
* ``fuse``               -- RecallFusion.fuse, recall/fusion.py:67-342
* ``ctx_features``       -- FeatureExtractor._extract_context_features,
                            features/feature_extractor.py:440-723

Pinning: tests/test_oracle_golden.py checks every function against the golden
fixtures produced by executing the reference (tests/golden/make_golden.py).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build():
    subprocess.run(["make", "-s", "-C", HERE], check=True)


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(HERE, "libnrk_oracle.so")
        if not os.path.exists(path):
            build()
        L = ctypes.CDLL(path)
        P = ctypes.c_void_p
        i64, i32, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_double
        L.oracle_ip_topk.argtypes = [P, i64, P, i64, ctypes.c_int, ctypes.c_int, P, P, P, ctypes.c_int]
        L.oracle_ip_topk.restype = None
        L.oracle_itemcf_sim.argtypes = [i64, P, P, P, P, i32, f64, f64, f64, f64, f64, i64, P, P, P, P, P]
        L.oracle_itemcf_sim.restype = i64
        L.oracle_itemcf_sim_omp.argtypes = [i64, P, P, P, P, i32, f64, f64, f64, f64, f64, ctypes.c_int, P, P, P,
                                            P, P]
        L.oracle_itemcf_sim_omp.restype = i64
        L.oracle_topn_rows.argtypes = [i64, P, P, P, ctypes.c_int, P, P, P]
        L.oracle_topn_rows.restype = None
        L.oracle_itemcf_recall.argtypes = [i64, P, P, P, P, P, P, ctypes.c_int, P, P, ctypes.c_int,
                                           ctypes.c_int, f64, f64, i32, P, P, P]
        L.oracle_itemcf_recall.restype = None
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# --------------------------------------------------------------------------
# Recall: exact top-K and the recall() wrapper
# --------------------------------------------------------------------------
def ip_topk(users, items, k, nthreads=0, exact=False):
    """Top-k rows of ``items`` by exact inner product with each user row.

    Returns (scores f32 [nu,k], rows i64 [nu,k]) (+ fp64 exact scores)."""
    users = np.ascontiguousarray(users, dtype=np.float32)
    items = np.ascontiguousarray(items, dtype=np.float32)
    nu, d = users.shape
    ni = items.shape[0]
    s = np.empty((nu, k), np.float32)
    r = np.empty((nu, k), np.int64)
    e = np.empty((nu, k), np.float64) if exact else None
    lib().oracle_ip_topk(_p(users), nu, _p(items), ni, d, k, _p(s), _p(r),
                         _p(e) if exact else None, int(nthreads))
    return (s, r, e) if exact else (s, r)


def youtubednn_recall(scores, rows, user_rawid_2_index, item_index_2_rawid, user_ids, topk):
    """YoutubeDNNRecaller.recall over a precomputed (k+1) search result.

    Drops rank 0 (:524), maps Faiss row r -> item_index_2_rawid[r] (:528-529,
    the A3 quirk), skips labels not in the mapping, unknown users -> []."""
    out = {}
    for u in user_ids:
        idx = user_rawid_2_index.get(u)
        if idx is None or idx >= scores.shape[0]:
            out[u] = []
            continue
        res = []
        for i in range(1, scores.shape[1]):
            r = int(rows[idx, i])
            if r in item_index_2_rawid:
                res.append((item_index_2_rawid[r], float(scores[idx, i])))
            if len(res) >= topk:
                break
        out[u] = res
    return out


def embedding_similarity(emb, topk, nthreads=0):
    """EmbeddingSimilarity.calculate's arithmetic (similarity/embedding.py:35-50):
    numpy float32 row normalisation (:41) then the IndexFlatIP self-search for
    topk+1 neighbours (:46-50).  Returns (normalised rows, scores, rows)."""
    x = np.ascontiguousarray(emb, dtype=np.float32)
    xn = np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))
    s, r = ip_topk(xn, xn, topk + 1, nthreads=nthreads)
    return xn, s, r


def embedding_sim_dict(ids, scores, rows):
    """The dict build of embedding.py:52-62: row -> raw id, column 0 dropped
    (whatever row it holds), later duplicate keys overwrite."""
    i2r = {n: int(x) for n, x in enumerate(ids)}
    out = {}
    for t in range(scores.shape[0]):
        d = out.setdefault(i2r[t], {})
        for r, v in zip(rows[t, 1:].tolist(), scores[t, 1:].tolist()):
            d[i2r[r]] = float(v)
    return out


# --------------------------------------------------------------------------
# Two-tower forward (fp32, numpy)
# --------------------------------------------------------------------------
def tower_user(user_emb, item_emb, uid, hist, hist_len, w0, b0, w1, b1):
    """YoutubeDNN.forward (youtubednn_recaller.py:129-182) + numpy re-norm (:467-470), two layers."""
    return tower_user_layers(user_emb, item_emb, uid, hist, hist_len, [(w0, b0), (w1, b1)])


def tower_user_layers(user_emb, item_emb, uid, hist, hist_len, layers):
    """Any depth: user_tower = [Linear, ReLU, Dropout] per hidden unit
    (youtubednn_recaller.py:105-112); ``layers`` = [(W_l, b_l), ...]."""
    f32 = np.float32
    ue = user_emb[uid].astype(f32)
    he = item_emb[hist].astype(f32)
    T = hist.shape[1]
    mask = (np.arange(T)[None, :] < hist_len[:, None]).astype(f32)[:, :, None]
    avg = (he * mask).sum(1, dtype=f32) / (hist_len.astype(f32)[:, None] + f32(1e-8))
    x = np.concatenate([ue, avg.astype(f32)], 1)
    for w, b in layers:
        x = np.maximum(x @ w.T.astype(f32) + b.astype(f32), 0).astype(f32)
    n = np.maximum(np.sqrt((x * x).sum(1, keepdims=True, dtype=f32)), f32(1e-12))
    x = (x / n).astype(f32)
    n2 = np.linalg.norm(x, axis=1, keepdims=True)
    n2[n2 == 0] = 1
    return (x / n2).astype(f32)


def tower_item(item_emb, ids):
    f32 = np.float32
    x = item_emb[ids].astype(f32)
    n = np.maximum(np.sqrt((x * x).sum(1, keepdims=True, dtype=f32)), f32(1e-12))
    x = (x / n).astype(f32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)


# --------------------------------------------------------------------------
# Two-tower forward, the same expression in float64 (the bar's yardstick:
# tests/test_tower_host.py measures the fp32 functions above against these)
# --------------------------------------------------------------------------
def tower_user_f64_parts(user_emb, item_emb, uid, hist, hist_len, layers, drop_last=False, len_plus=0):
    """``tower_user_layers`` with every operation in float64 on the fp32
    inputs.  Slots at or past ``hist_len`` are ignored by masking the indices
    before the gather (their contents are never read as rows to add); the
    divisor is float32(len) + float32(1e-8) widened.  Returns (out [n, D],
    [z_l [n, w_l] per layer]: every layer before its ReLU).

    Two deliberately wrong variants for the tests' sensitivity check:
    ``drop_last`` leaves history slot len - 1 out of the sum, ``len_plus``
    is added to the divisor's length."""
    f64 = np.float64
    hist_len = np.asarray(hist_len)
    n, T = hist.shape
    out = np.empty((n, layers[-1][0].shape[0]), f64)
    pre = [np.empty((n, w.shape[0]), f64) for w, _ in layers]
    for lo in range(0, n, 4096):  # bounds the [rows, T, D] float64 gather
        sl = slice(lo, min(n, lo + 4096))
        ln = hist_len[sl].astype(np.int64)
        live = np.arange(T)[None, :] < (ln - (1 if drop_last else 0))[:, None]
        he = item_emb[np.where(live, hist[sl], 0)].astype(f64)
        ssum = np.where(live[:, :, None], he, 0.0).sum(1)
        den = ((ln + len_plus).astype(np.float32) + np.float32(1e-8)).astype(f64)
        x = np.concatenate([user_emb[uid[sl]].astype(f64), ssum / den[:, None]], 1)
        for l, (w, b) in enumerate(layers):
            pre[l][sl] = x @ w.astype(f64).T + b.astype(f64)
            x = np.maximum(pre[l][sl], 0.0)
        x = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
        n2 = np.sqrt((x * x).sum(1, keepdims=True))
        n2[n2 == 0] = 1.0
        out[sl] = x / n2
    return out, pre


def tower_user_layers_f64(user_emb, item_emb, uid, hist, hist_len, layers):
    return tower_user_f64_parts(user_emb, item_emb, uid, hist, hist_len, layers)[0]


def tower_item_f64(item_emb, ids):
    """``tower_item`` in float64; like the reference (youtubednn_recaller.py:
    487-489) the second division is unguarded: an all-zero row gives NaN."""
    x = item_emb[ids].astype(np.float64)
    x = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
    with np.errstate(invalid="ignore"):
        return x / np.sqrt((x * x).sum(1, keepdims=True))


# --------------------------------------------------------------------------
# ItemCF
# --------------------------------------------------------------------------
LOC_ALPHA, LOC_ALPHA_REV, LOC_BETA, TIME_ALPHA, CREATED_ALPHA = 1.0, 0.7, 0.9, 0.7, 0.8


def itemcf_sim(offsets, items, ts, created, n_items):
    """Dense-id ItemCF similarity.  Returns (i, j, v, row_rank, cnt) with the
    (i, j) entries in global first-insertion order."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    items = np.ascontiguousarray(items, np.int32)
    ts = np.ascontiguousarray(ts, np.int64)
    created = np.ascontiguousarray(created, np.float64)
    L = np.diff(offsets)
    cap = int((L * L).sum()) + 1
    oi = np.empty(cap, np.int32)
    oj = np.empty(cap, np.int32)
    ov = np.empty(cap, np.float64)
    rank = np.empty(n_items, np.int64)
    cnt = np.empty(n_items, np.int64)
    n = lib().oracle_itemcf_sim(len(offsets) - 1, _p(offsets), _p(items), _p(ts), _p(created),
                                n_items, LOC_ALPHA, LOC_ALPHA_REV, LOC_BETA, TIME_ALPHA,
                                CREATED_ALPHA, cap, _p(oi), _p(oj), _p(ov), _p(rank), _p(cnt))
    assert n >= 0
    return oi[:n], oj[:n], ov[:n], rank, cnt


def itemcf_sim_omp(offsets, items, ts, created, n_items, nthreads):
    """oracle_itemcf_sim on ``nthreads`` OpenMP threads (rows partitioned by
    i % T; bit-identical values, per-thread first-insertion order).  A CPU
    baseline variant (bench.py ItemCF leg), not a checker.  Returns (i, j, v)."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    items = np.ascontiguousarray(items, np.int32)
    ts = np.ascontiguousarray(ts, np.int64)
    created = np.ascontiguousarray(created, np.float64)
    L = np.diff(offsets)
    cap = int((L * L).sum()) + 1
    oi = np.empty(cap, np.int32)
    oj = np.empty(cap, np.int32)
    ov = np.empty(cap, np.float64)
    base = np.zeros(nthreads, np.int64)
    n = np.zeros(nthreads, np.int64)
    lib().oracle_itemcf_sim_omp(len(offsets) - 1, _p(offsets), _p(items), _p(ts), _p(created), n_items,
                                LOC_ALPHA, LOC_ALPHA_REV, LOC_BETA, TIME_ALPHA, CREATED_ALPHA, int(nthreads),
                                _p(oi), _p(oj), _p(ov), _p(base), _p(n))
    take = np.concatenate([np.arange(b, b + c) for b, c in zip(base, n)]) if nthreads else np.zeros(0, np.int64)
    return oi[take], oj[take], ov[take]


def itemcf_sim_pyloop(user_item_time, created):
    """item_cf.py:33-84 as the reference writes it: Python dict loops over
    ``user_item_time`` ({user: [(item, time), ...]}) with WeightCalculator's
    np.exp / np.abs / math.log (weights.py:7-60) per pair.  A CPU baseline
    variant (the reference's own per-pair cost), not a checker.  Returns
    {i: {j: sim}}."""
    import math

    i2i, cnt = {}, {}
    for _, lst in user_item_time.items():
        for loc1, (i, ti) in enumerate(lst):
            cnt[i] = cnt.get(i, 0) + 1
            i2i.setdefault(i, {})
            for loc2, (j, tj) in enumerate(lst):
                if i == j:
                    continue
                la = LOC_ALPHA if loc2 > loc1 else LOC_ALPHA_REV
                loc_w = la * (LOC_BETA ** (np.abs(loc2 - loc1) - 1))
                click_w = np.exp(TIME_ALPHA ** np.abs(ti - tj))
                created_w = np.exp(CREATED_ALPHA ** np.abs(created[i] - created[j]))
                pen = 1.0 / math.log(len(lst) + 1)
                i2i[i].setdefault(j, 0)
                i2i[i][j] += loc_w * click_w * created_w * pen
    for i, row in i2i.items():
        for j, w in row.items():
            row[j] = w / math.sqrt(cnt[i] * cnt[j])
    return i2i


def sim_to_rows(i, j, v, n_items):
    """Group first-insertion-ordered entries into CSR rows (insertion order kept)."""
    order = np.argsort(i, kind="stable")
    off = np.zeros(n_items + 1, np.int64)
    np.add.at(off, i + 1, 1)
    return np.cumsum(off), j[order].astype(np.int32), v[order]


def itemcf_topn(row_off, cols, vals, topn=20):
    n_rows = len(row_off) - 1
    oc = np.full((n_rows, topn), -1, np.int32)
    ov = np.zeros((n_rows, topn), np.float64)
    cnt = np.zeros(n_rows, np.int32)
    lib().oracle_topn_rows(n_rows, _p(np.ascontiguousarray(row_off, np.int64)),
                           _p(np.ascontiguousarray(cols, np.int32)),
                           _p(np.ascontiguousarray(vals, np.float64)), topn, _p(oc), _p(ov), _p(cnt))
    return oc, ov, cnt


def itemcf_recall(q_slot, offsets, items, nbr_cols, nbr_vals, nbr_cnt, created, hot, topk, n_items):
    q_slot = np.ascontiguousarray(q_slot, np.int64)
    nq = len(q_slot)
    topn = nbr_cols.shape[1]
    oi = np.zeros((nq, topk), np.int32)
    os_ = np.zeros((nq, topk), np.float64)
    oc = np.zeros(nq, np.int32)
    hot = np.ascontiguousarray(hot, np.int32)
    lib().oracle_itemcf_recall(nq, _p(q_slot), _p(np.ascontiguousarray(offsets, np.int64)),
                               _p(np.ascontiguousarray(items, np.int32)),
                               _p(np.ascontiguousarray(nbr_cols, np.int32)),
                               _p(np.ascontiguousarray(nbr_vals, np.float64)),
                               _p(np.ascontiguousarray(nbr_cnt, np.int32)), topn,
                               _p(np.ascontiguousarray(created, np.float64)), _p(hot), len(hot),
                               topk, LOC_BETA, CREATED_ALPHA, n_items, _p(oi), _p(os_), _p(oc))
    return oi, os_, oc


# --------------------------------------------------------------------------
# DIN (fp32 numpy restatement of DIN.py:29-286)
# --------------------------------------------------------------------------
def _dice(x):
    f32 = np.float32
    x = x.astype(f32)
    mean = x.mean(0, keepdims=True, dtype=np.float64).astype(f32)
    std = x.astype(np.float64).std(0, ddof=1, keepdims=True).astype(f32)
    xn = (x - mean) / (std + f32(1e-8))
    p = (1.0 / (1.0 + np.exp(-xn.astype(np.float64)))).astype(f32)
    return (p * x + (f32(1) - p) * f32(0.01) * x).astype(f32)


def din_forward(sd, user, item, hist, ctx, mask, feats, round_bf16=False):
    """sd: DINModel state_dict as numpy; feats: (user_feats, item_feats, ctx_feats).

    Returns (probs [B], logits [B], att [B,T]).  ``round_bf16`` rounds every
    embedding table to bf16 first (storage-only bf16, fp32 math)."""
    f32 = np.float32
    uf, itf, cf = feats

    def tab(group, f):
        w = sd[f"{group}.{f}.weight"].astype(f32)
        return bf16_round(w) if round_bf16 else w

    U = np.concatenate([tab("user_profile_embedding_dict", f)[user[:, n]] for n, f in enumerate(uf)], 1)
    Q = np.concatenate([tab("item_embedding_dict", f)[item[:, n]] for n, f in enumerate(itf)], 1)
    K = np.concatenate([tab("item_embedding_dict", f)[hist[:, :, n]] for n, f in enumerate(itf)], 2)
    C = (np.concatenate([tab("context_embedding_dict", f)[ctx[:, n]] for n, f in enumerate(cf)], 1)
         if len(cf) else np.zeros((len(user), 0), f32))
    B, T, d = K.shape
    q = np.broadcast_to(Q[:, None, :], (B, T, d))
    X = np.concatenate([K, q, q - K, q * K], 2).astype(f32)
    a0w, a0b = sd["activation_unit.mlp.0.weight"].astype(f32), sd["activation_unit.mlp.0.bias"].astype(f32)
    a2w, a2b = sd["activation_unit.mlp.2.weight"].astype(f32), sd["activation_unit.mlp.2.bias"].astype(f32)
    h = (X @ a0w.T + a0b).astype(f32)
    h = _dice(h)
    w = (h @ a2w.T + a2b).astype(f32)[:, :, 0]
    w = (w * mask.astype(f32)).astype(f32)
    wh = (w[:, :, None] * K).sum(1, dtype=f32)
    x = np.concatenate([U, C, Q, wh], 1).astype(f32)
    for li in (0, 2):
        x = (x @ sd[f"mlp.{li}.weight"].astype(f32).T + sd[f"mlp.{li}.bias"].astype(f32)).astype(f32)
        x = _dice(x)
    logit = (x @ sd["mlp.4.weight"].astype(f32).T + sd["mlp.4.bias"].astype(f32)).astype(f32)[:, 0]
    prob = (1.0 / (1.0 + np.exp(-logit.astype(np.float64)))).astype(f32)
    return prob, logit, w


# --------------------------------------------------------------------------
# DIN forward, the same expression in float64 (the bar's yardstick:
# tests/test_din_host.py measures din_forward above against it)
# --------------------------------------------------------------------------
def _pow2_scale(mx):
    """The kernels' power-of-two scale: max |x| in [2^(e-1), 2^e) -> 2^(14-e)."""
    return 1.0 if not mx > 0 else float(np.ldexp(1.0, 14 - int(np.frexp(np.float32(mx))[1])))


def _fp16_at(x, s):
    """x rounded to the nearest fp16 at the power-of-two scale s."""
    with np.errstate(over="ignore"):
        return (np.asarray(x, np.float64) * s).astype(np.float16).astype(np.float64) / s


def _din_batch_f64(tabs, W, user, item, hist, ctx, mask, mut, stats=None):
    """One Dice batch of ``din_forward_f64``.  ``stats``: per Dice layer the
    (mean, std) to normalise with instead of the batch's own.  Returns
    (probs, logits, att, [(mean, std) per Dice layer])."""
    f64 = np.float64
    tu, ti, tc = tabs
    B, T = mask.shape
    ddof = mut.get("ddof", 1)
    used = []

    def dice(x, for_stats=None):
        """Dice (DIN.py:39-44): batch mean and std over axis 0."""
        given = stats[len(used)] if stats is not None else None
        if given is not None:
            mean, std = given
        else:
            xs = x if for_stats is None else for_stats
            with np.errstate(invalid="ignore", divide="ignore"):
                mean, std = xs.mean(0, keepdims=True), xs.std(0, ddof=ddof, keepdims=True)
        used.append((mean, std))
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-((x - mean) / (std + 1e-8))))
        return p * x + (1.0 - p) * 0.01 * x

    cat = lambda ts, idx: np.concatenate([t[idx[..., n]] for n, t in enumerate(ts)], -1)  # noqa: E731
    U, Q = cat(tu, user), cat(ti, item)
    C = cat(tc, ctx) if tc else np.zeros((B, 0), f64)
    h = np.empty((B, T, W["a0b"].shape[0]), f64)
    K = np.empty((B, T, Q.shape[1]), f64)
    for lo in range(0, B, 4096):  # bounds the [rows, T, 4d] concatenation (DIN.py:105-114)
        sl = slice(lo, min(B, lo + 4096))
        k = cat(ti, hist[sl])
        q = np.broadcast_to(Q[sl, None, :], k.shape)
        qk = q * k
        if mut.get("p_lo_dropped"):
            qk = _fp16_at(qk, mut["_s_tab"] ** 2)
        h[sl] = np.concatenate([k, q, q - k, qk], 2) @ W["a0w"].T + W["a0b"]
        K[sl] = k
    hs = None
    if mut.get("pad_row_zero"):
        hs = np.where(((mask == 0) & (hist == 0).all(2))[:, :, None], 0.0, h)
    w = (dice(h, hs) @ W["a2w"].T + W["a2b"])[:, :, 0] * mask.astype(f64)  # DIN.py:114-124
    if mut.get("drop_last"):
        live = mask != 0
        last = T - 1 - np.argmax(live[:, ::-1], 1)
        rows = np.flatnonzero(live.any(1))
        w[rows, last[rows]] = 0.0
    wh = (w[:, :, None] * K).sum(1)  # DIN.py:276
    x = np.concatenate([U, C, Q, wh], 1)  # DIN.py:279
    x = dice(x @ W["m0w"].T + W["m0b"])
    x = dice(x @ W["m2w"].T + W["m2b"])
    logit = (x @ W["m4w"].T + W["m4b"])[:, 0]
    with np.errstate(over="ignore"):
        prob = 1.0 / (1.0 + np.exp(-logit))
    return prob, logit, w, used


def din_forward_f64(sd, user, item, hist, ctx, mask, feats, round_bf16=False, batch_size=None, **mutations):
    """``din_forward`` (DIN.py:29-44 Dice, :105-124 ActivationUnit, :214-286
    DINModel.forward) with every operation in float64 on the fp32 (or
    bf16-rounded) parameters.  ``batch_size``: the samples are consecutive
    Dice batches of that many rows (DINRanker.predict's loop, DIN.py:1245-1283),
    gathered and scored one batch at a time; a batch of one row is NaN.
    Returns (probs [B], logits [B], att [B, T]) in float64.

    Deliberately wrong variants for tests/test_din_host.py's sensitivity check:
    ``drop_last`` zeroes the attention weight of the last position with a
    non-zero mask; ``ddof=0`` is the biased std; ``w0_hi_only`` /
    ``w1_hi_only`` keep only the fp16 part of mlp.0 / mlp.2's weight at the
    kernels' power-of-two scale (max |W| < 2^14); ``p_lo_dropped`` rounds q*k
    to fp16 at the position-major kernel's scale s^2 (max |table| s in
    [2^6, 2^7)); ``neighbour_stats=l`` normalises Dice layer l (0: attention,
    1, 2: the MLP) of batch s with the statistics batch s+1 has in a correct
    run (the last with the first's); ``pad_row_zero`` takes the attention
    hidden rows of padding positions (mask 0, every index 0) as 0 in the
    column statistics."""
    f64 = np.float64
    uf, itf, cf = feats

    def tab(group, f):
        w = sd[f"{group}.{f}.weight"].astype(np.float32)
        return (bf16_round(w) if round_bf16 else w).astype(f64)

    tabs = ([tab("user_profile_embedding_dict", f) for f in uf], [tab("item_embedding_dict", f) for f in itf],
            [tab("context_embedding_dict", f) for f in cf])
    g = lambda k: np.asarray(sd[k], np.float32).astype(f64)  # noqa: E731
    W = {"a0w": g("activation_unit.mlp.0.weight"), "a0b": g("activation_unit.mlp.0.bias"),
         "a2w": g("activation_unit.mlp.2.weight"), "a2b": g("activation_unit.mlp.2.bias")}
    for li in (0, 2, 4):
        W[f"m{li}w"], W[f"m{li}b"] = g(f"mlp.{li}.weight"), g(f"mlp.{li}.bias")
    mut = dict(mutations)
    unknown = set(mut) - {"drop_last", "ddof", "w0_hi_only", "w1_hi_only", "p_lo_dropped", "neighbour_stats",
                          "pad_row_zero"}
    assert not unknown, unknown
    for key, name in (("w0_hi_only", "m0w"), ("w1_hi_only", "m2w")):
        if mut.get(key):
            W[name] = _fp16_at(W[name], _pow2_scale(np.abs(W[name]).max()))
    if mut.get("p_lo_dropped"):
        mut["_s_tab"] = _pow2_scale(max(np.abs(t).max() for grp in tabs for t in grp)) / 128.0
    N, T = mask.shape
    S = N if batch_size is None or batch_size >= N else int(batch_size)
    segs = [slice(s, min(N, s + S)) for s in range(0, N, S)]
    prob, logit, att = np.empty(N, f64), np.empty(N, f64), np.empty((N, T), f64)

    def run(sl, stats=None):
        if sl.stop - sl.start < 2 and mut.get("ddof", 1) == 1:  # torch.std of one row (DIN.py:41)
            return np.full(1, np.nan), np.full(1, np.nan), np.full((1, T), np.nan), None
        return _din_batch_f64(tabs, W, user[sl], item[sl], hist[sl], ctx[sl], mask[sl], mut, stats)

    nb = mut.get("neighbour_stats")
    if nb is None or nb is False:
        for sl in segs:
            prob[sl], logit[sl], att[sl], _ = run(sl)
        return prob, logit, att
    own = [run(sl)[3] for sl in segs]
    for n, sl in enumerate(segs):
        if own[n] is None or own[(n + 1) % len(segs)] is None:  # a batch of one row has no statistics
            prob[sl], logit[sl], att[sl], _ = run(sl)
            continue
        st = list(own[n])
        st[int(nb)] = own[(n + 1) % len(segs)][int(nb)]
        # later layers keep this batch's own statistics of its (now different) values
        prob[sl], logit[sl], att[sl], _ = run(sl, _StatsFrom(st, int(nb)))
    return prob, logit, att


class _StatsFrom:
    """Dice statistics override for layer ``l`` only (None elsewhere)."""

    def __init__(self, st, l):
        self.st, self.l = st, l

    def __getitem__(self, n):
        return self.st[n] if n == self.l else None


class DinTorchCPU:
    """torch-CPU eval forward in the reference's own formulation
    (DINModel.forward, DIN.py:214-286: nn.Embedding lookups, ActivationUnit
    Linear(512->36) on [k, q, q-k, q*k] + Dice + Linear(36->1) * mask, the
    weighted history sum, Linear/Dice MLP, sigmoid) -- the CPU baseline of
    BASELINE.md §3 for config 3, run on pre-encoded int tensors with every
    host thread torch has.  Bench-only (cpu_baseline leg)."""

    def __init__(self, sd, feats, round_bf16=False):
        import torch

        uf, itf, cf = feats
        t = lambda a: torch.from_numpy(np.ascontiguousarray(bf16_round(a) if round_bf16 else a, np.float32))  # noqa
        self.U = [t(sd[f"user_profile_embedding_dict.{f}.weight"]) for f in uf]
        self.I = [t(sd[f"item_embedding_dict.{f}.weight"]) for f in itf]
        self.C = [t(sd[f"context_embedding_dict.{f}.weight"]) for f in cf]
        g = lambda k: torch.from_numpy(np.ascontiguousarray(sd[k], np.float32))  # noqa: E731
        self.a0w, self.a0b = g("activation_unit.mlp.0.weight"), g("activation_unit.mlp.0.bias")
        self.a2w, self.a2b = g("activation_unit.mlp.2.weight"), g("activation_unit.mlp.2.bias")
        self.m = [(g(f"mlp.{i}.weight"), g(f"mlp.{i}.bias")) for i in (0, 2, 4)]

    @staticmethod
    def _dice(x):
        import torch

        mean, std = x.mean(0), x.std(0)
        p = torch.sigmoid((x - mean) / (std + 1e-8))
        return p * x + (1 - p) * 0.01 * x

    def __call__(self, user, item, hist, ctx, mask):
        import torch
        import torch.nn.functional as F

        with torch.no_grad():
            u = torch.cat([E[user[:, n]] for n, E in enumerate(self.U)], 1)
            q = torch.cat([E[item[:, n]] for n, E in enumerate(self.I)], 1)
            k = torch.cat([E[hist[:, :, n]] for n, E in enumerate(self.I)], 2)
            c = torch.cat([E[ctx[:, n]] for n, E in enumerate(self.C)], 1)
            qq = q.unsqueeze(1).expand_as(k)
            h = self._dice(F.linear(torch.cat([k, qq, qq - k, qq * k], -1), self.a0w, self.a0b))
            w = F.linear(h, self.a2w, self.a2b) * mask.unsqueeze(-1)
            x = torch.cat([u, c, q, (w * k).sum(1)], 1)
            x = self._dice(F.linear(x, *self.m[0]))
            x = self._dice(F.linear(x, *self.m[1]))
            return torch.sigmoid(F.linear(x, *self.m[2]).squeeze(-1))


def bf16_round(x):
    """Round-to-nearest-even fp32 -> bf16 -> fp32 (finite inputs)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return (b.astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def fuse(methods, weights, strategy="weighted_avg", norm="local", topk=30, user_history=None, remove_seen=True):
    """RecallFusion.fuse (recall/fusion.py:267-342): ``methods`` = ordered
    {name: {user: [(item, score), ...]}}, ``weights`` = {name: w}.  Plain
    Python floats in the reference's operation order."""
    # normalisation (:289-304)
    normed = {}
    if norm == "global":  # _global_normalize :100-134
        allv = [s for d in methods.values() for lst in d.values() for _, s in lst]
        gmin, gmax = (min(allv), max(allv)) if allv else (0.0, 0.0)
        for m, d in methods.items():
            normed[m] = {u: [(i, (s - gmin) / (gmax - gmin) if gmax > gmin else 1.0) for i, s in lst]
                         for u, lst in d.items()}
    elif norm == "z-score":  # _zscore_normalize :136-187 (numpy mean / std, sigmoid via np.exp)
        for m, d in methods.items():
            allv = [s for lst in d.values() for _, s in lst]
            if not allv:
                normed[m] = {}
                continue
            mu, sd = np.mean(allv), np.std(allv)
            normed[m] = {u: [(i, 1.0 / (1.0 + np.exp(-((s - mu) / sd))) if sd > 0 else 0.5) for i, s in lst]
                         for u, lst in d.items()}
    else:  # _normalize_scores :71-98 per list
        for m, d in methods.items():
            out = {}
            for u, lst in d.items():
                if len(lst) <= 1:
                    out[u] = [(lst[0][0], 1.0)] if lst else []
                    continue
                mn, mx = min(s for _, s in lst), max(s for _, s in lst)
                out[u] = [(i, (s - mn) / (mx - mn) if mx > mn else 1.0) for i, s in lst]
            normed[m] = out
    users = set()
    for d in normed.values():
        users.update(d.keys())
    res = {}
    for u in users:
        src = {}
        for m, d in normed.items():  # _weighted_merge :189-265
            if u not in d:
                continue
            w = weights.get(m, 1.0)
            for r, (i, s) in enumerate(d[u]):
                src.setdefault(i, []).append((w, s, r))
        merged = {}
        for i, ss in src.items():
            if strategy == "weighted_sum":
                merged[i] = sum(w * s for w, s, _ in ss)
            elif strategy == "max_score":
                merged[i] = max(w * s for w, s, _ in ss)
            elif strategy == "harmonic_mean":
                merged[i] = len(ss) / sum(1.0 / (w * s + 1e-8) for w, s, _ in ss)
            elif strategy == "diversity_weighted":
                merged[i] = sum(w * s for w, s, _ in ss) * (1 + len(ss) * 0.1)
            elif strategy == "rrf":
                merged[i] = sum(w / (60 + r) for w, _, r in ss)
            else:
                tw = sum(w for w, _, _ in ss)
                merged[i] = sum(w * s for w, s, _ in ss) / tw if tw > 0 else 0
        if remove_seen and user_history and u in user_history:
            merged = {i: s for i, s in merged.items() if i not in user_history[u]}
        res[u] = sorted(merged.items(), key=lambda x: x[1], reverse=True)[:topk]
    return res


def ctx_features(main_users, main_items, main_scores, user_history, w2v, content, created, ctype, user_yt=None,
                 art_yt=None, last_n=3, emb_dim=64, content_dim=250, w2v_dim=None):
    """FeatureExtractor._extract_context_features
    (features/feature_extractor.py:440-723) restated in the reference's own
    numpy operations, per user group.  main_* are the main_df columns (str
    user / item ids, float64 scores); returns {feature: column}.  emb_dim is
    the YouTubeDNN width (the reference's one zero default, :523), w2v_dim
    the Word2Vec width when it differs, content_dim the content width."""
    import pandas as pd

    n = len(main_items)
    N = last_n
    sim = np.full((n, N), np.nan, dtype=np.float32)
    tdf = np.zeros((n, N), dtype=np.float32)
    wdf = np.zeros((n, N), dtype=np.float32)
    stats = np.full((n, 4), np.nan, dtype=np.float32)
    ius = np.zeros(n, dtype=np.float32)
    ric = np.zeros(n, dtype=np.int8)
    ucats = {}
    for u, h in user_history.items():  # :497-506
        ucats[u] = {ctype[i] for i in h if i in ctype}
    zid = np.zeros(emb_dim, dtype=np.float32)
    zw = zid if w2v_dim is None else np.zeros(w2v_dim, dtype=np.float32)
    zc = np.zeros(content_dim, dtype=np.float32)
    groups = pd.Series(np.arange(n)).groupby(pd.Series(main_users)).apply(lambda s: s.to_numpy())
    items = np.asarray(main_items, dtype=object)
    for u, rows in groups.items():  # :527-690
        u = str(u)
        if u not in user_history:
            continue
        hist = user_history[u][-N:]
        rec = items[rows]
        if user_yt is not None and art_yt is not None:
            ue = user_yt.get(u)
            if ue is not None:
                ie = np.array([art_yt.get(i, zid) for i in rec], dtype=np.float32)
                ius[rows] = ie @ ue
        rid = np.array([w2v.get(i, zw) for i in rec], dtype=np.float32)
        rc = np.array([content.get(i, zc) for i in rec], dtype=np.float32)
        rt = np.array([created.get(i, np.nan) for i in rec], dtype=np.float32)
        for k, h in enumerate(hist):
            hid, hc, ht = w2v.get(h), content.get(h), created.get(h, np.nan)
            s = rid @ hid if hid is not None else np.zeros(len(rows), dtype=np.float32)
            if not np.isnan(ht):
                t = np.abs(rt - ht)
                t = np.where(np.isnan(t), 0, t)
            else:
                t = np.zeros(len(rows), dtype=np.float32)
            if hc is not None:
                w = np.linalg.norm(rc - hc[np.newaxis, :], axis=1)
                w = np.where(np.any(rc != 0, axis=1), w, 0)
            else:
                w = np.zeros(len(rows), dtype=np.float32)
            sim[rows, k] = s
            tdf[rows, k] = t
            wdf[rows, k] = w
        us = sim[rows, :]
        with np.errstate(all="ignore"):
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                stats[rows, 0] = np.nanmax(us, axis=1)
                stats[rows, 1] = np.nanmean(us, axis=1)
                stats[rows, 2] = np.nanmin(us, axis=1)
                stats[rows, 3] = np.nanstd(us, axis=1)
        cats = ucats.get(u, set())
        if cats:
            ric[rows] = np.array([1 if ctype.get(i) in cats else 0 for i in rec], dtype=np.int8)
    out = {"score": np.asarray(main_scores, np.float64)}
    for k in range(N):
        out[f"sim_{k + 1}"], out[f"time_diff_{k + 1}"], out[f"word_diff_{k + 1}"] = sim[:, k], tdf[:, k], wdf[:, k]
    for k, f in enumerate(("sim_max", "sim_mean", "sim_min", "sim_std")):
        out[f] = stats[:, k]
    out["item_user_sim"], out["recall_in_user_cat"] = ius, ric
    return out
