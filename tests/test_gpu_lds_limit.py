"""A kernel's dynamic-LDS limit is raised once per device (lds_limit_once,
csrc/nrk_common.h), so it must be raised to the most any admissible call can
ask for, not to the first call's size.  A process that has already run other
tests cannot show the difference, so one fresh child process (this file run as
a script) calls each of the five entry points first at its smallest
dynamic-LDS request and then at its largest:

    itemcf_topn     topn 65, then 2048          one row of 2,100 entries
    itemcf_recall   topk 65, then 2048          four queries
    fuse_wide       65 entries, then 2,048      two users
    row_normalize   dim 1, then 256             64 rows
    tt_user_fwd     h0 1, then 128              dim 64, 8 users, seq_len 4

Every call must return without error (a launch that asks for more LDS than
the limit is an error return, not a fault), and the second result is held to
what the op's own test compares against, at that test's tolerance: the
oracle's top-n (exact), the oracle's recall (items exact, scores rtol 1e-12),
oracle.fuse (items exact, scores rtol 1e-14), numpy (bit for bit) and the
float64 tower with test_gpu_tower_shapes' bar.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
OK_LINE = "lds-limit: 5 entry points OK"


def test_first_call_does_not_pin_the_lds_limit():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0
    assert OK_LINE in r.stdout


# ------------------------------------------------------------- the child --
def _d(a):
    import numpy as np
    import torch

    return torch.from_numpy(np.array(a)).cuda()  # a contiguous copy: some case arrays are read-only


def _topn(np, ops, oracle):
    rng = np.random.default_rng(65)
    off = np.array([0, 2100], np.int64)
    vals = np.round(rng.random(2100) * 50) / 50  # many exact ties
    cols = rng.integers(0, 10**6, 2100).astype(np.int32)
    first = np.arange(2100, dtype=np.int64)
    for topn in (65, 2048):
        gc, gv, gn = ops.itemcf_topn(_d(off), _d(cols), _d(vals), _d(first), topn)
        oc, ov, on = oracle.itemcf_topn(off, cols, vals, topn)
        assert on.tolist() == [topn] and np.array_equal(gn.cpu().numpy(), on)
        assert np.array_equal(gc.cpu().numpy(), oc) and np.array_equal(gv.cpu().numpy(), ov)


def _recall(np, ops, oracle):
    rng = np.random.default_rng(2048)
    n_items, topn = 6000, 8
    nbr_cols = np.stack([rng.permutation(n_items - 1)[:topn] for _ in range(n_items)]).astype(np.int32)
    nbr_cols += nbr_cols >= np.arange(n_items)[:, None]  # never the row itself
    nbr_vals = rng.random((n_items, topn)) + 0.05
    nbr_cnt = np.full(n_items, topn, np.int32)
    created = rng.random(n_items)
    hists = [rng.permutation(n_items)[:hl].astype(np.int32) for hl in (1, 20, 400)]
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    items = np.concatenate(hists)
    distinct = len(np.setdiff1d(nbr_cols[hists[2]].ravel(), hists[2]))
    assert distinct > 2048  # the last query fills topk = 2048 with candidates
    q = np.array([0, 1, 2, -1], np.int64)
    hot = rng.permutation(n_items)[:100].astype(np.int32)
    for topk in (65, 2048):
        gi, gs, gsrc, gn = ops.itemcf_recall(_d(q), _d(offs), _d(items), _d(nbr_cols), _d(nbr_vals), _d(nbr_cnt),
                                             _d(created), _d(hot), topk)
        oi, os_, on = oracle.itemcf_recall(q, offs, items, nbr_cols, nbr_vals, nbr_cnt, created, hot, topk, n_items)
        gi, gs, gn = gi.cpu().numpy(), gs.cpu().numpy(), gn.cpu().numpy()
        assert np.array_equal(gn, on) and on[2] == topk
        for r in range(len(q)):
            assert np.array_equal(gi[r, :on[r]], oi[r, :on[r]]), (topk, r)
            np.testing.assert_allclose(gs[r, :on[r]], os_[r, :on[r]], rtol=1e-12, atol=0)


def _fuse(np, oracle):
    from nrk.recall.fusion import RecallFusion

    rng = np.random.default_rng(90112)
    for n_entries in (65, 2048):  # topk 300 > 256: nrk_fuse_wide whatever the entry count
        methods, weights = {}, {}
        for m in range(8):
            d = {}
            for u, k in ((0, n_entries // 8 + (1 if m < n_entries % 8 else 0)), (1, 4)):
                its = rng.choice(1500, size=k, replace=False).tolist()
                d[u] = [(int(i), float(np.round(rng.random() * 20) / 20)) for i in its]
            methods[f"m{m}"] = d
            weights[f"m{m}"] = float(rng.integers(1, 4)) / 2
        assert [sum(len(d[u]) for d in methods.values()) for u in (0, 1)] == [n_entries, 32]
        hist = {0: set(rng.choice(1500, size=40, replace=False).tolist())}
        f = RecallFusion(fusion_strategy="weighted_avg", normalize_method="local")
        for m, d in methods.items():
            f.add_recall_result(m, d, weight=weights[m])
        got = f.fuse(topk=300, user_history=hist, remove_seen=True)
        exp = oracle.fuse(methods, weights, strategy="weighted_avg", norm="local", topk=300, user_history=hist,
                          remove_seen=True)
        assert list(got) == list(exp)
        for u in exp:
            assert [i for i, _ in got[u]] == [i for i, _ in exp[u]], (n_entries, u)
            np.testing.assert_allclose([s for _, s in got[u]], [s for _, s in exp[u]], rtol=1e-14, atol=0)


def _normalize(np, ops):
    rng = np.random.default_rng(257)
    for d in (1, 256):
        x = (rng.standard_normal((64, d)) * rng.uniform(1e-3, 1e3, (64, 1))).astype(np.float32)
        out, nr = ops.row_normalize(_d(x), norms=True)
        assert np.array_equal(nr.cpu().numpy(), np.linalg.norm(x, axis=1))
        assert np.array_equal(out.cpu().numpy(), x / np.linalg.norm(x, axis=1, keepdims=True))


def _tower(ops):
    import torch

    import test_gpu_tower_shapes as ts

    c = ts.Case("lds-D64-T4-h128", 64, 4, (128, 64), 8)
    k = ts.make_case(c)
    (w0, b0), (w1, b1) = k["layers"]
    idx = [_d(k[n]).to(torch.int32) for n in ("uid", "hist", "hlen")]
    tabs = [_d(k["ue"]), _d(k["ie"])]
    # h0 = 1: the first hidden unit alone (its result is not judged, only that it runs)
    small = ops.tt_user_fwd(*tabs, *idx, _d(w0[:1]), _d(b0[:1]), _d(w1[:, :1]), _d(b1))
    assert small.shape == (8, 64) and bool(torch.isfinite(small).all())
    out = ops.tt_user_fwd(*tabs, *idx, _d(w0), _d(b0), _d(w1), _d(b1))
    err = ts.max_err(out.cpu().numpy(), ts.ref64(c))
    print(f"tt_user_fwd h0=128: max |gpu - f64| = {err:.3e} (bar {ts.BAR_USER:.1e})")
    assert err <= ts.BAR_USER


def _child():
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (here, os.path.join(repo, "news-recommendation-tc_amd"), repo):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch

    from nrk import ops
    from oracle import oracle

    _topn(np, ops, oracle)
    _recall(np, ops, oracle)
    _fuse(np, oracle)
    _normalize(np, ops)
    _tower(ops)
    torch.cuda.synchronize()
    print(OK_LINE)


if __name__ == "__main__":
    _child()
