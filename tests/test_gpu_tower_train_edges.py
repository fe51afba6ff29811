"""csrc/tower_train.hip at the edges of its chunks, compaction tiles, widths
and sample generator, and the shared Adam sweep (csrc/train_common.h) on
large tables.

The bar is test_gpu_tower_train.py's, unchanged: per compared tensor the
kernel's error against the fp64 restatement is <= 8 e_ref, e_ref = the fp32
restatement's error against the same fp64 result; Adam alone, given identical
gradients, <= 2 e_ref + 1 ulp.  Losses and one-element gradients are compared
as one tensor over the case's four batches.  The inputs come from
test_train_edges_host.py, which checks on the CPU that no row receives more
than 256 contributions and that no e_ref is 0.  Every figure is printed before
it is asserted.
"""
import numpy as np
import pytest
import torch

import test_train_edges_host as H
import tower_train_restated as R
from nrk import ops
from test_gpu_tower_train import assert_all, check, dev, device_state, kernel_grads

pytestmark = pytest.mark.gpu


def compare(case, what=""):
    """One nrk_tt_train_grad call per batch against H.tower_refs: the first
    batch's gradients per tensor, one-element gradients and the losses over
    all batches.  Returns (results, kernel outputs, fp32 refs, fp64 refs)."""
    r32, r64 = H.tower_refs(case)
    got = [kernel_grads(case.state, case.off, case.items, b, case.T, **case.kw) for b in case.batches]
    res = []
    for k, g64 in r64[0][1].items():
        if g64.size == 1:
            res.append(check(f"{what}grad {k} (all batches)", [x[1][k] for x in got], [x[1][k] for x in r32],
                             [x[1][k] for x in r64]))
        else:
            res.append(check(f"{what}grad {k}", got[0][1][k], r32[0][1][k], g64))
    res.append(check(f"{what}losses", [x[0] for x in got], [x[0] for x in r32], [x[0] for x in r64]))
    return res, got, r32, r64


def assert_row_lists(case, batch, g):
    """u_rows / i_rows strictly ascending, equal to np.unique of the touched rows, *_count to their number."""
    users, rows = H.tower_touched(case, batch)
    for name, want, (r, v), count in (("user", users, g.user_grad(), g.u_count),
                                      ("item", rows, g.item_grad(), g.i_count)):
        r = r.cpu().numpy()
        assert np.all(np.diff(r) > 0), name
        assert int(count) == len(want) and v.shape[0] == len(want), name
        assert np.array_equal(r, want), name


# ------------------------------------------------------ compaction tiles --
@pytest.mark.parametrize("U,I", H.COMPACTION)
def test_compaction_tiles(U, I):
    """TR_CT = 4096.  (4096, 4097): one tile against two, a table of exactly
    TR_CT rows (the last-tile test (blockIdx.x + 1) * TR_CT >= n at equality).
    (8192, 300) and (300, 12289): the smaller table's blocks return early from
    tile 1 on.  (270000, 4097) and (4097, 270000): 66 tiles, so `before` runs
    the t += WAVE prefix loop twice.  `+ before` and blk[] matter from tile 1
    on.  Twenty users and targets recur in all six chunks, so
    tt_emb_merge_kernel adds six terms.  That it adds them in chunk order is
    an order property, checked bit for bit and apart from the accuracy bar:
    a recurring user has one sample per chunk, so its row is the fp32 sum, in
    chunk order, of six terms, and the call on ``probe`` (the same samples
    handed to six clones of the user) returns each term on a row of its own."""
    case = H.compaction_case(U, I)
    res, got, _, _ = compare(case, f"U={U} I={I} ")
    assert_row_lists(case, case.batches[0], got[0][2])
    assert_all(res)
    _, again, g2 = kernel_grads(case.state, case.off, case.items, case.batches[0], case.T)
    assert all(np.array_equal(got[0][1][k], again[k]) for k in again)
    assert torch.equal(got[0][2].i_rows[:int(g2.i_count)], g2.i_rows[:int(g2.i_count)])
    _, terms, _ = kernel_grads(case.state, case.off, case.items, case.probe, case.T)
    k = "user_embedding.weight"
    for r, cs in zip(case.ru, case.clones):
        acc = np.zeros(terms[k].shape[1], np.float32)
        for c in cs:
            assert terms[k][c].any()
            acc = acc + terms[k][c]
        assert acc.dtype == np.float32 and np.array_equal(got[0][1][k][r], acc), f"user {r}: not the sum in chunk order"


def test_benchmark_shape():
    """TR_CT at tools/tower_train_bench.py's shape: 250,000 users (62 tiles),
    364,047 items (89 tiles), B = 4096 in 17 chunks.  The touched rows are
    gathered from the restatement's dense gradient."""
    case = H.bench_shape_case()
    r32, r64 = H.tower_refs(case)
    got = [kernel_grads(case.state, case.off, case.items, b, case.T) for b in case.batches]
    assert_row_lists(case, case.batches[0], got[0][2])
    users, rows = H.tower_touched(case, case.batches[0])
    res = []
    for k, g64 in r64[0][1].items():
        sel = users if k == "user_embedding.weight" else rows if k == "item_embedding.weight" else slice(None)
        res.append(check(f"grad {k}{' (touched rows)' if k.endswith('embedding.weight') else ''}", got[0][1][k][sel],
                         r32[0][1][k][sel], g64[sel]))
        if k.endswith("embedding.weight"):
            rest = np.ones(len(g64), bool)
            rest[sel] = False
            assert not got[0][1][k][rest].any()
    res.append(check("losses", [x[0] for x in got], [x[0] for x in r32], [x[0] for x in r64]))
    assert_all(res)


# ----------------------------------------------------------- chunk edges --
@pytest.mark.parametrize("T,B", H.CHUNK_EDGES)
def test_chunk_edges(T, B):
    """CS = min(256, 8192 / (T + 1)).  T = 30 (CS = 256): B = 257 leaves one
    sample in the last chunk, 512 fills two, 513 adds one; B = 8192 is TR_MAXB
    in 32 chunks.  T = 32 is the first T where the key budget sets CS (248):
    B = 249 and 497.  T = 1: two keys a sample.  T = 63 (CS = 128) and T = 64
    (CS = 126) with a one-sample last chunk; rows sampled at s_pos up to 90
    fill all 64 lanes."""
    case = H.chunk_case(T, B)
    res, got, _, _ = compare(case, f"T={T} B={B} ")
    assert_row_lists(case, case.batches[0], got[0][2])
    assert_all(res)


# ------------------------------------------------------ widths and depth --
@pytest.mark.parametrize("name", list(H.WIDTHS))
def test_widths_and_depth(name):
    """TT_MAXW = 256, TT_MAXL = 8 and `staged`.  [256, 32] and [128, 256, 32]:
    four rounds of the o += WAVE loops and the backward's q < in loop at
    in = 256; [65, 32]: a round of one lane; [1, 32]: one unit (its bias
    gradient is one element); eight layers; [256, 16]: unstaged at D = 16;
    D = 64 with [60, 64] (staged, 59,296 B of LDS) beside [64, 64] (unstaged:
    staging would take 62,464 B); "dropout": [256, 128, 32] at p = 0.5 with the
    restatement fed the masks."""
    case = H.width_case(name)
    if name == "dropout":
        for l, m in enumerate(case.masks[0]):
            k = ops.tt_dropout_mask(H.DROPOUT["seed"], H.DROPOUT["step"], l, m.shape[0], m.shape[1], H.DROPOUT["p"])
            assert np.array_equal(k.cpu().numpy(), m), f"layer {l}: ops.tt_dropout_mask differs from its restatement"
    res, got, _, _ = compare(case, f"{name} ")
    assert_row_lists(case, case.batches[0], got[0][2])
    assert_all(res)


# ----------------------------------------------- one full step, big tables --
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("U,I", [(270000, 4097), (4097, 270000)])
def test_adam_step_on_large_tables(U, I, t):
    """adam_sweep_kernel after a real gradient: 4,219 blocks of the 270,000-row
    table and 65 of the other, so the blocks0 hand-over falls inside the grid
    with a partial block on its first side ((270000, 4097)) or its second;
    (4097, 270000) puts ~20,000 rows in the binary-searched item list.
    Compared as test_adam_alone: torch.optim.Adam on the CPU from the same p,
    m, v and the kernel's own gradient, 2 e_ref + 1 ulp against fp64.  Rows
    with m = v = g = 0 stay bit-identical, rows with m, v != 0 and no gradient
    move."""
    case = H.compaction_case(U, I)
    batch = case.batches[0]
    _, dense, g = kernel_grads(case.state, case.off, case.items, batch, case.T)
    users, rows = H.tower_touched(case, batch)
    print(f"row lists: {len(users)} users, {len(rows)} items")
    assert len(rows) >= 10000 or I < U
    rng = np.random.default_rng([U, I, t])
    ue, ie, weights, widths = device_state(case.state)
    D = ue.shape[1]
    w_grad = g.w_grad.cpu().numpy()
    p = {"w": weights.cpu().numpy(), "u": case.state["user_embedding.weight"], "i": case.state["item_embedding.weight"]}
    grad = {"w": w_grad, "u": dense["user_embedding.weight"], "i": dense["item_embedding.weight"]}
    m = {k: (rng.standard_normal(x.shape) * 1e-2).astype(np.float32) for k, x in p.items()}
    v = {k: (rng.standard_normal(x.shape) ** 2 * 1e-4).astype(np.float32) for k, x in p.items()}
    never, moving = {}, {}
    for k, touched, n in (("u", users, U), ("i", rows, I)):
        rest = np.setdiff1d(np.arange(n), touched)
        never[k], moving[k] = rest[::2], rest[1::2]
        m[k][never[k]] = 0
        v[k][never[k]] = 0
        m[k][touched[:5]] = 0  # first gradient of a row
        v[k][touched[:5]] = 0
    ref = {}
    for dt in (torch.float32, torch.float64):
        ps = {k: torch.tensor(p[k], dtype=dt, requires_grad=True) for k in p}
        opt = torch.optim.Adam(list(ps.values()), lr=1e-3)
        for k in p:
            ps[k].grad = torch.tensor(grad[k], dtype=dt)
            opt.state[ps[k]] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.tensor(m[k], dtype=dt),
                                "exp_avg_sq": torch.tensor(v[k], dtype=dt)}
        opt.step()
        ref[dt] = {k: (ps[k].detach().numpy(), opt.state[ps[k]]["exp_avg"].numpy(),
                       opt.state[ps[k]]["exp_avg_sq"].numpy()) for k in p}
    d = {n: {k: dev(x[k], torch.float32) for k in p} for n, x in (("p", p), ("m", m), ("v", v))}
    ops.tt_adam_step(d["p"]["w"], d["m"]["w"], d["v"]["w"], d["p"]["u"], d["m"]["u"], d["v"]["u"], d["p"]["i"],
                     d["m"]["i"], d["v"]["i"], g, t=t, lr=1e-3)
    torch.cuda.synchronize()
    bad = []
    for k in p:
        for j, name in enumerate(("p", "m", "v")):
            got, r32, r64 = d[name][k].cpu().numpy(), ref[torch.float32][k][j], ref[torch.float64][k][j]
            e_ref = R.err(r32, r64)
            excess = np.abs(got.astype(np.float64) - r64) - (2 * e_ref + np.spacing(np.abs(r32)))
            print(f"t={t} {name}[{k}]: e_ref {e_ref:.3e} kernel {R.err(got, r64):.3e} "
                  f"bit-equal to torch fp32 {int((got == r32).sum())} of {got.size}")
            if excess.max() > 0:
                bad.append((name, k, float(excess.max())))
        if k in never:
            for name, src in (("p", p), ("m", m), ("v", v)):
                assert np.array_equal(d[name][k].cpu().numpy()[never[k]], src[k][never[k]]), (name, k)
            assert (d["p"][k].cpu().numpy()[moving[k]] != p[k][moving[k]]).any(axis=1).all(), k
    assert not bad, bad


# ------------------------------------------------------- sample generator --
def make_samples(off, items, *a, **kw):
    return [x.cpu().numpy() for x in ops.tt_make_samples(dev(off, torch.int64), dev(items, torch.int32), *a, **kw)]


@pytest.mark.parametrize("U", H.SAMPLE_USERS)
def test_make_samples_row_lengths(U):
    """tt_sample_count_kernel's per = ceil(U / 1024) split at U = 1, 2, 1023,
    1024, 1025 and 2049 (per = 1, 1, 1, 1, 2, 3; threads past the last user
    are idle), over shuffled rows of 0 .. 60 clicks: rows of 0, 1 and 2 clicks
    give no positive, 3 gives one (tr_n_pos)."""
    off, items = H.sample_log(U)
    su, sp, st, sl = make_samples(off, items)
    want = R.positives(off)
    assert np.array_equal(np.column_stack([su, sp]), want) and np.array_equal(st, items[off[want[:, 0]] + want[:, 1]])
    assert su.dtype == np.int32 and (sl == 1).all()


@pytest.mark.parametrize("U", [1, 1025])
def test_make_samples_no_positives(U):
    """n_pos == 0: every row has at most 2 clicks; four empty tensors, with and without negatives."""
    off, items = H.sample_log(U, short=True)
    pool = np.arange(5, dtype=np.int64)
    for out in (make_samples(off, items), make_samples(off, items, 3, dev(pool, torch.int32), seed=1)):
        assert [x.shape for x in out] == [(0,)] * 4
    off0 = np.zeros(U + 1, np.int64)  # no clicks at all
    assert [x.shape for x in make_samples(off0, np.zeros(0, np.int64))] == [(0,)] * 4


def test_make_samples_negatives_on_mixed_rows():
    """negsample = 3 over rows of every length: what test_make_samples_negatives checks."""
    off, items = H.sample_log(1025)
    pool = np.sort(np.random.default_rng(5).choice(1000, 40, replace=False)).astype(np.int64)
    want = R.positives(off)
    su, sp, st, sl = (a.reshape(len(want), 4) for a in make_samples(off, items, 3, dev(pool, torch.int32), seed=7))
    assert np.array_equal(np.column_stack([su[:, 0], sp[:, 0]]), want)
    assert np.array_equal(st[:, 0], items[off[want[:, 0]] + want[:, 1]])
    assert (sl[:, 0] == 1).all() and (sl[:, 1:] == 0).all()
    assert (su[:, 1:] == su[:, :1]).all() and (sp[:, 1:] == sp[:, :1]).all()
    assert np.isin(st[:, 1:], pool).all()
