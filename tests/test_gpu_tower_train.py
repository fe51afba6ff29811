"""YouTubeDNN training on the GPU (csrc/tower_train.hip) against the fixture
made by executing the reference and against the plain-torch restatement
(tests/tower_train_restated.py).

Tolerances: none is fixed in advance.  For every compared tensor the yardstick
is the reference arithmetic's own rounding, e_ref = max |fp32 torch-CPU result
- fp64 result|; the kernel's error against the same fp64 result must be
<= 8 e_ref (the batch and history sums run in another order over up to 256
terms).  For Adam alone, given identical gradients, <= 2 e_ref + 1 ulp.
Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import tower_train_restated as R
from nrk import ops
from nrk.config import RecallConfig
from nrk.recall.youtubednn_recaller import YoutubeDNNRecaller

pytestmark = pytest.mark.gpu
T = 30


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dt).contiguous()


def make_log(rng, n_users, n_items, lo=2, hi=45):
    lens = rng.integers(lo, hi + 1, n_users)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, rng.integers(0, n_items, off[-1]).astype(np.int64)


def make_batch(rng, off, n_items, B):
    u = rng.integers(0, len(off) - 1, B)
    pos = 1 + (rng.integers(0, 1 << 30, B) % (off[u + 1] - off[u]))
    return u.astype(np.int64), pos.astype(np.int64), rng.integers(0, n_items, B).astype(np.int64), \
        rng.integers(0, 2, B).astype(np.float32)


def device_state(state):
    layers = [(dev(state[f"user_tower.{3 * l}.weight"], torch.float32),
               dev(state[f"user_tower.{3 * l}.bias"], torch.float32)) for l in range(R.n_layers(state))]
    weights, widths = ops.tt_pack_layers(layers)
    return dev(state["user_embedding.weight"], torch.float32), dev(state["item_embedding.weight"], torch.float32), \
        weights, widths


def kernel_grads(state, off, items, batch, seq_len=T, **kw):
    """(loss, {key: dense gradient}, TtGrads) of one nrk_tt_train_grad call."""
    ue, ie, weights, widths = device_state(state)
    g = ops.tt_train_grad(ue, ie, weights, widths, dev(off, torch.int64), dev(items, torch.int32),
                          dev(batch[0], torch.int32), dev(batch[1], torch.int32), dev(batch[2], torch.int32),
                          dev(batch[3], torch.float32), seq_len, **kw)
    torch.cuda.synchronize()
    out = {}
    for key, (rows, vals), table in (("user_embedding.weight", g.user_grad(), ue),
                                     ("item_embedding.weight", g.item_grad(), ie)):
        r = rows.cpu().numpy()
        assert np.all(np.diff(r) > 0) and (r.size == 0 or (r[0] >= 0 and r[-1] < table.shape[0])), "ascending unique"
        dense = np.zeros(tuple(table.shape), np.float32)
        dense[r] = vals.cpu().numpy()
        out[key] = dense
    touched_u = np.unique(batch[0])
    assert np.array_equal(g.user_grad()[0].cpu().numpy(), touched_u)
    for l, (w, b) in enumerate(ops.tt_unpack_layers(g.w_grad, widths, ue.shape[1])):
        out[f"user_tower.{3 * l}.weight"], out[f"user_tower.{3 * l}.bias"] = w.cpu().numpy(), b.cpu().numpy()
    return float(g.loss), out, g


def check(what, got, r32, r64, factor=8.0, slack=0.0):
    e_ref, e_k = R.err(r32, r64), R.err(got, r64)
    print(f"{what}: e_ref {e_ref:.3e}  kernel {e_k:.3e}  ratio {e_k / e_ref if e_ref else float('nan'):.2f}")
    return (what, e_k, factor * e_ref + slack)


def assert_all(results):
    bad = [f"{w}: {e:.3e} > {b:.3e}" for w, e, b in results if not e <= b]
    assert not bad, bad


# ------------------------------------------------------------- 1. fixture --
def test_fixture_parity(golden):
    """Step-1 gradients, the 7 per-step losses and the final state of the
    reference's own run (6 batches of 64 and a short one of 37, dropout 0)."""
    g = golden("ytdnn_train_small")
    off, items, init, batches, seq_len = R.fixture_parts(g)
    _, g64 = R.grads(init, off, items, batches[0], seq_len, torch.float64)
    l64, f64 = R.train(init, off, items, batches, seq_len, torch.float64, lr=float(g["lr"]))
    loss, got, _ = kernel_grads(init, off, items, batches[0], seq_len)
    res = [check("grad " + k, got[k], g["grad." + k], g64[k]) for k in g64]
    rec = YoutubeDNNRecaller(RecallConfig(youtubednn_embedding_dim=int(g["dim"]),
                                          youtubednn_hidden_units=[int(x) for x in g["hidden"]],
                                          youtubednn_seq_max_len=seq_len), device="cuda")
    losses = rec.train_on_samples(init, off, items, g["s_user"], g["s_pos"], g["s_target"], g["s_label"],
                                  batch_size=64, epochs=1, learning_rate=float(g["lr"]), dropout=0.0)
    assert losses.shape == (7,) and abs(float(losses[0]) - loss) == 0
    res.append(check("losses", losses.numpy(), g["losses"], l64))
    final = rec.state_dict()
    assert list(final) == [k for k in R.state_keys(init)]
    res += [check("final " + k, final[k].numpy(), g["final." + k], f64[k]) for k in f64]
    assert_all(res)


# --------------------------------------------------------------- 2. sweep --
HIDDEN = {"64-D": lambda D: [64, D], "100-D": lambda D: [100, D], "D": lambda D: [D], "48-40-D": lambda D: [48, 40, D]}


@pytest.mark.parametrize("B", [1, 37, 256])
@pytest.mark.parametrize("hidden", list(HIDDEN))
@pytest.mark.parametrize("D", [16, 32, 64])
def test_shape_sweep(D, hidden, B):
    """Gradients of one batch per tensor, and the losses of four batches as
    one tensor (a single scalar's e_ref can be zero by accident)."""
    rng = np.random.default_rng([D, len(hidden), B])
    off, items = make_log(rng, 50, 80)
    state = R.random_state(rng, 50, 80, D, HIDDEN[hidden](D), bias_scale=0.05)
    batches = [make_batch(rng, off, 80, B) for _ in range(4)]
    r32 = [R.grads(state, off, items, b, T, torch.float32) for b in batches]
    r64 = [R.grads(state, off, items, b, T, torch.float64) for b in batches]
    got = [kernel_grads(state, off, items, b) for b in batches]
    res = [check(f"grad {k}", got[0][1][k], r32[0][1][k], r64[0][1][k]) for k in r64[0][1]]
    res.append(check("losses", [x[0] for x in got], [x[0] for x in r32], [x[0] for x in r64]))
    assert_all(res)


def test_batch_over_several_chunks():
    """T = 64 sorts 126 samples per workgroup: 700 samples take the chunk
    merge (mark, compact, per-row sums in chunk order)."""
    rng = np.random.default_rng(11)
    off, items = make_log(rng, 300, 200, 2, 90)
    state = R.random_state(rng, 300, 200, 32, [64, 32], bias_scale=0.05)
    batch = make_batch(rng, off, 200, 700)
    _, g32 = R.grads(state, off, items, batch, 64, torch.float32)
    _, g64 = R.grads(state, off, items, batch, 64, torch.float64)
    _, got, _ = kernel_grads(state, off, items, batch, 64)
    assert_all([check(f"grad {k}", got[k], g32[k], g64[k]) for k in g64])
    _, again, _ = kernel_grads(state, off, items, batch, 64)
    assert all(np.array_equal(got[k], again[k]) for k in got)


# --------------------------------------------------------------- 3. edges --
def edge_case():
    rng = np.random.default_rng(3)
    rows = [[5, 5, 0, 7, 5] + list(rng.integers(0, 20, 35)),  # user 0: repeats, item 0, 40 clicks
            [0, 3, 9, 9, 2, 7],                               # user 1
            [7, 0]]                                           # user 2: the shortest row with a sample
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    items = np.concatenate(rows).astype(np.int64)
    #          pos = 1   pos > T   target in its own history   item 0 as target   one target, several samples
    samples = [(0, 1, 5), (0, 38, 11), (0, 3, 5), (0, 4, 0), (1, 5, 9), (1, 2, 7), (2, 1, 7), (0, 40, 7), (0, 30, 7),
               (0, 31, 3), (1, 1, 0), (0, 2, 5)]
    u, p, t = (np.array(c, np.int64) for c in zip(*samples))
    return off, items, (u, p, t)


@pytest.mark.parametrize("labels", ["mixed", "zeros", "ones"])
def test_edge_cases(labels):
    off, items, (u, p, t) = edge_case()
    lab = {"mixed": np.arange(len(u)) % 2, "zeros": np.zeros(len(u)), "ones": np.ones(len(u))}[labels]
    batch = (u, p, t, lab.astype(np.float32))
    state = R.random_state(np.random.default_rng(4), 3, 20, 16, [64, 16], bias_scale=0.05)
    l32, g32 = R.grads(state, off, items, batch, T, torch.float32)
    l64, g64 = R.grads(state, off, items, batch, T, torch.float64)
    loss, got, g = kernel_grads(state, off, items, batch)
    assert np.array_equal(g.item_grad()[0].cpu().numpy(),
                          np.unique(np.concatenate([t] + [items[off[a]:off[a] + min(b, T)] for a, b in zip(u, p)])))
    assert_all([check(f"grad {k}", got[k], g32[k], g64[k]) for k in g64])
    print(f"loss: fp32 {l32!r} fp64 {l64!r} kernel {loss!r}")


def test_all_dead_last_layer_gives_exact_zeros():
    off, items, (u, p, t) = edge_case()
    batch = (u, p, t, (np.arange(len(u)) % 2).astype(np.float32))
    state = R.random_state(np.random.default_rng(4), 3, 20, 16, [64, 16])
    state["user_tower.3.bias"][:] = -100.0
    loss, got, g = kernel_grads(state, off, items, batch)
    assert loss == pytest.approx(np.log(2.0), rel=1e-6)  # u = 0: every logit is 0
    for k, v in got.items():
        assert np.isfinite(v).all() and not v.any(), k
    assert torch.isfinite(g.i_vals[:int(g.i_count)]).all()
    _, g32 = R.grads(state, off, items, batch, T, torch.float32)
    assert all(not v.any() for v in g32.values())  # and so says torch


# ----------------------------------------------------- 4. reproducibility --
def test_bitwise_reproducible():
    rng = np.random.default_rng(21)
    off, items = make_log(rng, 200, 150)
    state = R.random_state(rng, 200, 150, 32, [64, 32])
    batch = make_batch(rng, off, 150, 256)
    runs = [kernel_grads(state, off, items, batch, p=0.2, seed=5, step=3) for _ in range(2)]
    assert runs[0][0] == runs[1][0]
    for name in ("w_grad", "u_rows", "u_vals", "u_count", "i_rows", "i_vals", "i_count"):
        a, b = getattr(runs[0][2], name), getattr(runs[1][2], name)
        n = {"u_rows": int(runs[0][2].u_count), "u_vals": int(runs[0][2].u_count), "i_rows": int(runs[0][2].i_count),
             "i_vals": int(runs[0][2].i_count)}.get(name, a.shape[0])
        assert torch.equal(a[:n], b[:n]), name
    su, sp, st, sl = make_batch(rng, off, 150, 20 * 256)
    out = []
    for _ in range(2):
        rec = YoutubeDNNRecaller(RecallConfig(youtubednn_embedding_dim=32, youtubednn_hidden_units=[64, 32]), "cuda")
        losses = rec.train_on_samples(state, off, items, su, sp, st, sl, batch_size=256, dropout=0.2, seed=9)
        out.append((losses, rec.state_dict()))
    assert out[0][0].shape == (20,) and torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(out[0][1][k], out[1][1][k]) for k in out[0][1])
    assert not torch.equal(out[0][1]["user_tower.0.weight"], torch.as_tensor(state["user_tower.0.weight"]))


# -------------------------------------------------------------- 5. dropout --
def test_dropout_matches_restatement_fed_the_masks():
    rng = np.random.default_rng(31)
    off, items = make_log(rng, 60, 90)
    hidden = [64, 40, 32]
    state = R.random_state(rng, 60, 90, 32, hidden, bias_scale=0.05)
    batch = make_batch(rng, off, 90, 200)
    masks = [ops.tt_dropout_mask(77, 12, l, 200, w, 0.2).cpu().numpy() for l, w in enumerate(hidden)]
    assert all(set(np.unique(m)) == {0.0, 1.0} for m in masks)
    l32, g32 = R.grads(state, off, items, batch, T, torch.float32, masks, 0.2)
    l64, g64 = R.grads(state, off, items, batch, T, torch.float64, masks, 0.2)
    loss, got, _ = kernel_grads(state, off, items, batch, p=0.2, seed=77, step=12)
    res = [check(f"grad {k}", got[k], g32[k], g64[k]) for k in g64]
    print(f"loss: fp32 {l32!r} fp64 {l64!r} kernel {loss!r}")
    assert_all(res)


def test_dropout_keep_rate_and_counters():
    masks = [ops.tt_dropout_mask(123, s, 0, 256, 64, 0.2) for s in range(8)]
    rate = float(torch.stack(masks).double().mean())
    print(f"keep rate over {8 * 256 * 64} draws: {rate:.5f}")
    assert abs(rate - 0.8) <= 0.0055  # 5 sigma, sigma = sqrt(0.16 / 131072)
    assert not torch.equal(masks[0], masks[1])                                       # steps differ
    assert not torch.equal(masks[0], ops.tt_dropout_mask(123, 0, 1, 256, 64, 0.2))  # layers differ
    assert not torch.equal(masks[0], ops.tt_dropout_mask(124, 0, 0, 256, 64, 0.2))  # seeds differ
    assert torch.equal(masks[0], ops.tt_dropout_mask(123, 0, 0, 256, 64, 0.2))
    assert bool((ops.tt_dropout_mask(5, 0, 0, 37, 100, 0.0) == 1).all())


def test_p_zero_takes_no_random_path():
    rng = np.random.default_rng(41)
    off, items = make_log(rng, 60, 90)
    state = R.random_state(rng, 60, 90, 16, [64, 16])
    batch = make_batch(rng, off, 90, 100)
    a = kernel_grads(state, off, items, batch, p=0.0, seed=1, step=0)
    b = kernel_grads(state, off, items, batch, p=0.0, seed=2 ** 63 + 5, step=17)
    assert a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


# ----------------------------------------------------------------- 6. Adam --
@pytest.mark.parametrize("D", [32, 16, 64])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_alone(t, D):
    """torch.optim.Adam on the CPU from the same p, m, v, g.  Bit-equality is
    the target and holds except where torch's vectorised CPU sqrt is one ulp
    off the correctly rounded root the GPU computes; the bound is
    2 e_ref + 1 ulp against fp64 Adam.  The sweep is one kernel per D: at
    D = 16 and 64 the tables are small, so that with one full and one partial
    block of weights both table boundaries fall inside a block."""
    rng = np.random.default_rng(t)
    U, I, n_w = (300, 500, 1111) if D == 32 else (37, 53, 300)
    shapes = {"w": (n_w,), "u": (U, D), "i": (I, D)}
    p = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}
    m = {k: (rng.standard_normal(s) * 1e-2).astype(np.float32) for k, s in shapes.items()}
    v = {k: (rng.standard_normal(s) ** 2 * 1e-4).astype(np.float32) for k, s in shapes.items()}
    g = {k: (rng.standard_normal(s) * 1e-2).astype(np.float32) for k, s in shapes.items()}
    rows, never = {}, {}
    for k, n in (("u", U), ("i", I)):
        perm = rng.permutation(n)
        rows[k] = np.sort(perm[:n // 5])      # rows with a gradient
        never[k] = perm[n // 5:n // 2]        # m = v = 0 and no gradient: never touched
        m[k][never[k]] = 0
        v[k][never[k]] = 0
        m[k][rows[k][:5]] = 0                 # first gradient of a row
        v[k][rows[k][:5]] = 0
        dense = np.zeros_like(g[k])
        dense[rows[k]] = g[k][rows[k]]
        g[k] = dense                          # the other rows: m, v != 0, g = 0, still updated
    ref = {}
    for dt in (torch.float32, torch.float64):
        ps = {k: torch.tensor(p[k], dtype=dt, requires_grad=True) for k in shapes}
        opt = torch.optim.Adam(list(ps.values()), lr=1e-3)
        for k in shapes:
            ps[k].grad = torch.tensor(g[k], dtype=dt)
            opt.state[ps[k]] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.tensor(m[k], dtype=dt),
                                "exp_avg_sq": torch.tensor(v[k], dtype=dt)}
        opt.step()
        ref[dt] = {k: (ps[k].detach().numpy(), opt.state[ps[k]]["exp_avg"].numpy(),
                       opt.state[ps[k]]["exp_avg_sq"].numpy()) for k in shapes}
    d = {n: {k: dev(x[k], torch.float32) for k in shapes} for n, x in (("p", p), ("m", m), ("v", v))}
    gr = ops.TtGrads("cuda", 128, 4, D, n_w)
    gr.w_grad.copy_(dev(g["w"], torch.float32))
    for k, (r_, v_, c_) in (("u", (gr.u_rows, gr.u_vals, gr.u_count)), ("i", (gr.i_rows, gr.i_vals, gr.i_count))):
        n = len(rows[k])
        assert n <= r_.shape[0]
        r_[:n] = dev(rows[k], torch.int32)
        v_[:n] = dev(g[k][rows[k]], torch.float32)
        c_.fill_(n)
    ops.tt_adam_step(d["p"]["w"], d["m"]["w"], d["v"]["w"], d["p"]["u"], d["m"]["u"], d["v"]["u"], d["p"]["i"],
                     d["m"]["i"], d["v"]["i"], gr, t=t, lr=1e-3)
    torch.cuda.synchronize()
    bad = []
    for k in shapes:
        for j, name in enumerate(("p", "m", "v")):
            got, r32, r64 = d[name][k].cpu().numpy(), ref[torch.float32][k][j], ref[torch.float64][k][j]
            e_ref = R.err(r32, r64)
            excess = np.abs(got.astype(np.float64) - r64) - (2 * e_ref + np.spacing(np.abs(r32)))
            print(f"t={t} {name}[{k}]: e_ref {e_ref:.3e} kernel {R.err(got, r64):.3e} "
                  f"bit-equal to torch fp32 {int((got == r32).sum())} of {got.size}")
            if excess.max() > 0:
                bad.append((name, k, float(excess.max())))
        if k in rows:  # never-touched rows stay bit-identical; a row with m, v != 0 and g = 0 moves
            for name, src in (("p", p), ("m", m), ("v", v)):
                assert np.array_equal(d[name][k].cpu().numpy()[never[k]], src[k][never[k]]), (name, k)
            moving = np.setdiff1d(np.arange(shapes[k][0]), np.concatenate([rows[k], never[k]]))
            assert (d["p"][k].cpu().numpy()[moving] != p[k][moving]).any(axis=1).all()
    assert not bad, bad


# -------------------------------------------------------------- 7. samples --
def test_make_samples_positives_match_prepare_data(golden):
    g = golden("ytdnn_train_small")
    off, items = R.csr_from_clicks(g["click_user"], g["click_item"], g["click_ts"])
    su, sp, st, sl = ops.tt_make_samples(dev(off, torch.int64), dev(items, torch.int32))
    got = np.column_stack([a.cpu().numpy().astype(np.int64) for a in (su, sp, st)])
    assert np.array_equal(got, g["positives"]) and bool((sl == 1).all())


def test_make_samples_negatives():
    rng = np.random.default_rng(51)
    n_users, neg = 1250, 4  # 6 clicks: positions 1 .. 4 are training positives -> 5,000 positives, 20,000 draws
    off = (np.arange(n_users + 1) * 6).astype(np.int64)
    items = rng.integers(0, 1000, off[-1]).astype(np.int64)
    pool = np.sort(rng.choice(1000, 50, replace=False)).astype(np.int64)
    su, sp, st, sl = (a.cpu().numpy() for a in ops.tt_make_samples(dev(off, torch.int64), dev(items, torch.int32), neg,
                                                                   dev(pool, torch.int32), seed=7))
    assert len(su) == 5000 * (1 + neg)
    su, sp, st, sl = (a.reshape(5000, 1 + neg) for a in (su, sp, st, sl))
    assert np.array_equal(su[:, 0], np.repeat(np.arange(n_users), 4)) and np.array_equal(sp[:, 0], np.tile([1, 2, 3, 4], n_users))
    assert np.array_equal(st[:, 0], items[off[su[:, 0]] + sp[:, 0]])
    assert (sl[:, 0] == 1).all() and (sl[:, 1:] == 0).all()
    assert (su[:, 1:] == su[:, :1]).all() and (sp[:, 1:] == sp[:, :1]).all()
    assert np.isin(st[:, 1:], pool).all()
    counts = np.array([(st[:, 1:] == x).sum() for x in pool])
    print(f"negative counts over the 50-item pool: min {counts.min()} max {counts.max()}")
    assert counts.sum() == 20000 and (np.abs(counts - 400) <= 120).all()  # 6 sigma, sigma = 19.8
    again = ops.tt_make_samples(dev(off, torch.int64), dev(items, torch.int32), neg, dev(pool, torch.int32), seed=8)
    assert not np.array_equal(again[2].cpu().numpy().reshape(5000, 1 + neg), st)


# --------------------------------------------------------------- 8. plugin --
def test_plugin_end_to_end(capsys):
    import pandas as pd

    from nrk.data import synth

    log = synth.make_click_log(n_users=400, n_items=600, seed=13, max_len=40)
    click_df = pd.DataFrame({"user_id": log.user_id * 3 + 100, "click_article_id": log.click_article_id * 7 + 11,
                             "click_timestamp": log.click_timestamp})
    users = sorted(set(click_df["user_id"]))[:100]
    cfg = RecallConfig()
    runs = []
    for _ in range(2):
        rec = YoutubeDNNRecaller(cfg, device="cuda").train(click_df, epochs=2, batch_size=cfg.youtubednn_batch_size,
                                                           learning_rate=0.01, seed=3)
        runs.append((rec, rec.batch_recall(users, topk=10)))
    assert runs[0][1] == runs[1][1] and all(len(v) == 10 for v in runs[0][1].values())
    rec = runs[0][0]
    print(f"epoch losses {rec.epoch_losses}")
    assert len(rec.epoch_losses) == 2 and rec.epoch_losses[1] < rec.epoch_losses[0]
    assert "Epoch 2 - Avg Loss" in capsys.readouterr().out
    fresh = YoutubeDNNRecaller(cfg, device="cuda").load_model(rec.state_dict(), click_df)
    assert fresh.batch_recall(users, topk=10) == runs[0][1]
    assert rec.recall(-12345, topk=10) == []
    with pytest.raises(ValueError):
        YoutubeDNNRecaller(cfg, device="cuda").state_dict()
