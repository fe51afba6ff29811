"""DIN training on the GPU for 1 to 4 MLP hidden layers and either activation
(csrc/din_train.hip, nrk_din_train_grad_mlp) against the plain-torch
restatement (tests/din_train_layers_restated.py).

The bar is tests/test_gpu_din_train.py's: error = max |x - fp64 restatement|
per tensor, yardstick e_ref = the fp32 torch-CPU result's own error, kernel
<= 8 e_ref, never the kernel against itself (but for the two bit-equality
tests: the older entry point, and a second identical call).  Scalars are
compared as one tensor over the case's four batches: the losses, every
one-element parameter, and the L slope gradients together.  Every figure is
printed before it is asserted.

PReLU's derivative jumps at 0, so a PReLU case is compared on gradients only
where every pre-activation is clear of the kink in the fp64 restatement
(min |z| >= 16 e_z per PReLU layer and batch): a condition on the inputs,
asserted on the CPU for every case here by tests/test_din_train_layers_host.py
with seeds chosen there (tests/din_train_layers_cases.py).  The one case too
large for it compares the losses only.

Measured ratios (kernel error / e_ref, MI355X): see DESIGN.md section 4.11.1.
"""
import ctypes

import numpy as np
import pytest
import torch

import din_train_layers_cases as C
import din_train_layers_restated as RL
from nrk import _lib, ops
from test_gpu_din_train import _ranker, assert_all, dev_batch, kernel_grads, touched_rows

pytestmark = pytest.mark.gpu


def check(what, got, r32, r64, factor=8.0, slack=0.0):
    e_ref, e_k = RL.err(r32, r64), RL.err(got, r64)
    print(f"{what}: e_ref {e_ref:.3e}  kernel {e_k:.3e}  ratio {e_k / e_ref if e_ref else float('nan'):.2f}")
    assert e_ref > 0, f"{what}: e_ref 0 is no yardstick"
    return (what, e_k, factor * e_ref + slack)


def compare(state, feats, batches, what="", grads=True):
    """Gradients of the first batch per tensor; the losses, the one-element
    parameters and the slope gradients of all batches as one tensor each."""
    r32 = [RL.grads(state, feats, b, torch.float32) for b in batches]
    r64 = [RL.grads(state, feats, b, torch.float64) for b in batches]
    got = [kernel_grads(state, feats, b) for b in batches]
    res = [check(f"{what}losses", [x[0] for x in got], [x[0] for x in r32], [x[0] for x in r64])]
    if not grads:
        return res, got, r64
    slopes = RL.slope_keys(state)
    for k in r64[0][1]:
        if k in slopes:
            continue
        if r64[0][1][k].size == 1 and len(batches) > 1:
            res.append(check(f"{what}grad {k} (all batches)", [x[1][k] for x in got], [x[1][k] for x in r32],
                             [x[1][k] for x in r64]))
        else:
            res.append(check(f"{what}grad {k}", got[0][1][k], r32[0][1][k], r64[0][1][k]))
    if slopes:
        pick = lambda rs: [[x[1][k][0] for k in slopes] for x in rs]  # noqa: E731
        res.append(check(f"{what}grad slopes (all batches)", pick(got), pick(r32), pick(r64)))
    assert np.array_equal(got[0][2].table_grad()[0].cpu().numpy(), touched_rows(got[0][3], batches[0]))
    return res, got, r64


# ---------------------------------------------- 2, 3. shapes and gemm edges --
@pytest.mark.parametrize("case", C.sweep_cases() + C.edge_cases(), ids=lambda c: c["id"])
def test_shapes(case):
    state, feats, batches = C.build(case)
    res, got, _ = compare(state, feats, batches)
    assert got[0][3].widths == list(case["hidden"]) and got[0][3].activation == case["act"]
    assert_all(res)


def test_config3_like_batch_prelu_losses():
    """B = 4096, T = 50, the product's feature counts, PReLU [200, 80]: 1.1
    million PReLU elements, so no gradient is compared (the kink condition
    cannot hold); the forward is continuous at the kink and the losses meet
    the bar.  Everything is finite and the call is bit-reproducible."""
    case = C.loss_only_case()
    state, feats, batches = C.build(case)
    res, got, _ = compare(state, feats, batches, grads=False)
    _, grads, g, p = got[0]
    assert all(np.isfinite(v).all() for v in grads.values())
    again = ops.din_train_grad(p, *dev_batch(batches[0]))
    torch.cuda.synchronize()
    n = int(g.t_count)
    assert torch.equal(g.w_grad, again.w_grad) and torch.equal(g.t_count, again.t_count)
    assert torch.equal(g.t_rows[:n], again.t_rows[:n]) and torch.equal(g.t_vals[:n], again.t_vals[:n])
    assert_all(res)


# ---------------------------------------------------------------- 4. slopes --
@pytest.mark.parametrize("case", C.slope_cases(), ids=lambda c: c["id"])
def test_slopes(case):
    """Distinct slopes per layer from {0.25, 0, -0.5, 3}.  Under slope 0 the
    negative side passes no gradient down (an exact 0), yet the slope's own
    gradient is not 0."""
    state, feats, batches = C.build(case)
    res, got, r64 = compare(state, feats, batches)
    for n, a in enumerate(case["slopes"]):
        k = f"mlp.{2 * n + 1}.weight"
        print(f"slope {a} of layer {n}: d slope {got[0][1][k][0]:.6e} (fp64 {r64[0][1][k][0]:.6e})")
        assert got[0][1][k][0] != 0 and r64[0][1][k][0] != 0
    assert_all(res)


# ------------------------------------------------------ 5. old entry = new --
@pytest.mark.parametrize("hidden", [(200, 80), (40, 24)])
def test_old_entry_is_unchanged(golden, hidden):
    """Two Dice layers: nrk_din_train_grad gives, bit for bit, what it gave
    before the trainer got its layer loop (tests/golden/din_train_entry_small,
    recorded from that commit's build by make_golden_din_train_entry.py), and
    nrk_din_train_grad_mlp gives the same."""
    import din_train_restated as R

    rec = golden("din_train_entry_small")
    rng = np.random.default_rng([5, hidden[0]])
    vocabs = C.vocabs_for(4)
    state, feats = R.random_state(rng, vocabs, hidden)
    B, T = 300, 9
    args = dev_batch(R.random_batch(rng, vocabs, B, T))
    p = ops.DinTrainParams(state, *feats)
    new = ops.din_train_grad(p, *args)
    old = ops.DinGrads(p, B, T)
    L = _lib.lib()
    nb = L.nrk_din_train_workspace_bytes(p.n_rows, p.dim, 0, p.n_user, p.n_item, p.n_ctx, p.h1, p.h2, 0, B, T)
    assert nb == p.workspace_bytes(B, T) > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    user, item, hist, ctx, mask, labels = args
    _lib.call("nrk_din_train_grad", ptr(p.table), p.n_rows, p.dim, 0, ptr(p.row_base), p.n_user, p.n_item, p.n_ctx,
              ptr(p.weights), p.h1, p.h2, 0, ptr(user), ptr(item), ptr(hist), ptr(ctx), ptr(mask), ptr(labels), B, T,
              ptr(old.loss), ptr(old.w_grad), ptr(old.t_rows), ptr(old.t_vals), ptr(old.t_count), ptr(ws), nb,
              ops._stream())
    torch.cuda.synchronize()
    pre = f"h{hidden[0]}."
    n = int(rec[pre + "t_count"][0])
    for what, g in (("nrk_din_train_grad", old), ("nrk_din_train_grad_mlp", new)):
        assert int(g.t_count) == n > 0, what
        for k, got in (("loss", g.loss), ("w_grad", g.w_grad), ("t_rows", g.t_rows[:n]), ("t_vals", g.t_vals[:n])):
            assert np.array_equal(got.cpu().numpy(), rec[pre + k]), f"{what} {k}"


# ------------------------------------------------------- 6. reproducibility --
@pytest.mark.parametrize("hidden,act", [((24, 16, 12, 8), "prelu"), ((64, 65, 8), "dice")])
def test_bit_reproducible(hidden, act, tmp_path):
    """The same call twice, and 20 steps of train_on_encoded twice."""
    rng = np.random.default_rng([6, len(hidden)])
    vocabs = C.vocabs_for(4)
    state, feats = RL.random_state(rng, vocabs, hidden, act)
    batch = RL.random_batch(rng, vocabs, 200, 9)
    p = ops.DinTrainParams(state, *feats)
    args = dev_batch(batch)
    a = ops.din_train_grad(p, *args)
    b = ops.din_train_grad(p, *args, out=ops.DinGrads(p, 200, 9))
    torch.cuda.synchronize()
    n = int(a.t_count)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.w_grad, b.w_grad) and torch.equal(a.t_count, b.t_count)
    assert torch.equal(a.t_rows[:n], b.t_rows[:n]) and torch.equal(a.t_vals[:n], b.t_vals[:n])
    assert bool(torch.isfinite(a.w_grad).all()) and bool(torch.isfinite(a.t_vals[:n]).all())
    enc = {k: batch[k] for k in ("user", "item", "hist", "ctx", "mask")}
    order = np.stack([rng.permutation(200) for _ in range(4)])
    runs = []
    for _ in range(2):
        rk = _ranker(feats, tmp_path, din_activation=act, din_mlp_hidden_units=list(hidden))
        losses = rk.train_on_encoded(enc, batch["label"], batch_size=40, epochs=4, learning_rate=1e-3, order=order,
                                     init_state=state)
        runs.append((losses, rk.state_dict()))
    assert runs[0][0].shape == (20,) and torch.equal(runs[0][0], runs[1][0])
    assert list(runs[0][1]) == RL.state_keys(feats, len(hidden), act)
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    assert bool(torch.isfinite(runs[0][0]).all())


# ---------------------------------------------------------------- 1. fixture --
@pytest.mark.parametrize("model", list(RL.MODELS))
def test_fixture_parity(golden, tmp_path, model):
    """Step-1 gradients, the 7 per-step losses and the final state of the
    reference's own run, the last two through DINRanker.train_on_encoded with
    the identity order.  (The kink condition over the 7 steps is the
    fixture's, asserted again on the CPU.)"""
    gs, g = golden("din_train_small"), golden("din_train_layers_small")
    init, feats, batches, lr = RL.fixture_parts(gs, g, model)
    hidden, act = RL.MODELS[model]
    _, g64 = RL.grads(init, feats, batches[0], torch.float64)
    l64, f64 = RL.train(init, feats, batches, torch.float64, lr=lr)
    loss, got, _, _ = kernel_grads(init, feats, batches[0])
    slopes = RL.slope_keys(init)
    res = [check("grad " + k, got[k], g[f"{model}.grad.{k}"], g64[k]) for k in g64 if k not in slopes]
    if slopes:
        res.append(check("grad slopes", [got[k] for k in slopes], [g[f"{model}.grad.{k}"] for k in slopes],
                         [g64[k] for k in slopes]))
    rk = _ranker(feats, tmp_path, din_activation=act, din_mlp_hidden_units=list(hidden))
    n = len(gs["label"])
    enc = {k: gs[k] for k in ("user", "item", "hist", "ctx", "mask")}
    losses = rk.train_on_encoded(enc, gs["label"], batch_size=64, epochs=1, learning_rate=lr,
                                 order=np.arange(n)[None, :], init_state=init)
    assert losses.shape == (7,) and float(losses[0]) == loss
    res.append(check("losses", losses.numpy(), g[f"{model}.losses"], l64))
    final = rk.state_dict()
    assert list(final) == RL.state_keys(feats, len(hidden), act)
    for k in final:
        if k.endswith(".alpha"):
            assert np.array_equal(final[k].numpy(), init[k]), "alphas are never updated"
        elif k not in slopes:
            res.append(check("final " + k, final[k].numpy(), g[f"{model}.final.{k}"], f64[k]))
    if slopes:
        res.append(check("final slopes", [final[k].numpy() for k in slopes], [g[f"{model}.final.{k}"] for k in slopes],
                         [f64[k] for k in slopes]))
        assert all(float(final[k]) != 0.25 for k in slopes), "the slopes are trained"
    assert_all(res)


# ------------------------------------------------------------- 7. end to end --
def test_train_save_load_predict_prelu_three_layers(golden, tmp_path):
    """DINRanker.train() with din_activation="prelu" and three hidden layers
    on the rank_pipeline_small data: the loss falls, the saved metadata holds
    the config's activation and widths, and save_model -> load_model ->
    predict() gives the probabilities of the in-memory trained model."""
    from nrk.config import RankConfig
    from nrk.rank.base import load_pickle
    from nrk.rank.din import DINRanker
    from test_rank_pipeline import write_artifacts

    write_artifacts(golden("rank_pipeline_small"), 32, str(tmp_path))
    for name in ("din_model.pth", "din_model_metadata.pkl", "label_encoders.pkl"):
        (tmp_path / "temp" / name).unlink()
    kw = dict(_project_root=str(tmp_path), epochs=2, batch_size=32)
    cfg = RankConfig(din_activation="prelu", din_mlp_hidden_units=[24, 10, 4], **kw)
    rk = DINRanker(cfg, device="cuda")
    rk.load()
    rk.set_data(rk.main_df, rk.user_profile_dict, rk.item_features_dict, rk.user_history_dict,
                rk.user_profile_features, rk.item_features, rk.context_features, {}).train()
    losses = [v for _, v in rk.loss_history]
    print(f"{len(losses)} steps, first 10 {np.mean(losses[:10]):.4f}, last 10 {np.mean(losses[-10:]):.4f}, "
          f"val {rk.val_loss_history}, metrics {rk.final_metrics}")
    assert len(losses) >= 20 and np.mean(losses[-10:]) < np.mean(losses[:10])
    assert rk.trainer.activation == "prelu" and rk.trainer.widths == [24, 10, 4]
    meta = load_pickle(str(tmp_path / "temp" / "din_model_metadata.pkl"))
    assert meta["din_activation"] == "prelu" and meta["din_mlp_hidden_units"] == [24, 10, 4]
    trained = rk.predict()
    again = DINRanker(cfg, device="cuda")
    again.load()
    again.load_model()
    assert np.array_equal(trained, again.predict(), equal_nan=True)
    assert np.isfinite(trained).sum() >= len(trained) - 1
    for bad in (dict(din_mlp_hidden_units=[8] * 5), dict(din_activation="relu")):
        other = DINRanker(RankConfig(**kw, **bad), device="cuda")
        other.load()
        with pytest.raises(NotImplementedError):
            other.set_data(other.main_df, other.user_profile_dict, other.item_features_dict, other.user_history_dict,
                           other.user_profile_features, other.item_features, other.context_features, {}).train()
