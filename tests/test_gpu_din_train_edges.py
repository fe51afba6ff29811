"""csrc/din_train.hip at the shapes its first tests left out: dt_run<8>,
T up to DT_MAXT, no context features and DT_MAXF of them, widening and
one-unit MLPs up to DT_MAXH, the ksplit edges, the DT_PIECE piece and tile
arithmetic of the embedding gradients, and tables of 2^k rows.

The bar is test_gpu_din_train.py's, unchanged (compare(): 8 e_ref per tensor
against the fp64 restatement, losses and one-element gradients over the four
batches as one tensor; Adam alone 2 e_ref + 1 ulp).  The inputs come from
test_train_edges_host.py, which checks on the CPU that no Dice column has
batch std 0 and that no e_ref is 0.  Every figure is printed before it is
asserted.
"""
import numpy as np
import pytest
import torch

import din_train_restated as R
import test_train_edges_host as H
from nrk import ops
from test_gpu_din_train import assert_all, check, compare, dev_batch, touched_rows

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ n_item = 8 --
@pytest.mark.parametrize("B,T", H.NI8_SHAPES)
def test_eight_item_features(B, T):
    """dt_run<8>: Di = 256, so dt_att_bwd_kernel has HG = 1, HPG = 36 and
    every thread takes the tid < Di branch.  (16, 128) is the largest dynamic
    LDS launch of the file, 63,280 B; (300, 20) spans 38 dt_att_bwd blocks."""
    if (B, T) == (16, 128):
        assert 4 * (36 * 257 + 2 * 256 + 256 + 40 + T + T * 36) + 4 * T * 8 == 63280
    state, feats, batches = H.ni8_case(B, T)
    res, _, _ = compare(state, feats, batches)
    assert_all(res)


def test_eight_item_features_twice_is_bit_equal():
    """dt_run<8> at B = 100, T = 50: test_same_call_twice_is_bit_equal's check."""
    state, feats, batches = H.ni8_case(100, 50)
    p = ops.DinTrainParams(state, *feats)
    args = dev_batch(batches[0])
    a = ops.din_train_grad(p, *args)
    b = ops.din_train_grad(p, *args, out=ops.DinGrads(p, 100, 50))
    torch.cuda.synchronize()
    assert torch.equal(a.loss, b.loss) and torch.equal(a.w_grad, b.w_grad) and torch.equal(a.t_count, b.t_count)
    n = int(a.t_count)
    assert torch.equal(a.t_rows[:n], b.t_rows[:n]) and torch.equal(a.t_vals[:n], b.t_vals[:n])
    assert bool(torch.isfinite(a.w_grad).all()) and bool(torch.isfinite(a.t_vals[:n]).all())


# --------------------------------------------------------------- T edges --
@pytest.mark.parametrize("T", [64, 65, 128])
@pytest.mark.parametrize("n_item", [1, 2, 4])
def test_long_histories(n_item, T):
    """T = 64, 65 and DT_MAXT = 128 at B = 24: the per-sample loops over
    T * 36 columns and T * NI history rows beyond the tested T <= 50."""
    res, _, _ = compare(*H.t_edge_case(n_item, T))
    assert_all(res)


# ------------------------------------------------------- feature counts --
def test_no_context_features():
    """n_ctx = 0: the C entry point takes a null ctx_idx; ctx is a [B, 0] tensor."""
    state, feats, batches = H.no_ctx_case()
    assert feats[2] == [] and batches[0]["ctx"].shape == (37, 0)
    res, got, _ = compare(state, feats, batches)
    assert got[0][3].n_ctx == 0
    assert_all(res)


def test_most_features():
    """DT_MAXF: 64 user and 64 context features."""
    res, got, _ = compare(*H.max_feats_case())
    assert (got[0][3].n_user, got[0][3].n_ctx) == (64, 64)
    assert_all(res)


# ------------------------------------------------------------ MLP shapes --
@pytest.mark.parametrize("hidden", H.MLP_SHAPES)
def test_mlp_shapes(hidden):
    """H2 > H1 ((24, 200), (17, 1024)), one unit ((1, 1), (1024, 1)), DT_MAXH
    = 1024 on either side, and 64 / 65 / 63 around dt_gemm_kernel's 64-wide
    tiles.  One-element tensors (a bias or weight of a one-unit layer) are
    compared over the four batches."""
    res, got, _ = compare(*H.mlp_case(hidden))
    assert (got[0][3].h1, got[0][3].h2) == hidden
    assert_all(res)


# ----------------------------------------------------------------- ksplit --
@pytest.mark.parametrize("B", H.KSPLIT_B)
def test_ksplit_edges(B):
    """ksplit = min(16, B / 256): 1 at B = 511, 2 at 512 and 513 (k slices of
    256 and of 272 + 241), 16 at DT_MAXB = 8192."""
    res, _, _ = compare(*H.ksplit_case(B))
    assert_all(res)


# ------------------------------------------------------- pieces and tiles --
def test_piece_and_tile_arithmetic():
    """DT_PIECE = 512 in dt_emb_piece_kernel / dt_emb_long_kernel: segments of
    exactly 512 (direct: en - st <= DT_PIECE at equality), 513 starting on a
    tile boundary (part[2 tile + 1], then part[2 (tile + 1)]), 1024, 1025
    (three pieces, a one-term tail) and 511 terms, at sorted positions 0, 512,
    1025, 2049 and 3074.  Their five rows are also compared one by one."""
    state, feats, batches = H.piece_case()
    counts = np.bincount(batches[0]["user"][:, 0], minlength=12)
    assert list(counts[:5]) == H.PIECE_COUNTS
    assert list(np.concatenate([[0], np.cumsum(counts[:4])])) == H.PIECE_STARTS
    res, got, r64 = compare(state, feats, batches)
    k = "user_profile_embedding_dict.u0.weight"
    assert got[0][3].row_base.cpu().numpy()[0] == 0  # u0's rows sort first
    g32 = R.grads(state, feats, batches[0])[1][k]
    for row, n in enumerate(H.PIECE_COUNTS):
        res.append(check(f"row {row} ({n} terms)", got[0][1][k][row], g32[row], r64[0][1][k][row]))
    assert_all(res)


# ------------------------------------------------------------ table sizes --
@pytest.mark.parametrize("R_", H.TABLE_ROWS)
def test_table_rows_around_a_power_of_two(R_):
    """dt_sort_bits(R) at R = 2^10 - 1, 2^10, 2^10 + 1 with the last row of
    the last table touched: the radix sort must keep its highest key."""
    state, feats, batches = H.table_rows_case(R_)
    res, got, _ = compare(state, feats, batches)
    p, g = got[0][3], got[0][2]
    rows = g.table_grad()[0].cpu().numpy()
    assert p.n_rows == R_ and rows[-1] == R_ - 1 and np.array_equal(rows, touched_rows(p, batches[0]))
    assert_all(res)


# ------------------------------------------------------------------- Adam --
@pytest.mark.parametrize("t", [1, 1000])
def test_adam_after_eight_item_gradient(t):
    """adam_sweep_kernel<32, 1> after a dt_run<8> gradient, as test_adam_alone:
    m and v bit-equal to torch.optim.Adam on the CPU, p within 2 e_ref + 1
    ulp, rows with m = v = g = 0 bit-unchanged."""
    rng = np.random.default_rng([8, t])
    state, feats, batches = H.ni8_case(37, 7)
    p = ops.DinTrainParams(state, *feats)
    g = ops.din_train_grad(p, *dev_batch(batches[0]))
    torch.cuda.synchronize()
    rows = g.table_grad()[0].long().cpu()
    untouched = np.setdiff1d(np.arange(p.n_rows), rows.numpy())
    assert untouched.size
    dense = {k: v.cpu() for k, v in g.dense(p).items()}
    keys = list(dense)
    m0 = {k: torch.from_numpy(rng.standard_normal(tuple(dense[k].shape)).astype(np.float32) * 1e-3) for k in keys}
    v0 = {k: torch.from_numpy(rng.random(tuple(dense[k].shape)).astype(np.float32) * 1e-6) for k in keys}
    tm, tv = p.split_table(p.t_m), p.split_table(p.t_v)
    wm, wv = p.split_weights(p.w_m), p.split_weights(p.w_v)
    for k in keys:
        (tm if k in tm else wm)[k].copy_(m0[k])
        (tv if k in tv else wv)[k].copy_(v0[k])
    still = torch.from_numpy(untouched[::2])
    p.t_m[still] = 0
    p.t_v[still] = 0
    m0 = {**{k: v.cpu().clone() for k, v in p.split_table(p.t_m).items()}, **{k: m0[k] for k in wm}}
    v0 = {**{k: v.cpu().clone() for k, v in p.split_table(p.t_v).items()}, **{k: v0[k] for k in wv}}
    before = p.table.cpu().clone()
    outs = {}
    for dt in (torch.float32, torch.float64):
        params = [torch.tensor(np.asarray(state[k]), dtype=dt, requires_grad=True) for k in keys]
        opt = torch.optim.Adam(params, lr=1e-3)
        for q, k in zip(params, keys):
            q.grad = dense[k].to(dt)
            opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0[k].to(dt).clone(),
                            "exp_avg_sq": v0[k].to(dt).clone()}
        opt.step()
        outs[dt] = ({k: q.detach() for q, k in zip(params, keys)},
                    {k: opt.state[q]["exp_avg"] for q, k in zip(params, keys)},
                    {k: opt.state[q]["exp_avg_sq"] for q, k in zip(params, keys)})
    p.t = t - 1
    ops.din_adam_step(p, g, lr=1e-3)
    torch.cuda.synchronize()
    got_p = {**p.split_table(p.table), **p.split_weights(p.weights)}
    got_m = {**p.split_table(p.t_m), **p.split_weights(p.w_m)}
    got_v = {**p.split_table(p.t_v), **p.split_weights(p.w_v)}
    res = []
    for k in keys:
        assert torch.equal(got_m[k].cpu(), outs[torch.float32][1][k]), f"m {k}"
        assert torch.equal(got_v[k].cpu(), outs[torch.float32][2][k]), f"v {k}"
        ulp = float(np.spacing(np.abs(outs[torch.float64][0][k].numpy()).max().astype(np.float32)))
        res.append(check(f"t={t} p {k}", got_p[k].cpu().numpy(), outs[torch.float32][0][k].numpy(),
                         outs[torch.float64][0][k].numpy(), factor=2.0, slack=ulp))
    assert torch.equal(p.table.cpu()[still], before[still]), "rows with m = v = g = 0 are left untouched"
    assert_all(res)
