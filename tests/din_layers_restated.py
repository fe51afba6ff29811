"""DINModel.forward (src/rank/DIN.py:29-44 Dice, :105-124 ActivationUnit,
:196-212 the final MLP, :214-286 forward) restated in numpy for any number of
MLP hidden layers and either ``din_activation``: the yardstick of
tests/test_din_layers_host.py and tests/test_gpu_din_layers.py.
oracle.din_forward / oracle.din_forward_f64 are the two-layer Dice model and
stay as they are; on such a model ``forward_f64`` below is the same sequence
of float64 operations (test_din_layers_host ties the two bit for bit).

The attention unit is Dice with hidden width 36 whatever the activation
(DINModel builds ActivationUnit with its defaults, DIN.py:188).  Under
"prelu" every Dice of the final MLP is an nn.PReLU() with ONE slope, stored as
``mlp.{2n+1}.weight`` of shape (1,); Dice layers carry an unused
``mlp.{2n+1}.alpha`` or nothing.
"""
import numpy as np

from oracle.oracle import bf16_round
from test_gpu_din import synth_model


def mlp_shape(sd):
    """(hidden widths, "dice" | "prelu") read off the state_dict's keys."""
    L = 0
    while f"mlp.{2 * (L + 1)}.weight" in sd:
        L += 1
    widths = [int(np.shape(sd[f"mlp.{2 * n}.weight"])[0]) for n in range(L)]
    prelu = [f"mlp.{2 * n + 1}.weight" in sd for n in range(L)]
    assert all(prelu) or not any(prelu), "mixed activations"
    return widths, "prelu" if L and prelu[0] else "dice"


def _tables(sd, feats, round_bf16, dtype):
    def tab(group, f):
        w = np.asarray(sd[f"{group}.{f}.weight"], np.float32)
        return (bf16_round(w) if round_bf16 else w).astype(dtype)

    uf, itf, cf = feats
    return ([tab("user_profile_embedding_dict", f) for f in uf], [tab("item_embedding_dict", f) for f in itf],
            [tab("context_embedding_dict", f) for f in cf])


# ------------------------------------------------------------------ float32 --
def _dice32(x):
    f32 = np.float32
    x = x.astype(f32)
    mean = x.mean(0, keepdims=True, dtype=np.float64).astype(f32)
    std = x.astype(np.float64).std(0, ddof=1, keepdims=True).astype(f32)
    xn = (x - mean) / (std + f32(1e-8))
    p = (1.0 / (1.0 + np.exp(-xn.astype(np.float64)))).astype(f32)
    return (p * x + (f32(1) - p) * f32(0.01) * x).astype(f32)


def forward_f32(sd, user, item, hist, ctx, mask, feats, round_bf16=False):
    """One Dice batch in float32, operation for operation what the reference's
    torch modules compute.  Returns (probs [B], logits [B])."""
    f32 = np.float32
    widths, act = mlp_shape(sd)
    tu, ti, tc = _tables(sd, feats, round_bf16, f32)
    cat = lambda ts, idx: np.concatenate([t[idx[..., n]] for n, t in enumerate(ts)], -1)  # noqa: E731
    g = lambda k: np.asarray(sd[k], f32)  # noqa: E731
    U, Q, K = cat(tu, user), cat(ti, item), cat(ti, hist)
    C = cat(tc, ctx) if tc else np.zeros((len(user), 0), f32)
    q = np.broadcast_to(Q[:, None, :], K.shape)
    X = np.concatenate([K, q, q - K, q * K], 2).astype(f32)
    h = _dice32((X @ g("activation_unit.mlp.0.weight").T + g("activation_unit.mlp.0.bias")).astype(f32))
    w = (h @ g("activation_unit.mlp.2.weight").T + g("activation_unit.mlp.2.bias")).astype(f32)[:, :, 0]
    w = (w * mask.astype(f32)).astype(f32)
    x = np.concatenate([U, C, Q, (w[:, :, None] * K).sum(1, dtype=f32)], 1).astype(f32)
    for n in range(len(widths)):
        x = (x @ g(f"mlp.{2 * n}.weight").T + g(f"mlp.{2 * n}.bias")).astype(f32)
        if act == "dice":
            x = _dice32(x)
        else:
            a = g(f"mlp.{2 * n + 1}.weight")[0]
            x = np.where(x > 0, x, (a * x).astype(f32)).astype(f32)  # nn.PReLU: max(0, x) + a min(0, x)
    L = len(widths)
    logit = (x @ g(f"mlp.{2 * L}.weight").T + g(f"mlp.{2 * L}.bias")).astype(f32)[:, 0]
    prob = (1.0 / (1.0 + np.exp(-logit.astype(np.float64)))).astype(f32)
    return prob, logit


# ------------------------------------------------------------------ float64 --
def _batch_f64(tabs, W, L, act, slopes, user, item, hist, ctx, mask):
    f64 = np.float64
    tu, ti, tc = tabs
    B, T = mask.shape

    def dice(x):
        with np.errstate(invalid="ignore", divide="ignore"):
            mean, std = x.mean(0, keepdims=True), x.std(0, ddof=1, keepdims=True)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-((x - mean) / (std + 1e-8))))
        return p * x + (1.0 - p) * 0.01 * x

    cat = lambda ts, idx: np.concatenate([t[idx[..., n]] for n, t in enumerate(ts)], -1)  # noqa: E731
    U, Q = cat(tu, user), cat(ti, item)
    C = cat(tc, ctx) if tc else np.zeros((B, 0), f64)
    h = np.empty((B, T, W["a0b"].shape[0]), f64)
    K = np.empty((B, T, Q.shape[1]), f64)
    for lo in range(0, B, 4096):  # oracle.din_forward_f64's chunks of the [rows, T, 4d] concatenation
        sl = slice(lo, min(B, lo + 4096))
        k = cat(ti, hist[sl])
        q = np.broadcast_to(Q[sl, None, :], k.shape)
        h[sl] = np.concatenate([k, q, q - k, q * k], 2) @ W["a0w"].T + W["a0b"]
        K[sl] = k
    w = (dice(h) @ W["a2w"].T + W["a2b"])[:, :, 0] * mask.astype(f64)
    wh = (w[:, :, None] * K).sum(1)
    x = np.concatenate([U, C, Q, wh], 1)
    for n in range(L):
        x = x @ W[f"m{2 * n}w"].T + W[f"m{2 * n}b"]
        x = dice(x) if act == "dice" else np.where(x > 0, x, slopes[n] * x)
    logit = (x @ W[f"m{2 * L}w"].T + W[f"m{2 * L}b"])[:, 0]
    with np.errstate(over="ignore"):
        prob = 1.0 / (1.0 + np.exp(-logit))
    return prob, logit


def forward_f64(sd, user, item, hist, ctx, mask, feats, round_bf16=False, batch_size=None, slope_as_one=False):
    """``forward_f32`` with every operation in float64 on the fp32 (or
    bf16-rounded) parameters.  ``batch_size``: consecutive Dice batches of that
    many rows (DINRanker.predict's loop, DIN.py:1245-1283); a batch of one row
    is NaN under either activation (the attention unit's Dice has no std).
    Returns (probs [N], logits [N]) in float64.

    ``slope_as_one`` is the deliberately wrong variant of the sensitivity
    check: every PReLU slope ignored, i.e. taken as 1 (the identity)."""
    f64 = np.float64
    widths, act = mlp_shape(sd)
    L = len(widths)
    tabs = _tables(sd, feats, round_bf16, f64)
    g = lambda k: np.asarray(sd[k], np.float32).astype(f64)  # noqa: E731
    W = {"a0w": g("activation_unit.mlp.0.weight"), "a0b": g("activation_unit.mlp.0.bias"),
         "a2w": g("activation_unit.mlp.2.weight"), "a2b": g("activation_unit.mlp.2.bias")}
    for li in range(0, 2 * L + 1, 2):
        W[f"m{li}w"], W[f"m{li}b"] = g(f"mlp.{li}.weight"), g(f"mlp.{li}.bias")
    slopes = None
    if act == "prelu":
        slopes = [1.0 if slope_as_one else float(g(f"mlp.{2 * n + 1}.weight")[0]) for n in range(L)]
    N = mask.shape[0]
    S = N if batch_size is None or batch_size >= N else int(batch_size)
    prob, logit = np.empty(N, f64), np.empty(N, f64)
    for s in range(0, N, S):
        sl = slice(s, min(N, s + S))
        if sl.stop - sl.start < 2:  # torch.std of one row (DIN.py:41)
            prob[sl], logit[sl] = np.nan, np.nan
            continue
        prob[sl], logit[sl] = _batch_f64(tabs, W, L, act, slopes, user[sl], item[sl], hist[sl], ctx[sl], mask[sl])
    return prob, logit


# -------------------------------------------------------------------- models --
def synth_layers(rng, vocab_u, vocab_i, vocab_c, widths, activation="dice", slopes=None, scale=0.05):
    """test_gpu_din.synth_model's tables, attention unit and first layer, and
    its key naming and weight scale carried on to ``len(widths)`` hidden
    layers; ``activation`` "prelu" adds ``mlp.{2n+1}.weight`` of shape (1,)
    (``slopes``: one per layer, default nn.PReLU's 0.25).  Returns (state_dict,
    (user_feats, item_feats, ctx_feats))."""
    f32 = np.float32
    widths = [int(h) for h in widths]
    sd, feats = synth_model(rng, vocab_u, vocab_i, vocab_c, h1=widths[0], h2=1, scale=scale)
    for k in ("mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias"):
        del sd[k]
    lin = lambda o, i: (rng.standard_normal((o, i)) * (scale * 8 / np.sqrt(i))).astype(f32)  # noqa: E731
    L = len(widths)
    for n in range(1, L):
        sd[f"mlp.{2 * n}.weight"] = lin(widths[n], widths[n - 1])
        sd[f"mlp.{2 * n}.bias"] = (rng.standard_normal(widths[n]) * 0.1).astype(f32)
    sd[f"mlp.{2 * L}.weight"], sd[f"mlp.{2 * L}.bias"] = lin(1, widths[-1]), np.array([-0.2], f32)
    if activation == "prelu":
        slopes = [0.25] * L if slopes is None else list(slopes)
        assert len(slopes) == L
        for n in range(L):
            sd[f"mlp.{2 * n + 1}.weight"] = np.array([slopes[n]], f32)
    else:
        assert activation == "dice" and slopes is None
    return sd, feats
