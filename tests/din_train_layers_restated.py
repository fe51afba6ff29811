"""tests/din_train_restated.py for any DINModel the trainer serves: 1 to 4
MLP hidden layers and either ``din_activation`` (src/rank/DIN.py:196-212).
The embedding gathers, the attention unit (Dice, hidden width 36 under either
activation, DIN.py:188), Dice itself, the batches and the error measure are
din_train_restated's, imported unchanged; this module restates the final MLP
as a loop over its layers.  Under "prelu" every hidden layer is Linear ->
nn.PReLU() with ONE trained slope ``mlp.{2n+1}.weight`` of shape (1,)
(initialised to 0.25) that Adam updates like any other parameter; under "dice"
it is Linear -> Dice with an unused, never-trained ``alpha``.

Depth and activation are read off the state's keys.  On a two-layer Dice state
every function here runs the torch operations of din_train_restated in the
same order (test_din_train_layers_host ties the two bit for bit).
"""
from __future__ import annotations

import numpy as np
import torch

import din_train_restated as R
from din_train_restated import GROUPS, err, random_batch  # noqa: F401  (shared, re-exported)


def mlp_shape(state):
    """(hidden widths, "dice" | "prelu") read off the state's keys."""
    L = 0
    while f"mlp.{2 * (L + 1)}.weight" in state:
        L += 1
    widths = [int(np.shape(state[f"mlp.{2 * n}.weight"])[0]) for n in range(L)]
    prelu = [f"mlp.{2 * n + 1}.weight" in state for n in range(L)]
    assert all(prelu) or not any(prelu), "mixed activations"
    return widths, "prelu" if prelu[0] else "dice"


def state_keys(feats, n_layers=2, activation="dice", alphas=True):
    """DINModel.state_dict()'s key order; ``alphas=False``: the trained keys
    (the slopes are trained, the alphas are not)."""
    keys = [f"{g}.{f}.weight" for g, fs in zip(GROUPS, feats) for f in fs]
    keys += ["activation_unit.mlp.0.weight", "activation_unit.mlp.0.bias"]
    keys += ["activation_unit.mlp.1.alpha"] if alphas else []
    keys += ["activation_unit.mlp.2.weight", "activation_unit.mlp.2.bias"]
    for n in range(n_layers):
        keys += [f"mlp.{2 * n}.weight", f"mlp.{2 * n}.bias"]
        if activation == "prelu":
            keys += [f"mlp.{2 * n + 1}.weight"]
        elif alphas:
            keys += [f"mlp.{2 * n + 1}.alpha"]
    return keys + [f"mlp.{2 * n_layers}.weight", f"mlp.{2 * n_layers}.bias"]


def slope_keys(state):
    widths, act = mlp_shape(state)
    return [f"mlp.{2 * n + 1}.weight" for n in range(len(widths))] if act == "prelu" else []


def to_tensors(state, feats, dtype):
    widths, act = mlp_shape(state)
    return {k: torch.tensor(np.asarray(state[k]), dtype=dtype, requires_grad=True)
            for k in state_keys(feats, len(widths), act, alphas=False)}


def probs_of(params, feats, batch, stds=None, pre=None):
    """``stds`` receives the batch std of every Dice column (the attention's,
    then each Dice layer's); ``pre`` the pre-activation of every PReLU layer."""
    uf, itf, cf = feats
    lin = torch.nn.functional.linear
    widths, act = mlp_shape(params)
    dtype = params["mlp.0.weight"].dtype
    idx = lambda a: torch.as_tensor(np.asarray(a, np.int64))  # noqa: E731
    user, item, hist, ctx = idx(batch["user"]), idx(batch["item"]), idx(batch["hist"]), idx(batch["ctx"])
    B = user.shape[0]
    ue = torch.cat([params[f"{GROUPS[0]}.{f}.weight"][user[:, i]] for i, f in enumerate(uf)], dim=1)
    he = torch.cat([params[f"{GROUPS[1]}.{f}.weight"][hist[:, :, i]] for i, f in enumerate(itf)], dim=2)
    re = torch.cat([params[f"{GROUPS[1]}.{f}.weight"][item[:, i]] for i, f in enumerate(itf)], dim=1)
    ce = (torch.cat([params[f"{GROUPS[2]}.{f}.weight"][ctx[:, i]] for i, f in enumerate(cf)], dim=1)
          if cf else torch.zeros((B, 0), dtype=dtype))
    q = re.unsqueeze(1).expand(B, he.shape[1], re.shape[1])
    cat = torch.cat([he, q, q - he, q * he], dim=-1)
    a = R.dice(lin(cat, params["activation_unit.mlp.0.weight"], params["activation_unit.mlp.0.bias"]), stds=stds)
    w = lin(a, params["activation_unit.mlp.2.weight"], params["activation_unit.mlp.2.bias"])
    w = w * torch.as_tensor(np.asarray(batch["mask"]), dtype=dtype).unsqueeze(-1)
    wh = (w * he).sum(dim=1)
    x = torch.cat([ue, ce, re, wh], dim=1)
    for n in range(len(widths)):
        x = lin(x, params[f"mlp.{2 * n}.weight"], params[f"mlp.{2 * n}.bias"])
        if act == "prelu":
            if pre is not None:
                pre.append(x.detach().numpy().copy())
            x = torch.nn.functional.prelu(x, params[f"mlp.{2 * n + 1}.weight"])
        else:
            x = R.dice(x, stds=stds)
    L = len(widths)
    return torch.sigmoid(lin(x, params[f"mlp.{2 * L}.weight"], params[f"mlp.{2 * L}.bias"])).squeeze(-1)


def loss_of(params, feats, batch):
    p = probs_of(params, feats, batch)
    return torch.nn.BCELoss()(p, torch.as_tensor(np.asarray(batch["label"]), dtype=p.dtype))


def min_dice_std(state, feats, batch, dtype=torch.float64):
    """The smallest batch std over every Dice column of the forward."""
    stds = []
    with torch.no_grad():
        probs_of(to_tensors(state, feats, dtype), feats, batch, stds)
    return float(min(s.min() for s in stds))


def prelu_gaps(state, feats, batch):
    """Per PReLU layer: (min |z| over its pre-activation in fp64, e_z = max
    |z_fp32 - z_fp64| over the same elements).  PReLU's derivative jumps at 0:
    where min |z| is not well above e_z an element can fall on different sides
    in fp32 and fp64, and its whole gradient contribution then differs."""
    pre = {}
    for dt in (torch.float32, torch.float64):
        pre[dt] = []
        with torch.no_grad():
            probs_of(to_tensors(state, feats, dt), feats, batch, pre=pre[dt])
    assert pre[torch.float64], "no PReLU layer"
    return [(float(np.abs(z64).min()), float(np.abs(z32.astype(np.float64) - z64).max()))
            for z32, z64 in zip(pre[torch.float32], pre[torch.float64])]


def prelu_gap(state, feats, batch):
    """prelu_gaps over all PReLU layers as one set of elements: (min |z|,
    e_z).  min |z| >= c e_z here implies it for each layer."""
    gaps = prelu_gaps(state, feats, batch)
    return min(z for z, _ in gaps), max(e for _, e in gaps)


def loss_only(state, feats, batch, dtype=torch.float32):
    with torch.no_grad():
        return loss_of(to_tensors(state, feats, dtype), feats, batch).item()


def grads(state, feats, batch, dtype=torch.float32):
    """One forward + backward: (loss, {key: dense gradient}) as numpy."""
    params = to_tensors(state, feats, dtype)
    loss = loss_of(params, feats, batch)
    loss.backward()
    return loss.item(), {k: v.grad.numpy() for k, v in params.items()}


def train(state, feats, batches, dtype=torch.float32, lr=1e-3, gaps=None):
    """Adam over the batches: (per-step losses, final state; alphas as given).
    ``gaps``: a list that receives prelu_gap of every step's state and batch."""
    widths, act = mlp_shape(state)
    params = to_tensors(state, feats, dtype)
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    losses = []
    for batch in batches:
        if gaps is not None:
            now = {k: (params[k].detach().numpy() if k in params else state[k]) for k in state}
            gaps.append(prelu_gap(now, feats, batch))
        opt.zero_grad()
        loss = loss_of(params, feats, batch)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    final = {k: (params[k].detach().numpy() if k in params else np.asarray(state[k]))
             for k in state_keys(feats, len(widths), act)}
    return np.array(losses, np.float64), final


def random_state(rng, vocabs, hidden=(200, 80), activation="dice", slopes=None, dim=32, emb_scale=1.0):
    """din_train_restated.random_state for any depth and either activation:
    the same draws in the same order (a PReLU draws nothing), ``slopes`` one
    per layer (default nn.PReLU's 0.25).  Returns (state, feats)."""
    feats = tuple(list(v) for v in vocabs)
    st = {}
    for g, v in zip(GROUPS, vocabs):
        for f, n in v.items():
            st[f"{g}.{f}.weight"] = (rng.standard_normal((n, dim)) * emb_scale).astype(np.float32)

    def linear(name, out, fan_in):
        a = 1.0 / np.sqrt(fan_in)
        st[name + ".weight"] = rng.uniform(-a, a, (out, fan_in)).astype(np.float32)
        st[name + ".bias"] = rng.uniform(-a, a, out).astype(np.float32)

    item_dim = len(vocabs[1]) * dim
    linear("activation_unit.mlp.0", 36, 4 * item_dim)
    st["activation_unit.mlp.1.alpha"] = np.float32(36.0)
    linear("activation_unit.mlp.2", 1, 36)
    cur = (len(vocabs[0]) + len(vocabs[2])) * dim + 2 * item_dim
    slopes = [0.25] * len(hidden) if slopes is None else list(slopes)
    assert len(slopes) == len(hidden)
    for n, unit in enumerate(hidden):
        linear(f"mlp.{2 * n}", unit, cur)
        if activation == "prelu":
            st[f"mlp.{2 * n + 1}.weight"] = np.array([slopes[n]], np.float32)
        else:
            st[f"mlp.{2 * n + 1}.alpha"] = np.float32(unit)
        cur = unit
    linear(f"mlp.{2 * len(hidden)}", 1, cur)
    return {k: st[k] for k in state_keys(feats, len(hidden), activation)}, feats


MODELS = {"prelu_24x10": ((24, 10), "prelu"), "prelu_12": ((12,), "prelu"),
          "prelu_16x12x8x6": ((16, 12, 8, 6), "prelu"), "dice_20x12x6": ((20, 12, 6), "dice")}


def fixture_parts(g_small, g_layers, model):
    """tests/golden/din_train_small (data, tables, attention unit) and
    din_train_layers_small (the model's MLP) -> (initial state, feats,
    batches, lr)."""
    init0, feats, batches, lr = R.fixture_parts(g_small)
    hidden, act = MODELS[model]
    pre = f"{model}.init."
    init = {k: v for k, v in init0.items() if not k.startswith("mlp.")}
    init.update({k[len(pre):]: g_layers[k] for k in g_layers.files if k.startswith(pre)})
    return {k: init[k] for k in state_keys(feats, len(hidden), act)}, feats, batches, lr
