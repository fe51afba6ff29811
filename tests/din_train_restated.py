"""The DIN training step restated in plain torch on the CPU, in fp32 or fp64:
DINModel.forward in train mode (src/rank/DIN.py:214-286: the embedding
gathers, ActivationUnit :82-130 with its Dice :39-44 over the batch, the
masked weighted history, the MLP with two Dice layers, sigmoid), nn.BCELoss
and torch.optim.Adam (DIN.py:881-912).  The Dice ``alpha`` parameters take no
part in the forward, get no gradient and are never updated.

test_din_train_host.py pins this module to a fixture made by executing the
reference; the GPU tests then compare the kernels with it at any shape, and
take the reference arithmetic's own rounding (fp32 against fp64 here) as the
yardstick of their tolerances.

A batch is a dict of numpy arrays: user [B, Fu], item [B, Fi], hist
[B, T, Fi], ctx [B, Fc] (int), mask [B, T] and label [B] (float).  ``feats``
is (user feature names, item feature names, context feature names).
"""
from __future__ import annotations

import numpy as np
import torch

GROUPS = ("user_profile_embedding_dict", "item_embedding_dict", "context_embedding_dict")


def state_keys(feats, alphas=True):
    """DINModel.state_dict()'s key order (without the alphas: the trained keys)."""
    keys = [f"{g}.{f}.weight" for g, fs in zip(GROUPS, feats) for f in fs]
    keys += ["activation_unit.mlp.0.weight", "activation_unit.mlp.0.bias"]
    keys += ["activation_unit.mlp.1.alpha"] if alphas else []
    keys += ["activation_unit.mlp.2.weight", "activation_unit.mlp.2.bias", "mlp.0.weight", "mlp.0.bias"]
    keys += ["mlp.1.alpha"] if alphas else []
    keys += ["mlp.2.weight", "mlp.2.bias"]
    keys += ["mlp.3.alpha"] if alphas else []
    return keys + ["mlp.4.weight", "mlp.4.bias"]


def to_tensors(state, feats, dtype):
    return {k: torch.tensor(np.asarray(state[k]), dtype=dtype, requires_grad=True)
            for k in state_keys(feats, alphas=False)}


def dice(x, eps=1e-8, stds=None):
    mean = x.mean(dim=0, keepdim=True)
    std = x.std(dim=0, keepdim=True)
    if stds is not None:
        stds.append(std.detach().reshape(-1).numpy())
    p = torch.sigmoid((x - mean) / (std + eps))
    return p * x + (1 - p) * 0.01 * x


def probs_of(params, feats, batch, stds=None):
    """``stds``: a list that receives the batch std of every Dice column (the
    attention's, then the two MLP layers')."""
    uf, itf, cf = feats
    lin = torch.nn.functional.linear
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
    a = dice(lin(cat, params["activation_unit.mlp.0.weight"], params["activation_unit.mlp.0.bias"]), stds=stds)
    w = lin(a, params["activation_unit.mlp.2.weight"], params["activation_unit.mlp.2.bias"])
    w = w * torch.as_tensor(np.asarray(batch["mask"]), dtype=dtype).unsqueeze(-1)
    wh = (w * he).sum(dim=1)
    x = torch.cat([ue, ce, re, wh], dim=1)
    x = dice(lin(x, params["mlp.0.weight"], params["mlp.0.bias"]), stds=stds)
    x = dice(lin(x, params["mlp.2.weight"], params["mlp.2.bias"]), stds=stds)
    return torch.sigmoid(lin(x, params["mlp.4.weight"], params["mlp.4.bias"])).squeeze(-1)


def loss_of(params, feats, batch):
    p = probs_of(params, feats, batch)
    return torch.nn.BCELoss()(p, torch.as_tensor(np.asarray(batch["label"]), dtype=p.dtype))


def min_dice_std(state, feats, batch, dtype=torch.float64):
    """The smallest batch std over every Dice column of the forward: a column
    with std exactly 0 is outside the trainer's contract (din_train.hip)."""
    stds = []
    with torch.no_grad():
        probs_of(to_tensors(state, feats, dtype), feats, batch, stds)
    return float(min(s.min() for s in stds))


def loss_only(state, feats, batch, dtype=torch.float32):
    """The forward alone: the loss as a float."""
    with torch.no_grad():
        return loss_of(to_tensors(state, feats, dtype), feats, batch).item()


def grads(state, feats, batch, dtype=torch.float32):
    """One forward + backward: (loss, {key: dense gradient}) as numpy."""
    params = to_tensors(state, feats, dtype)
    loss = loss_of(params, feats, batch)
    loss.backward()
    return loss.item(), {k: v.grad.numpy() for k, v in params.items()}


def train(state, feats, batches, dtype=torch.float32, lr=1e-3):
    """Adam over the batches: (per-step losses, final state; alphas as given)."""
    params = to_tensors(state, feats, dtype)
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    losses = []
    for batch in batches:
        opt.zero_grad()
        loss = loss_of(params, feats, batch)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    final = {k: (params[k].detach().numpy() if k in params else np.asarray(state[k])) for k in state_keys(feats)}
    return np.array(losses, np.float64), final


def err(a, ref64):
    """The measure every tolerance uses: max |a - ref| over the tensor."""
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(ref64, np.float64)))) if np.size(a) else 0.0


def random_state(rng, vocabs, hidden=(200, 80), dim=32, emb_scale=1.0):
    """DINModel's default initialisation from a numpy generator: nn.Embedding
    N(0, 1), nn.Linear U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias.
    ``vocabs``: three dicts feature -> vocabulary size.  Returns (state, feats)."""
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
    st["activation_unit.mlp.1.alpha"] = np.float32(36.0)  # Dice(unit): alpha holds the width
    linear("activation_unit.mlp.2", 1, 36)
    cur = (len(vocabs[0]) + len(vocabs[2])) * dim + 2 * item_dim
    for n, unit in enumerate(hidden):
        linear(f"mlp.{2 * n}", unit, cur)
        st[f"mlp.{2 * n + 1}.alpha"] = np.float32(unit)
        cur = unit
    linear(f"mlp.{2 * len(hidden)}", 1, cur)
    return {k: st[k] for k in state_keys(feats)}, feats


def random_batch(rng, vocabs, B, T, all_pad=0.2, full=False, distinct=False):
    """Index tensors as collate_fn builds them: the history left aligned with a
    prefix mask and index 0 on padding; ``all_pad`` of the rows have no
    history at all, ``full`` gives every row T valid positions, ``distinct``
    gives sample b candidate index 1 + b in every item table (vocabulary
    permitting)."""
    uv, iv, cv = (list(v.values()) for v in vocabs)
    user = np.stack([rng.integers(0, n, B) for n in uv], 1)
    item = np.stack([rng.integers(1, n, B) for n in iv], 1)
    if distinct:
        item = np.stack([1 + np.arange(B) % (n - 1) for n in iv], 1)
    ctx = np.stack([rng.integers(0, n, B) for n in cv], 1) if cv else np.zeros((B, 0), np.int64)
    hist = np.stack([rng.integers(1, n, (B, T)) for n in iv], 2)
    lens = np.full(B, T) if full else np.where(rng.random(B) < all_pad, 0, rng.integers(1, T + 1, B))
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
    hist = hist * mask[:, :, None].astype(np.int64)
    return {"user": user.astype(np.int64), "item": item.astype(np.int64), "hist": hist.astype(np.int64),
            "ctx": ctx.astype(np.int64), "mask": mask, "label": rng.integers(0, 2, B).astype(np.float32)}


def fixture_parts(g):
    """tests/golden/din_train_small -> (initial state, feats, batches, lr)."""
    feats = tuple([str(x) for x in g[k]] for k in ("user_features", "item_features", "context_features"))
    init = {k[len("init."):]: g[k] for k in g.files if k.startswith("init.")}
    bounds = np.concatenate([[0], np.cumsum(g["batch_sizes"])])
    batches = [{k: g[k][a:b] for k in ("user", "item", "hist", "ctx", "mask", "label")}
               for a, b in zip(bounds[:-1], bounds[1:])]
    return init, feats, batches, float(g["lr"])
