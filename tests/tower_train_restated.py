"""The YouTubeDNN training step restated in plain torch on the CPU, in fp32 or
fp64: YoutubeDNN.forward in train mode (youtubednn_recaller.py:129-176), the
logit and BCEWithLogitsLoss (:405-408), torch.optim.Adam (:381), collate_fn's
histories (:43-83) and _prepare_data's split rule (:248-297).  Dropout takes
its keep masks from outside (torch's generator cannot be reproduced by a
counter-based one), scaled by 1 / (1 - p) as nn.Dropout does.

test_tower_train_host.py pins this module to a fixture made by executing the
reference; the GPU tests then compare the kernels with it at any shape, and
take the reference arithmetic's own rounding (fp32 against fp64 here) as the
yardstick of their tolerances.
"""
from __future__ import annotations

import numpy as np
import torch


def n_layers(state):
    return len([k for k in state if k.startswith("user_tower.") and k.endswith(".weight")])


def state_keys(state):
    keys = ["user_embedding.weight", "item_embedding.weight"]
    for l in range(n_layers(state)):
        keys += [f"user_tower.{3 * l}.weight", f"user_tower.{3 * l}.bias"]
    return keys


def csr_from_clicks(user, item, ts):
    """Encoded click log -> (off int64 [U + 1], items int64), rows in time order."""
    user, item, ts = (np.asarray(a, np.int64) for a in (user, item, ts))
    order = np.lexsort((ts, user))
    n_users = int(user.max()) + 1
    off = np.concatenate([[0], np.cumsum(np.bincount(user, minlength=n_users))]).astype(np.int64)
    return off, item[order]


def histories(off, items, s_user, s_pos, T):
    """collate_fn: the first T items of pos_list[:pos], zero-padded."""
    B = len(s_user)
    hist = np.zeros((B, T), np.int64)
    hlen = np.minimum(np.asarray(s_pos, np.int64), T)
    for b in range(B):
        hist[b, :hlen[b]] = items[off[s_user[b]]:off[s_user[b]] + hlen[b]]
    return hist, hlen


def positives(off):
    """(user, pos) of every training positive, in (user, pos) order."""
    out = []
    for u in range(len(off) - 1):
        n = int(off[u + 1] - off[u])
        if n < 2:
            continue
        train_end = n - max(1, int(n * 0.2))
        out += [(u, i) for i in range(1, n) if i < train_end]
    return np.array(out, np.int64).reshape(-1, 2)


def to_tensors(state, dtype):
    return {k: torch.tensor(np.asarray(state[k]), dtype=dtype, requires_grad=True) for k in state_keys(state)}


def loss_of(params, off, items, s_user, s_pos, s_target, s_label, T, masks=None, p=0.0):
    dtype = params["user_embedding.weight"].dtype
    hist, hlen = histories(off, items, s_user, s_pos, T)
    hist_t, hlen_t = torch.from_numpy(hist), torch.from_numpy(hlen)
    user_emb = params["user_embedding.weight"][torch.as_tensor(np.asarray(s_user, np.int64))]
    hist_emb = params["item_embedding.weight"][hist_t]
    mask = (torch.arange(T).unsqueeze(0) < hlen_t.unsqueeze(1)).unsqueeze(2).to(dtype)
    avg = (hist_emb * mask).sum(dim=1) / (hlen_t.unsqueeze(1).to(dtype) + 1e-8)
    x = torch.cat([user_emb, avg], dim=1)
    for l in range(len([k for k in params if k.endswith(".bias")])):
        x = torch.relu(torch.nn.functional.linear(x, params[f"user_tower.{3 * l}.weight"],
                                                  params[f"user_tower.{3 * l}.bias"]))
        if masks is not None:
            x = x * (torch.as_tensor(np.asarray(masks[l]), dtype=dtype) * (1.0 / (1.0 - p)))
    u = torch.nn.functional.normalize(x, p=2, dim=1)
    v = torch.nn.functional.normalize(params["item_embedding.weight"][torch.as_tensor(np.asarray(s_target, np.int64))],
                                      p=2, dim=1)
    logits = (u * v).sum(dim=1)
    return torch.nn.BCEWithLogitsLoss()(logits, torch.as_tensor(np.asarray(s_label), dtype=dtype))


def grads(state, off, items, batch, T, dtype=torch.float32, masks=None, p=0.0):
    """One forward + backward: (loss, {key: dense gradient}) as numpy."""
    params = to_tensors(state, dtype)
    loss = loss_of(params, off, items, *batch, T, masks, p)
    loss.backward()
    return loss.item(), {k: v.grad.numpy() for k, v in params.items()}


def train(state, off, items, batches, T, dtype=torch.float32, lr=1e-3, masks_fn=None, p=0.0):
    """Adam over the batches: (per-step losses, final state).  ``masks_fn(step,
    batch_size)`` gives the step's dropout masks (one per layer) or is None."""
    params = to_tensors(state, dtype)
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    losses = []
    for s, batch in enumerate(batches):
        opt.zero_grad()
        loss = loss_of(params, off, items, *batch, T, masks_fn(s, len(batch[0])) if masks_fn else None, p)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses, np.float64), {k: v.detach().numpy() for k, v in params.items()}


def fixture_parts(g):
    """tests/golden/ytdnn_train_small -> (off, items, initial state, batches, T)."""
    off, items = csr_from_clicks(g["click_user"], g["click_item"], g["click_ts"])
    init = {k[len("init."):]: g[k] for k in g.files if k.startswith("init.")}
    bounds = np.concatenate([[0], np.cumsum(g["batch_sizes"])])
    batches = [(g["s_user"][a:b], g["s_pos"][a:b], g["s_target"][a:b], g["s_label"][a:b])
               for a, b in zip(bounds[:-1], bounds[1:])]
    return off, items, init, batches, int(g["seq_max_len"])


def loss_only(state, off, items, batch, T, dtype=torch.float32, masks=None, p=0.0):
    """The forward alone (no dense table gradients): the loss as a float."""
    with torch.no_grad():
        return loss_of(to_tensors(state, dtype), off, items, *batch, T, masks, p).item()


def log_with_lengths(rng, lens, n_items):
    """A click log whose row u has lens[u] clicks: (off int64 [U + 1], items int64)."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, rng.integers(0, n_items, off[-1]).astype(np.int64)


def gathered_items(off, items, s_user, s_pos, T):
    """Every history item a batch gathers, one entry per gather (repeats kept)."""
    hist, hlen = histories(off, items, s_user, s_pos, T)
    return hist[np.arange(T)[None, :] < hlen[:, None]]


_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def dropout_mask(seed, step, layer, batch, width, p):
    """The trainer's counter-based keep mask [batch, width] (tower_train.hip:
    splitmix64's finaliser over (seed, step, layer, sample), one draw per
    unit, kept iff the draw's high word is >= p * 2^32), in numpy."""
    if not p > 0:
        return np.ones((batch, width), np.float32)
    thr = np.uint64(max(1, int(min(float(np.float32(p)) * 4294967296.0, 4294967295.0))))
    with np.errstate(over="ignore"):
        k = _mix(np.array([seed % 2 ** 64], np.uint64) + _GOLD * np.uint64(step + 1))
        key = _mix(k ^ ((np.uint64(layer) << np.uint64(32)) | np.arange(batch, dtype=np.uint64)))
        draw = _mix(key[:, None] + _GOLD * (np.arange(width, dtype=np.uint64) + np.uint64(1))[None, :]) >> np.uint64(32)
    return (draw >= thr).astype(np.float32)


def err(a, ref64):
    """The measure every tolerance uses: max |a - ref| over the tensor."""
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(ref64, np.float64)))) if np.size(a) else 0.0


def random_state(rng, n_users, n_items, dim, hidden, bias_scale=0.0):
    """_init_weights' distributions (:119-127) from a numpy generator."""
    st = {"user_embedding.weight": (rng.standard_normal((n_users, dim)) * 0.01).astype(np.float32),
          "item_embedding.weight": (rng.standard_normal((n_items, dim)) * 0.01).astype(np.float32)}
    fan_in = 2 * dim
    for l, w in enumerate(hidden):
        a = np.sqrt(6.0 / (fan_in + w))
        st[f"user_tower.{3 * l}.weight"] = rng.uniform(-a, a, (w, fan_in)).astype(np.float32)
        st[f"user_tower.{3 * l}.bias"] = (rng.standard_normal(w) * bias_scale).astype(np.float32)
        fan_in = w
    return st
