"""Torch-tensor front end of the C ABI (include/nrk.h).

Every op validates shapes / dtypes / devices on the host before it launches
(the kernels trust their arguments), runs on the current HIP stream, and
allocates its outputs and workspace with the torch caching allocator.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

_P = _lib.P


def _stream():
    return _P(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return _P(t.data_ptr()) if t is not None else None


def _dev(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("nrk ops need device (cuda/HIP) tensors")
        if not t.is_contiguous():
            raise ValueError("nrk ops need contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("tensors on different devices")
    return dev


def _need(t, dtype, shape=None, name="tensor"):
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def _finite(t, name):
    """The screen kernels are built with -fno-honor-nans (Makefile): NaN / inf
    inputs would silently break their max chains, so the entry points that
    take outside vectors check them here (one reduction + sync)."""
    if t.numel() and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} must be finite (NaN / inf found)")


# ------------------------------------------------------------------ tower --
def _tt_in_range(t, hi, what):
    """One min / max reduction pair and one host read (a device sync)."""
    if t.numel():
        lo_v, hi_v = torch.stack([t.min(), t.max()]).tolist()
        if lo_v < 0 or hi_v >= hi:
            raise ValueError(f"{what} out of [0, {hi})")


def tt_validate(uid, hist, hist_len, n_user_rows, n_item_rows):
    """Raise ValueError unless hist_len is in [0, T], uid in [0, n_user_rows)
    and every live history slot (t < hist_len[u]) in [0, n_item_rows): the
    tower kernels gather without bounds checks.  Slots at or past hist_len
    may hold anything (the kernels never use them as a row).  CPU or device
    tensors; on the device this is a handful of reductions and syncs, meant to
    run once per input set, outside any timed loop."""
    n, T = hist.shape
    if n == 0:
        return
    _tt_in_range(hist_len, T + 1, "hist_len")
    _tt_in_range(uid, int(n_user_rows), "uid")
    if T:
        live = torch.arange(T, device=hist.device)[None, :] < hist_len[:, None]
        _tt_in_range(torch.where(live, hist, torch.zeros((), dtype=hist.dtype, device=hist.device)),
                     int(n_item_rows), "live hist entry")


def tt_user_fwd(user_table, item_table, uid, hist, hist_len, w0, b0, w1, b1, validate: bool = True, out=None):
    """YoutubeDNN user tower + re-normalisation (youtubednn_recaller.py:129-178, :467-470).
    ``validate`` runs tt_validate (hist_len, uid and the live hist entries in
    range: device syncs); a caller that re-runs the tower on inputs it already
    validated (the bench's timed steps) may pass False.  ``out``: a preallocated fp32 [n, w1 rows] output
    (a pipelining caller's double buffer)."""
    _dev(user_table, item_table, uid, hist, hist_len, w0, b0, w1, b1)
    n, T = hist.shape
    D = user_table.shape[1]
    h0, h1 = w0.shape[0], w1.shape[0]
    _need(user_table, torch.float32, name="user_table")
    _need(item_table, torch.float32, (item_table.shape[0], D), "item_table")
    _need(uid, torch.int32, (n,), "uid")
    _need(hist, torch.int32, name="hist")
    _need(hist_len, torch.int32, (n,), "hist_len")
    _need(w0, torch.float32, (h0, 2 * D), "w0")
    _need(b0, torch.float32, (h0,), "b0")
    _need(w1, torch.float32, (h1, h0), "w1")
    _need(b1, torch.float32, (h1,), "b1")
    if validate:
        tt_validate(uid, hist, hist_len, user_table.shape[0], item_table.shape[0])
    if out is None:
        out = torch.empty((n, h1), dtype=torch.float32, device=uid.device)
    else:
        _dev(out)
        _need(out, torch.float32, (n, h1), "out")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
    _lib.call("nrk_tt_user_fwd", _ptr(user_table), user_table.shape[0], _ptr(item_table),
              item_table.shape[0], D, _ptr(uid), _ptr(hist), _ptr(hist_len), n, T,
              _ptr(w0), _ptr(b0), h0, _ptr(w1), _ptr(b1), h1, _ptr(out), _stream())
    return out


def tt_user_pass_users(d: int, h0: int) -> int:
    """Users that one wave pass of tt_user_fwd's kernel handles together at
    (d, h0), 0 where the one-user-per-wave kernel runs:
    nrk_tt_user_pass_users (no device work)."""
    L = _lib.lib()
    g = L.nrk_tt_user_pass_users(int(d), int(h0))
    if g == 0 and L.nrk_last_error():
        raise ValueError(L.nrk_last_error().decode(errors="replace"))
    return g


def tt_user_fwd_layers(user_table, item_table, uid, hist, hist_len, layers):
    """The user tower at any depth (youtubednn_recaller.py:105-112):
    ``layers`` = [(W_l [w_l, in_l], b_l [w_l]), ...] fp32 device tensors, the
    last width equal to the embedding dim."""
    import ctypes

    _dev(user_table, item_table, uid, hist, hist_len, *[t for wb in layers for t in wb])
    n, T = hist.shape
    D = user_table.shape[1]
    _need(user_table, torch.float32, name="user_table")
    _need(item_table, torch.float32, (item_table.shape[0], D), "item_table")
    _need(uid, torch.int32, (n,), "uid")
    _need(hist, torch.int32, name="hist")
    _need(hist_len, torch.int32, (n,), "hist_len")
    widths, packed, fan_in = [], [], 2 * D
    for l, (w, b) in enumerate(layers):
        _need(w, torch.float32, (w.shape[0], fan_in), f"W{l}")
        _need(b, torch.float32, (w.shape[0],), f"b{l}")
        widths.append(int(w.shape[0]))
        packed += [w.reshape(-1), b]
        fan_in = w.shape[0]
    tt_validate(uid, hist, hist_len, user_table.shape[0], item_table.shape[0])
    wts = torch.cat(packed).contiguous()
    out = torch.empty((n, D), dtype=torch.float32, device=uid.device)
    wv = (ctypes.c_int * len(widths))(*widths)
    _lib.call("nrk_tt_user_fwd_layers", _ptr(user_table), user_table.shape[0], _ptr(item_table),
              item_table.shape[0], D, _ptr(uid), _ptr(hist), _ptr(hist_len), n, T, _ptr(wts), len(widths),
              ctypes.cast(wv, _P), _ptr(out), _stream())
    return out


def tt_item_fwd(item_table, ids, validate: bool = True):
    """get_item_embedding + re-normalisation (youtubednn_recaller.py:184-188, :485-489).
    ``validate`` checks ids against [0, item rows) (one device sync)."""
    _dev(item_table, ids)
    _need(item_table, torch.float32, name="item_table")
    _need(ids, torch.int32, name="ids")
    n, D = ids.shape[0], item_table.shape[1]
    if validate:
        _tt_in_range(ids, item_table.shape[0], "ids")
    out = torch.empty((n, D), dtype=torch.float32, device=ids.device)
    _lib.call("nrk_tt_item_fwd", _ptr(item_table), item_table.shape[0], D, _ptr(ids), n,
              _ptr(out), _stream())
    return out


# --------------------------------------------------------- tower training --
TT_MAX_BATCH = 8192
_tt_ws_cache = {}


def _tt_ws(dev, nbytes):
    """One workspace per device, grown to the largest request (a training loop
    asks for the same size every step)."""
    ws = _tt_ws_cache.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
        _tt_ws_cache[dev] = ws
    return ws


def tt_pack_layers(layers):
    """[(W_l, b_l), ...] -> (packed fp32 vector, widths): the weight layout of
    nrk_tt_user_fwd_layers and the training entry points."""
    return (torch.cat([t.reshape(-1) for wb in layers for t in wb]).contiguous(),
            [int(w.shape[0]) for w, _ in layers])


def tt_unpack_layers(weights, widths, dim):
    out, off, fan_in = [], 0, 2 * dim
    for w in widths:
        out.append((weights[off:off + w * fan_in].view(w, fan_in), weights[off + w * fan_in:off + w * fan_in + w]))
        off += w * fan_in + w
        fan_in = w
    return out


def _tt_n_weights(widths, dim):
    n, fan_in = 0, 2 * dim
    for w in widths:
        n += w * (fan_in + 1)
        fan_in = w
    return n


class TtGrads:
    """Outputs of tt_train_grad.  ``loss`` [1]; ``w_grad`` dense over the
    packed weights; each table's gradient as ``*_count`` [1] ascending unique
    ``*_rows`` with ``*_vals`` [rows, dim] (the buffers have the capacity of
    the batch; ``user_grad()`` / ``item_grad()`` slice them, one sync)."""

    def __init__(self, dev, batch, seq_len, dim, n_weights):
        f = dict(dtype=torch.float32, device=dev)
        i = dict(dtype=torch.int32, device=dev)
        self.batch, self.seq_len, self.dim = batch, seq_len, dim
        self.loss = torch.zeros(1, **f)
        self.w_grad = torch.empty(n_weights, **f)
        self.u_rows, self.u_vals, self.u_count = torch.empty(batch, **i), torch.empty((batch, dim), **f), torch.zeros(1, **i)
        cap = batch * (seq_len + 1)
        self.i_rows, self.i_vals, self.i_count = torch.empty(cap, **i), torch.empty((cap, dim), **f), torch.zeros(1, **i)

    def user_grad(self):
        n = int(self.u_count)
        return self.u_rows[:n], self.u_vals[:n]

    def item_grad(self):
        n = int(self.i_count)
        return self.i_rows[:n], self.i_vals[:n]


def tt_check_samples(n_user_rows, n_item_rows, log_off, log_items, s_user, s_pos, s_target, seq_len):
    """Range checks of a click log and samples over it (device syncs): what
    tt_train_grad's kernels trust."""
    if int(log_off[0]) != 0 or int(log_off[-1]) != log_items.shape[0] or bool((log_off[1:] < log_off[:-1]).any()):
        raise ValueError("log_off is not a CSR offset vector over log_items")
    if log_items.numel() and (int(log_items.min()) < 0 or int(log_items.max()) >= n_item_rows):
        raise ValueError("log_items out of [0, n_item_rows)")
    if not s_user.numel():
        return
    if int(s_user.min()) < 0 or int(s_user.max()) >= n_user_rows:
        raise ValueError("s_user out of [0, n_user_rows)")
    if int(s_target.min()) < 0 or int(s_target.max()) >= n_item_rows:
        raise ValueError("s_target out of [0, n_item_rows)")
    su = s_user.long()
    rowlen = log_off[su + 1] - log_off[su]
    if int(s_pos.min()) < 1 or bool((s_pos.long().clamp(max=seq_len) > rowlen).any()):
        raise ValueError("s_pos must be >= 1 and min(s_pos, seq_len) within the user's log row")


def tt_train_grad(user_table, item_table, weights, widths, log_off, log_items, s_user, s_pos, s_target, s_label,
                  seq_len, p: float = 0.0, seed: int = 0, step: int = 0, validate: bool = True, out=None, loss=None):
    """One YoutubeDNN training batch (youtubednn_recaller.py:390-411 without the
    optimiser): forward in train mode, mean BCE-with-logits loss, backward.
    ``weights`` / ``widths`` as tt_pack_layers; the click log as CSR
    (``log_off`` int64 [U + 1], ``log_items`` int32, rows in time order); a
    sample b is (s_user, s_pos, s_target, s_label)[b] and its history the first
    min(s_pos, seq_len) items of its user's row.  ``validate`` range-checks the
    indices (device syncs); a loop over samples it validated once passes False.
    ``out``: a TtGrads of the same shapes to reuse; ``loss``: a fp32 [1] device
    tensor (e.g. a slice of a per-step loss vector) to write instead of out.loss."""
    import ctypes

    dev = _dev(user_table, item_table, weights, log_off, log_items, s_user, s_pos, s_target, s_label, loss)
    U, D = user_table.shape
    I = item_table.shape[0]
    B = s_user.shape[0]
    _need(user_table, torch.float32, name="user_table")
    _need(item_table, torch.float32, (I, D), "item_table")
    _need(weights, torch.float32, (_tt_n_weights(widths, D),), "weights")
    _need(log_off, torch.int64, (U + 1,), "log_off")
    _need(log_items, torch.int32, name="log_items")
    _need(s_user, torch.int32, (B,), "s_user")
    _need(s_pos, torch.int32, (B,), "s_pos")
    _need(s_target, torch.int32, (B,), "s_target")
    _need(s_label, torch.float32, (B,), "s_label")
    if loss is not None:
        _need(loss, torch.float32, (1,), "loss")
    if validate and B:
        tt_check_samples(U, I, log_off, log_items, s_user, s_pos, s_target, seq_len)
    wv = (ctypes.c_int * len(widths))(*widths)
    wp = ctypes.cast(wv, _P)
    nbytes = _lib.lib().nrk_tt_train_workspace_bytes(U, I, D, len(widths), wp, seq_len, B)
    if not nbytes:  # shapes outside the compiled variants: the query left the reason in nrk_last_error
        raise ValueError("nrk_tt_train_workspace_bytes: " + _lib.lib().nrk_last_error().decode(errors="replace"))
    ws = _tt_ws(dev, nbytes)
    if out is None:
        out = TtGrads(dev, B, seq_len, D, weights.numel())
    elif (out.batch, out.seq_len, out.dim, out.w_grad.numel()) != (B, seq_len, D, weights.numel()):
        raise ValueError("out: a TtGrads of another shape")
    _lib.call("nrk_tt_train_grad", _ptr(user_table), U, _ptr(item_table), I, D, _ptr(weights), len(widths), wp,
              _ptr(log_off), _ptr(log_items), _ptr(s_user), _ptr(s_pos), _ptr(s_target), _ptr(s_label), B,
              seq_len, float(p), int(seed) & (2 ** 64 - 1), int(step), _ptr(out.loss if loss is None else loss),
              _ptr(out.w_grad), _ptr(out.u_rows), _ptr(out.u_vals), _ptr(out.u_count), _ptr(out.i_rows),
              _ptr(out.i_vals), _ptr(out.i_count), _ptr(ws), ws.numel(), _stream())
    return out


def tt_dropout_mask(seed: int, step: int, layer: int, batch: int, width: int, p: float, device="cuda"):
    """The 0 / 1 keep mask [batch, width] tt_train_grad applies to ``layer``'s
    outputs at (seed, step): a pure function of its counters."""
    out = torch.empty((batch, width), dtype=torch.float32, device=device)
    _lib.call("nrk_tt_dropout_mask", int(seed) & (2 ** 64 - 1), int(step), layer, batch, width, float(p), _ptr(out),
              _stream())
    return out


def tt_adam_step(weights, w_m, w_v, user_table, u_m, u_v, item_table, i_m, i_v, grads: TtGrads, t: int,
                 lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
    """One torch.optim.Adam step (dense semantics) in place over the packed
    weights and both tables from tt_train_grad's outputs; ``t`` is the 1-based
    step number, the moments are fp32 tensors of the parameters' shapes."""
    _dev(weights, w_m, w_v, user_table, u_m, u_v, item_table, i_m, i_v, grads.w_grad, grads.u_rows, grads.u_vals,
         grads.i_rows, grads.i_vals)
    D = user_table.shape[1]
    for name, ts in (("weights", (weights, w_m, w_v, grads.w_grad)), ("user_table", (user_table, u_m, u_v)),
                     ("item_table", (item_table, i_m, i_v))):
        for x in ts:
            _need(x, torch.float32, ts[0].shape, name)
    if item_table.shape[1] != D or grads.dim != D:
        raise ValueError("tables and gradients of different dims")
    _lib.call("nrk_tt_adam_step", _ptr(weights), _ptr(w_m), _ptr(w_v), _ptr(grads.w_grad), weights.numel(),
              _ptr(user_table), _ptr(u_m), _ptr(u_v), user_table.shape[0], _ptr(grads.u_rows), _ptr(grads.u_vals),
              _ptr(grads.u_count), _ptr(item_table), _ptr(i_m), _ptr(i_v), item_table.shape[0], _ptr(grads.i_rows),
              _ptr(grads.i_vals), _ptr(grads.i_count), D, float(lr), float(betas[0]), float(betas[1]), float(eps),
              int(t), _stream())


def tt_make_samples(log_off, log_items, negsample: int = 0, pool=None, seed: int = 0):
    """_prepare_data's training set (youtubednn_recaller.py:230-297) before
    the shuffle: per user with n >= 2 clicks and position i in
    [1, n - max(1, int(0.2 n))), the positive (user, i, row[i], 1) followed by
    ``negsample`` negatives (user, i, uniform draw from ``pool``, 0).
    Returns (s_user, s_pos, s_target int32, s_label fp32)."""
    dev = _dev(log_off, log_items, pool)
    U = log_off.shape[0] - 1
    _need(log_off, torch.int64, name="log_off")
    _need(log_items, torch.int32, name="log_items")
    if negsample:
        if pool is None or not pool.numel():
            raise ValueError("negatives need a non-empty pool")
        _need(pool, torch.int32, name="pool")
    pos_off = torch.empty(U + 1, dtype=torch.int64, device=dev)
    _lib.call("nrk_tt_make_samples_count", _ptr(log_off), U, _ptr(pos_off), _stream())
    n_pos = int(pos_off[-1])
    n = n_pos * (1 + negsample)
    s_user, s_pos, s_target = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    s_label = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.call("nrk_tt_make_samples", _ptr(log_off), _ptr(log_items), U, _ptr(pos_off), n_pos, negsample, _ptr(pool),
              pool.numel() if pool is not None else 0, int(seed) & (2 ** 64 - 1), _ptr(s_user), _ptr(s_pos),
              _ptr(s_target), _ptr(s_label), _stream())
    return s_user, s_pos, s_target, s_label


# ------------------------------------------------------------------ top-k --
IP_KFAST = 128  # k on the MFMA screen path (csrc/ip_topk.hip); larger k takes the exact path
IP_KMAX = 2048   # largest k compiled
CF_TOPK_MAX = 2048  # nrk_itemcf_topn / nrk_itemcf_recall (register path <= 64, LDS path above)


class Catalog:
    """The search index: fp32 rows (kept for exact rescoring) + a scaled fp16
    copy packed in MFMA fragment order.  = faiss.IndexFlatIP(d).add(items);
    rejects NaN / inf rows."""

    def __init__(self, items: torch.Tensor):
        _dev(items)
        _need(items, torch.float32, name="items")
        if items.dim() != 2 or not (1 <= items.shape[1] <= 256):
            raise ValueError("items must be [n, d] with 1 <= d <= 256")
        _finite(items, "items")
        self.items = items
        self.n, self.d = items.shape
        nbytes = _lib.lib().nrk_ip_catalog_bytes(self.n, self.d)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=items.device)
        _lib.call("nrk_ip_catalog_build", _ptr(items), self.n, self.d, _ptr(self.packed), _stream())

    @property
    def ntotal(self):
        return self.n


def ip_topk(users, catalog: Catalog, k: int, row_offset: int = 0, exact: bool = False, workspace=None,
            check_finite: bool = True):
    """Exact top-k rows per user (scores f32 [n,k], rows i32 [n,k] (+ fp64)).
    ``check_finite`` rejects NaN / inf users (one device sync); the split
    screen entry points (ip_topk_screen*, the bench / catalog-sharded path)
    leave that to the caller."""
    _dev(users, catalog.items)
    _need(users, torch.float32, name="users")
    if users.dim() != 2 or users.shape[1] != catalog.d:
        raise ValueError(f"users must be [n, {catalog.d}]")
    if check_finite:
        _finite(users, "users")
    if not (1 <= k <= IP_KMAX):
        raise ValueError(f"k must be in [1, {IP_KMAX}]")
    n = users.shape[0]
    dev = users.device
    s = torch.empty((n, k), dtype=torch.float32, device=dev)
    r = torch.empty((n, k), dtype=torch.int32, device=dev)
    e = torch.empty((n, k), dtype=torch.float64, device=dev) if exact else None
    ws_bytes = _lib.lib().nrk_ip_topk_workspace_bytes(n, catalog.n, catalog.d, k)
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call("nrk_ip_topk", _ptr(users), n, _ptr(catalog.items), _ptr(catalog.packed), catalog.n,
              catalog.d, k, int(row_offset), _ptr(s), _ptr(r), _ptr(e), _ptr(workspace),
              workspace.numel(), _stream())
    return (s, r, e) if exact else (s, r)


def ip_topk_workspace(n_users, catalog: Catalog, k, device):
    nb = _lib.lib().nrk_ip_topk_workspace_bytes(n_users, catalog.n, catalog.d, k)
    return torch.empty(nb, dtype=torch.uint8, device=device)


IP_QUERY_KMAX = 128          # nrk_ip_query's k; larger k is ip_topk's exact path
IP_QUERY_MAX_USERS = 4096    # NRK_IP_QUERY_MAX_USERS (include/nrk.h)


def _ip_query_sizes(n_users, n_items, dim, k):
    if not (1 <= k <= IP_QUERY_KMAX):
        raise ValueError(f"k must be in [1, {IP_QUERY_KMAX}] (ip_topk takes larger k)")
    if not (1 <= dim <= 256):
        raise ValueError("dim must be in [1, 256]")
    if not (0 <= n_users <= IP_QUERY_MAX_USERS):
        raise ValueError(f"n_users must be <= {IP_QUERY_MAX_USERS} (ip_topk takes larger batches)")
    if not (0 <= n_items < 2 ** 30):
        raise ValueError("n_items must be < 2^30")


def ip_query_plan(n_users: int, n_items: int, dim: int, k: int):
    """(users per workgroup tile, items per round, workgroups along the
    catalog, list capacity) of an ip_query call of these sizes; no device work."""
    import ctypes

    _ip_query_sizes(n_users, n_items, dim, k)
    out = (ctypes.c_int32 * 4)()
    _lib.call("nrk_ip_query_plan", n_users, n_items, dim, k, ctypes.cast(out, _P))
    return tuple(out)


def ip_query_workspace(n_users, catalog: Catalog, k, device):
    _ip_query_sizes(n_users, catalog.n, catalog.d, k)
    nb = _lib.lib().nrk_ip_query_workspace_bytes(n_users, catalog.n, catalog.d, k)
    return torch.empty(nb, dtype=torch.uint8, device=device)


def ip_query(users, catalog: Catalog, k: int, row_offset: int = 0, exact: bool = False, workspace=None,
             check_finite: bool = True):
    """ip_topk's result for a small user batch (at most IP_QUERY_MAX_USERS
    users, k <= 128): the catalog is split across the chip instead of the
    users, every score is the exact one (catalog.items; the packed copy is not
    read).  Same checks, return shapes and dtypes as ip_topk, bit-identical
    values."""
    _need(users, torch.float32, name="users")
    if users.dim() != 2 or users.shape[1] != catalog.d:
        raise ValueError(f"users must be [n, {catalog.d}]")
    n = users.shape[0]
    _ip_query_sizes(n, catalog.n, catalog.d, k)
    if check_finite:
        _finite(users, "users")
    _dev(users, catalog.items)
    dev = users.device
    s = torch.empty((n, k), dtype=torch.float32, device=dev)
    r = torch.empty((n, k), dtype=torch.int32, device=dev)
    e = torch.empty((n, k), dtype=torch.float64, device=dev) if exact else None
    ws_bytes = _lib.lib().nrk_ip_query_workspace_bytes(n, catalog.n, catalog.d, k)
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call("nrk_ip_query", _ptr(users), n, _ptr(catalog.items), catalog.n, catalog.d, k, int(row_offset),
              _ptr(s), _ptr(r), _ptr(e), _ptr(workspace), workspace.numel(), _stream())
    return (s, r, e) if exact else (s, r)


def topk_merge(exact_lists, row_lists, k_out):
    """Merge [G, n, k_in] per-shard lists (fp64 scores + global rows)."""
    _dev(exact_lists, row_lists)
    _need(exact_lists, torch.float64, name="exact_lists")
    _need(row_lists, torch.int32, tuple(exact_lists.shape), "row_lists")
    G, n, k_in = exact_lists.shape
    if G * k_in > 1024 or k_out > G * k_in:
        raise ValueError("need G*k_in <= 1024 and k_out <= G*k_in")
    dev = exact_lists.device
    s = torch.empty((n, k_out), dtype=torch.float32, device=dev)
    r = torch.empty((n, k_out), dtype=torch.int32, device=dev)
    e = torch.empty((n, k_out), dtype=torch.float64, device=dev)
    _lib.call("nrk_topk_merge", _ptr(exact_lists), _ptr(row_lists), G, n * k_in, n, k_in, k_out,
              _ptr(s), _ptr(r), _ptr(e), _stream())
    return s, r, e


def ip_topk_screen(users, catalog: Catalog, k: int, workspace):
    """Phase 1 of ip_topk (fp16 MFMA scan -> per-user append lists in ``workspace``).
    ``users`` must be finite (not checked here: the hot path)."""
    _dev(users, workspace)
    n = users.shape[0]
    _lib.call("nrk_ip_topk_screen", _ptr(users), n, _ptr(catalog.packed), catalog.n, catalog.d, k,
              _ptr(workspace), workspace.numel(), _stream())


def ip_topk_scan(users, catalog: Catalog, k: int, workspace):
    """ip_topk_screen's first launch alone: the fp16 MFMA scan (appends)."""
    _dev(users, workspace)
    _lib.call("nrk_ip_topk_scan", _ptr(users), users.shape[0], _ptr(catalog.packed), catalog.n, catalog.d, k,
              _ptr(workspace), workspace.numel(), _stream())


def ip_topk_select(users, catalog: Catalog, k: int, workspace):
    """ip_topk_screen's second part alone: the cleared workspace header (the
    finish then takes its band from the scan's append lists; the per-user
    select runs in ip_topk_bound)."""
    _dev(users, workspace)
    _lib.call("nrk_ip_topk_select", _ptr(users), users.shape[0], _ptr(catalog.packed), catalog.n, catalog.d, k,
              _ptr(workspace), workspace.numel(), _stream())


def ip_topk_finish(users, catalog: Catalog, k: int, workspace, out_scores, out_rows,
                   out_exact=None, row_offset: int = 0):
    """Phase 2 of ip_topk (exact rescoring + ordering) into preallocated outputs."""
    _dev(users, workspace, out_scores, out_rows, out_exact)
    n = users.shape[0]
    _lib.call("nrk_ip_topk_finish", _ptr(users), n, _ptr(catalog.items), _ptr(catalog.packed), catalog.n, catalog.d, k,
              int(row_offset), _ptr(out_scores), _ptr(out_rows), _ptr(out_exact), _ptr(workspace),
              workspace.numel(), _stream())


def ip_topk_bound(users, catalog: Catalog, k: int, m: int, workspace):
    """After ip_topk_screen (same k): per user the m largest exact lower
    bounds of this shard (fp32 [n, m], descending, -inf padded), each
    bounding a distinct item's exact score."""
    _dev(users, workspace)
    n = users.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=users.device)
    _lib.call("nrk_ip_topk_bound", _ptr(users), n, _ptr(catalog.packed), catalog.n, catalog.d, int(k), int(m),
              _ptr(out),
              _ptr(workspace), workspace.numel(), _stream())
    return out


def ip_topk_tile_blocks(d: int) -> int:
    """32-item blocks per screen tile (shard ranges start on a tile):
    nrk_ip_topk_tile_blocks, the scan's own constant (no device work)."""
    tb = _lib.lib().nrk_ip_topk_tile_blocks(int(d))
    if tb <= 0:
        raise ValueError(f"dim must be in [1, 256], got {d}")
    return tb


def ip_topk_shard_screen(users, catalog: Catalog, k: int, blk_lo: int, blk_hi: int, m: int, workspace):
    """Config-4 shard, select-free: the scan of the blocks [blk_lo, blk_hi)
    for every user + per user the m largest appended maxima as exact lower
    bounds (fp32 [n, m], descending, -inf padded)."""
    _dev(users, workspace)
    n = users.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=users.device)
    _lib.call("nrk_ip_topk_shard_screen", _ptr(users), n, _ptr(catalog.packed), catalog.n, catalog.d, int(k),
              int(blk_lo), int(blk_hi), int(m), _ptr(out), _ptr(workspace), workspace.numel(), _stream())
    return out


IP_X_CAP = 32  # band half-block ids per user and shard in the fixed-slot exchange (4 B each)


def ip_topk_shard_band(n_users, catalog: Catalog, k: int, bounds, workspace, x_cap: int = IP_X_CAP):
    """After ip_topk_shard_screen and the all_gather of every shard's bounds
    (``bounds`` [n_lists, n_users, m] f32, or None): cut = max(own list bound
    - 2 eps, k-th largest bound - eps), the half-blocks >= cut packed: (cnt
    int32 [n] (-1 = more than x_cap: exact path), ids int32 [n, x_cap]
    (global half-block ids)); the cut goes to ucut."""
    cap = int(x_cap)
    dev = workspace.device
    cnt = torch.empty(n_users, dtype=torch.int32, device=dev)
    ent = torch.empty((n_users, cap), dtype=torch.int32, device=dev)
    nl, m = (0, 1) if bounds is None else (bounds.shape[0], bounds.shape[2])
    if bounds is not None:
        _dev(bounds, workspace)
        _need(bounds, torch.float32, (nl, n_users, m), "bounds")
    _lib.call("nrk_ip_topk_shard_band", n_users, catalog.n, catalog.d, int(k), _ptr(bounds), nl, m, cap,
              _ptr(workspace), workspace.numel(), _ptr(ent), _ptr(cnt), _stream())
    return cnt, ent


def ip_topk_refine_x(users, catalog: Catalog, k: int, src_cnt, src_ent, ucut, ovf=None, row_offset: int = 0,
                     workspace=None):
    """The config-4 owner's exact refine over the fixed-slot exchange:
    ``src_ent`` int32 [n_src, src_users, x_cap] (source s's band half-block
    ids of user u), ``src_cnt`` int32 [n_src, src_users] (-1: exact path), users
    [n <= src_users, D].  Returns (scores f32 [n, k], rows i32 [n, k],
    exact f64 [n, k])."""
    _dev(users, src_cnt, src_ent, ucut, ovf)
    n = users.shape[0]
    ns, su, x = src_ent.shape
    _need(src_ent, torch.int32, name="src_ent")
    _need(src_cnt, torch.int32, (ns, su), "src_cnt")
    if su < n:
        raise ValueError("src_users must cover the users")
    dev = users.device
    s = torch.empty((n, k), dtype=torch.float32, device=dev)
    r = torch.empty((n, k), dtype=torch.int32, device=dev)
    e = torch.empty((n, k), dtype=torch.float64, device=dev)
    nb = _lib.lib().nrk_ip_topk_workspace_bytes(n, catalog.n, catalog.d, k)
    if workspace is None or workspace.numel() < nb:
        workspace = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.call("nrk_ip_topk_refine_x", _ptr(users), n, _ptr(catalog.items), _ptr(catalog.packed), catalog.n,
              catalog.d, int(k), int(row_offset), _ptr(src_ent), ns, su, x, _ptr(src_cnt), _ptr(ucut), _ptr(ovf),
              _ptr(s), _ptr(r), _ptr(e), _ptr(workspace), workspace.numel(), _stream())
    return s, r, e


def ip_topk_ucut(workspace, n_users):
    """The per-user (cut, eps) float32 [n, 2] of a top-k workspace (ip_ws_layout: after the 256-B header)."""
    return workspace[256: 256 + 8 * n_users].view(torch.float32).view(n_users, 2)


def ip_topk_apply_bound(bounds, k: int, workspace):
    """bounds [n_lists, n, m] fp32 (every shard's ip_topk_bound): raise this
    shard's refine cut to the k-th largest of each user's n_lists * m values."""
    _dev(bounds, workspace)
    _need(bounds, torch.float32, name="bounds")
    if bounds.dim() != 3:
        raise ValueError("bounds must be [n_lists, n_users, m]")
    L, n, m = bounds.shape
    _lib.call("nrk_ip_topk_apply_bound", n, _ptr(bounds), L, m, int(k), _ptr(workspace), workspace.numel(),
              _stream())


def row_normalize(x, norms=False):
    """x / ||x|| per row, bit-identical to numpy float32 (similarity/embedding.py:41)."""
    _dev(x)
    _need(x, torch.float32, name="x")
    if x.dim() != 2 or not (1 <= x.shape[1] <= 256):
        raise ValueError("x must be [n, d] with 1 <= d <= 256")
    n, d = x.shape
    out = torch.empty_like(x)
    nr = torch.empty(n, dtype=torch.float32, device=x.device) if norms else None
    _lib.call("nrk_row_normalize", _ptr(x), n, d, _ptr(out), _ptr(nr), _stream())
    return (out, nr) if norms else out


# -------------------------------------------------------------------- DIN --
DIN_KERNEL_ITEM_FEATS = (1, 2, 4, 8)  # item-feature counts the attention kernels are instantiated for
DIN_MAX_LAYERS = 4  # hidden layers of the final MLP (csrc/din_tail.hip); widths up to 1024
DIN_ACTIVATIONS = ("dice", "prelu")  # din_activation (config.py:118): nrk_din_forward_mlp's codes 0, 1


class DinParams:
    """Device-resident DIN weights in kernel layout (DINModel state_dict,
    DIN.py:133-212): concatenated embedding table (fp32 or bf16 storage),
    per-feature row offsets, prepared attention matrices and the MLP.

    Any embedding width D (``din_embedding_dim``, config.py:115; the
    state_dict's table width) and any item-feature count up to 8 32-wide
    features: the kernels read 32-wide VIRTUAL features.  Every table is
    zero-padded to m = ceil(D / 32) * 32 columns and viewed as [m * vocab, 32]
    (feature f's index i -> virtual indices m i + h), att_w0 / mlp_w0 get
    zero columns at the padded positions, and the item features are padded
    with a shared all-zero row up to 1, 2, 4 or 8 -- every extra product is
    an exact 0, so the results are those of the D-wide model.  ``n_user`` /
    ``n_item`` / ``n_ctx`` / ``vocab`` describe the caller's features;
    ``kn_*`` the kernel's (include/nrk.h, nrk_din_remap_index).

    The final MLP is read off the state_dict: ``widths`` (1 to 4 hidden
    layers, ``din_mlp_hidden_units``), ``activation`` ("dice" or "prelu",
    ``din_activation``) and, under PReLU, ``slopes`` (device float32 [L], one
    per layer).  Two-layer models also expose ``h2`` / ``mlp_w1`` / ``mlp_b1``
    / ``mlp_w2`` / ``mlp_b2``."""

    def __init__(self, state_dict, user_feats, item_feats, ctx_feats, table_dtype="fp32",
                 device="cuda"):
        import numpy as np

        def arr(k):
            v = state_dict[k]
            v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            return np.ascontiguousarray(v, dtype=np.float32)

        user_feats, item_feats, ctx_feats = list(user_feats), list(item_feats), list(ctx_feats)
        groups = ([("user_profile_embedding_dict", f) for f in user_feats]
                  + [("item_embedding_dict", f) for f in item_feats]
                  + [("context_embedding_dict", f) for f in ctx_feats])
        tabs = [arr(f"{g}.{f}.weight") for g, f in groups]
        if not tabs or not item_feats or not user_feats:
            raise ValueError("DIN needs at least one user and one item feature")
        D = tabs[0].shape[1]
        if any(t.ndim != 2 or t.shape[1] != D for t in tabs):
            raise ValueError("every embedding table must have the same width (din_embedding_dim)")
        m = -(-D // 32)
        Fu, Fi, Fc = len(user_feats), len(item_feats), len(ctx_feats)
        niv = m * Fi
        kni = next((n for n in DIN_KERNEL_ITEM_FEATS if n >= niv), None)
        if kni is None:
            raise NotImplementedError(f"DIN item features x ceil(dim / 32) must be <= 8, got {Fi} x {m}")
        self.dim, self.m = D, m
        self.n_user, self.n_item, self.n_ctx = Fu, Fi, Fc
        self.vocab = [t.shape[0] for t in tabs]
        self.kn_user, self.kn_item, self.kn_ctx = m * Fu, kni, m * Fc

        def virt(t):  # [v, D] -> [m v, 32], zero-padded columns
            if D == 32 * m:
                return t.reshape(-1, 32)
            tp = np.zeros((t.shape[0], 32 * m), np.float32)
            tp[:, :D] = t
            return tp.reshape(-1, 32)

        vt = [virt(t) for t in tabs]
        pieces = vt[:Fu] + vt[Fu:Fu + Fi] + ([np.zeros((1, 32), np.float32)] if kni > niv else []) + vt[Fu + Fi:]
        starts = np.cumsum([0] + [pc.shape[0] for pc in pieces[:-1]]).astype(np.int64)
        fb = list(starts[:Fu + Fi]) + list(starts[Fu + Fi + (1 if kni > niv else 0):])  # per caller feature
        zero_row = int(starts[Fu + Fi]) if kni > niv else 0
        # virtual feature (f, hh) of a caller feature f: row fb[f] + hh + m i for caller
        # index i -- base fb[f] + hh, virtual index m i -- so caller index 0 (the
        # collate's padding) stays virtual index 0 in every half, which is what the
        # position-major plan's padding test (mask 0, every index 0) and its pad row
        # (row 0 of each feature) assume (with index m i + hh no padding
        # row of a D > 32 model was ever recognised)
        base = ([fb[f] + hh for f in range(Fu) for hh in range(m)]
                + [fb[Fu + f] + hh for f in range(Fi) for hh in range(m)] + [zero_row] * (kni - niv)
                + [fb[Fu + Fi + f] + hh for f in range(Fc) for hh in range(m)])
        table = torch.from_numpy(np.concatenate(pieces, 0))
        _finite(table, "DIN embedding tables")
        if table_dtype == "bf16":
            self.table = table.to(torch.bfloat16).to(device).contiguous()
            self.table_code = 1
        elif table_dtype == "fp32":
            self.table = table.to(device).contiguous()
            self.table_code = 0
        else:
            raise ValueError("table_dtype must be 'fp32' or 'bf16'")
        self.row_base = torch.from_numpy(np.asarray(base, np.int64)).to(device)

        # index maps to the virtual layout (None: identity, no remap launch)
        def idx_map(F, pad_to):
            src = [f for f in range(F) for _ in range(m)] + [-1] * (pad_to - m * F)
            mul = [m] * (m * F) + [0] * (pad_to - m * F)
            add = [0] * pad_to
            return torch.tensor([src, mul, add], dtype=torch.int32).to(device).contiguous()

        self.map_user = None if m == 1 else idx_map(Fu, m * Fu)
        self.map_item = None if m == 1 and kni == Fi else idx_map(Fi, kni)
        self.map_ctx = None if m == 1 or Fc == 0 else idx_map(Fc, m * Fc)

        d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device).contiguous()  # noqa: E731
        aw0 = arr("activation_unit.mlp.0.weight")
        w0 = arr("mlp.0.weight")
        if aw0.shape != (36, 4 * Fi * D) or w0.shape[1] != D * (Fu + Fc + 2 * Fi):
            raise ValueError("state_dict shapes do not match the feature lists")

        def expand(w, F, pad_to):  # [rows, F D] -> [rows, pad_to * 32]
            x = np.zeros((w.shape[0], F, 32 * m), np.float32)
            x[:, :, :D] = w.reshape(w.shape[0], F, D)
            x = x.reshape(w.shape[0], F * m * 32)
            if pad_to * 32 > x.shape[1]:
                x = np.concatenate([x, np.zeros((w.shape[0], pad_to * 32 - x.shape[1]), np.float32)], 1)
            return x

        self.att_w0 = d(np.concatenate([expand(aw0[:, q * Fi * D:(q + 1) * Fi * D], Fi, kni) for q in range(4)], 1))
        cuts = np.cumsum([0, Fu * D, Fc * D, Fi * D, Fi * D])
        segs = [(0, Fu, m * Fu), (1, Fc, m * Fc), (2, Fi, kni), (3, Fi, kni)]
        self.mlp_w0 = d(np.concatenate([expand(w0[:, cuts[i]:cuts[i + 1]], F, pt) for i, F, pt in segs], 1))
        self.att_b0 = d(arr("activation_unit.mlp.0.bias"))
        self.att_w1 = d(arr("activation_unit.mlp.2.weight").reshape(-1))
        self.att_b1 = d(arr("activation_unit.mlp.2.bias"))
        self.mlp_b0 = d(arr("mlp.0.bias"))
        # the final MLP (DIN.py:196-212): Linear mlp.{2n} per hidden layer n < L with its
        # activation at mlp.{2n+1} (Dice: an unused ``alpha``; nn.PReLU(): ``weight`` (1,)),
        # then the one-row Linear mlp.{2L}
        L = 0
        while f"mlp.{2 * L}.weight" in state_dict:
            L += 1
        L -= 1
        if L < 1 or L > DIN_MAX_LAYERS:
            raise NotImplementedError(f"the DIN kernels implement 1 to {DIN_MAX_LAYERS} MLP hidden layers, "
                                      f"the state_dict has {L}")
        kinds = {"prelu" if f"mlp.{2 * n + 1}.weight" in state_dict else "dice" for n in range(L)}
        if any(f"mlp.{2 * n + 1}.weight" in state_dict and f"mlp.{2 * n + 1}.alpha" in state_dict
               for n in range(L)) or len(kinds) != 1:
            raise ValueError("the MLP's activations mix Dice (alpha) and PReLU (weight) layers")
        self.activation = kinds.pop()
        ws = [w0] + [arr(f"mlp.{2 * n}.weight") for n in range(1, L + 1)]
        bs = [arr(f"mlp.{2 * n}.bias") for n in range(L + 1)]
        self.widths = [int(w.shape[0]) for w in ws[:L]]
        for n in range(1, L + 1):
            if ws[n].ndim != 2 or ws[n].shape[1] != self.widths[n - 1] or bs[n].shape != (ws[n].shape[0],):
                raise ValueError("state_dict shapes do not match the feature lists")
        if ws[L].shape[0] != 1 or bs[0].shape != (self.widths[0],) or min(self.widths) < 1:
            raise ValueError("state_dict shapes do not match the feature lists")
        if max(self.widths) > 1024:
            raise NotImplementedError("the DIN kernels implement MLP widths up to 1024")
        self.mlp_ws = [d(w) for w in ws[1:L]] + [d(ws[L].reshape(-1))]  # layers 2..L, then the output row
        self.mlp_bs = [d(b) for b in bs[1:]]
        if self.activation == "prelu":
            sl = [arr(f"mlp.{2 * n + 1}.weight") for n in range(L)]
            if any(a.shape != (1,) for a in sl):
                raise NotImplementedError("nn.PReLU() with one slope per layer only (mlp.{2n+1}.weight of shape (1,))")
            self.slopes = d(np.concatenate(sl))
            _finite(self.slopes, "DIN PReLU slopes")
        else:
            self.slopes = None
        for name in ("att_w0", "att_b0", "att_w1", "att_b1", "mlp_w0", "mlp_b0"):
            _finite(getattr(self, name), f"DIN weight {name}")
        for n, t in enumerate(self.mlp_ws + self.mlp_bs):
            _finite(t, f"DIN weight mlp.{2 * (n % L + 1)}")
        if self.att_w1.numel() != 36:
            raise ValueError("state_dict shapes do not match the feature lists")
        self.h1 = self.widths[0]
        if L == 2:  # what two-layer callers have always read
            self.h2 = self.widths[1]
            self.mlp_w1, self.mlp_b1 = self.mlp_ws[0], self.mlp_bs[0]
            self.mlp_w2, self.mlp_b2 = self.mlp_ws[1], self.mlp_bs[1]
        # host arrays of nrk_din_forward_mlp (kept alive with the tensors they point to)
        self._c_widths = (ctypes.c_int * L)(*self.widths)
        self._c_w = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.mlp_ws])
        self._c_b = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.mlp_bs])
        nb = _lib.lib().nrk_din_prep_bytes(self.kn_item, self.table.shape[0])
        self.prep = torch.empty(nb, dtype=torch.uint8, device=device)
        _lib.call("nrk_din_prepare", _ptr(self.att_w0), self.kn_item, _ptr(self.table), self.table_code,
                  self.table.shape[0], _ptr(self.prep), _stream())

    def kernel_indices(self, user, item, hist, ctx):
        """Caller index tensors -> the kernel's virtual-feature layout
        (nrk_din_remap_index); identity for 32-wide models with 1/2/4/8 item
        features."""
        def remap(t, mp, f_in):
            if mp is None:
                return t
            rows = t.numel() // f_in
            out = torch.empty(t.shape[:-1] + (mp.shape[1],), dtype=torch.int32, device=t.device)
            _lib.call("nrk_din_remap_index", _ptr(t), rows, f_in, _ptr(mp), mp.shape[1], _ptr(out), _stream())
            return out

        return (remap(user, self.map_user, self.n_user), remap(item, self.map_item, self.n_item),
                remap(hist, self.map_item, self.n_item), remap(ctx, self.map_ctx, self.n_ctx))


def din_validate(p: DinParams, user, item, hist, ctx):
    """Raise ValueError if any index falls outside its embedding table (the
    kernels gather without bounds checks)."""
    for t, off in ((user, 0), (item, p.n_user), (ctx, p.n_user + p.n_item)):
        if t.numel():
            mx = t.reshape(-1, t.shape[-1]).amax(0).cpu().tolist()
            mn = int(t.min())
            if mn < 0 or any(m >= p.vocab[off + f] for f, m in enumerate(mx)):
                raise ValueError("feature index out of its embedding table")
    if hist.numel():
        mx = hist.reshape(-1, p.n_item).amax(0).cpu().tolist()
        if int(hist.min()) < 0 or any(m >= p.vocab[p.n_user + f] for f, m in enumerate(mx)):
            raise ValueError("history index out of its embedding table")


def _din_seg(B, batch_size):
    S = B if batch_size is None or batch_size >= B else int(batch_size)
    if S < B and S % 64:
        raise ValueError("batch_size must be a multiple of 64 when the samples span several batches")
    if S == B and B < 2:
        raise ValueError("batch must be >= 2 (Dice uses the batch std; B = 1 is NaN in the reference)")
    return S


def _din_two_dice(p):
    """Two Dice hidden layers: the shape nrk_din_forward_segments serves."""
    return len(p.widths) == 2 and p.activation == "dice"


def _din_workspace_bytes(p, B, S, T):
    L = _lib.lib()
    if _din_two_dice(p):
        return L.nrk_din_segments_workspace_bytes(B, S, T, p.kn_user, p.kn_item, p.kn_ctx, p.h1, p.h2)
    return L.nrk_din_mlp_workspace_bytes(B, S, T, p.kn_user, p.kn_item, p.kn_ctx, len(p.widths),
                                         ctypes.cast(p._c_widths, _P), DIN_ACTIVATIONS.index(p.activation))


def din_forward(p: DinParams, user, item, hist, ctx, mask, logits=False, workspace=None,
                out=None, validate=True, batch_size=None):
    """DIN scores of B samples: int32 index tensors user [B,Fu], item [B,Fi],
    hist [B,T,Fi], ctx [B,Fc], mask [B,T] f32 -> probs [B] (+ logits).
    ``batch_size=None``: the B samples are one Dice batch (B >= 2).
    Otherwise they are scored as consecutive batches of ``batch_size`` (a
    multiple of 64), each with its own Dice statistics -- DINRanker.predict's
    loop (DIN.py:1245-1283) in one call; a trailing batch of one row is NaN
    as in the reference.
    ``validate=False`` skips the host-side index range check (one device sync)
    for callers that validated the resident index tensors once up front."""
    _dev(user, item, hist, ctx, mask)
    B, T = mask.shape
    S = _din_seg(B, batch_size)
    _need(user, torch.int32, (B, p.n_user), "user")
    _need(item, torch.int32, (B, p.n_item), "item")
    _need(hist, torch.int32, (B, T, p.n_item), "hist")
    _need(ctx, torch.int32, (B, p.n_ctx), "ctx")
    _need(mask, torch.float32, (B, T), "mask")
    if validate:
        din_validate(p, user, item, hist, ctx)
    user, item, hist, ctx = p.kernel_indices(user, item, hist, ctx)
    if out is not None:
        _need(out, torch.float32, (B,), "out")
        probs = out
    else:
        probs = torch.empty(B, dtype=torch.float32, device=mask.device)
    lg = torch.empty(B, dtype=torch.float32, device=mask.device) if logits else None
    nb = _din_workspace_bytes(p, B, S, T)
    if workspace is None or workspace.numel() < nb:
        workspace = torch.empty(nb, dtype=torch.uint8, device=mask.device)
    if _din_two_dice(p):
        _lib.call("nrk_din_forward_segments", _ptr(p.table), p.table_code, _ptr(p.row_base), p.kn_user,
                  p.kn_item, p.kn_ctx, _ptr(user), _ptr(item), _ptr(hist), _ptr(ctx), _ptr(mask), B, S, T,
                  _ptr(p.prep), _ptr(p.att_b0), _ptr(p.att_w1), _ptr(p.att_b1), _ptr(p.mlp_w0),
                  _ptr(p.mlp_b0), p.h1, _ptr(p.mlp_w1), _ptr(p.mlp_b1), p.h2, _ptr(p.mlp_w2),
                  _ptr(p.mlp_b2), _ptr(probs), _ptr(lg), _ptr(workspace), workspace.numel(), _stream())
    else:  # other depths, PReLU: the general entry (csrc/din_tail.hip behind the same front)
        _lib.call("nrk_din_forward_mlp", _ptr(p.table), p.table_code, _ptr(p.row_base), p.kn_user,
                  p.kn_item, p.kn_ctx, _ptr(user), _ptr(item), _ptr(hist), _ptr(ctx), _ptr(mask), B, S, T,
                  _ptr(p.prep), _ptr(p.att_b0), _ptr(p.att_w1), _ptr(p.att_b1), _ptr(p.mlp_w0),
                  _ptr(p.mlp_b0), len(p.widths), ctypes.cast(p._c_widths, _P), ctypes.cast(p._c_w, _P),
                  ctypes.cast(p._c_b, _P), DIN_ACTIVATIONS.index(p.activation), _ptr(p.slopes), _ptr(probs),
                  _ptr(lg), _ptr(workspace), workspace.numel(), _stream())
    if S < B and B % S == 1:  # trailing batch of one row: std undefined -> NaN (reference)
        probs[B - 1] = float("nan")
        if lg is not None:
            lg[B - 1] = float("nan")
    return (probs, lg) if logits else probs


def din_workspace(p: DinParams, B, T, device, batch_size=None):
    S = _din_seg(B, batch_size)
    return torch.empty(_din_workspace_bytes(p, B, S, T), dtype=torch.uint8, device=device)


# ----------------------------------------------------------- DIN training --
DIN_GROUPS = ("user_profile_embedding_dict", "item_embedding_dict", "context_embedding_dict")


def din_state_keys(user_feats, item_feats, ctx_feats, hidden=(200, 80), activation="dice"):
    """(table keys, packed-weight keys, alpha keys, DINModel.state_dict() key
    order) of a DINModel (DIN.py:133-212) with ``len(hidden)`` MLP hidden
    layers.  The packed-weight keys are in the order of the packed vector;
    under "prelu" they hold each layer's slope ``mlp.{2n+1}.weight`` after its
    bias, and only the attention's Dice has an alpha."""
    L = len(hidden)
    tabs = [f"{g}.{f}.weight" for g, fs in zip(DIN_GROUPS, (user_feats, item_feats, ctx_feats)) for f in fs]
    wts = ["activation_unit.mlp.0.weight", "activation_unit.mlp.0.bias", "activation_unit.mlp.2.weight",
           "activation_unit.mlp.2.bias"]
    alphas = ["activation_unit.mlp.1.alpha"]
    order = tabs + wts[:2] + alphas + wts[2:]
    for n in range(L):
        act = f"mlp.{2 * n + 1}.weight" if activation == "prelu" else f"mlp.{2 * n + 1}.alpha"
        layer = [f"mlp.{2 * n}.weight", f"mlp.{2 * n}.bias"]
        wts += layer + ([act] if activation == "prelu" else [])
        alphas += [] if activation == "prelu" else [act]
        order += layer + [act]
    wts += [f"mlp.{2 * L}.weight", f"mlp.{2 * L}.bias"]
    return tabs, wts, alphas, order + wts[-2:]


class DinTrainParams:
    """A DINModel's parameters with their Adam moments on the device in the
    layout of nrk_din_train_grad_mlp: the per-feature embedding tables
    concatenated row-wise (``row_base`` as DinParams), the Linear layers and
    the PReLU slopes as one packed vector, the Dice alphas (no gradient, never
    updated) as given.  Depth (1 to 4 hidden layers), ``widths`` and
    ``activation`` ("dice" or "prelu") are read off the state_dict's keys as
    DinParams reads them; ``h1`` / ``h2`` name the widths of a two-layer model.
    Shapes outside the compiled training variants (din_embedding_dim != 32,
    item-feature counts other than 1, 2, 4, 8, bf16 tables, ...) raise
    NotImplementedError: they stay inference-only."""

    def __init__(self, state_dict, user_feats, item_feats, ctx_feats, table_dtype="fp32", device="cuda"):
        import numpy as np

        def arr(k):
            v = state_dict[k]
            v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            return np.ascontiguousarray(v, dtype=np.float32)

        self.feats = (list(user_feats), list(item_feats), list(ctx_feats))
        # depth and activation off the keys (DIN.py:196-212): Linear mlp.{2n}, its activation at
        # mlp.{2n+1} (Dice: ``alpha``; nn.PReLU(): ``weight`` (1,)), then the one-row Linear mlp.{2L}
        L = 0
        while f"mlp.{2 * L}.weight" in state_dict:
            L += 1
        L -= 1
        if L < 1 or L > DIN_MAX_LAYERS:
            raise NotImplementedError(f"the DIN kernels implement 1 to {DIN_MAX_LAYERS} MLP hidden layers, "
                                      f"the state_dict has {L}")
        kinds = {"prelu" if f"mlp.{2 * n + 1}.weight" in state_dict else "dice" for n in range(L)}
        if any(f"mlp.{2 * n + 1}.weight" in state_dict and f"mlp.{2 * n + 1}.alpha" in state_dict
               for n in range(L)) or len(kinds) != 1:
            raise NotImplementedError("the MLP's activations mix Dice (alpha) and PReLU (weight) layers")
        self.activation = kinds.pop()
        self.widths = [int(np.shape(state_dict[f"mlp.{2 * n}.weight"])[0]) for n in range(L)]
        if min(self.widths) < 1 or max(self.widths) > 1024:
            raise NotImplementedError("the DIN kernels implement MLP widths of 1 to 1024")
        self.tab_keys, self.w_keys, self.alpha_keys, self.order = din_state_keys(*self.feats, self.widths,
                                                                                 self.activation)
        if table_dtype not in ("fp32", "bf16"):
            raise ValueError("table_dtype must be 'fp32' or 'bf16'")
        self.table_code = 0 if table_dtype == "fp32" else 1
        tabs = [arr(k) for k in self.tab_keys]
        if not self.feats[0] or not self.feats[1]:
            raise ValueError("DIN needs at least one user and one item feature")
        self.dim = int(tabs[0].shape[1])
        if any(t.ndim != 2 or t.shape[1] != self.dim for t in tabs):
            raise ValueError("every embedding table must have the same width (din_embedding_dim)")
        self.n_user, self.n_item, self.n_ctx = (len(f) for f in self.feats)
        self.vocab = [int(t.shape[0]) for t in tabs]
        self.n_rows = sum(self.vocab)
        ws = [arr(k) for k in self.w_keys]
        self.w_shapes = [w.shape for w in ws]
        self.h1 = self.widths[0]
        if L == 2:
            self.h2 = self.widths[1]
        self._c_widths = (ctypes.c_int32 * L)(*self.widths)
        self.workspace_bytes(2, 1)  # refuses what the kernels are not built for
        cur = self.dim * (self.n_user + self.n_ctx + 2 * self.n_item)
        exp = [(36, 4 * self.n_item * self.dim), (36,), (1, 36), (1,)]
        for unit in self.widths:
            exp += [(unit, cur), (unit,)] + ([(1,)] if self.activation == "prelu" else [])
            cur = unit
        exp += [(1, cur), (1,)]
        if self.activation == "prelu" and any(np.shape(state_dict[f"mlp.{2 * n + 1}.weight"]) != (1,)
                                              for n in range(L)):
            raise NotImplementedError("nn.PReLU() with one slope per layer only (mlp.{2n+1}.weight of shape (1,))")
        if [tuple(s) for s in self.w_shapes] != exp:
            raise ValueError("state_dict shapes do not match the feature lists")
        n_w = _lib.lib().nrk_din_train_mlp_n_weights(self.dim, self.n_user, self.n_item, self.n_ctx, L,
                                                     ctypes.cast(self._c_widths, _P),
                                                     DIN_ACTIVATIONS.index(self.activation))
        if n_w != sum(int(np.prod(s)) for s in exp):
            raise RuntimeError("nrk_din_train_mlp_n_weights disagrees with the packed layout")
        self.device = torch.device(device)
        self.table = torch.from_numpy(np.concatenate(tabs, 0)).to(self.device).contiguous()
        self.row_base = torch.from_numpy(np.cumsum([0] + self.vocab[:-1]).astype(np.int64)).to(self.device)
        self.weights = torch.from_numpy(np.concatenate([w.reshape(-1) for w in ws])).to(self.device).contiguous()
        # as given, shape included (0-d in the reference): no gradient, never updated
        self.alphas = {k: torch.as_tensor(np.array(arr(k), np.float32).reshape(np.shape(state_dict[k]))).clone()
                       for k in self.alpha_keys}
        self.t_m, self.t_v = torch.zeros_like(self.table), torch.zeros_like(self.table)
        self.w_m, self.w_v = torch.zeros_like(self.weights), torch.zeros_like(self.weights)
        self.t = 0  # Adam steps taken

    def workspace_bytes(self, batch, seq_len):
        L = _lib.lib()
        nb = L.nrk_din_train_mlp_workspace_bytes(self.n_rows, self.dim, self.table_code, self.n_user, self.n_item,
                                                 self.n_ctx, len(self.widths), ctypes.cast(self._c_widths, _P),
                                                 DIN_ACTIVATIONS.index(self.activation), batch, seq_len)
        if not nb:
            raise NotImplementedError("nrk_din_train_mlp_workspace_bytes: "
                                      + L.nrk_last_error().decode(errors="replace"))
        return nb

    def split_weights(self, packed):
        """Packed vector -> {state_dict key: view of its shape}."""
        out, off = {}, 0
        for k, s in zip(self.w_keys, self.w_shapes):
            n = 1
            for x in s:
                n *= int(x)
            out[k] = packed[off:off + n].view(*s)
            off += n
        return out

    def split_table(self, table):
        out, off = {}, 0
        for k, v in zip(self.tab_keys, self.vocab):
            out[k] = table[off:off + v]
            off += v
        return out

    def state_dict(self):
        """CPU tensors under DINModel.state_dict()'s keys, in its order."""
        sd = {**self.split_table(self.table), **self.split_weights(self.weights)}
        sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
        sd.update({k: v.clone() for k, v in self.alphas.items()})
        return {k: sd[k] for k in self.order}


class DinGrads:
    """Outputs of din_train_grad.  ``loss`` [1]; ``w_grad`` dense over the
    packed weights; the table's gradient as ``t_count`` [1] ascending unique
    virtual rows ``t_rows`` with ``t_vals`` [rows, 32] (capacity: the batch's
    contributions or the table, whichever is smaller)."""

    def __init__(self, p: DinTrainParams, batch, seq_len):
        f = dict(dtype=torch.float32, device=p.device)
        self.batch, self.seq_len = batch, seq_len
        cap = min(p.n_rows, batch * (p.n_user + p.n_ctx + p.n_item * (1 + seq_len)))
        self.loss = torch.zeros(1, **f)
        self.w_grad = torch.empty(p.weights.numel(), **f)
        self.t_rows = torch.empty(cap, dtype=torch.int32, device=p.device)
        self.t_vals = torch.empty((cap, 32), **f)
        self.t_count = torch.zeros(1, dtype=torch.int32, device=p.device)

    def table_grad(self):
        n = int(self.t_count)
        return self.t_rows[:n], self.t_vals[:n]

    def dense(self, p: DinTrainParams):
        """{state_dict key: dense gradient} of every trained parameter: the
        compact list scattered back to per-feature [vocab, 32] tables."""
        rows, vals = self.table_grad()
        table = torch.zeros_like(p.table)
        table[rows.long()] = vals
        return {**p.split_table(table), **p.split_weights(self.w_grad)}


def din_train_check(p: DinTrainParams, user, item, hist, ctx, labels):
    """Range check of index tensors and labels (device syncs), once before the
    first step: what din_train_grad's kernels trust."""
    din_validate(p, user, item, hist, ctx)
    if labels.numel() and not bool(((labels == 0) | (labels == 1)).all()):
        raise ValueError("labels must be 0 or 1")


def din_train_grad(p: DinTrainParams, user, item, hist, ctx, mask, labels, out=None, loss=None, validate=True):
    """One DIN training batch without the optimiser (DIN.py:907-912): forward
    in train mode, mean BCELoss, backward.  Index tensors and mask as
    din_forward, ``labels`` [B] fp32 of 0 / 1.  ``out``: a DinGrads of the
    same shapes to reuse; ``loss``: a fp32 [1] device tensor (e.g. a slice of
    a per-step loss vector) to write instead of out.loss.  ``validate=False``
    skips the range checks for a loop over data it checked once."""
    _dev(user, item, hist, ctx, mask, labels, loss)
    B, T = mask.shape
    _need(user, torch.int32, (B, p.n_user), "user")
    _need(item, torch.int32, (B, p.n_item), "item")
    _need(hist, torch.int32, (B, T, p.n_item), "hist")
    _need(ctx, torch.int32, (B, p.n_ctx), "ctx")
    _need(mask, torch.float32, (B, T), "mask")
    _need(labels, torch.float32, (B,), "labels")
    if loss is not None:
        _need(loss, torch.float32, (1,), "loss")
    nbytes = p.workspace_bytes(B, T)
    if validate:
        din_train_check(p, user, item, hist, ctx, labels)
    ws = _tt_ws(p.device, nbytes)
    if out is None:
        out = DinGrads(p, B, T)
    elif (out.batch, out.seq_len) != (B, T):
        raise ValueError("out: a DinGrads of another shape")
    # two Dice layers run exactly what nrk_din_train_grad runs: one dispatch path behind both entries
    _lib.call("nrk_din_train_grad_mlp", _ptr(p.table), p.n_rows, p.dim, p.table_code, _ptr(p.row_base), p.n_user,
              p.n_item, p.n_ctx, _ptr(p.weights), len(p.widths), ctypes.cast(p._c_widths, _P),
              DIN_ACTIVATIONS.index(p.activation), _ptr(user), _ptr(item), _ptr(hist), _ptr(ctx),
              _ptr(mask), _ptr(labels), B, T, _ptr(out.loss if loss is None else loss), _ptr(out.w_grad),
              _ptr(out.t_rows), _ptr(out.t_vals), _ptr(out.t_count), _ptr(ws), ws.numel(), _stream())
    return out


def din_adam_step(p: DinTrainParams, grads: DinGrads, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
    """One torch.optim.Adam step (dense semantics) in place over the packed
    weights and the whole table from din_train_grad's outputs."""
    p.t += 1
    _lib.call("nrk_din_adam_step", _ptr(p.weights), _ptr(p.w_m), _ptr(p.w_v), _ptr(grads.w_grad), p.weights.numel(),
              _ptr(p.table), _ptr(p.t_m), _ptr(p.t_v), p.n_rows, p.dim, _ptr(grads.t_rows), _ptr(grads.t_vals),
              _ptr(grads.t_count), float(lr), float(betas[0]), float(betas[1]), float(eps), p.t, _stream())


# ----------------------------------------------------------------- itemcf --
class ItemCFSim:
    """Device result of nrk_itemcf_sim: one entry per distinct (i, j), sorted
    by (i, j), dense item ids.  ``first`` is the entry's first-encounter slot
    (the reference's dict insertion order); ``cnt`` the per-item click count."""

    def __init__(self, i, j, v, first, cnt, n_items):
        self.i, self.j, self.v, self.first, self.cnt = i, j, v, first, cnt
        self.n_items = n_items

    def row_offsets(self):
        """CSR offsets over dense item rows (entries are sorted by i)."""
        off = torch.empty(self.n_items + 1, dtype=torch.int64, device=self.i.device)
        _lib.call("nrk_itemcf_row_offsets", _ptr(self.i), self.i.numel(), self.n_items, _ptr(off), _stream())
        return off


def itemcf_sim(offsets, items, ts, created, n_items, loc_alpha=1.0, loc_alpha_rev=0.7,
               loc_beta=0.9, time_alpha=0.7, created_alpha=0.8):
    """ItemCF similarity (item_cf.py:17-89) over user click lists in CSR:
    offsets int64 [U+1], items int32 dense ids [N], ts int64 ms [N], created
    float64 per dense item [n_items]."""
    _dev(offsets, items, ts, created)
    _need(offsets, torch.int64, name="offsets")
    _need(items, torch.int32, (items.numel(),), "items")
    _need(ts, torch.int64, (items.numel(),), "ts")
    _need(created, torch.float64, (n_items,), "created")
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets must be 1-D with n_users + 1 entries")
    n_users = offsets.numel() - 1
    dev = offsets.device
    if items.numel():
        if int(items.min()) < 0 or int(items.max()) >= n_items:
            raise ValueError("item id out of [0, n_items)")
    if int(offsets[0]) != 0 or int(offsets[-1]) != items.numel() or bool((offsets[1:] < offsets[:-1]).any()):
        raise ValueError("offsets must be non-decreasing from 0 to len(items)")
    pair_off = torch.empty(n_users + 1, dtype=torch.int64, device=dev)
    _lib.call("nrk_itemcf_pair_offsets", _ptr(offsets), n_users, _ptr(pair_off), _stream())
    n_pairs = int(pair_off[-1])
    cap = max(n_pairs, 1)
    oi = torch.empty(cap, dtype=torch.int32, device=dev)
    oj = torch.empty(cap, dtype=torch.int32, device=dev)
    ov = torch.empty(cap, dtype=torch.float64, device=dev)
    of = torch.empty(cap, dtype=torch.int64, device=dev)
    on = torch.zeros(1, dtype=torch.int64, device=dev)
    cnt = torch.empty(n_items, dtype=torch.int64, device=dev)
    nb = _lib.lib().nrk_itemcf_workspace_bytes(n_pairs, n_items)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.call("nrk_itemcf_sim", _ptr(offsets), n_users, _ptr(items), _ptr(ts), _ptr(created),
              n_items, _ptr(pair_off), n_pairs, float(loc_alpha), float(loc_alpha_rev),
              float(loc_beta), float(time_alpha), float(created_alpha), _ptr(oi), _ptr(oj),
              _ptr(ov), _ptr(of), _ptr(on), _ptr(cnt), _ptr(ws), nb, _stream())
    n = int(on.item())
    return ItemCFSim(oi[:n], oj[:n], ov[:n], of[:n], cnt, n_items)


def itemcf_topn(row_off, cols, vals, first, topn=20):
    """Per-row top-n by (score desc, first asc) -- the reference's stable
    ``sorted(..., reverse=True)[:topn]`` (itemcf_recaller.py:41-54).
    Returns (cols [R, topn] int32 -1 padded, vals [R, topn] f64, cnt [R])."""
    if not (1 <= topn <= CF_TOPK_MAX):
        raise NotImplementedError(f"topn must be in [1, {CF_TOPK_MAX}]")
    _dev(row_off, cols, vals, first)
    _need(row_off, torch.int64, name="row_off")
    _need(cols, torch.int32, name="cols")
    _need(vals, torch.float64, (cols.numel(),), "vals")
    _need(first, torch.int64, (cols.numel(),), "first")
    n_rows = row_off.numel() - 1
    dev = row_off.device
    oc = torch.empty((n_rows, topn), dtype=torch.int32, device=dev)
    ov = torch.empty((n_rows, topn), dtype=torch.float64, device=dev)
    cnt = torch.empty(n_rows, dtype=torch.int32, device=dev)
    _lib.call("nrk_itemcf_topn", _ptr(row_off), n_rows, _ptr(cols), _ptr(vals), _ptr(first), int(topn),
              _ptr(oc), _ptr(ov), _ptr(cnt), _stream())
    return oc, ov, cnt


def itemcf_recall(q_slot, offsets, items, nbr_cols, nbr_vals, nbr_cnt, created, hot, topk,
                  loc_beta=0.9, created_alpha=0.8, emb_cols=None, emb_vals=None, emb_cnt=None):
    """ItemCFRecaller.recall (itemcf_recaller.py:56-129) for every query user at
    once.  Dense ids: q_slot [Q] int64 (CSR row or -1 = unknown user),
    offsets/items = the user_item_time_dict CSR, nbr_* = per-item top-n
    neighbours [I, topn] (itemcf_topn), created [I] f64, hot [H] int32,
    optional emb_* [I, ke] content-weight neighbours.  Returns (items [Q, topk]
    int32 -1 padded, scores [Q, topk] f64, src [Q, topk] int32 (0 candidate,
    1 hot fill, 2 cold start), cnt [Q] int32)."""
    _dev(q_slot, offsets, items, nbr_cols, nbr_vals, nbr_cnt, created, hot, emb_cols, emb_vals, emb_cnt)
    _need(q_slot, torch.int64, name="q_slot")
    _need(offsets, torch.int64, name="offsets")
    _need(items, torch.int32, name="items")
    n_items, topn = nbr_cols.shape
    _need(nbr_cols, torch.int32, name="nbr_cols")
    _need(nbr_vals, torch.float64, (n_items, topn), "nbr_vals")
    _need(nbr_cnt, torch.int32, (n_items,), "nbr_cnt")
    _need(created, torch.float64, (n_items,), "created")
    _need(hot, torch.int32, name="hot")
    ke = 0
    if emb_cols is not None:
        ke = emb_cols.shape[1]
        _need(emb_cols, torch.int32, (n_items, ke), "emb_cols")
        _need(emb_vals, torch.float64, (n_items, ke), "emb_vals")
        _need(emb_cnt, torch.int32, (n_items,), "emb_cnt")
    if not (1 <= topk <= CF_TOPK_MAX):
        raise NotImplementedError(f"topk must be in [1, {CF_TOPK_MAX}]")
    nq = q_slot.numel()
    dev = q_slot.device
    cand_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    _lib.call("nrk_itemcf_recall_offsets", _ptr(q_slot), nq, _ptr(offsets), _ptr(items), _ptr(nbr_cnt),
              _ptr(cand_off), _stream())
    n_cand = int(cand_off[nq].item())
    ws = torch.empty(_lib.lib().nrk_itemcf_recall_workspace_bytes(n_cand), dtype=torch.uint8, device=dev)
    oi = torch.empty((nq, topk), dtype=torch.int32, device=dev)
    osc = torch.empty((nq, topk), dtype=torch.float64, device=dev)
    osrc = torch.empty((nq, topk), dtype=torch.int32, device=dev)
    ocnt = torch.empty(nq, dtype=torch.int32, device=dev)
    _lib.call("nrk_itemcf_recall", _ptr(q_slot), nq, _ptr(offsets), _ptr(items), _ptr(nbr_cols),
              _ptr(nbr_vals), _ptr(nbr_cnt), topn, _ptr(created), n_items, _ptr(hot), hot.numel(),
              _ptr(emb_cols), _ptr(emb_vals), _ptr(emb_cnt), ke, float(loc_beta), float(created_alpha),
              _ptr(cand_off), n_cand, int(topk), _ptr(oi), _ptr(osc), _ptr(osrc), _ptr(ocnt), _ptr(ws),
              ws.numel(), _stream())
    return oi, osc, osrc, ocnt


# ----------------------------------------------------------------- usercf --
UC_TOPN_MAX = 1024  # nrk_usercf_topn's LDS selection


def _csr_ok(off, idx, n_cols, what):
    """offsets non-decreasing from 0 to len(idx), ids in [0, n_cols): on the
    device an id out of range is an out-of-bounds access."""
    if off.dim() != 1 or off.numel() < 1:
        raise ValueError(f"{what} offsets must be 1-D with rows + 1 entries")
    if int(off[0]) != 0 or int(off[-1]) != idx.numel() or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"{what} offsets must be non-decreasing from 0 to len({what} ids)")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_cols):
        raise ValueError(f"{what} id out of [0, {n_cols})")


def _usercf_inputs(i_off, i_users, u_off, u_items, act, pen):
    dev = _dev(i_off, i_users, u_off, u_items, act, pen)
    _need(i_off, torch.int64, name="i_off")
    _need(u_off, torch.int64, name="u_off")
    n = i_users.numel()
    _need(i_users, torch.int32, (n,), "i_users")
    _need(u_items, torch.int32, (n,), "u_items")
    n_items, n_users = i_off.numel() - 1, u_off.numel() - 1
    _need(act, torch.float64, (n_users,), "act")
    _need(pen, torch.float64, (n_items,), "pen")
    _csr_ok(i_off, i_users, n_users, "i_users")
    _csr_ok(u_off, u_items, n_items, "u_items")
    _finite(act, "act")
    _finite(pen, "pen")
    if n and n_users >= 2**31 - 1:
        raise ValueError("n_users must be < 2^31 - 1")
    # every user's clicks sorted by item: the duplicate-click test bisects them
    if n > 1:
        row = torch.repeat_interleave(torch.arange(n_users, device=dev), u_off[1:] - u_off[:-1])
        if bool(((row[1:] == row[:-1]) & (u_items[1:] < u_items[:-1])).any()):
            raise ValueError("u_items must be sorted by item inside every user")
    return dev, n_items, n_users, n


def usercf_topn(i_off, i_users, u_off, u_items, act, pen, topn=20, workspace=None):
    """UserCF similarity (user_cf.py:31-66), each user's top-n neighbours by
    (value desc, first slot asc) without materialising the u2u matrix.  Dense
    ids: i_off [I+1] / i_users [N] the item -> user CSR (items ascending,
    entries in the reference's list order), u_off [U+1] / u_items [N] every
    user's clicks sorted by item, act [U], pen [I] = 1 / log(n_i + 1) f64.
    Returns (cols [U, topn] int32 -1 padded, vals [U, topn] f64, cnt [U]
    int64 click rows, nnz [U] int32 distinct neighbours)."""
    if not (1 <= topn <= UC_TOPN_MAX):
        raise NotImplementedError(f"topn must be in [1, {UC_TOPN_MAX}]")
    dev, n_items, n_users, n = _usercf_inputs(i_off, i_users, u_off, u_items, act, pen)
    oc = torch.empty((n_users, topn), dtype=torch.int32, device=dev)
    ov = torch.empty((n_users, topn), dtype=torch.float64, device=dev)
    cnt = torch.empty(n_users, dtype=torch.int64, device=dev)
    nnz = torch.empty(n_users, dtype=torch.int32, device=dev)
    nb = _lib.lib().nrk_usercf_workspace_bytes(n_users, n, int(topn))
    ws = workspace if workspace is not None else torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.call("nrk_usercf_topn", _ptr(i_off), n_items, _ptr(i_users), _ptr(u_off), n_users, _ptr(u_items), n,
              _ptr(act), _ptr(pen), int(topn), _ptr(oc), _ptr(ov), _ptr(cnt), _ptr(nnz), _ptr(ws), ws.numel(),
              _stream())
    return oc, ov, cnt, nnz


def usercf_sim(i_off, i_users, u_off, u_items, act, pen, nnz):
    """Every entry of every u2u row (small logs, tests): nnz from usercf_topn.
    Returns (row_off [U+1] int64, v int32, value f64, first int64), a row's
    entries in no particular order (sort by first for the dict order)."""
    dev, n_items, n_users, n = _usercf_inputs(i_off, i_users, u_off, u_items, act, pen)
    _need(nnz, torch.int32, (n_users,), "nnz")
    row_off = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    row_off[1:] = torch.cumsum(nnz.to(torch.int64), 0)
    total = int(row_off[-1])
    if total >= 2**31:
        raise ValueError("the u2u matrix has >= 2^31 entries")
    cap = max(total, 1)
    ov = torch.empty(cap, dtype=torch.int32, device=dev)
    os_ = torch.empty(cap, dtype=torch.float64, device=dev)
    of = torch.empty(cap, dtype=torch.int64, device=dev)
    nb = _lib.lib().nrk_usercf_workspace_bytes(n_users, n, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.call("nrk_usercf_sim", _ptr(i_off), n_items, _ptr(i_users), _ptr(u_off), n_users, _ptr(u_items), n,
              _ptr(act), _ptr(pen), _ptr(row_off), total, _ptr(ov), _ptr(os_), _ptr(of), _ptr(ws), ws.numel(),
              _stream())
    return row_off, ov[:total], os_[:total], of[:total]


def usercf_recall(q_slot, offsets, items, nbr_cols, nbr_vals, nbr_cnt, loc_w, created, hot, topk,
                  created_alpha=0.8, emb_cols=None, emb_vals=None, emb_cnt=None):
    """UserCFRecaller.recall (usercf_recaller.py:37-118) for every query user at
    once.  Dense ids: q_slot [Q] int64 (CSR row or -1 = cold start),
    offsets / items = the user_item_time_dict CSR, nbr_* = per-user top-n
    neighbour rows [U, topn], loc_w [U] f64, created [I] f64, hot [H] int32,
    optional emb_* [I, ke].  Returns itemcf_recall's four outputs."""
    _dev(q_slot, offsets, items, nbr_cols, nbr_vals, nbr_cnt, loc_w, created, hot, emb_cols, emb_vals, emb_cnt)
    _need(q_slot, torch.int64, name="q_slot")
    _need(offsets, torch.int64, name="offsets")
    _need(items, torch.int32, name="items")
    _need(nbr_cols, torch.int32, name="nbr_cols")
    if nbr_cols.dim() != 2 or nbr_cols.shape[1] < 1:
        raise ValueError("nbr_cols must be [n_users, topn]")
    n_users, topn = nbr_cols.shape
    if offsets.numel() != n_users + 1:
        raise ValueError("offsets must have n_users + 1 entries")
    _need(nbr_vals, torch.float64, (n_users, topn), "nbr_vals")
    _need(nbr_cnt, torch.int32, (n_users,), "nbr_cnt")
    _need(loc_w, torch.float64, (n_users,), "loc_w")
    _need(created, torch.float64, name="created")
    _need(hot, torch.int32, name="hot")
    n_items = created.numel()
    if n_items < 1:
        raise ValueError("created must have one entry per item")
    _csr_ok(offsets, items, n_items, "items")
    if hot.numel() and (int(hot.min()) < 0 or int(hot.max()) >= n_items):
        raise ValueError("hot item out of range")
    if q_slot.numel() and (int(q_slot.min()) < -1 or int(q_slot.max()) >= n_users):
        raise ValueError("q_slot out of [-1, n_users)")
    if n_users:
        if int(nbr_cnt.min()) < 0 or int(nbr_cnt.max()) > topn:
            raise ValueError("nbr_cnt out of [0, topn]")
        valid = torch.arange(topn, device=nbr_cols.device)[None, :] < nbr_cnt[:, None]
        if bool((valid & ((nbr_cols < 0) | (nbr_cols >= n_users))).any()):
            raise ValueError("neighbour row out of [0, n_users)")
    ke = 0
    if emb_cols is not None:
        ke = emb_cols.shape[1]
        _need(emb_cols, torch.int32, (n_items, ke), "emb_cols")
        _need(emb_vals, torch.float64, (n_items, ke), "emb_vals")
        _need(emb_cnt, torch.int32, (n_items,), "emb_cnt")
        if n_items and (int(emb_cnt.min()) < 0 or int(emb_cnt.max()) > ke):
            raise ValueError("emb_cnt out of [0, ke]")
    if not (1 <= topk <= CF_TOPK_MAX):
        raise NotImplementedError(f"topk must be in [1, {CF_TOPK_MAX}]")
    nq = q_slot.numel()
    dev = q_slot.device
    cand_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    _lib.call("nrk_usercf_recall_offsets", _ptr(q_slot), nq, _ptr(offsets), _ptr(nbr_cols), _ptr(nbr_cnt), topn,
              _ptr(cand_off), _stream())
    n_cand = int(cand_off[nq].item())
    ws = torch.empty(_lib.lib().nrk_usercf_recall_workspace_bytes(n_cand), dtype=torch.uint8, device=dev)
    oi = torch.empty((nq, topk), dtype=torch.int32, device=dev)
    osc = torch.empty((nq, topk), dtype=torch.float64, device=dev)
    osrc = torch.empty((nq, topk), dtype=torch.int32, device=dev)
    ocnt = torch.empty(nq, dtype=torch.int32, device=dev)
    _lib.call("nrk_usercf_recall", _ptr(q_slot), nq, _ptr(offsets), _ptr(items), _ptr(nbr_cols), _ptr(nbr_vals),
              _ptr(nbr_cnt), topn, _ptr(loc_w), _ptr(created), n_items, _ptr(hot), hot.numel(), _ptr(emb_cols),
              _ptr(emb_vals), _ptr(emb_cnt), ke, float(created_alpha), _ptr(cand_off), n_cand, int(topk), _ptr(oi),
              _ptr(osc), _ptr(osrc), _ptr(ocnt), _ptr(ws), ws.numel(), _stream())
    return oi, osc, osrc, ocnt


# ------------------------------------------------------------- cold start --
CS_MAX = 2048          # survivors per user and topk of nrk_coldstart_recall
CS_WORDS_TOL = 200.0   # coldstart_recaller.py:108
CS_TIME_TOL = 0.25     # coldstart_recaller.py:114


def _coldstart_inputs(list_off, item, prof, cat_off, cat, mean_words, last_created, item_type, item_words,
                      item_created, item_clicked, validate):
    """dtype / shape checks of the arguments both cold-start ops share and,
    with ``validate``, the range checks (device reductions and host reads): a
    row out of range is an out-of-bounds access on the device.  ``item`` may
    have any shape ([U, K] rows of ip_topk); it is read flat, in list order.
    Returns the argument tuple of the C entry points from list_off to n_items
    (score left out) and the device."""
    dev = _dev(list_off, item, prof, cat_off, cat, mean_words, last_created, item_type, item_words, item_created,
               item_clicked)
    _need(list_off, torch.int64, name="list_off")
    _need(item, torch.int32, name="item")
    _need(cat_off, torch.int64, name="cat_off")
    _need(cat, torch.int32, name="cat")
    if list_off.dim() != 1 or list_off.numel() < 1 or cat_off.dim() != 1 or cat_off.numel() < 1 or cat.dim() != 1:
        raise ValueError("list_off / cat_off must be 1-D with rows + 1 entries, cat 1-D")
    n_lists, n_prof, n_items, n = list_off.numel() - 1, cat_off.numel() - 1, item_type.numel(), item.numel()
    _need(prof, torch.int32, (n_lists,), "prof")
    _need(mean_words, torch.float64, (n_prof,), "mean_words")
    _need(last_created, torch.float64, (n_prof,), "last_created")
    _need(item_type, torch.int32, (n_items,), "item_type")
    _need(item_words, torch.float64, (n_items,), "item_words")
    _need(item_created, torch.float64, (n_items,), "item_created")
    _need(item_clicked, torch.uint8, (n_items,), "item_clicked")
    if max(n, n_prof, n_items) >= 2**31:
        raise ValueError("entries, profile rows and item rows must be < 2^31")
    if validate:
        for off, m, what in ((list_off, n, "list"), (cat_off, cat.numel(), "cat")):
            if int(off[0]) != 0 or int(off[-1]) != m or bool((off[1:] < off[:-1]).any()):
                raise ValueError(f"{what} offsets must be non-decreasing from 0 to the number of {what} entries")
        if n and (int(item.min()) < -1 or int(item.max()) >= n_items):
            raise ValueError(f"item out of [-1, {n_items})")
        if n_lists and (int(prof.min()) < -1 or int(prof.max()) >= n_prof):
            raise ValueError(f"prof out of [-1, {n_prof})")
        if cat.numel() > 1:  # ascending inside every user: the kernel bisects them
            row = torch.repeat_interleave(torch.arange(n_prof, device=dev), cat_off[1:] - cat_off[:-1])
            if bool(((row[1:] == row[:-1]) & (cat[1:] <= cat[:-1])).any()):
                raise ValueError("cat must be strictly ascending inside every user")
    args = (_ptr(list_off), n_lists, _ptr(item), n, _ptr(prof), _ptr(cat_off), _ptr(cat), cat.numel(),
            _ptr(mean_words), _ptr(last_created), n_prof, _ptr(item_type), _ptr(item_words), _ptr(item_created),
            _ptr(item_clicked), n_items)
    return args, dev


def coldstart_filter(list_off, item, prof, cat_off, cat, mean_words, last_created, item_type, item_words,
                     item_created, item_clicked, words_tol=CS_WORDS_TOL, time_tol=CS_TIME_TOL, validate=True):
    """ColdStartRecaller._apply_filtering (coldstart_recaller.py:54-126) for
    every list at once, over dense ids (include/nrk.h: nrk_coldstart_filter).
    Returns (keep [N] uint8, kept [L] int32)."""
    args, dev = _coldstart_inputs(list_off, item, prof, cat_off, cat, mean_words, last_created, item_type,
                                  item_words, item_created, item_clicked, validate)
    keep = torch.empty(item.numel(), dtype=torch.uint8, device=dev)
    kept = torch.empty(list_off.numel() - 1, dtype=torch.int32, device=dev)
    _lib.call("nrk_coldstart_filter", *args, float(words_tol), float(time_tol), _ptr(keep), _ptr(kept), _stream())
    return keep, kept


def coldstart_recall(q, list_off, item, score, prof, cat_off, cat, mean_words, last_created, item_type, item_words,
                     item_created, item_clicked, topk, words_tol=CS_WORDS_TOL, time_tol=CS_TIME_TOL, validate=True):
    """ColdStartRecaller.recall (coldstart_recaller.py:128-147) for every query
    user at once: q [Q] int64 = list index or -1 (unknown user).  score is f64,
    or fp32 widened here (exact); NaN scores are refused.  Returns (pos
    [Q, topk] int32 = position inside the list, -1 padded; score [Q, topk] f64;
    cnt [Q] int32).  More than 2,048 survivors for one user raises
    NotImplementedError."""
    if score.dtype == torch.float32:
        score = score.to(torch.float64)
    _dev(q, score)
    _need(q, torch.int64, name="q")
    _need(score, torch.float64, name="score")
    if q.dim() != 1 or score.numel() != item.numel():
        raise ValueError("q must be 1-D and score must have one entry per item")
    if not (1 <= topk <= CS_MAX):
        raise NotImplementedError(f"topk must be in [1, {CS_MAX}]")
    args, dev = _coldstart_inputs(list_off, item, prof, cat_off, cat, mean_words, last_created, item_type,
                                  item_words, item_created, item_clicked, validate)
    nq, n_lists = q.numel(), list_off.numel() - 1
    if nq and (int(q.min()) < -1 or int(q.max()) >= n_lists):
        raise ValueError(f"q out of [-1, {n_lists})")
    if score.numel() and bool(torch.isnan(score).any()):
        raise ValueError("score must not hold NaN")
    opos = torch.empty((nq, topk), dtype=torch.int32, device=dev)
    osc = torch.empty((nq, topk), dtype=torch.float64, device=dev)
    ocnt = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq == 0:
        return opos, osc, ocnt
    # LDS slots per user: the longest queried list bounds its survivors
    cap = 1
    if n_lists:
        lens = (list_off[1:] - list_off[:-1])[q.clamp(min=0)]
        cap = min(max(int(torch.where(q >= 0, lens, torch.zeros_like(lens)).max()), 1), CS_MAX)
    _lib.call("nrk_coldstart_recall", _ptr(q), nq, *args[:3], _ptr(score), *args[3:], float(words_tol),
              float(time_tol), cap, int(topk), _ptr(opos), _ptr(osc), _ptr(ocnt), _stream())
    if bool((ocnt < 0).any()):
        raise NotImplementedError(f"more than {CS_MAX} survivors for one user")
    return opos, osc, ocnt


# ------------------------------------------------- profiles, popularity, labels --
def profile_user(u_off, item, ts, dev_code, n_codes, words, n_rows, validate=True):
    """FeatureExtractor._extract_user_profile_features (feature_extractor.py:
    296-389) before scaling, for every user at once (include/nrk.h:
    nrk_profile_user).  u_off [U + 1] int64, item / dev_code [N] int32, ts [N]
    int64; ``words`` [n_items] int64 with n_items <= n_rows, item rows in
    [0, n_rows) (a row past the words table is an article without a words
    entry: distinct, 0 words).  The per-user ascending item rows the kernel
    dedups over come from one torch sort of (user, item) keys here.  Returns
    (count int64, gap f64, mean_ts f64, mode int32, mean_words f64, last_item
    int32), each [U].  More than 64 codes raise NotImplementedError."""
    dev = _dev(u_off, item, ts, dev_code, words)
    _need(u_off, torch.int64, name="u_off")
    if u_off.dim() != 1 or u_off.numel() < 1:
        raise ValueError("u_off must be 1-D with users + 1 entries")
    U, N, n_items = u_off.numel() - 1, item.numel(), words.numel()
    _need(item, torch.int32, (N,), "item")
    _need(ts, torch.int64, (N,), "ts")
    _need(dev_code, torch.int32, (N,), "dev_code")
    _need(words, torch.int64, (n_items,), "words")
    if not (0 <= n_items <= n_rows < 2**31) or N >= 2**31:
        raise ValueError("need n_items <= n_rows < 2^31 and fewer than 2^31 clicks")
    lens = u_off[1:] - u_off[:-1]
    if validate:
        if int(u_off[0]) != 0 or int(u_off[-1]) != N or bool((lens < 0).any()):
            raise ValueError("u_off must be non-decreasing from 0 to the number of clicks")
        if N and (int(item.min()) < 0 or int(item.max()) >= n_rows):
            raise ValueError(f"item out of [0, {n_rows})")
        if N and (int(dev_code.min()) < 0 or int(dev_code.max()) >= n_codes):
            raise ValueError(f"dev_code out of [0, {n_codes})")
        # the mean word count is exact in any order while every partial sum is below 2^53
        if n_items and U and int(words.abs().max()) * max(int(lens.max()), 1) >= 2**53:
            raise ValueError("word counts too large for an exact sum")
    row = torch.repeat_interleave(torch.arange(U, dtype=torch.int64, device=dev), lens)
    key, _ = torch.sort(row * max(n_rows, 1) + item)
    sorted_item = (key - row * max(n_rows, 1)).to(torch.int32)
    out = [torch.empty(U, dtype=dt, device=dev) for dt in (torch.int64, torch.float64, torch.float64, torch.int32,
                                                           torch.float64, torch.int32)]
    _lib.call("nrk_profile_user", _ptr(u_off), U, _ptr(item), _ptr(ts), _ptr(dev_code), N, int(n_codes),
              _ptr(sorted_item), _ptr(words), n_items, *(_ptr(o) for o in out), _stream())
    return tuple(out)


def profile_item_count(item, n_items):
    """Clicks per item row, int64 [n_items] (value_counts of feature_extractor.py:396-398); rows outside
    [0, n_items) are ignored."""
    dev = _dev(item)
    _need(item, torch.int32, name="item")
    cnt = torch.empty(n_items, dtype=torch.int64, device=dev)
    _lib.call("nrk_profile_item_count", _ptr(item), item.numel(), n_items, _ptr(cnt), _stream())
    return cnt


def profile_minmax_scale(x, fit=None, skip_zero=False):
    """sklearn's MinMaxScaler.fit_transform of one f64 column, bit for bit
    (nrk_fuse_minmax + nrk_profile_scale).  ``fit``: the entries the scaler is
    fitted on (default: x itself).  ``skip_zero`` leaves zeros at 0.0."""
    dev = _dev(x, fit)
    _need(x, torch.float64, name="x")
    fit = x if fit is None else fit
    _need(fit, torch.float64, name="fit")
    mm = torch.zeros(2, dtype=torch.float64, device=dev)
    if fit.numel():
        _lib.call("nrk_fuse_minmax", _ptr(fit), fit.numel(), _ptr(mm), _stream())
    out = torch.empty_like(x)
    _lib.call("nrk_profile_scale", _ptr(x), x.numel(), _ptr(mm), 1 if skip_zero else 0, _ptr(out), _stream())
    return out


def profile_labels(user_rows, item_rows, last_item, offline=True):
    """FeatureExtractor._add_labels (feature_extractor.py:752-836) for (user
    row, item row) pairs, -1 = unknown: int32 [n], 1 where the item is the
    user's last click, else 0; -1 everywhere in online mode."""
    dev = _dev(user_rows, item_rows, last_item)
    n = user_rows.numel()
    _need(user_rows, torch.int32, (n,), "user_rows")
    _need(item_rows, torch.int32, (n,), "item_rows")
    _need(last_item, torch.int32, name="last_item")
    out = torch.empty(n, dtype=torch.int32, device=dev)  # the kernel bounds-checks the rows: no sync here
    _lib.call("nrk_profile_labels", _ptr(user_rows), _ptr(item_rows), n, _ptr(last_item), last_item.numel(),
              1 if offline else 0, _ptr(out), _stream())
    return out


def din_assemble(rec_rows, rec_scores, user_feat, item_feat, user_hist, hist_len, u0, nu, k_use=30, skip=1,
                 n_ctx=16, ctx_bins=10, score_lo=-1.0, score_hi=1.0, seed=23, out=None, validate=True,
                 ctx_width=None):
    """DIN inputs of the recalled pairs of users [u0, u0 + nu) (nrk_din_assemble).
    Returns dict user [P, Fu], item [P, Fi], hist [P, T, Fi], ctx [P, ctx_width]
    (the first n_ctx columns filled: synthetic score / hash bins),
    mask [P, T] f32, cand [P] (item rows), P = nu * k_use.  ``validate``
    checks every index the kernel gathers (rec_rows, user_hist, hist_len);
    callers that validated their resident tables once pass False."""
    _dev(rec_rows, rec_scores, user_feat, item_feat, user_hist, hist_len)
    n_users, k_in = rec_rows.shape
    _need(rec_rows, torch.int32, name="rec_rows")
    _need(rec_scores, torch.float32, (n_users, k_in), "rec_scores")
    _need(user_feat, torch.int32, name="user_feat")
    _need(item_feat, torch.int32, name="item_feat")
    _need(user_hist, torch.int32, name="user_hist")
    _need(hist_len, torch.int32, (n_users,), "hist_len")
    Fu, Fi, T = user_feat.shape[1], item_feat.shape[1], user_hist.shape[1]
    if user_feat.shape[0] != n_users or user_hist.shape[0] != n_users:
        raise ValueError("user tables must have one row per recalled user")
    if not (0 <= u0 and u0 + nu <= n_users):
        raise ValueError("user range out of bounds")
    if validate and nu:
        n_items = item_feat.shape[0]
        r = rec_rows[u0:u0 + nu]
        if int(r.max()) >= n_items:
            raise ValueError("rec_rows out of [0, n_items)")
        if int(user_hist.min()) < 0 or int(user_hist.max()) >= n_items:
            raise ValueError("user_hist rows out of [0, n_items)")
        if int(hist_len.min()) < 0 or int(hist_len.max()) > T:
            raise ValueError("hist_len out of [0, T]")
    W = n_ctx if ctx_width is None else ctx_width
    if n_ctx and W != n_ctx:
        raise ValueError("ctx_width must equal n_ctx when the assembly fills the context block")
    P = nu * k_use
    dev = rec_rows.device
    if out is None:
        out = {"user": torch.empty((P, Fu), dtype=torch.int32, device=dev),
               "item": torch.empty((P, Fi), dtype=torch.int32, device=dev),
               "hist": torch.empty((P, T, Fi), dtype=torch.int32, device=dev),
               "ctx": torch.empty((P, W), dtype=torch.int32, device=dev),
               "mask": torch.empty((P, T), dtype=torch.float32, device=dev),
               "cand": torch.empty(P, dtype=torch.int32, device=dev)}
    _lib.call("nrk_din_assemble", _ptr(rec_rows), _ptr(rec_scores), n_users, k_in, int(skip), int(k_use),
              _ptr(user_feat), Fu, _ptr(item_feat), item_feat.shape[0], Fi, _ptr(user_hist), _ptr(hist_len), T,
              int(n_ctx), int(ctx_bins), float(score_lo), float(score_hi), int(seed) & 0xFFFFFFFF, int(u0), int(nu),
              _ptr(out["user"]), _ptr(out["item"]), _ptr(out["hist"]), _ptr(out["ctx"]), _ptr(out["mask"]),
              _ptr(out["cand"]), _stream())
    return out


def gather_rows(src, idx):
    """out[b] = src[idx[b]] for a [n_rows, ...] table of 4-byte elements
    (int32 / float32); rows whose index is outside [0, n_rows) are zeros."""
    _dev(src, idx)
    _need(idx, torch.int32, name="idx")
    if src.dtype not in (torch.int32, torch.float32):
        raise ValueError("src must be int32 or float32")
    W = 1
    for d in src.shape[1:]:
        W *= int(d)
    n = idx.numel()
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=idx.device)
    _lib.call("nrk_gather_rows", _ptr(src), src.shape[0], W, _ptr(idx), n, _ptr(out), _stream())
    return out


# ---------------------------------------------------- users-sharded ItemCF --
def itemcf_pairs(offsets, items, ts, created, n_items, slot_base=0, loc_alpha=1.0, loc_alpha_rev=0.7,
                 loc_beta=0.9, time_alpha=0.7, created_alpha=0.8):
    """Pair tuples of a user range (nrk_itemcf_pairs): keys u64 (as int64),
    global slots int32, weights f64, local click counts int64 [n_items]."""
    _dev(offsets, items, ts, created)
    _need(offsets, torch.int64, name="offsets")
    _need(items, torch.int32, (items.numel(),), "items")
    _need(ts, torch.int64, (items.numel(),), "ts")
    _need(created, torch.float64, (n_items,), "created")
    n_users = offsets.numel() - 1
    dev = offsets.device
    pair_off = torch.empty(n_users + 1, dtype=torch.int64, device=dev)
    _lib.call("nrk_itemcf_pair_offsets", _ptr(offsets), n_users, _ptr(pair_off), _stream())
    n = int(pair_off[-1])
    if int(slot_base) < 0 or int(slot_base) + n >= (1 << 31) - (1 << 16):
        raise ValueError("slot_base + pairs must stay below 2^31 (int32 global slots)")
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    slots = torch.empty(n, dtype=torch.int32, device=dev)
    w = torch.empty(n, dtype=torch.float64, device=dev)
    cnt = torch.zeros(n_items, dtype=torch.int64, device=dev)
    _lib.call("nrk_itemcf_pairs", _ptr(offsets), n_users, _ptr(items), _ptr(ts), _ptr(created), n_items,
              _ptr(pair_off), int(slot_base), float(loc_alpha), float(loc_alpha_rev), float(loc_beta),
              float(time_alpha), float(created_alpha), _ptr(keys), _ptr(slots), _ptr(w), _ptr(cnt), _stream())
    return keys, slots, w, cnt


def itemcf_reduce(keys, slots, w, n_items, item_cnt):
    """The owner's pass (nrk_itemcf_reduce) over tuples in global slot order ->
    ItemCFSim of its items (entries sorted by (i, j))."""
    _dev(keys, slots, w, item_cnt)
    n = keys.numel()
    _need(keys, torch.int64, name="keys")
    _need(slots, torch.int32, (n,), "slots")
    _need(w, torch.float64, (n,), "w")
    _need(item_cnt, torch.int64, (n_items,), "item_cnt")
    dev = item_cnt.device
    cap = max(n, 1)
    oi = torch.empty(cap, dtype=torch.int32, device=dev)
    oj = torch.empty(cap, dtype=torch.int32, device=dev)
    ov = torch.empty(cap, dtype=torch.float64, device=dev)
    of = torch.empty(cap, dtype=torch.int64, device=dev)
    on = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.lib().nrk_itemcf_reduce_workspace_bytes(n), dtype=torch.uint8, device=dev)
    _lib.call("nrk_itemcf_reduce", _ptr(keys), _ptr(slots), _ptr(w), n, n_items, _ptr(item_cnt), _ptr(oi),
              _ptr(oj), _ptr(ov), _ptr(of), _ptr(on), _ptr(ws), ws.numel(), _stream())
    m = int(on.item())
    return ItemCFSim(oi[:m], oj[:m], ov[:m], of[:m], item_cnt, n_items)
