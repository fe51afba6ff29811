"""Time the DIN training step at the config-3 vocabularies (5 user, 4 item and
16 context features, D = 32, MLP [200, 80], T = 50) at B = 256 and B = 4096,
beside the same step as eager PyTorch on the same card.

usage: python tools/din_train_bench.py [--steps 200] [--warmup 20] [--rounds 3] [--batch 256 4096] [--skip-eager]
                                       [--hidden 200 80] [--activation dice|prelu]

nrk's step is ops.din_train_grad + ops.din_adam_step (the loop body of
DINRanker.train_on_encoded).  The eager step is the reference's way of running
it, restated here because this tool carries no other code with it: one
nn.Embedding per feature, the activation unit (Linear, Dice, Linear), the
masked weighted history, the MLP (--hidden widths with Dice or nn.PReLU() per
--activation; by default two Dice layers), sigmoid, nn.BCELoss and
optim.Adam(lr) with torch's defaults, on batches already collated on the device
(the reference encodes and collates on the host per batch; that cost is left
out, in eager's favour).  The two alternate for --rounds rounds in one
process; every time is device events around --steps steps after --warmup.  The
gradient launches and the Adam sweep are also timed alone, the sweep with its
bytes counted from the shapes: m and v read for every row, p read and p, m, v
written for the rows that move.  Prints one JSON line.  --skip-eager --batch B
leaves only nrk's kernels of one batch size in the process, for a kernel trace.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "news-recommendation-tc_amd"))
VOCAB_U, VOCAB_I, N_CTX, VOCAB_C = [200, 5000, 6, 200000, 3000], [462, 3000, 300000, 1500], 16, 11
D, HIDDEN, T, LR, NB = 32, [200, 80], 50, 1e-3, 16


def events_ms(fn, n):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(n):
        fn(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--hidden", type=int, nargs="+", default=HIDDEN, help="MLP hidden widths (1 to 4)")
    ap.add_argument("--activation", choices=["dice", "prelu"], default="dice")
    a = ap.parse_args()
    import torch
    import torch.nn as nn

    from nrk import ops

    assert torch.cuda.is_available(), "needs the GPU: a CPU run gives no time"
    dev = torch.device("cuda")
    torch.manual_seed(23)
    rng = np.random.default_rng(23)
    uf, itf, cf = ([f"{c}{i}" for i in range(n)] for c, n in (("u", len(VOCAB_U)), ("i", len(VOCAB_I)), ("c", N_CTX)))
    vocab = dict(zip(uf + itf + cf, VOCAB_U + VOCAB_I + [VOCAB_C] * N_CTX))

    class Dice(nn.Module):
        def __init__(self):
            super().__init__()
            self.alpha = nn.Parameter(torch.tensor(0.1))  # unused by the forward, as in the reference

        def forward(self, x):
            p = torch.sigmoid((x - x.mean(dim=0, keepdim=True)) / (x.std(dim=0, keepdim=True) + 1e-8))
            return p * x + (1 - p) * 0.01 * x

    class Eager(nn.Module):
        def __init__(self):
            super().__init__()
            self.user_profile_embedding_dict = nn.ModuleDict({f: nn.Embedding(vocab[f], D) for f in uf})
            self.item_embedding_dict = nn.ModuleDict({f: nn.Embedding(vocab[f], D) for f in itf})
            self.context_embedding_dict = nn.ModuleDict({f: nn.Embedding(vocab[f], D) for f in cf})
            item_dim = len(itf) * D
            self.activation_unit = nn.Module()
            self.activation_unit.mlp = nn.Sequential(nn.Linear(4 * item_dim, 36), Dice(), nn.Linear(36, 1))
            cur, layers = (len(uf) + len(cf)) * D + 2 * item_dim, []
            for h in a.hidden:
                layers += [nn.Linear(cur, h), Dice() if a.activation == "dice" else nn.PReLU()]
                cur = h
            self.mlp = nn.Sequential(*layers, nn.Linear(cur, 1))

        def forward(self, user, item, hist, ctx, mask):
            ue = torch.cat([self.user_profile_embedding_dict[f](user[:, i]) for i, f in enumerate(uf)], dim=1)
            he = torch.cat([self.item_embedding_dict[f](hist[:, :, i]) for i, f in enumerate(itf)], dim=2)
            re = torch.cat([self.item_embedding_dict[f](item[:, i]) for i, f in enumerate(itf)], dim=1)
            ce = torch.cat([self.context_embedding_dict[f](ctx[:, i]) for i, f in enumerate(cf)], dim=1)
            q = re.unsqueeze(1).expand(-1, he.shape[1], -1)
            w = self.activation_unit.mlp(torch.cat([he, q, q - he, q * he], dim=-1)) * mask.unsqueeze(-1)
            x = torch.cat([ue, ce, re, (w * he).sum(dim=1)], dim=1)
            return torch.sigmoid(self.mlp(x)).squeeze(-1)

    out = {"vocab_user": VOCAB_U, "vocab_item": VOCAB_I, "n_ctx": N_CTX, "dim": D, "hidden": a.hidden, "activation": a.activation,
           "seq_len": T,
           "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds}
    for B in a.batch:
        n = NB * B  # distinct batches the loops cycle through
        lens = np.where(rng.random(n) < 0.2, 0, rng.integers(1, T + 1, n))
        mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
        host = {"user": np.stack([rng.integers(0, v, n) for v in VOCAB_U], 1),
                "item": np.stack([rng.integers(1, v, n) for v in VOCAB_I], 1),
                "hist": np.stack([rng.integers(1, v, (n, T)) for v in VOCAB_I], 2) * mask[:, :, None].astype(np.int64),
                "ctx": rng.integers(0, VOCAB_C, (n, N_CTX)), "mask": mask,
                "label": rng.integers(0, 2, n).astype(np.float32)}
        model = Eager().to(dev)
        model.train()
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}
        # ---- nrk
        p = ops.DinTrainParams(init, uf, itf, cf, device=dev)
        data = [torch.as_tensor(host[k]).to(dev, torch.int32).contiguous() for k in ("user", "item", "hist", "ctx")]
        data += [torch.as_tensor(host[k]).to(dev, torch.float32).contiguous() for k in ("mask", "label")]
        ops.din_train_check(p, data[0], data[1], data[2], data[3], data[5])
        buf = ops.DinGrads(p, B, T)
        losses = torch.zeros(a.steps + a.warmup, dtype=torch.float32, device=dev)

        def nrk_grad_only(s):
            k = (s % NB) * B
            return ops.din_train_grad(p, *[x[k:k + B] for x in data], out=buf, loss=losses[s:s + 1], validate=False)

        def nrk_adam_only(s):
            ops.din_adam_step(p, buf, lr=LR)

        def nrk_step(s):
            ops.din_adam_step(p, nrk_grad_only(s), lr=LR)

        # ---- eager torch
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        crit = nn.BCELoss()
        batches = [[x[k * B:(k + 1) * B].long() if x.dtype == torch.int32 else x[k * B:(k + 1) * B] for x in data]
                   for k in range(NB)]

        def eager_step(s):
            user, item, hist, ctx, msk, lab = batches[s % NB]
            opt.zero_grad()
            loss = crit(model(user, item, hist, ctx, msk), lab)
            loss.backward()
            opt.step()

        for s in range(a.warmup):
            nrk_step(s)
            if not a.skip_eager:
                eager_step(s)
        torch.cuda.synchronize()
        t_nrk, t_eager = [], []
        for _ in range(a.rounds):
            t_nrk.append(events_ms(nrk_step, a.steps))
            t_eager.append(float("nan") if a.skip_eager else events_ms(eager_step, a.steps))
        t_grad = events_ms(nrk_grad_only, a.steps)
        t_adam = events_ms(nrk_adam_only, a.steps)
        active = int(((p.t_m != 0) | (p.t_v != 0)).any(dim=1).sum())
        adam_bytes = 4 * D * (2 * p.n_rows + 4 * active) + 24 * p.weights.numel()
        med = lambda x: float(np.median(x))  # noqa: E731
        out[f"B{B}"] = {
            "nrk_step_us": [round(t * 1e3, 1) for t in t_nrk], "eager_step_us": [round(t * 1e3, 1) for t in t_eager],
            "nrk_over_eager": round(med(t_nrk) / med(t_eager), 3),
            "nrk_grad_only_us": round(t_grad * 1e3, 1), "nrk_adam_only_us": round(t_adam * 1e3, 1),
            "adam_share_of_step": round(t_adam / med(t_nrk), 3), "adam_rows_moving": active,
            "adam_bytes": adam_bytes, "adam_TBps": round(adam_bytes / (t_adam * 1e-3) / 1e12, 3),
            "nrk_loss_first_last": [round(float(losses[0]), 4), round(float(losses[a.steps - 1]), 4)],
        }
        del model, opt, batches, p, data, buf
    print(json.dumps(out))


if __name__ == "__main__":
    main()
