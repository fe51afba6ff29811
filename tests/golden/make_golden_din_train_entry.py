"""Record tests/golden/din_train_entry_small.npz: the outputs of
ops.din_train_grad (nrk_din_train_grad: two Dice hidden layers) on one MI355X
for the inputs of tests/test_gpu_din_train_layers.py::test_old_entry_is_unchanged,
from the build of a chosen commit.  The committed file was recorded from commit
71879b8, the last one before the trainer's layer loop, so that the test pins
nrk_din_train_grad to what that commit computed, bit for bit.

Usage (needs a GPU):
    python tests/golden/make_golden_din_train_entry.py [--pkg <checkout>/news-recommendation-tc_amd] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

HIDDEN = [(200, 80), (40, 24)]
B, T = 300, 9


def inputs(hidden):
    """(state, feats, batch) of one case; the test builds the same."""
    import din_train_restated as R

    rng = np.random.default_rng([5, hidden[0]])
    vocabs = ({f"u{i}": 24 - i for i in range(2)}, {f"i{i}": 24 + 3 * i for i in range(4)},
              {f"c{i}": 5 + i for i in range(3)})
    state, feats = R.random_state(rng, vocabs, hidden)
    return state, feats, R.random_batch(rng, vocabs, B, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "news-recommendation-tc_amd"))
    ap.add_argument("--out", default=os.path.join(HERE, "din_train_entry_small.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch

    from nrk import ops

    arrays = {}
    for hidden in HIDDEN:
        state, feats, batch = inputs(hidden)
        dev = lambda k, dt: torch.as_tensor(np.ascontiguousarray(batch[k])).to("cuda", dt).contiguous()  # noqa: E731
        p = ops.DinTrainParams(state, *feats)
        g = ops.din_train_grad(p, *[dev(k, torch.int32) for k in ("user", "item", "hist", "ctx")],
                               dev("mask", torch.float32), dev("label", torch.float32))
        torch.cuda.synchronize()
        n = int(g.t_count)
        pre = f"h{hidden[0]}."
        arrays.update({pre + "loss": g.loss.cpu().numpy(), pre + "w_grad": g.w_grad.cpu().numpy(),
                       pre + "t_count": g.t_count.cpu().numpy(), pre + "t_rows": g.t_rows[:n].cpu().numpy(),
                       pre + "t_vals": g.t_vals[:n].cpu().numpy()})
        print(hidden, "loss", float(g.loss), "rows", n)
    np.savez_compressed(a.out, **arrays)
    assert os.path.getsize(a.out) < 1 << 20
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
