"""The inputs of tests/test_gpu_din_train_layers.py, built here so that
tests/test_din_train_layers_host.py can assert on the CPU what every GPU case
presumes of them: no Dice column of std 0, no e_ref of 0, and for every PReLU
case compared on gradients the kink condition (min |z| >= 16 e_z in the fp64
restatement, every PReLU layer, every batch).  The condition holds batch by
batch, so each batch of a case is drawn on its own: ``find_draws`` (run on the
CPU when the tests were written) takes for every batch the first draw that
meets the condition with the case's state, at most 32 re-draws per case in
all, and the chosen draws are hard-coded in DRAWS; a case without an entry
uses draw 0 for every batch.
"""
import numpy as np

import din_train_layers_restated as RL

KINK = 16.0
MAX_DRAWS = 32
SLOPES = (0.25, 0.0, -0.5, 3.0)
WIDTHS = {1: (40,), 2: (40, 24), 3: (64, 65, 8), 4: (24, 16, 12, 8)}


def vocabs_for(n_item, n_user=2, n_ctx=3, v=24):
    return ({f"u{i}": v - i for i in range(n_user)}, {f"i{i}": v + 3 * i for i in range(n_item)},
            {f"c{i}": 5 + i for i in range(n_ctx)})


def product_vocabs():
    """The product's feature counts (5 user, 4 item, 16 context features)."""
    rng = np.random.default_rng(3)
    return ({f"u{i}": int(n) for i, n in enumerate(rng.integers(3, 2000, 5))},
            {f"i{i}": int(n) for i, n in enumerate([2000, 400, 60, 9])},
            {f"c{i}": int(n) for i, n in enumerate(rng.integers(3, 40, 16))})


def _case(cid, hidden, act, Bs, T, n_item, slopes=None, vocabs=None, grads=True):
    return dict(id=cid, hidden=tuple(hidden), act=act, Bs=tuple(Bs), T=T, n_item=n_item, slopes=slopes,
                vocabs=vocabs, grads=grads)


def sweep_cases():
    """Depth x activation (minus two Dice layers: test_gpu_din_train's sweep)
    x batch x history length x item features."""
    out = []
    for L in (1, 2, 3, 4):
        for act in ("dice", "prelu"):
            if (L, act) == (2, "dice"):
                continue
            for B in (2, 37, 513):
                for T in (1, 7):
                    for n_item in (1, 4):
                        out.append(_case(f"sweep-{act}-L{L}-B{B}-T{T}-ni{n_item}", WIDTHS[L], act, [B] * 4, T,
                                         n_item))
    return out


def edge_cases():
    """Tile (64) and split-K edges of dt_gemm in every role a layer's width
    plays (N of its own product, K of the next, M and N of the two dW)."""
    out = []
    for act in ("dice", "prelu"):
        for mid in (1, 63, 64, 65, 1024):
            B = 8 if mid == 1024 else 37
            out.append(_case(f"edge-{act}-mid{mid}", (24, mid, 8), act, [B] * 4, 3, 2))
        out.append(_case(f"edge-{act}-last1", (24, 10, 1), act, [37] * 4, 3, 2))
        out.append(_case(f"edge-{act}-widening", (8, 40, 72), act, [37] * 4, 3, 2))
    # ksplit = 16 (B / 256): every dW through sixteen slices
    out.append(_case("edge-prelu-B4096", (24, 10), "prelu", [4096, 64, 64, 64], 2, 1, vocabs="few"))
    return out


def slope_cases():
    return [_case("slopes-L4", WIDTHS[4], "prelu", [37] * 4, 7, 4, slopes=SLOPES),
            _case("slopes-L3-B513", WIDTHS[3], "prelu", [513] * 4, 7, 1, slopes=(0.0, 3.0, -0.5)),
            _case("slopes-L1", WIDTHS[1], "prelu", [200] * 4, 1, 2, slopes=(-0.5,))]


def loss_only_case():
    """Too many PReLU elements (4096 x 280) for the kink condition: the forward
    is continuous at the kink, so the losses are compared, nothing else."""
    return _case("config3-prelu-200x80", (200, 80), "prelu", [4096, 64, 64, 64], 50, 4, vocabs="product", grads=False)


def grad_cases():
    return sweep_cases() + edge_cases() + slope_cases()


# case id -> the draw of each of its batches, where some batch misses the kink condition at draw 0
# (find_draws; PReLU cases only)
DRAWS = {
    "sweep-prelu-L1-B37-T7-ni4": (0, 0, 1, 0),
    "sweep-prelu-L1-B513-T1-ni1": (0, 0, 0, 1),
    "sweep-prelu-L1-B513-T7-ni1": (1, 0, 0, 0),
    "sweep-prelu-L1-B513-T7-ni4": (1, 0, 0, 0),
    "sweep-prelu-L2-B37-T1-ni1": (0, 1, 0, 0),
    "sweep-prelu-L2-B37-T7-ni1": (0, 0, 0, 2),
    "sweep-prelu-L2-B513-T1-ni1": (0, 0, 3, 2),
    "sweep-prelu-L2-B513-T1-ni4": (1, 2, 3, 2),
    "sweep-prelu-L2-B513-T7-ni1": (4, 2, 1, 0),
    "sweep-prelu-L2-B513-T7-ni4": (1, 2, 0, 4),
    "sweep-prelu-L3-B37-T1-ni1": (0, 1, 0, 0),
    "sweep-prelu-L3-B37-T1-ni4": (0, 1, 0, 1),
    "sweep-prelu-L3-B37-T7-ni4": (0, 1, 0, 0),
    "sweep-prelu-L3-B513-T1-ni1": (2, 3, 1, 3),
    "sweep-prelu-L3-B513-T1-ni4": (1, 0, 0, 2),
    "sweep-prelu-L3-B513-T7-ni1": (0, 4, 4, 2),
    "sweep-prelu-L3-B513-T7-ni4": (0, 12, 8, 1),
    "sweep-prelu-L4-B513-T1-ni1": (0, 0, 2, 0),
    "sweep-prelu-L4-B513-T1-ni4": (1, 1, 0, 1),
    "sweep-prelu-L4-B513-T7-ni1": (1, 0, 2, 1),
    "sweep-prelu-L4-B513-T7-ni4": (1, 1, 0, 0),
    "edge-prelu-mid1024": (0, 1, 1, 0),
    "edge-prelu-last1": (0, 1, 0, 0),
    "edge-prelu-B4096": (25, 0, 0, 0),
    "slopes-L3-B513": (2, 5, 3, 2),
}


def _vocabs(case):
    if case["vocabs"] == "product":
        return product_vocabs()
    if case["vocabs"] == "few":  # a short MLP input row: a smaller e_z where B x widths is large
        return vocabs_for(case["n_item"], n_user=1, n_ctx=1, v=40)
    return vocabs_for(case["n_item"])


def _key(case):
    import zlib

    return zlib.crc32(case["id"].encode())


def build_state(case):
    return RL.random_state(np.random.default_rng([_key(case), 0]), _vocabs(case), case["hidden"], case["act"],
                           case["slopes"])


def build_batch(case, j, draw):
    """Batch j of a case; B = 2: distinct candidates and full histories, so
    that no Dice column has std 0."""
    B = case["Bs"][j]
    return RL.random_batch(np.random.default_rng([_key(case), 1 + j, draw]), _vocabs(case), B, case["T"],
                           full=B == 2, distinct=B == 2)


def build(case, draws=None):
    """(state, feats, batches) of a case."""
    draws = DRAWS.get(case["id"], (0,) * len(case["Bs"])) if draws is None else draws
    state, feats = build_state(case)
    return state, feats, [build_batch(case, j, d) for j, d in enumerate(draws)]


def kink_ratio(state, feats, batches):
    """min over the batches and the PReLU layers of min |z| / e_z."""
    return min(z / e for b in batches for z, e in RL.prelu_gaps(state, feats, b))


def find_draws(case):
    """Per batch the first draw that meets the kink condition, within
    MAX_DRAWS re-draws for the whole case; None where they do not suffice."""
    state, feats = build_state(case)
    left, draws = MAX_DRAWS, []
    for j in range(len(case["Bs"])):
        d = 0
        while kink_ratio(state, feats, [build_batch(case, j, d)]) < KINK:
            d, left = d + 1, left - 1
            if left < 0:
                return None
        draws.append(d)
    return tuple(draws)


if __name__ == "__main__":  # prints the DRAWS table
    for c in grad_cases():
        if c["act"] == "prelu":
            d = find_draws(c)
            if d is None or any(d):
                print(f'    "{c["id"]}": {d},', flush=True)
