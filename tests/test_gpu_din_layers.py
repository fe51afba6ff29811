"""GPU parity of the DIN forward for 1 to 4 MLP hidden layers and both
``din_activation`` values (nrk_din_forward_mlp: the front of
nrk_din_forward_segments, then csrc/din_tail.hip) against the float64
restatement tests/din_layers_restated.py, at every new kernel instantiation,
both sides of the layer kernel's tiles and of din_mlp2_prelu's rungs, and at
the plugin level on checkpoints of the reference's own models
(tests/golden/din_layers_small.npz).

Model: din_layers_restated.synth_layers (test_gpu_din.synth_model's naming
and scale carried on to L layers) at SCALE = 0.3, inputs redrawn until the
logits spread (std >= 0.3, |logit| <= 12) as in tests/test_gpu_din_shapes.py.

Bars: 8 x E32 rounded up to one digit, capped at the suite's 1e-5, where E32 =
max |restated fp32 - float64| over every case of a family, measured on the CPU
by tests/test_din_layers_host.py (which imports the case lists below and runs
without a GPU) and pinned here.  Probabilities: absolute.  Logits:
|d| <= bar (1 + |ref|).  Every sample of every case is checked.

Slopes: the issue's 0.25, 0, -0.5 and 3.0.  3.0 times a value scaled into
[2^13, 2^14) still fits fp16 (< 65504), so a split scale that ignored the slope
would survive it; the slope-16 cases are the ones that scale would overflow.
"""
import collections
import functools
import os
import pickle

import numpy as np
import pytest

import din_layers_restated as R
import test_gpu_din_shapes as S

pytestmark = pytest.mark.gpu

SCALE = S.SCALE

# E32 per family (logits: |d| / (1 + |ref|); probabilities: |d|), measured by
# tests/test_din_layers_host.py::test_bars_are_eight_times_the_fp32_noise on the CPU
E32 = {"fp32": (2.46e-6, 8.99e-7), "bf16": (1.90e-6, 5.40e-7), "seg": (3.10e-6, 1.05e-6)}  # (logits, probs)
# 8 x E32 rounded up to one digit, never past the 1e-5 of test_gpu_din.py
BAR = {"fp32": (1e-5, 8e-6), "bf16": (1e-5, 5e-6), "seg": (1e-5, 9e-6)}

Case = collections.namedtuple("Case", "name N S T ni h act slopes dtype lens special nu nc scale")


def case(name, N, T, ni, h, act, dtype, S=None, slopes=None, lens="ragged", special=None, nu=2, nc=2, scale=SCALE):
    h = tuple(h)
    if act == "prelu" and slopes is None:
        slopes = (0.25, 0.1, -0.2, 0.6)[:len(h)]  # different per layer: a swap moves the logits
    return Case(name, N, S, T, ni, h, act, None if slopes is None else tuple(slopes), dtype, lens, special, nu, nc,
                scale)


WIDTHS = {1: (40,), 2: (50, 24), 3: (50, 24, 10), 4: (50, 24, 10, 6)}  # 50, 10, 6: K no multiple of 4
COMBOS = [(L, act) for L in (1, 2, 3, 4) for act in ("dice", "prelu") if (L, act) != (2, "dice")]
SEG_N, SEG_S = 64 * 5 + 3, 64  # a 3-row last Dice batch, empty attention workgroups

# depth x activation: one batch of 130 (a 128-row block partly empty) and segments, both table types
DEPTH_CASES = [case(f"L{L}-{act}-{dt}-{'B130' if Sg is None else 'seg'}", N, 20, 2, WIDTHS[L], act, dt, S=Sg)
               for L, act in COMBOS for dt in ("fp32", "bf16") for N, Sg in ((130, None), (SEG_N, SEG_S))]

# the layer kernel's 64-column tile and 16-wide K chunk from both sides (a middle width is the N
# of one layer and the K of the next), h = 1024, the last hidden width 2 and 1, B = 2
WIDTH_CASES = [case(f"mid{hm}-{act}-{dt}", 130, 20, 2, (64, hm, 8), act, dt)
               for hm in (1, 63, 64, 65, 1024) for act, dt in (("dice", "fp32"), ("prelu", "bf16"))]
WIDTH_CASES += [
    case("default-200x80x2-dice", 130, 20, 4, (200, 80, 2), "dice", "bf16"),
    case("last1-200x80x1-prelu", 130, 20, 4, (200, 80, 1), "prelu", "fp32"),
    case("B2-200x80x2-dice", 2, 20, 4, (200, 80, 2), "dice", "fp32"),
    case("B2-64x65x8-prelu", 2, 20, 2, (64, 65, 8), "prelu", "bf16"),
    case("B2-40-prelu", 2, 20, 2, (40,), "prelu", "fp32"),
]

# the general front (din_att_out + din_gemm<false>: T > 64 or h1 > 256) feeding the new tail
GENERAL_CASES = [
    case("general-T70-dice-L3", 130, 70, 2, (64, 32, 8), "dice", "fp32"),
    case("general-h272-prelu-L2", 130, 20, 2, (272, 40), "prelu", "bf16"),
    case("general-T70-prelu-L1", SEG_N, 70, 1, (48,), "prelu", "bf16", S=SEG_S),
    case("general-h272-dice-L1", SEG_N, 20, 4, (272,), "dice", "fp32", S=SEG_S),
]

# din_mlp2_prelu: both sides of every din_mlp2_nt rung, the h2 edges of the shipped path's
# RUNG_SHAPES (those on its fast front: h1 <= 256, T <= 64), one batch of 130
FAST_SHAPES = [(T, h1, h2, ni) for T, h1, h2, ni, B in S.RUNG_SHAPES if h1 <= 256 and B == 130]
FAST_CASES = [case(f"fast-{('fp32', 'bf16')[n % 2]}-T{T}-h{h1}x{h2}-ni{ni}", 130, T, ni, (h1, h2), "prelu",
                   ("fp32", "bf16")[n % 2]) for n, (T, h1, h2, ni) in enumerate(FAST_SHAPES)]
FAST_CASES.append(case("fast-200x80-seg", SEG_N, 20, 4, (200, 80), "prelu", "bf16", S=SEG_S))


def persist_case():
    """More than 512 row blocks of 128 rows: din_mlp2_prelu's persistent loop runs twice."""
    return case("fast-persist", 256 * 257 + 5, 1, 1, (65, 33), "prelu", "bf16", S=256, lens="persist", nu=1, nc=0)


# slopes: nn.PReLU's 0.25, 0 (the negative side exactly 0), a negative one, one above 1, in both
# orders; 16 is past what a split scale taken from max |z1| alone could hold (module docstring)
SLOPE_CASES = [
    case("slopes-fast-0.25-0", 130, 20, 2, (64, 32), "prelu", "fp32", slopes=(0.25, 0.0)),
    case("slopes-fast--0.5-3", 130, 20, 2, (64, 32), "prelu", "bf16", slopes=(-0.5, 3.0)),
    case("slopes-fast-3-0.25", 130, 20, 2, (64, 32), "prelu", "fp32", slopes=(3.0, 0.25)),
    case("slopes-fast-16-0.25", 130, 20, 2, (64, 32), "prelu", "bf16", slopes=(16.0, 0.25), scale=0.2),
    case("slopes-fast--16-0", 130, 20, 2, (200, 80), "prelu", "fp32", slopes=(-16.0, 0.0), scale=0.2),
    case("slopes-layer-3--0.5-0", 130, 20, 2, (64, 32, 8), "prelu", "fp32", slopes=(3.0, -0.5, 0.0)),
    case("slopes-layer-0-0.25-3", 130, 20, 2, (64, 32, 8), "prelu", "bf16", slopes=(0.0, 0.25, 3.0)),
    case("slopes-head-3", 130, 20, 2, (40,), "prelu", "fp32", slopes=(3.0,)),
]

DEGENERATE_CASES = [
    # constant columns of a middle layer under Dice: std = 0, p = 0.5
    case("const-col-dice", 130, 20, 2, (64, 32, 8), "dice", "fp32", special="const_col"),
    case("const-col-dice-seg", SEG_N, 20, 2, (64, 32, 8), "dice", "bf16", S=SEG_S, special="const_col"),
    # an all-zero middle weight matrix: every sample's logit is the same
    case("zero-mid-dice", 130, 20, 2, (64, 32, 8), "dice", "bf16", special="zero_mid"),
    case("zero-mid-prelu", 130, 20, 2, (64, 32, 8), "prelu", "fp32", special="zero_mid"),
    case("zero-w1-prelu-fast", 130, 20, 2, (64, 32), "prelu", "bf16", special="zero_mid"),
]
CONSTANT_LOGITS = ("zero_mid",)

# a trailing Dice batch of ONE row: NaN in the last sample only, under either activation
ONE_ROW_CASES = [
    case("one-row-dice-L3", 64 * 2 + 1, 20, 2, (50, 24, 10), "dice", "fp32", S=64),
    case("one-row-prelu-L2", 64 * 2 + 1, 20, 2, (50, 24), "prelu", "bf16", S=64),
    case("one-row-prelu-L1", 64 * 2 + 1, 20, 2, (40,), "prelu", "fp32", S=64),
]

STATIC_CASES = DEPTH_CASES + WIDTH_CASES + GENERAL_CASES + FAST_CASES + SLOPE_CASES + DEGENERATE_CASES

# workspace hygiene + determinism: every new kernel (din_layer<dice>, din_layer<prelu>,
# din_mlp2_prelu, din_tail_head<dice>, din_tail_head<prelu>) in a segmented run
HYGIENE_CASES = ["L3-dice-fp32-seg", "L3-prelu-bf16-seg", "fast-200x80-seg", "L1-dice-bf16-seg", "L1-prelu-fp32-seg"]


def all_cases():
    return [persist_case()] + STATIC_CASES


def family(c):
    return "seg" if c.S is not None else c.dtype


# ----------------------------------------------------------------- dispatch --
def tail_kernels_of(c):
    """din_run's tail dispatch (csrc/din.hip) restated: the kernels a case runs past z1's col_stats."""
    L, act = len(c.h), c.act
    if (L, act) == (2, "dice"):  # the shipped path, untouched
        return S.kernels_of(S.case("", c.N, c.T, c.ni, c.h[0], c.h[1], c.dtype))[-4:]
    fast2 = L == 2 and c.T <= 64 and c.h[0] <= 256 and c.h[1] <= 128
    k = []
    for n in range(1, L):
        if fast2:
            nt = S.rung(-(-c.h[1] // 16), (2, 4, 5, 8))
            k += ["din_absmax", f"din_w1_pack<{nt}>", f"din_mlp2_prelu<{nt}>"]
        else:
            k.append(f"din_layer<{act}>")
        if act == "dice":
            k.append("col_stats")
    return k + [f"din_tail_head<{act}>"]


def reachable_tail_kernels():
    out = set()
    for L, act in COMBOS:
        for T in (20, 70):
            for h1 in (64, 272):
                for h2 in (1, 33, 65, 81, 129):
                    out.update(tail_kernels_of(case("", 2, T, 1, (h1, h2, 8, 8)[:L], act, "fp32")))
    return out


# -------------------------------------------------------------------- inputs --
def _draw(c, seed):
    rng = np.random.default_rng(seed)
    vu, vi, vc = S.V_USER[:c.nu], S.V_ITEM[:c.ni], S.V_CTX[:c.nc]
    sd, feats = R.synth_layers(rng, vu, vi, vc, c.h, c.act, slopes=c.slopes, scale=c.scale)
    N, T = c.N, c.T
    mask = (np.arange(T)[None] < S._lengths(rng, c)[:, None]).astype(np.float32)
    b = {"user": np.stack([rng.integers(0, v, N) for v in vu], 1),
         "item": np.stack([rng.integers(0, v, N) for v in vi], 1),
         "hist": np.stack([rng.integers(1, v, (N, T)) for v in vi], 2) * mask[:, :, None].astype(np.int64),
         "ctx": np.stack([rng.integers(0, v, N) for v in vc], 1) if vc else np.zeros((N, 0), np.int64),
         "mask": mask}
    if c.special == "const_col":
        sd["mlp.2.weight"][[1, c.h[1] - 1]] = 0
    elif c.special == "zero_mid":
        sd["mlp.2.weight"][:] = 0
    return sd, feats, b


def ref64(sd, feats, b, c, **kw):
    return R.forward_f64(sd, b["user"], b["item"], b["hist"], b["ctx"], b["mask"], feats,
                         round_bf16=c.dtype == "bf16", batch_size=c.S, **kw)


def one_row_tail(c):
    return c.S is not None and c.N % c.S == 1


@functools.lru_cache(maxsize=None)
def make_case(c):
    """Model, inputs and the float64 reference of a case; redrawn until the
    logits spread (std >= 0.3 over the case's samples) and stay below 12."""
    for attempt in range(40):
        sd, feats, b = _draw(c, attempt * 7919 + sum(map(ord, c.name)))
        p64, l64 = ref64(sd, feats, b, c)
        live = slice(0, c.N - 1) if one_row_tail(c) else slice(None)
        assert np.isfinite(l64[live]).all() and np.isfinite(p64[live]).all()
        if (c.special in CONSTANT_LOGITS or l64[live].std() >= 0.3) and np.abs(l64[live]).max() <= 12:
            for a in list(b.values()) + [p64, l64]:
                a.setflags(write=False)
            return {"sd": sd, "feats": feats, "b": b, "p64": p64, "l64": l64}
    raise AssertionError(f"{c.name}: no draw with std(logit) >= 0.3 and |logit| <= 12")


def errs(probs, lg, k, live=slice(None)):
    """(logit error in units of 1 + |ref|, probability error), max over every sample."""
    return (float(np.max(np.abs(lg[live] - k["l64"][live]) / (1.0 + np.abs(k["l64"][live])))),
            float(np.max(np.abs(probs[live] - k["p64"][live]))))


# ----------------------------------------------------------------------- GPU --
def _gpu(c, k):
    import torch

    from nrk import ops

    p = ops.DinParams(k["sd"], *k["feats"], table_dtype=c.dtype, device="cuda")
    assert p.widths == list(c.h) and p.activation == c.act
    d = lambda a, dt: torch.from_numpy(np.array(a)).to("cuda", dt)  # noqa: E731
    b = k["b"]
    args = (d(b["user"], torch.int32), d(b["item"], torch.int32), d(b["hist"], torch.int32),
            d(b["ctx"], torch.int32), d(b["mask"], torch.float32))

    def run(ws=None):
        probs, lg = ops.din_forward(p, *args, logits=True, batch_size=c.S, workspace=ws)
        torch.cuda.synchronize()
        return probs.cpu().numpy(), lg.cpu().numpy()

    return run, (lambda: ops.din_workspace(p, c.N, c.T, "cuda", batch_size=c.S)), p, args


def check(c):
    k = make_case(c)
    run = _gpu(c, k)[0]
    probs, lg = run()
    assert np.isfinite(probs).all() and np.isfinite(lg).all()
    el, ep = errs(probs, lg, k)
    bl, bp = BAR[family(c)]
    print(f"{c.name}: logit err {el:.3e} (bar {bl:.0e}), prob err {ep:.3e} (bar {bp:.0e})")
    assert el <= bl and ep <= bp, (c.name, el, ep)


@pytest.mark.parametrize("c", DEPTH_CASES, ids=lambda c: c.name)
def test_din_depth_and_activation(c):
    """1 to 4 hidden layers under Dice and PReLU (all but the shipped two-layer
    Dice), one batch of 130 and five Dice batches with a 3-row sixth."""
    check(c)


@pytest.mark.parametrize("c", WIDTH_CASES, ids=lambda c: c.name)
def test_din_layer_width_edges(c):
    """A middle width of 1, 63, 64, 65 and 1024 (din_layer's column tile as N
    and its K chunk and scalar tail as the next layer's K), the last hidden
    width 2 and 1, batches of 2."""
    check(c)


@pytest.mark.parametrize("c", GENERAL_CASES, ids=lambda c: c.name)
def test_din_general_front_feeds_the_tail(c):
    """T = 70 and h1 = 272: din_att_out + din_gemm<false> write the z1 the tail reads."""
    assert "din_gemm<false>" in S.kernels_of(S.case("", c.N, c.T, c.ni, c.h[0], 1, c.dtype))
    check(c)


@pytest.mark.parametrize("c", FAST_CASES, ids=lambda c: c.name)
def test_din_prelu_fast_path_rungs(c):
    """din_mlp2_prelu on both sides of each din_mlp2_nt rung; h2 = 129 falls to din_layer."""
    assert any(x.startswith("din_mlp2_prelu") for x in tail_kernels_of(c)) == (c.h[1] <= 128)
    check(c)


def test_din_prelu_fast_path_persistent_loop():
    c = persist_case()
    assert c.N > 65536 and c.N / 128 > 512 and c.S == 256 and c.T == 1
    assert "din_mlp2_prelu<4>" in tail_kernels_of(c)
    check(c)


@pytest.mark.parametrize("c", SLOPE_CASES, ids=lambda c: c.name)
def test_din_prelu_slopes(c):
    check(c)


@pytest.mark.parametrize("c", DEGENERATE_CASES, ids=lambda c: c.name)
def test_din_tail_degenerate(c):
    k = make_case(c)
    if c.special in CONSTANT_LOGITS:
        assert k["l64"].std() < 1e-12
    check(c)


@pytest.mark.parametrize("c", ONE_ROW_CASES, ids=lambda c: c.name)
def test_din_trailing_batch_of_one_row_is_nan(c):
    k = make_case(c)
    assert np.isnan(k["l64"][-1]) and np.isfinite(k["l64"][:-1]).all()
    probs, lg = _gpu(c, k)[0]()
    assert np.isnan(probs[-1]) and np.isnan(lg[-1])
    assert np.isfinite(probs[:-1]).all() and np.isfinite(lg[:-1]).all()
    el, ep = errs(probs, lg, k, slice(0, c.N - 1))
    assert el <= BAR["seg"][0] and ep <= BAR["seg"][1], (el, ep)


@pytest.mark.parametrize("name", HYGIENE_CASES)
def test_din_tail_workspace_hygiene_and_determinism(name):
    """A 0xFF-filled caller workspace, a zeroed one and a reused one give the same bits."""
    c = next(x for x in STATIC_CASES if x.name == name)
    k = make_case(c)
    run, make_ws = _gpu(c, k)[:2]
    ws = make_ws()
    ws.fill_(255)
    a = run(ws)
    ws.zero_()
    b = run(ws)
    r = run(ws)
    for x in a:
        assert np.isfinite(x).all()
    for x, y, z in zip(a, b, r):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert np.array_equal(x.view(np.uint32), z.view(np.uint32))
    el, ep = errs(*a, k)
    assert el <= BAR["seg"][0] and ep <= BAR["seg"][1], (el, ep)


# -------------------------------------------------------------------- plugin --
def golden_model(g, tag):
    """(state_dict, feats, hidden, activation) of one model of din_layers_small."""
    sd = {k[len("front::sd::"):]: g[k] for k in g.files if k.startswith("front::sd::")}
    sd.update({k[len(tag) + 6:]: g[k] for k in g.files if k.startswith(tag + "::sd::")})
    feats = [list(map(str, g[k])) for k in ("user_feats", "item_feats", "ctx_feats")]
    return sd, feats, [int(x) for x in g[tag + "::hidden"]], str(g[tag + "::activation"])


def write_checkpoint(g, tag, root, hidden=None, activation=None):
    """The artifact directory DINRanker.load / load_model read, with plain
    torch.save / pickle: the fixture's frames and dicts through
    test_rank_pipeline.write_artifacts, then this model's state_dict and metadata."""
    import torch

    from test_rank_pipeline import write_artifacts

    sd, (uf, itf, cf), hid, act = golden_model(g, tag)
    view = {"d32_" + k: g[k] for k in g.files if "::sd::" not in k}
    view.update({"d32_sd::" + k: v for k, v in sd.items()})
    view.update({k: g[k] for k in ("user_feats", "item_feats", "ctx_feats")})
    Files = type("Files", (dict,), {"files": property(lambda self: list(self))})
    save = write_artifacts(Files(view), 32, root)
    meta = {"user_profile_features": uf, "item_features": itf, "context_features": cf, "din_embedding_dim": 32,
            "din_attention_hidden_units": [36], "din_mlp_hidden_units": hidden or hid,
            "din_activation": activation or act, "din_seq_max_len": 30}
    with open(os.path.join(save, "din_model_metadata.pkl"), "wb") as fh:
        pickle.dump(meta, fh)
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, os.path.join(save, "din_model.pth"))
    return save


@pytest.mark.parametrize("tag", ["prelu_24x10", "dice_24x10x2", "prelu_12"])
def test_ranker_serves_reference_checkpoints(golden, tag, tmp_path):
    """DINRanker.load_model + predict on a checkpoint of the reference's own
    PReLU / three-layer / one-layer model: the reference's probabilities."""
    from nrk.config import RankConfig
    from nrk.rank.din import DINRanker

    g = golden("din_layers_small")
    write_checkpoint(g, tag, str(tmp_path))
    r = DINRanker(RankConfig(_project_root=str(tmp_path), batch_size=int(g["batch_size"])))
    r.load()
    r.load_model()
    p = r.model.params
    assert p.widths == [int(x) for x in g[tag + "::hidden"]] and p.activation == str(g[tag + "::activation"])
    probs = np.asarray(r.predict(), np.float32)
    np.testing.assert_allclose(probs, g[tag + "::probs"], atol=1e-5, rtol=0)


@pytest.mark.parametrize("hidden,activation,match", [([24, 10, 8, 4, 2], None, "1 to 4"), (None, "relu", "relu")])
def test_ranker_refuses_what_is_not_built(golden, hidden, activation, match, tmp_path):
    from nrk.config import RankConfig
    from nrk.rank.din import DINRanker

    g = golden("din_layers_small")
    write_checkpoint(g, "prelu_24x10", str(tmp_path), hidden=hidden, activation=activation)
    r = DINRanker(RankConfig(_project_root=str(tmp_path)))
    r.load()
    with pytest.raises(NotImplementedError, match=match):
        r.load_model()


def test_fused_recall_rank_with_a_prelu_model():
    """FusedRecallRank.rank with a PReLU DinParams scores its pairs exactly as
    ops.din_forward scores the same pairs."""
    import torch

    from nrk import ops
    from nrk.pipeline import FusedRecallRank
    from test_gpu_fused import _world

    rng = np.random.default_rng(11)
    U, I, D, T, k, bs = 64, 500, 32, 20, 8, 128
    vu, vi, vc = [50, 7], [60, 90], [11] * 16
    users, items, user_feat, item_feat, user_hist, hist_len = _world(rng, U, I, D, T, vu, vi)
    sd, feats = R.synth_layers(rng, vu, vi, vc, (200, 80), "prelu", slopes=(0.25, -0.4), scale=SCALE)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    p = ops.DinParams(sd, *feats, table_dtype="bf16")
    assert p.activation == "prelu" and p.widths == [200, 80]
    fused = FusedRecallRank(ops.Catalog(d(items)), p, d(user_feat), d(item_feat), d(user_hist), d(hist_len),
                            k=k, batch_size=bs, chunk_users=U)
    s, r = fused.recall(d(users))
    probs, cand = fused.rank(s, r)
    a = ops.din_assemble(r, s, fused.user_feat, fused.item_feat, fused.user_hist, fused.hist_len, 0, U, k_use=k,
                         skip=1, n_ctx=16, ctx_bins=fused.ctx_bins, seed=fused.seed, ctx_width=16)
    P = U * k
    direct = ops.din_forward(p, a["user"][:P], a["item"][:P], a["hist"][:P], a["ctx"][:P], a["mask"][:P],
                             batch_size=bs)
    torch.cuda.synchronize()
    assert torch.equal(cand, a["cand"][:P])
    assert torch.isfinite(probs).all() and float(probs.std()) > 1e-3
    assert torch.equal(probs.view(torch.int32), direct.view(torch.int32))
    # and the pairs score as the float64 restatement scores them
    h = {x: a[x][:P].cpu().numpy().astype(np.int64) for x in ("user", "item", "hist", "ctx")}
    p64, _ = R.forward_f64(sd, h["user"], h["item"], h["hist"], h["ctx"], a["mask"][:P].cpu().numpy(), feats,
                           round_bf16=True, batch_size=bs)
    assert np.abs(probs.cpu().numpy() - p64).max() <= 1e-5


@pytest.mark.parametrize("name", S.HYGIENE_CASES[:2])
def test_two_layer_dice_routing_is_the_shipped_entry(name):
    """ops.din_forward on a two-layer Dice model returns the bits of a direct
    nrk_din_forward_segments call: the new routing leaves that path alone."""
    import torch

    from nrk import _lib, ops
    from nrk.ops import _ptr, _stream

    c = next(x for x in S.SEG_CASES if x.name == name)
    k = S.make_case(c)
    p = ops.DinParams(k["sd"], *k["feats"], table_dtype=c.dtype, device="cuda")
    assert p.widths == [c.h1, c.h2] and p.activation == "dice" and p.slopes is None
    d = lambda a, dt: torch.from_numpy(np.array(a)).to("cuda", dt)  # noqa: E731
    b = k["b"]
    user, item, hist, ctx, mask = (d(b["user"], torch.int32), d(b["item"], torch.int32), d(b["hist"], torch.int32),
                                   d(b["ctx"], torch.int32), d(b["mask"], torch.float32))
    probs, lg = ops.din_forward(p, user, item, hist, ctx, mask, logits=True, batch_size=c.S)
    ku, ki, kh, kc = p.kernel_indices(user, item, hist, ctx)
    nb = _lib.lib().nrk_din_segments_workspace_bytes(c.N, c.S, c.T, p.kn_user, p.kn_item, p.kn_ctx, p.h1, p.h2)
    assert ops.din_workspace(p, c.N, c.T, "cuda", batch_size=c.S).numel() == nb
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    p2, l2 = torch.empty_like(probs), torch.empty_like(lg)
    _lib.call("nrk_din_forward_segments", _ptr(p.table), p.table_code, _ptr(p.row_base), p.kn_user, p.kn_item,
              p.kn_ctx, _ptr(ku), _ptr(ki), _ptr(kh), _ptr(kc), _ptr(mask), c.N, c.S, c.T, _ptr(p.prep),
              _ptr(p.att_b0), _ptr(p.att_w1), _ptr(p.att_b1), _ptr(p.mlp_w0), _ptr(p.mlp_b0), p.h1,
              _ptr(p.mlp_w1), _ptr(p.mlp_b1), p.h2, _ptr(p.mlp_w2), _ptr(p.mlp_b2), _ptr(p2), _ptr(l2), _ptr(ws),
              ws.numel(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(probs.view(torch.int32), p2.view(torch.int32))
    assert torch.equal(lg.view(torch.int32), l2.view(torch.int32))
    # nrk_din_forward_mlp handed the same two Dice layers restates them for the same kernels
    import ctypes

    P = ctypes.c_void_p
    nb3 = _lib.lib().nrk_din_mlp_workspace_bytes(c.N, c.S, c.T, p.kn_user, p.kn_item, p.kn_ctx, 2,
                                                 ctypes.cast(p._c_widths, P), 0)
    assert nb3 == nb
    ws.fill_(255)
    p3, l3 = torch.empty_like(probs), torch.empty_like(lg)
    _lib.call("nrk_din_forward_mlp", _ptr(p.table), p.table_code, _ptr(p.row_base), p.kn_user, p.kn_item,
              p.kn_ctx, _ptr(ku), _ptr(ki), _ptr(kh), _ptr(kc), _ptr(mask), c.N, c.S, c.T, _ptr(p.prep),
              _ptr(p.att_b0), _ptr(p.att_w1), _ptr(p.att_b1), _ptr(p.mlp_w0), _ptr(p.mlp_b0), 2,
              ctypes.cast(p._c_widths, P), ctypes.cast(p._c_w, P), ctypes.cast(p._c_b, P), 0, None, _ptr(p3),
              _ptr(l3), _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(probs.view(torch.int32), p3.view(torch.int32))
    assert torch.equal(lg.view(torch.int32), l3.view(torch.int32))
