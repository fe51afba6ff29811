"""GPU parity of the DIN forward (nrk_din_forward_segments) against the
float64 yardstick oracle.din_forward_f64, at every dispatch path, every rung
edge of the run-time ladders and every persistent loop's second trip.

Model: test_gpu_din.synth_model at SCALE = 0.3, so the logits spread over a
batch (std >= 0.3, |logit| <= 12: asserted per case, inputs are redrawn until
they hold) and a wrong statistic, a lost weight half or a dropped position
moves them by hundreds of fp32 roundings (tests/test_din_host.py shows it).

Bars: 8 x E32 rounded up to one digit, capped at the suite's 1e-5, where E32 =
max |oracle.din_forward (fp32 numpy) - float64| over every case of a family
(tests/test_din_host.py measures and pins the figures below; DESIGN.md
§tolerances).  Probabilities: absolute.  Logits: |d| <= bar (1 + |ref|).
Every sample of every case is checked.

The case lists live here and are imported by tests/test_din_host.py, which
runs without a GPU.
"""
import collections
import functools

import numpy as np
import pytest

from oracle import oracle
from test_gpu_din import synth_model

pytestmark = pytest.mark.gpu

SCALE = 0.3  # synth_model's weight scale for these tests (test_gpu_din keeps 0.05)
CUS = 256    # MI355X; the GPU tests read the real count from the device properties

# E32 per family (logits: |d| / (1 + |ref|); probabilities: |d|), measured by
# tests/test_din_host.py::test_bars_are_eight_times_the_fp32_noise on the CPU
E32 = {"fp32": (1.93e-6, 5.14e-7), "bf16": (5.33e-6, 1.58e-6), "seg": (2.18e-6, 6.46e-7)}  # (logits, probs)
# 8 x E32 rounded up to one digit, never past the 1e-5 of test_gpu_din.py
BAR = {"fp32": (1e-5, 5e-6), "bf16": (1e-5, 1e-5), "seg": (1e-5, 6e-6)}

Case = collections.namedtuple("Case", "name N S T ni h1 h2 dtype lens special nu nc")
V_USER, V_ITEM, V_CTX = [50, 300, 7], [60, 900, 5000, 70, 40, 33, 21, 19], [12, 9]


def case(name, N, T, ni, h1, h2, dtype, S=None, lens="uniform", special=None, nu=2, nc=2):
    return Case(name, N, S, T, ni, h1, h2, dtype, lens, special, nu, nc)


def persist_n_seg(cus):
    return max(260, cus + 8)


def persist_case(cus=CUS):
    """bf16, batches of 256: more position-major runs than CUs, two samples
    per din_wh2 wave, more than 512 din_mlp2 row blocks."""
    n_seg = persist_n_seg(cus)
    return case(f"persist-{n_seg}", 256 * n_seg + 5, 17, 2, 65, 33, "bf16", S=256, lens="persist")


LOOP_CASES = [
    case("pw2-fp32", 33000, 9, 2, 64, 32, "fp32"),
    case("pw2-bf16", 33000, 9, 4, 64, 32, "bf16"),
    case("attout-fp32", 8192 + 300, 70, 1, 48, 40, "fp32", nu=1, nc=0),
    case("attout-bf16", 8192 + 300, 70, 1, 48, 40, "bf16", nu=1, nc=0),
    case("head-stride", 131072 + 200, 1, 1, 64, 32, "bf16", S=4096, nu=1, nc=0),
]

# segments x general path: short last segments of 3 and 70 samples (empty
# attention workgroups), T > 64 and h1 > 256, every item-feature count
SEG_SHAPES = [(64 * 5 + 3, 64), (3 * 192 + 70, 192)]
SEG_CASES = []
for _d, _dt in enumerate(("fp32", "bf16")):
    for _n, _ni in enumerate((1, 2, 4, 8)):
        for _g, (_T, _h1) in enumerate(((70, 64), (20, 272))):
            for _s, (_N, _S) in enumerate(SEG_SHAPES):
                _h2 = (48, 144)[(_n + _s + _g) % 2]
                SEG_CASES.append(case(f"seg-{_dt}-ni{_ni}-T{_T}-h{_h1}x{_h2}-S{_S}", _N, _T, _ni, _h1, _h2, _dt,
                                      S=_S, lens="ragged"))
# the same tails on the fast path
for _ni, _dt, (_N, _S) in ((2, "fp32", SEG_SHAPES[0]), (4, "fp32", SEG_SHAPES[1]), (8, "fp32", SEG_SHAPES[0]),
                           (8, "bf16", SEG_SHAPES[1]), (4, "bf16", SEG_SHAPES[0])):
    SEG_CASES.append(case(f"segfast-{_dt}-ni{_ni}-S{_S}", _N, 20, _ni, 64, 48, _dt, S=_S, lens="ragged"))

# rung edges of din_wh2's NCH (T), din_mlp1_nt (h1), din_mlp2_nt (h2), the
# din_gemm tile edges; B = 130 and B = 2 leave a 128-row MLP block partly empty
RUNG_SHAPES = [  # (T, h1, h2, ni, B)
    (28, 1, 1, 1, 130), (29, 16, 33, 2, 130), (56, 64, 65, 4, 130), (57, 65, 32, 8, 130), (64, 128, 81, 1, 130),
    (28, 129, 64, 2, 130), (29, 208, 80, 4, 130), (56, 209, 128, 8, 130), (57, 256, 129, 2, 130),
    (64, 257, 1024, 4, 130), (28, 1024, 1, 8, 130), (29, 1024, 1024, 1, 2), (57, 200, 80, 4, 2),
    (28, 64, 32, 4, 130), (28, 256, 128, 8, 130), (29, 64, 64, 1, 130),
]
RUNG_CASES = [case(f"rung-{dt}-T{T}-h{h1}x{h2}-ni{ni}-B{B}", B, T, ni, h1, h2, dt, lens="ragged")
              for T, h1, h2, ni, B in RUNG_SHAPES for dt in ("fp32", "bf16")]
RUNG_CASES.append(case("tm1-ragged", 700, 50, 1, 200, 80, "bf16", lens="ragged"))
# item tables 1.5 x as wide: q .* k carries a larger share of h (the P_lo term of DESIGN.md §4.4)
RUNG_CASES.append(case("tm4-wide-tables", 700, 50, 4, 200, 80, "bf16", lens="ragged", special="wide"))

DEGENERATE_CASES = [
    case("allmask-bf16", 300, 50, 4, 200, 80, "bf16", special="allmask"),
    case("allmask-bf16-seg", 64 * 4, 50, 4, 200, 80, "bf16", S=64, special="allmask_seg"),
    case("zero-rows-bf16", 300, 50, 4, 200, 80, "bf16", special="zero_rows"),
    case("zero-rows-fp32", 300, 20, 2, 64, 32, "fp32", special="zero_rows"),
    case("zero-rows-general", 300, 70, 2, 272, 144, "fp32", special="zero_rows"),
    case("zero-w0-bf16", 300, 50, 4, 200, 80, "bf16", special="zero_w0"),
    case("zero-w0-fp32", 300, 20, 2, 64, 32, "fp32", special="zero_w0"),
    case("zero-w1-bf16", 300, 50, 4, 200, 80, "bf16", special="zero_w1"),
    case("zero-w1-fp32", 300, 20, 2, 64, 32, "fp32", special="zero_w1"),
    case("big-user-bf16", 300, 50, 4, 200, 80, "bf16", special="big_user"),
    case("big-item-bf16", 300, 50, 4, 200, 80, "bf16", special="big_item"),
]
# all-zero mlp.0 / mlp.2 weight: every sample's logit is the same by construction
CONSTANT_LOGITS = ("zero_w0", "zero_w1")

STATIC_CASES = LOOP_CASES + SEG_CASES + RUNG_CASES + DEGENERATE_CASES

# workspace hygiene + determinism: one shape per attention kernel
HYGIENE_CASES = ["segfast-bf16-ni4-S64", "segfast-fp32-ni2-S64", "segfast-fp32-ni4-S192",
                 "seg-fp32-ni2-T70-h64x144-S64", "seg-bf16-ni4-T20-h272x144-S64"]


def all_cases(cus=CUS):
    return [persist_case(cus)] + STATIC_CASES


def family(c):
    return "seg" if c.S is not None else c.dtype


# ----------------------------------------------------------------- dispatch --
def rung(v, rungs):
    return next((r for r in rungs if v <= r), rungs[-1])


def wh2_pw(N, S, n_seg):
    """din_wh2's samples per wave for a full segment (its launch arithmetic)."""
    gw = max(1, min(S, -(-8192 // n_seg)))
    return -(-(-(-min(S, N) // gw)) // 4)


def kernels_of(c):
    """nrk_din_forward_segments' dispatch restated: the kernel instantiations a case runs."""
    tt, NI, T, h1, h2 = c.dtype, c.ni, c.T, c.h1, c.h2
    fast = T <= 64 and h1 <= 256
    if tt == "bf16" and fast and NI <= 4:
        k = [f"din_tm_plan<{NI}>", f"din_att_tm<{NI}>"]
    elif T > 64:
        k = [f"din_att_h<{tt},{NI},2>"]
    elif NI <= 4 and (tt == "bf16" or NI < 4):
        k = [f"din_att_h2<{tt},{NI}>"]
    else:
        k = [f"din_att_h<{tt},{NI},1>"]
    if fast:
        nt1 = rung(-(-h1 // 16), (4, 8, 13, 16))
        k += [f"din_w1_pack<{nt1}>", f"din_wh2<{tt},{NI},{rung(-(-9 * T // 64), (4, 8, 9))}>",
              f"din_mlp1<{tt},{nt1}>"]
    else:
        k += [f"din_att_out<{tt}>", "din_gemm<false>"]
    if fast and h2 <= 128:
        nt2 = rung(-(-h2 // 16), (2, 4, 5, 8))
        k += [f"din_w1_pack<{nt2}>", f"din_mlp2<{nt2}>"]
    else:
        k.append("din_gemm<true>")
    return k + ["col_stats", "din_absmax", "din_head"]


def reachable_kernels():
    out = set()
    for tt in ("fp32", "bf16"):
        for NI in (1, 2, 4, 8):
            for T in (1, 29, 57, 65):
                for h1 in (16, 65, 129, 209, 257):
                    for h2 in (1, 33, 65, 81, 129):
                        out.update(kernels_of(case("", 2, T, NI, h1, h2, tt)))
    return out


# -------------------------------------------------------------------- inputs --
def _lengths(rng, c):
    N, T = c.N, c.T
    if c.lens == "uniform":
        L = rng.integers(0, T + 1, N)
        L[rng.random(N) < 0.05] = 0
    elif c.lens == "ragged":  # around the 16-row tiles, empty and full
        L = np.minimum(rng.choice([0, 1, 15, 16, 17, 31, 32, 33, T - 1, T], size=N), T)
    else:  # persist: around 16 / 17; whole segments and one whole 128-run empty
        L = rng.choice([0, 1, 15, 16, 17], size=N, p=[0.1, 0.1, 0.2, 0.3, 0.3])
        for s in (0, 3, 4, c.N // c.S - 1):
            L[s * c.S:(s + 1) * c.S] = 0
        L[7 * c.S + 128:8 * c.S] = 0
    if c.special == "allmask":
        L[:] = 0
    elif c.special == "allmask_seg":
        L[c.S:2 * c.S] = 0
    return L


def _draw(c, seed):
    rng = np.random.default_rng(seed)
    vu, vi, vc = V_USER[:c.nu], V_ITEM[:c.ni], V_CTX[:c.nc]
    sd, feats = synth_model(rng, vu, vi, vc, c.h1, c.h2, scale=SCALE)
    N, T = c.N, c.T
    mask = (np.arange(T)[None] < _lengths(rng, c)[:, None]).astype(np.float32)
    b = {"user": np.stack([rng.integers(0, v, N) for v in vu], 1),
         "item": np.stack([rng.integers(0, v, N) for v in vi], 1),
         "hist": np.stack([rng.integers(1, v, (N, T)) for v in vi], 2) * mask[:, :, None].astype(np.int64),
         "ctx": np.stack([rng.integers(0, v, N) for v in vc], 1) if vc else np.zeros((N, 0), np.int64),
         "mask": mask}
    if c.special == "zero_rows":  # constant columns: std = 0, Dice's p = 0.5
        sd["activation_unit.mlp.0.weight"][[3, 35]] = 0
        sd["mlp.0.weight"][[0, c.h1 // 2, c.h1 - 1]] = 0
        sd["mlp.2.weight"][[1, c.h2 - 1]] = 0
    elif c.special == "wide":
        for f in feats[1]:
            sd[f"item_embedding_dict.{f}.weight"] *= 1.5
    elif c.special == "zero_w0":
        sd["mlp.0.weight"][:] = 0
    elif c.special == "zero_w1":
        sd["mlp.2.weight"][:] = 0
    elif c.special in ("big_user", "big_item"):
        # one entry 64 x the largest other entry of any table: the fp16 table
        # copy's scale is taken over the whole table
        big = 64 * max(np.abs(v).max() for k, v in sd.items() if "embedding_dict" in k)
        if c.special == "big_user":
            sd[f"user_profile_embedding_dict.{feats[0][1]}.weight"][17, 5] = big
            b["user"][:4, 1] = 17
        else:
            sd[f"item_embedding_dict.{feats[1][2]}.weight"][123, 9] = -big
            b["hist"][:6, 0, 2] = 123
            b["mask"][:6, 0] = 1.0
    return sd, feats, b


def ref64(sd, feats, b, c, **mut):
    return oracle.din_forward_f64(sd, b["user"], b["item"], b["hist"], b["ctx"], b["mask"], feats,
                                  round_bf16=c.dtype == "bf16", batch_size=c.S, **mut)


def spread_ok(c, logit):
    return (c.special in CONSTANT_LOGITS or logit.std() >= 0.3) and np.abs(logit).max() <= 12


@functools.lru_cache(maxsize=None)
def make_case(c):
    """Model, inputs and the float64 reference of a case; redrawn until the
    logits spread (std >= 0.3 over the case's samples) and stay below 12."""
    for attempt in range(20):
        sd, feats, b = _draw(c, attempt * 7919 + sum(map(ord, c.name)))
        p64, l64, _ = ref64(sd, feats, b, c)
        assert np.isfinite(l64).all() and np.isfinite(p64).all()
        if spread_ok(c, l64):
            for a in list(b.values()) + [p64, l64]:
                a.setflags(write=False)
            return {"sd": sd, "feats": feats, "b": b, "p64": p64, "l64": l64}
    raise AssertionError(f"{c.name}: no draw with std(logit) >= 0.3 and |logit| <= 12")


def errs(probs, lg, k):
    """(logit error in units of 1 + |ref|, probability error), max over every sample."""
    return (float(np.max(np.abs(lg - k["l64"]) / (1.0 + np.abs(k["l64"])))),
            float(np.max(np.abs(probs - k["p64"]))))


# ----------------------------------------------------------------------- GPU --
def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _gpu(c, k, workspace=None):
    import torch

    from nrk import ops

    p = ops.DinParams(k["sd"], *k["feats"], table_dtype=c.dtype, device="cuda")
    d = lambda a, dt: torch.from_numpy(np.array(a)).to("cuda", dt)  # noqa: E731
    b = k["b"]
    args = (d(b["user"], torch.int32), d(b["item"], torch.int32), d(b["hist"], torch.int32),
            d(b["ctx"], torch.int32), d(b["mask"], torch.float32))

    def run(ws=None):
        probs, lg = ops.din_forward(p, *args, logits=True, batch_size=c.S, workspace=ws)
        torch.cuda.synchronize()
        return probs.cpu().numpy(), lg.cpu().numpy()

    return run, (lambda: ops.din_workspace(p, c.N, c.T, "cuda", batch_size=c.S))


def check(c):
    k = make_case(c)
    run, _ = _gpu(c, k)
    probs, lg = run()
    assert np.isfinite(probs).all() and np.isfinite(lg).all()
    el, ep = errs(probs, lg, k)
    bl, bp = BAR[family(c)]
    print(f"{c.name}: logit err {el:.3e} (bar {bl:.0e}), prob err {ep:.3e} (bar {bp:.0e})")
    assert el <= bl and ep <= bp, (c.name, el, ep)


def test_din_persistent_loops():
    """din_att_tm's second trip (more 128-sample runs than CUs), din_wh2 with
    two samples per wave, din_mlp2's row-block loop (more than 512 blocks)."""
    cus = _cus()
    c = persist_case(cus)
    n_seg = -(-c.N // c.S)  # the 5 samples past the last whole batch are one more
    assert n_seg == persist_n_seg(cus) + 1 and 2 * persist_n_seg(cus) > cus  # position-major runs > workgroups
    assert wh2_pw(c.N, c.S, n_seg) >= 2
    assert c.N / 128 > 512
    assert kernels_of(c)[:2] == ["din_tm_plan<2>", "din_att_tm<2>"] and "din_mlp2<4>" in kernels_of(c)
    empty = ~make_case(c)["b"]["mask"][:c.N // 128 * 128].reshape(-1, 128, c.T).any((1, 2))
    assert empty.sum() >= 9 and empty[14:16].tolist() == [False, True]  # whole segments and one lone 128-run
    check(c)


@pytest.mark.parametrize("c", LOOP_CASES, ids=lambda c: c.name)
def test_din_grid_strides(c):
    """Loops over a capped grid entered a second time: din_wh2's sample
    pipeline in one Dice batch, din_att_out past 8,192 samples, din_head past
    8,192 x 16."""
    if c.name.startswith("pw2"):
        assert wh2_pw(c.N, c.N, 1) >= 2
    elif c.name.startswith("attout"):
        assert c.N > 8192 and "din_att_out<%s>" % c.dtype in kernels_of(c)
    else:
        assert c.N > 8192 * 16
    check(c)


@pytest.mark.parametrize("c", SEG_CASES, ids=lambda c: c.name)
def test_din_segments_general_path(c):
    """Several Dice batches with a short last one (3 and 70 samples: empty
    attention workgroups write zero partial rows) on din_att_h<.,NI,2> (T = 70),
    din_att_h2 / din_att_h<.,NI,1> with din_att_out + din_gemm (h1 = 272),
    h2 on either side of 128, and the same tails on the fast path."""
    check(c)


@pytest.mark.parametrize("c", RUNG_CASES, ids=lambda c: c.name)
def test_din_rung_edges(c):
    """Both sides of every rung of din_wh2's chunk count (T), din_mlp1_nt
    (h1) and din_mlp2_nt (h2), the 64-column din_gemm tile edges and
    h = 1024, in batches of 130 and 2."""
    check(c)


@pytest.mark.parametrize("c", DEGENERATE_CASES, ids=lambda c: c.name)
def test_din_degenerate_statistics(c):
    """All-masked histories on the position-major path (every c_t = 0, max
    |wh| = 0), constant columns (std = 0: Dice's p is 0.5), all-zero weight
    matrices (max |W| = 0 behind the split scale), one table entry 64 x the
    rest (the fp16 table copy's scale)."""
    check(c)


@pytest.mark.parametrize("name", HYGIENE_CASES)
def test_din_workspace_hygiene_and_determinism(name):
    """Nothing is read before it is written (h rows past a sample's last live
    position, the partial rows of empty workgroups), and the result does not
    depend on run-to-run scheduling: a 0xFF-filled caller workspace, a zeroed
    one and a reused one give the same bits."""
    c = next(x for x in SEG_CASES if x.name == name)
    k = make_case(c)
    run, make_ws = _gpu(c, k)
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
