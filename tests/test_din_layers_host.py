"""CPU side of the DIN depth / activation tests: the numpy restatement
tests/din_layers_restated.py against what the reference computed
(tests/golden/din_layers_small.npz) and against oracle.din_forward_f64, the
bars tests/test_gpu_din_layers.py pins (its case lists are imported, so they
cannot drift), the cases' power to see a lost PReLU slope, the C ABI's argument
checks and the coverage of the new dispatch.

Measured here (restated fp32 against float64, max over every sample of every
case of a family; logits as |d| / (1 + |ref|), probabilities as |d|):

    family              E32 logits   E32 probs   bar logits   bar probs
    fp32 tables         2.46e-6      8.99e-7     1e-5         8e-6
    bf16 tables         1.90e-6      5.40e-7     1e-5         5e-6
    segmented runs      3.10e-6      1.05e-6     1e-5         9e-6

Bars are 8 x E32 rounded up to one digit and capped at 1e-5, the bar of
tests/test_gpu_din.py; the logit bars sit at the cap (3 to 5 x E32).  The fp32
and bf16 figures are set by the slope-16 cases, the segmented one by the
four-layer PReLU model.  "Slope taken as 1" moves a logit of every PReLU case
by more than 100 bars (the smallest: 2.3e-1 = 25,000 bars, on the constant-logit
case zero-w1-prelu-fast).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import din_layers_restated as R
import test_gpu_din_layers as G
import test_gpu_din_shapes as S

CASES = G.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODELS = ["prelu_24x10", "dice_24x10x2", "prelu_12"]


# -------------------------------------------------------------------- golden --
def _inputs(g):
    return {k: g[k].astype(np.int64 if k != "mask" else np.float32) for k in ("user", "item", "hist", "ctx", "mask")}


@pytest.mark.parametrize("tag", MODELS)
def test_restated_fp32_reproduces_the_reference(golden, tag):
    """The bar tests/test_oracle_golden.py holds oracle.din_forward to on din_small."""
    g = golden("din_layers_small")
    sd, feats, hidden, act = G.golden_model(g, tag)
    assert R.mlp_shape(sd) == (hidden, act)
    b, bs = _inputs(g), int(g["batch_size"])
    n = len(b["mask"])
    assert n % bs >= 2  # no one-row batch in the fixture
    for s in range(0, n, bs):
        sl = slice(s, min(n, s + bs))
        p, lg = R.forward_f32(sd, *(b[x][sl] for x in ("user", "item", "hist", "ctx", "mask")), feats)
        np.testing.assert_allclose(lg, g[tag + "::logits"][sl], atol=1e-5, rtol=1e-5)
        np.testing.assert_allclose(p, g[tag + "::probs"][sl], atol=1e-5, rtol=0)
    # the float64 form, batched the same way, within the fp32-table bars
    p64, l64 = R.forward_f64(sd, b["user"], b["item"], b["hist"], b["ctx"], b["mask"], feats, batch_size=bs)
    bl, bp = G.BAR["seg"]
    assert np.max(np.abs(g[tag + "::logits"] - l64) / (1 + np.abs(l64))) <= bl
    assert np.max(np.abs(g[tag + "::probs"] - p64)) <= bp


def test_golden_slopes_are_trained_values(golden):
    g = golden("din_layers_small")
    assert [float(g[f"prelu_24x10::sd::mlp.{n}.weight"][0]) for n in (1, 3)] == [1.5, np.float32(-0.3)]
    assert g["prelu_24x10::sd::mlp.1.weight"].shape == (1,) and "dice_24x10x2::sd::mlp.1.alpha" in g.files
    assert g["dice_24x10x2::sd::mlp.6.weight"].shape == (1, 2) and g["prelu_12::sd::mlp.2.weight"].shape == (1, 12)


@pytest.mark.parametrize("tag", MODELS)
def test_expected_state_is_exact_under_both_activations(golden, tag):
    """_expected_state(activation) is the reference state_dict's key and shape set."""
    from nrk.rank.din import _expected_state

    g = golden("din_layers_small")
    sd, (uf, itf, cf), hidden, act = G.golden_model(g, tag)
    voc = lambda grp, fs: {f: sd[f"{grp}.{f}.weight"].shape[0] for f in fs}  # noqa: E731
    exp = _expected_state(voc("user_profile_embedding_dict", uf), voc("item_embedding_dict", itf),
                          voc("context_embedding_dict", cf), 32, hidden, act)
    assert {k: tuple(v.shape) for k, v in sd.items()} == exp
    other = _expected_state(voc("user_profile_embedding_dict", uf), voc("item_embedding_dict", itf),
                            voc("context_embedding_dict", cf), 32, hidden, "dice" if act == "prelu" else "prelu")
    assert set(other) != set(exp)


# ---------------------------------------------------------- the old yardstick --
@pytest.mark.parametrize("name", ["segfast-bf16-ni4-S64", "rung-fp32-T56-h64x65-ni4-B130", "zero-rows-general",
                                  "seg-fp32-ni2-T70-h64x144-S64"])
def test_f64_restatement_is_the_oracle_on_two_layer_dice(name):
    c = next(x for x in S.all_cases() if x.name == name)
    k = S.make_case(c)
    b = k["b"]
    assert R.mlp_shape(k["sd"]) == ([c.h1, c.h2], "dice")
    p, lg = R.forward_f64(k["sd"], b["user"], b["item"], b["hist"], b["ctx"], b["mask"], k["feats"],
                          round_bf16=c.dtype == "bf16", batch_size=c.S)
    assert np.array_equal(p, k["p64"]) and np.array_equal(lg, k["l64"])


def test_f64_one_row_batch_is_nan():
    c = G.ONE_ROW_CASES[1]
    k = G.make_case(c)
    assert np.isnan(k["p64"][-1]) and np.isnan(k["l64"][-1]) and np.isfinite(k["l64"][:-1]).all()


# ---------------------------------------------------------------------- bars --
@functools.lru_cache(maxsize=None)
def _e32(c):
    """(logits, probs) error of the restated fp32 forward against float64, batch by batch."""
    k = G.make_case(c)
    b = k["b"]
    seg = c.S or c.N
    pr, lg = np.empty(c.N, np.float32), np.empty(c.N, np.float32)
    for s in range(0, c.N, seg):
        sl = slice(s, min(c.N, s + seg))
        pr[sl], lg[sl] = R.forward_f32(k["sd"], *(b[x][sl] for x in ("user", "item", "hist", "ctx", "mask")),
                                       k["feats"], round_bf16=c.dtype == "bf16")
    assert np.isfinite(lg).all()
    return G.errs(pr, lg, k)


def _ceil1(x):
    """x rounded up to one significant digit."""
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


def test_bars_are_eight_times_the_fp32_noise():
    for fam in ("fp32", "bf16", "seg"):
        e = {c.name: _e32(c) for c in CASES if G.family(c) == fam}
        el, ep = max(v[0] for v in e.values()), max(v[1] for v in e.values())
        print(f"E32 {fam}: logits {el:.3e} at {max(e, key=lambda n: e[n][0])}, "
              f"probs {ep:.3e} at {max(e, key=lambda n: e[n][1])}")
        for got, rec, bar in zip((el, ep), G.E32[fam], G.BAR[fam]):
            # the recorded figure is this one up to the host BLAS's summation order, and
            # the bar is 8 x it rounded up to one digit, never past the suite's 1e-5
            assert 0.5 * rec <= got <= 1.5 * rec, (fam, got, rec)
            assert bar == pytest.approx(min(_ceil1(8 * rec), 1e-5), rel=1e-9), (fam, rec, bar)
            # and 8 x the figure measured here, rounded up the same way, stays within the pinned bar
            assert min(_ceil1(8 * got), 1e-5) <= bar * (1 + 1e-9), (fam, got, bar)
            assert got < bar


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_logits_spread_and_fp32_meets_the_bar(c):
    k = G.make_case(c)
    lg = k["l64"]
    assert np.abs(lg).max() <= 12
    if c.special in G.CONSTANT_LOGITS:
        assert lg.std() < 1e-12 and not k["sd"]["mlp.2.weight"].any()
    else:
        assert lg.std() >= 0.3
    if c.special == "const_col":  # the constant columns are there: z2 of a zero row is its bias
        assert not k["sd"]["mlp.2.weight"][[1, c.h[1] - 1]].any()
    assert R.mlp_shape(k["sd"]) == (list(c.h), c.act)
    el, ep = _e32(c)
    bl, bp = G.BAR[G.family(c)]
    assert el <= bl and ep <= bp, (el, ep)


# --------------------------------------------------------------- sensitivity --
PRELU_CASES = [c for c in CASES + G.ONE_ROW_CASES if c.act == "prelu"]


@pytest.mark.parametrize("c", PRELU_CASES, ids=lambda c: c.name)
def test_a_lost_slope_moves_the_logits_past_100_bars(c):
    k = G.make_case(c)
    _, lg = G.ref64(k["sd"], k["feats"], k["b"], c, slope_as_one=True)
    live = slice(0, c.N - 1) if G.one_row_tail(c) else slice(None)
    move = float(np.max(np.abs(lg[live] - k["l64"][live]) / (1.0 + np.abs(k["l64"][live]))))
    bar = G.BAR[G.family(c)][0]
    print(f"slope as 1 on {c.name}: moves a logit by {move:.3e} = {move / bar:.0f} bars")
    assert move > 100 * bar, move


def test_swapped_slopes_move_the_logits():
    """Different slopes per layer: handing layer n the slope of layer n + 1 is seen."""
    for c in (BY_NAME["L3-prelu-fp32-B130"], BY_NAME["slopes-fast--0.5-3"], BY_NAME["L4-prelu-bf16-seg"]):
        k = G.make_case(c)
        sd = dict(k["sd"])
        L = len(c.h)
        for n in range(L):
            sd[f"mlp.{2 * n + 1}.weight"] = k["sd"][f"mlp.{2 * ((n + 1) % L) + 1}.weight"]
        _, lg = G.ref64(sd, k["feats"], k["b"], c)
        move = float(np.max(np.abs(lg - k["l64"]) / (1.0 + np.abs(k["l64"]))))
        assert move > 100 * G.BAR[G.family(c)][0], (c.name, move)


# ------------------------------------------------------------------ dispatch --
def test_case_lists_cover_the_new_dispatch():
    assert len({c.name for c in CASES + G.ONE_ROW_CASES}) == len(CASES) + len(G.ONE_ROW_CASES)
    covered = set().union(*(G.tail_kernels_of(c) for c in CASES))
    reach = G.reachable_tail_kernels()
    assert covered >= reach, sorted(reach - covered)
    new = {"din_layer<dice>", "din_layer<prelu>", "din_tail_head<dice>", "din_tail_head<prelu>",
           "din_mlp2_prelu<2>", "din_mlp2_prelu<4>", "din_mlp2_prelu<5>", "din_mlp2_prelu<8>"}
    assert new <= reach
    # a PReLU tail runs no statistics pass; a Dice tail one per layer past the first
    for c in CASES:
        assert G.tail_kernels_of(c).count("col_stats") == (len(c.h) - 1 if c.act == "dice" else 0)
    assert G.tail_kernels_of(G.case("", 130, 20, 2, (200, 80), "dice", "bf16")) == \
        ["din_w1_pack<5>", "din_mlp2<5>", "col_stats", "din_absmax", "din_head"][-4:]
    # depth x activation, both table types, one batch and segments with a 3-row tail
    assert {(len(c.h), c.act, c.dtype, c.S) for c in G.DEPTH_CASES} == \
        {(L, a, dt, Sg) for L, a in G.COMBOS for dt in ("fp32", "bf16") for Sg in (None, 64)}
    assert (2, "dice") not in G.COMBOS and len(G.COMBOS) == 7 and G.SEG_N % G.SEG_S == 3
    assert all((c.N, c.T, c.ni) in ((130, 20, 2), (G.SEG_N, 20, 2)) for c in G.DEPTH_CASES)
    # width edges, K no multiple of 4, last widths 2 and 1, B = 2
    assert {1, 63, 64, 65, 1024} <= {c.h[1] for c in G.WIDTH_CASES if len(c.h) == 3}
    assert any(h % 4 for c in CASES for h in c.h[:-1])
    assert {(200, 80, 2), (200, 80, 1)} <= {c.h for c in G.WIDTH_CASES} and 2 in {c.N for c in G.WIDTH_CASES}
    # the general front, the fast path's rungs from both sides, its persistent loop
    assert {(c.T > 64, c.h[0] > 256) for c in G.GENERAL_CASES} == {(True, False), (False, True)}
    assert {1, 32, 33, 64, 65, 80, 81, 128, 129} <= {c.h[1] for c in G.FAST_CASES}
    p = G.persist_case()
    assert p.N > 65536 and p.S == 256 and p.T == 1 and -(-p.N // 128) > 512
    # slopes
    used = {a for c in G.SLOPE_CASES for a in c.slopes}
    assert {0.25, 0.0, -0.5, 3.0} <= used and max(abs(a) for a in used) >= 16
    assert all(len(set(c.slopes)) == len(c.slopes) for c in CASES if c.act == "prelu" and len(c.h) > 1)
    # one hygiene case per new kernel
    hk = set().union(*(G.tail_kernels_of(BY_NAME[n]) for n in G.HYGIENE_CASES))
    assert {"din_layer<dice>", "din_layer<prelu>", "din_mlp2_prelu<5>", "din_tail_head<dice>",
            "din_tail_head<prelu>"} <= hk
    assert all(BY_NAME[n].S is not None for n in G.HYGIENE_CASES)


# --------------------------------------------------------------------- C ABI --
P = ctypes.c_void_p


def _call(**over):
    """nrk_din_forward_mlp with plausible arguments (fake non-null device
    addresses: every check fires before anything is launched or read)."""
    from nrk import _lib

    a = dict(table=P(4096), table_dtype=1, row_base=P(4096), n_user=2, n_item=2, n_ctx=2, user=P(4096),
             item=P(4096), hist=P(4096), ctx=P(4096), mask=P(4096), n=130, seg=130, T=20, prep=P(4096),
             att_b0=P(4096), att_w1=P(4096), att_b1=P(4096), w0=P(4096), b0=P(4096), L=3, widths=[64, 32, 8],
             mw=[4096] * 3, mb=[4096] * 3, act=1, slopes=P(4096), probs=P(4096), logits=None, ws=P(4096), ws_bytes=1)
    a.update(over)
    arr = lambda v, t: None if v is None else ctypes.cast((t * len(v))(*v), P)  # noqa: E731
    L = _lib.lib()
    rc = L.nrk_din_forward_mlp(a["table"], a["table_dtype"], a["row_base"], a["n_user"], a["n_item"], a["n_ctx"],
                               a["user"], a["item"], a["hist"], a["ctx"], a["mask"], a["n"], a["seg"], a["T"],
                               a["prep"], a["att_b0"], a["att_w1"], a["att_b1"], a["w0"], a["b0"], a["L"],
                               arr(a["widths"], ctypes.c_int), arr(a["mw"], ctypes.c_void_p),
                               arr(a["mb"], ctypes.c_void_p), a["act"], a["slopes"], a["probs"], a["logits"],
                               a["ws"], a["ws_bytes"], None)
    return rc, L.nrk_last_error().decode()


def test_new_entries_are_bound_and_the_abi_version_stays():
    from nrk import _lib

    L = _lib.lib()
    assert L.nrk_abi_version() == 3
    for name in ("nrk_din_forward_mlp", "nrk_din_mlp_workspace_bytes"):
        assert name in _lib.SIGNATURES and getattr(L, name, None) is not None
    w = (ctypes.c_int * 2)(200, 80)
    two = L.nrk_din_mlp_workspace_bytes(675653, 4096, 50, 5, 4, 16, 2, ctypes.cast(w, P), 0)
    assert two == L.nrk_din_segments_workspace_bytes(675653, 4096, 50, 5, 4, 16, 200, 80)  # the same layout
    # a PReLU tail reserves no partial or statistics buffer past z1's
    pre = L.nrk_din_mlp_workspace_bytes(675653, 4096, 50, 5, 4, 16, 2, ctypes.cast(w, P), 1)
    n_seg, nb_m = -(-675653 // 4096), -(-675653 // 64)
    r256 = lambda x: -(-x // 256) * 256  # noqa: E731
    assert two - pre == r256(nb_m * 80 * 16) + r256(n_seg * 80 * 8)
    w3 = (ctypes.c_int * 3)(200, 80, 2)
    assert L.nrk_din_mlp_workspace_bytes(675653, 4096, 50, 5, 4, 16, 3, ctypes.cast(w3, P), 0) > two
    for bad in ((0, w, 0), (5, w, 0), (2, None, 0), (2, w, 2)):
        assert L.nrk_din_mlp_workspace_bytes(130, 130, 20, 2, 2, 2, bad[0], ctypes.cast(bad[1], P) if bad[1] else None,
                                             bad[2]) == 0
    w0 = (ctypes.c_int * 2)(200, 1025)
    assert L.nrk_din_mlp_workspace_bytes(130, 130, 20, 2, 2, 2, 2, ctypes.cast(w0, P), 0) == 0


@pytest.mark.parametrize("over,rc,msg", [
    ({}, 1, "workspace too small"),
    ({"L": 0}, 3, "n_layers must be in [1, 4]"),
    ({"L": 5, "widths": [8] * 5, "mw": [4096] * 5, "mb": [4096] * 5}, 3, "n_layers must be in [1, 4]"),
    ({"widths": [64, 0, 8]}, 3, "hidden widths must be in [1, 1024]"),
    ({"widths": [64, 32, 1025]}, 3, "hidden widths must be in [1, 1024]"),
    ({"act": 2}, 1, "activation must be 0 (dice) or 1 (prelu)"),
    ({"act": -1}, 1, "activation must be 0 (dice) or 1 (prelu)"),
    ({"slopes": None}, 1, "slopes null under prelu"),
    ({"widths": None}, 1, "null pointer (widths, mlp_w or mlp_b)"),
    ({"mw": None}, 1, "null pointer (widths, mlp_w or mlp_b)"),
    ({"mb": None}, 1, "null pointer (widths, mlp_w or mlp_b)"),
    ({"mw": [4096, 0, 4096]}, 1, "null pointer in mlp_w / mlp_b"),
    ({"mb": [4096, 4096, 0]}, 1, "null pointer in mlp_w / mlp_b"),
    ({"probs": None}, 1, "null pointer"),
    ({"w0": None}, 1, "null pointer"),
    ({"ws": None}, 1, "null pointer"),
    ({"ctx": None}, 1, "ctx_idx null"),
    ({"table_dtype": 2}, 1, "table_dtype must be"),
    ({"n": 1, "seg": 1}, 1, "batch must be >= 2"),
    ({"n": 200, "seg": 100}, 1, "seg_len must be a multiple of 64"),
    ({"T": 129}, 1, "seq_len must be in [1, 128]"),
    ({"n_item": 3}, 3, "n_item must be 1, 2, 4 or 8"),
])
def test_forward_mlp_argument_checks(over, rc, msg):
    got, err = _call(**over)
    assert got == rc and msg in err and err.startswith("nrk_din_forward_mlp: "), (got, err)


def test_slopes_may_be_null_under_dice():
    got, err = _call(act=0, slopes=None)
    assert got == 1 and "workspace too small" in err  # every other check passed
