"""CPU side of the DIN forward tests: the float64 yardstick
(oracle.din_forward_f64) against the fp32 oracle over every case of
tests/test_gpu_din_shapes.py (imported, so the lists cannot drift), the bars
recorded there, and the cases' power to see the mistakes the kernels could
make.

Measured here (numpy fp32 oracle against float64, max over every sample of
every case of a family; logits as |d| / (1 + |ref|), probabilities as |d|):

    family              E32 logits   E32 probs   bar logits   bar probs
    fp32 tables         1.93e-6      5.14e-7     1e-5         5e-6
    bf16 tables         5.33e-6      1.58e-6     1e-5         1e-5
    segmented runs      2.18e-6      6.46e-7     1e-5         6e-6

Bars are 8 x E32 rounded up to one digit and capped at 1e-5, the bar of
tests/test_gpu_din.py, which these tests never loosen.  The logit bars all
sit at the cap (3 to 5 x E32).  The bf16 figures are set by the
``big-item-bf16`` case (one table entry 64 x the others'); without it they
are 2.96e-6 and 6.55e-7.

Mutations (oracle.din_forward_f64's switches), smallest logit movement over
their cases in the same units: drop_last 3.1e-1, ddof=0 8.5e-4,
neighbour_stats 1.8e-1, pad_row_zero 1.1e-1 (all > 10 bars = 1e-4);
w0_hi_only 3.8e-4, w1_hi_only 3.4e-4, p_lo_dropped 3.6e-5 (> 3 bars = 3e-5).
"""
import functools
import math

import numpy as np
import pytest

import test_gpu_din_shapes as S
from oracle import oracle

CASES = S.all_cases()
BY_NAME = {c.name: c for c in CASES}
PERSIST = S.persist_case().name


@functools.lru_cache(maxsize=None)
def _e32(c):
    """(logits, probs) error of the fp32 oracle against float64, every sample, batch by batch."""
    k = S.make_case(c)
    b = k["b"]
    seg = c.S or c.N
    pr, lg = np.empty(c.N, np.float32), np.empty(c.N, np.float32)
    for s in range(0, c.N, seg):
        sl = slice(s, min(c.N, s + seg))
        pr[sl], lg[sl], _ = oracle.din_forward(k["sd"], *(b[x][sl] for x in ("user", "item", "hist", "ctx", "mask")),
                                               k["feats"], round_bf16=c.dtype == "bf16")
    assert np.isfinite(lg).all()
    return S.errs(pr, lg, k)


def _ceil1(x):
    """x rounded up to one significant digit."""
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


def test_case_lists_cover_the_issue():
    assert len({c.name for c in CASES}) == len(CASES)
    # every kernel instantiation nrk_din_forward_segments can dispatch is run by a case
    covered = set().union(*(S.kernels_of(c) for c in CASES))
    assert covered == S.reachable_kernels(), sorted(S.reachable_kernels() - covered)
    for k in ("din_att_h2<bf16,1>", "din_att_h2<bf16,4>", "din_att_h<fp32,1,2>", "din_att_h<bf16,1,2>",
              "din_att_h<fp32,8,2>", "din_att_h<bf16,8,2>", "din_att_h<bf16,4,2>", "din_att_tm<1>"):
        assert k in covered
    # rung edges, each with both table types; each h1 rung with two or more h2 rungs
    rungs = [c for c in S.RUNG_CASES if c.name.startswith("rung-")]
    for dt in ("fp32", "bf16"):
        assert {28, 29, 56, 57, 64} <= {c.T for c in rungs if c.dtype == dt}
        assert {1, 16, 64, 65, 128, 129, 208, 209, 256, 257, 1024} <= {c.h1 for c in rungs if c.dtype == dt}
        assert {1, 32, 33, 64, 65, 80, 81, 128, 129, 1024} <= {c.h2 for c in rungs if c.dtype == dt}
        assert {130, 2} <= {c.N for c in rungs if c.dtype == dt}
    r1 = lambda h: S.rung(-(-h // 16), (4, 8, 13, 16)) if h <= 256 else 0  # noqa: E731
    r2 = lambda h: S.rung(-(-h // 16), (2, 4, 5, 8)) if h <= 128 else 0  # noqa: E731
    for a in {r1(c.h1) for c in rungs}:
        assert len({r2(c.h2) for c in rungs if r1(c.h1) == a}) >= 2, a
    # the loops' second trips, at the CU count of an MI355X
    c = BY_NAME[PERSIST]
    n_seg = -(-c.N // c.S)
    assert (c.dtype, c.S, c.T, c.ni, c.h1, c.h2) == ("bf16", 256, 17, 2, 65, 33) and c.N % 256 == 5
    assert 2 * (n_seg - 1) > S.CUS and S.wh2_pw(c.N, c.S, n_seg) >= 2 and c.N / 128 > 512
    assert all(S.wh2_pw(BY_NAME[n].N, BY_NAME[n].N, 1) >= 2 for n in ("pw2-fp32", "pw2-bf16"))
    assert BY_NAME["attout-fp32"].N == BY_NAME["attout-bf16"].N == 8192 + 300
    h = BY_NAME["head-stride"]
    assert (h.N, h.T, h.ni, h.S) == (131072 + 200, 1, 1, 4096)
    # segments x general path: both tails, every item-feature count, both table types
    seg = {(c.dtype, c.ni, c.T, c.h1, c.N, c.S) for c in S.SEG_CASES}
    assert all((dt, ni, T, h1, N, Sg) in seg for dt in ("fp32", "bf16") for ni in (1, 2, 4, 8)
               for T, h1 in ((70, 64), (20, 272)) for N, Sg in S.SEG_SHAPES)
    for dt in ("fp32", "bf16"):
        for T in (70, 20):
            assert {48, 144} <= {c.h2 for c in S.SEG_CASES if (c.dtype, c.T) == (dt, T) and c.h1 in (64, 272)}
    assert [N % Sg for N, Sg in S.SEG_SHAPES] == [3, 70]
    # one hygiene shape per attention kernel family
    att = [next(k for k in S.kernels_of(BY_NAME[n]) if k.startswith("din_att_")) for n in S.HYGIENE_CASES]
    assert att == ["din_att_tm<4>", "din_att_h2<fp32,2>", "din_att_h<fp32,4,1>", "din_att_h<fp32,2,2>",
                   "din_att_h2<bf16,4>"], att
    # vocabularies stay small, the embedding width is synth_model's 32
    assert max(S.V_USER + S.V_ITEM + S.V_CTX) <= 5000


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_logits_spread_and_fp32_oracle_meets_the_bar(c):
    k = S.make_case(c)
    lg = k["l64"]
    assert np.abs(lg).max() <= 12
    if c.special in S.CONSTANT_LOGITS:
        assert lg.std() < 1e-12  # an all-zero layer: every sample scores the same, by construction
    else:
        assert lg.std() >= 0.3
    if c.special == "zero_rows":  # the constant columns are there: z1 of a zero row is its bias
        assert not k["sd"]["mlp.0.weight"][[0, c.h1 - 1]].any()
    el, ep = _e32(c)
    bl, bp = S.BAR[S.family(c)]
    assert el <= bl and ep <= bp, (el, ep)


def test_bars_are_eight_times_the_fp32_noise():
    for fam in ("fp32", "bf16", "seg"):
        e = {c.name: _e32(c) for c in CASES if S.family(c) == fam}
        el, ep = max(v[0] for v in e.values()), max(v[1] for v in e.values())
        print(f"E32 {fam}: logits {el:.3e} at {max(e, key=lambda n: e[n][0])}, "
              f"probs {ep:.3e} at {max(e, key=lambda n: e[n][1])}")
        for got, rec, bar in zip((el, ep), S.E32[fam], S.BAR[fam]):
            # the recorded figure is this one up to the host BLAS's summation order, and
            # the bar is 8 x it rounded up to one digit, never past the suite's 1e-5
            assert 0.5 * rec <= got <= 1.5 * rec, (fam, got, rec)
            assert bar == pytest.approx(min(_ceil1(8 * rec), 1e-5), rel=1e-9), (fam, rec, bar)
            assert got < bar


MUTATIONS = [  # (switch, factor of the logit bar it must exceed, cases)
    ({"drop_last": True}, 10, ["tm1-ragged", "seg-fp32-ni2-T70-h64x144-S64", "segfast-fp32-ni2-S64"]),
    ({"ddof": 0}, 10, ["tm1-ragged", PERSIST, "head-stride", "seg-fp32-ni2-T70-h64x144-S64"]),
    ({"w0_hi_only": True}, 3, ["tm1-ragged", "rung-fp32-T56-h64x65-ni4-B130", PERSIST, "pw2-bf16"]),
    ({"w1_hi_only": True}, 3, ["tm1-ragged", "rung-fp32-T56-h64x65-ni4-B130", PERSIST, "pw2-bf16"]),
    ({"p_lo_dropped": True}, 3, [PERSIST, "tm4-wide-tables"]),
    ({"neighbour_stats": 0}, 10, ["segfast-bf16-ni4-S64", "seg-fp32-ni2-T70-h64x144-S64"]),
    ({"neighbour_stats": 1}, 10, ["segfast-bf16-ni4-S64", "seg-fp32-ni2-T70-h64x144-S64"]),
    ({"neighbour_stats": 2}, 10, ["segfast-bf16-ni4-S64", "seg-fp32-ni2-T70-h64x144-S64"]),
    ({"pad_row_zero": True}, 10, ["tm1-ragged", PERSIST, "segfast-bf16-ni4-S64"]),
]


@pytest.mark.parametrize("mut,factor,name", [(m, f, n) for m, f, names in MUTATIONS for n in names],
                         ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)) if isinstance(v, dict) else "")
def test_mutation_moves_a_logit_past_the_bar(mut, factor, name):
    c = BY_NAME[name]
    k = S.make_case(c)
    _, lg, _ = S.ref64(k["sd"], k["feats"], k["b"], c, **mut)
    move = float(np.max(np.abs(lg - k["l64"]) / (1.0 + np.abs(k["l64"]))))
    print(f"{mut} on {name}: moves a logit by {move:.3e} = {move / S.BAR[S.family(c)][0]:.1f} bars")
    assert move > factor * S.BAR[S.family(c)][0], move


@pytest.mark.parametrize("tag", ["b512", "b4096", "b37"])
def test_f64_yardstick_agrees_with_the_reference_outputs(golden, tag):
    """din_forward_f64 against what the reference itself computed (fp32
    torch) on the committed din_small batches, within the fp32-table bar."""
    g = golden("din_small")
    sd = {k[4:]: g[k] for k in g.files if k.startswith("sd::")}
    feats = [list(map(str, g[k])) for k in ("user_feats", "item_feats", "ctx_feats")]
    b = {k: g[f"{tag}_{k}"].astype(np.int64 if k != "mask" else np.float32)
         for k in ("user", "item", "hist", "ctx", "mask")}
    p64, l64, _ = oracle.din_forward_f64(sd, b["user"], b["item"], b["hist"], b["ctx"], b["mask"], feats)
    bl, bp = S.BAR["fp32"]
    np.testing.assert_allclose(g[f"{tag}_logits"], l64, atol=bl, rtol=bl)
    np.testing.assert_allclose(g[f"{tag}_probs"], p64, atol=bp, rtol=0)
    # the batch_size form is the same function applied per batch
    if tag == "b512":
        p2, l2, _ = oracle.din_forward_f64(sd, b["user"], b["item"], b["hist"], b["ctx"], b["mask"], feats,
                                           batch_size=128)
        for s in range(0, 512, 128):
            one = oracle.din_forward_f64(sd, *(b[x][s:s + 128] for x in ("user", "item", "hist", "ctx", "mask")),
                                         feats)
            assert np.array_equal(l2[s:s + 128], one[1]) and np.array_equal(p2[s:s + 128], one[0])
