"""YouTubeDNN tower forward (csrc/tower.hip) at the shapes where its tuned
paths change: the persistent multi-user wave loop with its deferred row
store, every gather round and phase boundary, h0 either side of 64 and off a
multiple of 4, the layers kernel's width / depth limits, dead ReLU outputs
and the item kernel's grid-stride loop.

Checker: the float64 statement of the operation (oracle.tower_user_layers_f64
/ tower_item_f64).  The bars below are 4 x the measured error of the fp32 numpy
oracle against that reference over every case of this file; the CPU test
tests/test_tower_host.py imports the case lists from here, recomputes both
figures and checks the constants, the conditioning of every case and that
each case would see a one-slot error.
"""
import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

# max |fp32 oracle - fp64 reference| over every user-tower case below (all
# rows; tests/test_tower_host.py recomputes it).  The kernels and the numpy
# oracle are both fp32 evaluations of one expression, differing in summation
# order and fma contraction only: the bar is 4 x that noise, rounded up to one
# digit.  4 x 6.03e-7 = 2.41e-6 -> 3e-6 (the bar before this file: 1e-5).
E32_USER = 6.03e-7
BAR_USER = 3e-6
# the same for the item tower (two divisions and a D-term sum of squares):
# 4 x 9.33e-8 = 3.73e-7 -> 4e-7 (before: 1e-6)
E32_ITEM = 9.33e-8
BAR_ITEM = 4e-7

NOMINAL_CUS = 256  # the CPU test sizes the loop cases for this many CUs
N_GRID = 1023      # not a multiple of the 4 users a block starts with
U_ROWS, I_ROWS = 500, 3000


def loop_n(cus):
    """Every wave handles at least 3 users whatever the occupancy API answers:
    32 waves per CU is the hardware ceiling for 256-thread blocks."""
    return 3 * 32 * int(cus) + 7


class Case(NamedTuple):
    name: str
    D: int
    T: int
    widths: Tuple[int, ...]      # hidden widths, the last one == D
    n: Optional[int] = N_GRID    # None: loop_n(CUs)
    lens: str = "mod"            # mod | perm | zero_ends | full_ends
    special: str = ""            # "" | dead_all | dead_l0 | dead_some


def _grid_cases():
    """(D, T, h0): every D with every T, every D with every h0, and T = 64
    with h0 in {3, 65, 127, 128} at each D."""
    out = []
    rest_t, rest_h = [1, 2, 31, 33], [1, 2, 5, 63, 64, 100]
    for k, D in enumerate((16, 32, 64)):
        trip = [(64, h0) for h0 in (3, 65, 127, 128)]
        trip += [(rest_t[(i + k) % 4], h0) for i, h0 in enumerate(rest_h)]
        out += [Case(f"grid-D{D}-T{T}-h{h0}", D, T, (h0, D)) for T, h0 in trip]
    return out


GRID_CASES = _grid_cases()

# the multi-user loop: two-layer shapes, each with the batch's first and last
# user forced to len 0 and to len T
LOOP_CASES = [Case(f"loop-D{D}-T{T}-h{h0}-{v}", D, T, (h0, D), None, v)
              for D, h0, T in ((32, 64, 30), (16, 65, 64)) for v in ("zero_ends", "full_ends")]
# the layers kernel over the same n (its 2048-block grid loops too)
LOOP_DEEP_CASE = Case("loop-D32-T30-w96-48-32", 32, 30, (96, 48, 32), None, "zero_ends")

# the layers kernel's limits: one layer, widths 1 / 65 / 255 / 256, 8 layers
LAYER_CASES = [Case(f"layers-D{D}-" + "-".join(map(str, w)), D, 64, tuple(w) + (D,), N_GRID, "perm")
               for D in (16, 64)
               for w in ((), (1,), (65,), (255,), (256, 256), (64, 48, 256, 33, 128, 17, 64))]

DEAD_CASES = [Case(f"{s}-D{D}-T{T}-h{h0}", D, T, (h0, D), N_GRID, "mod", s)
              for s in ("dead_all", "dead_l0", "dead_some") for D, h0, T in ((32, 64, 30), (16, 65, 64))]

USER_CASES = GRID_CASES + LOOP_CASES + [LOOP_DEEP_CASE] + LAYER_CASES + DEAD_CASES

# (D, n, table rows, zero row); the last n runs past the item kernel's
# 4096 x 256-thread grid, ids drawn with repeats from a small table
ITEM_CASES = ([(D, n, I_ROWS, None) for D in (16, 32, 64) for n in (1, 255, 257)]
              + [(16, 4096 * 256 + 1001, 5000, None)]
              + [(D, 257, 300, 7) for D in (16, 32, 64)])

# Conditioning.  The output is z+ / |z+| of the last layer, so a row whose live
# part |z+| is tiny (at any layer) turns the ~1e-8 rounding of a pre-activation
# into an error of any size that says nothing about the code under test, and a
# row with a dead hidden layer or a single live output does not depend on its
# history at all.  make_case therefore redraws the ids of a row until, in the
# fp64 reference,
#  * every hidden layer's live norm is at least LIVE_FRAC of the case's median;
#  * the last layer is either dead by a clear margin (every pre-activation
#    <= -DEAD_MARGIN) or live with the same floor;
#  * if it has a history and is not dead, dropping slot len - 1 and dividing by
#    len + 1 each move its output by at least SENS_FLOOR = 10 x 1e-5, ten times
#    the weakest bar this file may record.
# Nothing here looks at an fp32 result.
DEAD_MARGIN = 1e-4
LIVE_FRAC = 0.25
SENS_FLOOR = 1e-4
N_TASTES = 50  # item clusters; a user's history comes from one of them


def _live_norm(z):
    zp = np.maximum(z, 0.0)
    return np.sqrt((zp * zp).sum(1))


def _floors(pres):
    out = []
    for z in pres:
        live = _live_norm(z)
        out.append(LIVE_FRAC * np.median(live[live > 0]) if (live > 0).any() else 0.0)
    return out


def _ill(c, f64, uid, hist, hlen, layers, floors):
    ref, pres = f64(uid, hist, hlen, layers)
    first = 1 if c.special == "dead_l0" else 0  # that case's layer 0 is dead on purpose
    bad = np.zeros(len(uid), bool)
    for z, fl in zip(pres[first:-1], floors[first:-1]):
        bad |= _live_norm(z) < fl
    dead = pres[-1].max(1) <= -DEAD_MARGIN
    bad |= ~(dead | (_live_norm(pres[-1]) >= floors[-1]))
    if c.special != "dead_l0":
        touched = (hlen >= 1) & ~dead
        for kw in (dict(drop_last=True), dict(len_plus=1)):
            moved = np.abs(f64(uid, hist, hlen, layers, **kw)[0] - ref).max(1)
            bad |= touched & (moved < SENS_FLOOR)
    return bad


@functools.lru_cache(maxsize=None)
def make_case(c, cus=NOMINAL_CUS):
    """Inputs of a case as numpy arrays (fp32 tables / weights, int64 ids).
    Tables are about 0.01 N(0, 1): an item row is its cluster's centre plus
    noise, 0.01 N(0, 1) each, and a user's history comes from one cluster, so
    the mean does not fade with the length as it would for unrelated items.
    Slots at or past hist_len hold random in-range non-zero ids."""
    n = c.n if c.n is not None else loop_n(cus)
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    D, T = c.D, c.T
    ue = (rng.standard_normal((U_ROWS, D)) * 0.01).astype(np.float32)
    centre = rng.standard_normal((N_TASTES, D)) * 0.01
    ie = (centre[np.arange(I_ROWS) % N_TASTES] + rng.standard_normal((I_ROWS, D)) * 0.01).astype(np.float32)
    layers, fan = [], 2 * D
    for w in c.widths:
        layers.append([(rng.standard_normal((w, fan)) * 0.2).astype(np.float32),
                       (rng.standard_normal(w) * 0.01).astype(np.float32)])
        fan = w
    if c.lens in ("mod", "perm"):
        hlen = np.arange(n) % (T + 1)
        if c.lens == "perm":
            hlen = rng.permutation(hlen)
    else:  # about 30 % empty histories, so runs of len == 0 users meet in one wave
        hlen = np.where(rng.random(n) < 0.3, 0, rng.integers(1, T + 1, n))
        hlen[[0, -1]] = 0 if c.lens == "zero_ends" else T

    def draw(m):  # ids 50 .. I_ROWS - 1 of one cluster per user: in range, never 0
        taste = rng.integers(0, N_TASTES, (m, 1))
        return rng.integers(0, U_ROWS, m), taste + N_TASTES * rng.integers(1, I_ROWS // N_TASTES, (m, T))

    uid, hist = draw(n)
    f64 = functools.partial(oracle.tower_user_f64_parts, ue, ie)
    if c.special == "dead_all":  # y >= 0, so every last pre-activation <= b < 0
        layers[-1] = [-np.abs(layers[-1][0]), -np.abs(layers[-1][1]) - np.float32(1e-3)]
    elif c.special == "dead_l0":  # layer 0 outputs 0 for every user: out = normalise(relu(b1))
        layers[0] = [np.zeros_like(layers[0][0]), -np.abs(layers[0][1]) - np.float32(1e-3)]
    floors = _floors(f64(uid, hist, hlen, layers)[1])
    if c.special == "dead_some":
        # a slightly negative b1 that kills a good part of the users; the live
        # floor stays the one of the unshifted layer, so survivors are well alive
        layers[-1][1] = layers[-1][1] - np.float32(np.quantile(f64(uid, hist, hlen, layers)[1][-1].max(1), 0.25))
    layers = tuple((w, b) for w, b in layers)
    bad = np.arange(n)
    for _ in range(400):
        bad = bad[_ill(c, f64, uid[bad], hist[bad], hlen[bad], layers, floors)]
        if bad.size == 0:
            break
        uid[bad], hist[bad] = draw(bad.size)
    else:
        raise AssertionError(f"{c.name}: could not condition every row ({bad.size} left)")
    for a in (ue, ie, uid, hist, hlen) + tuple(t for wb in layers for t in wb):
        a.setflags(write=False)
    return dict(ue=ue, ie=ie, uid=uid, hist=hist, hlen=hlen, layers=layers, n=n)


@functools.lru_cache(maxsize=None)
def ref64(c, cus=NOMINAL_CUS):
    k = make_case(c, cus)
    out = oracle.tower_user_layers_f64(k["ue"], k["ie"], k["uid"], k["hist"], k["hlen"], k["layers"])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_item_case(D, n, rows, zero_row):
    rng = np.random.default_rng(zlib.crc32(f"item-{D}-{n}-{rows}-{zero_row}".encode()))
    table = (rng.standard_normal((rows, D)) * 0.01).astype(np.float32)
    ids = rng.integers(0, rows, n)
    if zero_row is not None:
        table[zero_row] = 0
        ids[[3, n // 2]] = zero_row
    ref = oracle.tower_item_f64(table, ids)
    for a in (table, ids, ref):
        a.setflags(write=False)
    return table, ids, ref


def max_err(got, ref):
    """max |got - ref| over every element; NaN must sit at the same places."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs from the reference"
    d = np.abs(got - ref)
    return float(np.nanmax(d)) if d.size and not np.isnan(d).all() else 0.0


# ------------------------------------------------------------------ GPU side --
@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # a copy: the cases' arrays are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


@functools.lru_cache(maxsize=4)
def _dev_case(c, cus):
    k = make_case(c, cus)
    return dict(tabs=(_dev(k["ue"]), _dev(k["ie"])),
                idx=(_dev(k["uid"], torch.int32), _dev(k["hist"], torch.int32), _dev(k["hlen"], torch.int32)),
                layers=[(_dev(w), _dev(b)) for w, b in k["layers"]])


def _two(ops, d, sl=slice(None), out=None):
    (w0, b0), (w1, b1) = d["layers"]
    return ops.tt_user_fwd(*d["tabs"], *(t[sl].contiguous() for t in d["idx"]), w0, b0, w1, b1, out=out)


def _deep(ops, d):
    return ops.tt_user_fwd_layers(*d["tabs"], *d["idx"], d["layers"])


def _check_rows(out, ref, name):
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), name
    err = max_err(got, ref)
    print(f"{name}: max |gpu - f64| = {err:.3e} (bar {BAR_USER:.1e})")
    assert err <= BAR_USER, (name, err)
    nrm = np.sqrt((got.astype(np.float64) ** 2).sum(1))
    zero = ~got.any(1)
    assert (zero | (np.abs(nrm - 1.0) <= BAR_USER)).all(), name
    return got, zero


@pytest.mark.parametrize("c", GRID_CASES, ids=lambda c: c.name)
def test_two_layer_shape_grid(ops, cus, c):
    d = _dev_case(c, cus)
    _check_rows(_two(ops, d), ref64(c, cus), c.name)


@pytest.mark.parametrize("c", LOOP_CASES, ids=lambda c: c.name)
def test_wave_loop_vs_f64(ops, cus, c):
    """n users so that each wave loops at least 3 times: the prefetch hand-over
    and both deferred stores (behind the next user's gathers / len == 0)."""
    d = _dev_case(c, cus)
    n = make_case(c, cus)["n"]
    assert n == loop_n(cus) and n >= 3 * 32 * cus
    big = _two(ops, d)
    _check_rows(big, ref64(c, cus), c.name)
    # determinism
    assert torch.equal(big, _two(ops, d))
    # batch invariance: the same users as a batch of their own (one per wave)
    for sl in (slice(0, 256), slice(n // 2, n // 2 + 256), slice(n - 255, n)):
        assert torch.equal(big[sl], _two(ops, d, sl)), (c.name, sl)


@pytest.mark.parametrize("c", LOOP_CASES[::2], ids=lambda c: c.name)
def test_wave_loop_guard_rows(ops, cus, c):
    """out= a slice of a NaN buffer: every row is written, nothing beside it
    (at D = 16 lanes >= h1 of the deferred store must stay silent)."""
    d = _dev_case(c, cus)
    n = make_case(c, cus)["n"]
    buf = torch.full((n + 2, c.D), float("nan"), device="cuda")
    out = _two(ops, d, out=buf[1:-1])
    assert out.data_ptr() == buf[1:-1].data_ptr()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
    assert bool(torch.isfinite(buf[1:-1]).all())
    assert torch.equal(buf[1:-1], _two(ops, d))


def test_wave_loop_layers_same_bits(ops, cus):
    """[64, 32] through the layers kernel == the two-layer kernel, bit for
    bit, with both grids looping."""
    c = LOOP_CASES[0]
    assert c.widths == (64, 32)
    d = _dev_case(c, cus)
    deep = _deep(ops, d)
    _check_rows(deep, ref64(c, cus), c.name + "/layers")
    assert torch.equal(deep, _two(ops, d))


def test_wave_loop_layers_deep(ops, cus):
    c = LOOP_DEEP_CASE
    d = _dev_case(c, cus)
    deep = _deep(ops, d)
    _check_rows(deep, ref64(c, cus), c.name)
    assert torch.equal(deep, _deep(ops, d))


@pytest.mark.parametrize("c", LAYER_CASES, ids=lambda c: c.name)
def test_layers_limits(ops, cus, c):
    _check_rows(_deep(ops, _dev_case(c, cus)), ref64(c, cus), c.name)


@pytest.mark.parametrize("c", GRID_CASES, ids=lambda c: c.name)
def test_layers_kernel_matches_two_layer_bits(ops, cus, c):
    """tower.hip: each output of the layers kernel is "the same q-ascending
    chain as the two-layer kernel", at every h0 path of the latter (one or
    two chains per lane, 4-wide loop and scalar tail)."""
    d = _dev_case(c, cus)
    assert torch.equal(_deep(ops, d), _two(ops, d))


@pytest.mark.parametrize("c", DEAD_CASES, ids=lambda c: c.name)
def test_dead_outputs(ops, cus, c):
    d = _dev_case(c, cus)
    ref = ref64(c, cus)
    for run in (_two, _deep):
        got, zero = _check_rows(run(ops, d), ref, c.name)
        assert np.array_equal(zero, ~ref.any(1))  # dead rows are exactly zero, and only those
        if c.special == "dead_all":
            assert zero.all()
        elif c.special == "dead_l0":
            assert not zero.any() and (got == got[0]).all()
        else:
            assert 0.1 < zero.mean() < 0.9  # both kinds of row, in numbers


@pytest.mark.parametrize("D,n,rows,zero_row", ITEM_CASES)
def test_item_tower(ops, D, n, rows, zero_row):
    table, ids, ref = make_item_case(D, n, rows, zero_row)
    got = ops.tt_item_fwd(_dev(table), _dev(ids, torch.int32)).cpu().numpy()
    err = max_err(got, ref)  # also: NaN exactly where the reference has it
    print(f"item D={D} n={n}: max |gpu - f64| = {err:.3e} (bar {BAR_ITEM:.1e})")
    assert err <= BAR_ITEM
    if zero_row is not None:
        assert np.isnan(got[ids == zero_row]).all() and (ids == zero_row).sum() >= 2
        assert np.isfinite(got[ids != zero_row]).all()
    else:
        assert np.isfinite(got).all()
