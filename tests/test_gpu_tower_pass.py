"""The user tower's multi-user wave pass (csrc/tower.hip, tt_user_kernel_pass):
G = nrk_tt_user_pass_users(D, h0) users share one pass of the two layers.

Checker for bits: ops.tt_user_fwd_layers with the same two layers (the layers
kernel is a different kernel, one user per wave, and
tests/test_gpu_tower_shapes.py already holds it to the one-user two-layer
kernel bit for bit).  Checker for value: oracle.tower_user_layers_f64 within
BAR_USER of tests/test_gpu_tower_shapes.py, on the rows of one of that file's
own cases (SAMPLE_CASE, made and conditioned by its make_case) spread through
the wave-loop batch (tests/test_tower_pass_host.py checks the cases on the CPU).
There is no 4 GiB item-table case: the 32-bit gather offsets it was meant for
were measured and left out (profiles/r12_tower.txt), the gathers keep 64-bit
addresses.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import test_gpu_tower_shapes as S

pytestmark = pytest.mark.gpu

G_NOMINAL = 4     # what the CPU test sizes the cases for; the GPU tests ask the library
T_MAIN = 30
SENTINEL = -7.0   # no output row holds it: rows are unit vectors or zero
N_SAMPLE = 256    # rows of the wave-loop case held to the fp64 reference
# those rows: a case of tests/test_gpu_tower_shapes.py, whose tables and layers the wave-loop batch uses
SAMPLE_CASE = S.Case("pass-loop-sample", 32, T_MAIN, (64, 32), N_SAMPLE, "zero_ends")
BOUNDARY = ([(32, h0) for h0 in (1, 3, 60, 63, 64, 65, 128)]
            + [(D, h0) for D in (16, 64) for h0 in (64, 65)])
POS_LENS = (0, 1, T_MAIN, 9, 17)  # 9 and 17 straddle a gather round at D = 32


def loop_n(g, cus):
    """Every wave runs at least three passes whatever the occupancy is: 32
    waves per CU is the hardware ceiling for 256-thread blocks."""
    return 3 * g * 32 * int(cus) + 7


@functools.lru_cache(maxsize=None)
def make_inputs(name, n, D=32, h0=64, T=T_MAIN, lens="mixed"):
    """Inputs drawn as tests/test_gpu_tower_shapes.make_case draws them (tables
    about 0.01 N(0, 1), a user's history from one item cluster, slots at or past
    hist_len random in-range non-zero ids).  lens: mixed (about 30 % empty,
    the rest 1 .. T) | mod (u % (T + 1)).  These rows are compared for bits
    only, so they are not conditioned."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ue = (rng.standard_normal((S.U_ROWS, D)) * 0.01).astype(np.float32)
    centre = rng.standard_normal((S.N_TASTES, D)) * 0.01
    ie = (centre[np.arange(S.I_ROWS) % S.N_TASTES] + rng.standard_normal((S.I_ROWS, D)) * 0.01).astype(np.float32)
    layers, fan = [], 2 * D
    for w in (h0, D):
        layers.append((((rng.standard_normal((w, fan)) * 0.2).astype(np.float32)),
                       (rng.standard_normal(w) * 0.01).astype(np.float32)))
        fan = w
    layers = tuple(layers)
    if lens == "mod":
        hlen = np.arange(n) % (T + 1)
    else:
        hlen = _mixed_lens(rng, n, T)
    uid, hist = _draw(rng, n, T)
    return dict(ue=ue, ie=ie, uid=uid, hist=hist, hlen=hlen, layers=layers, n=n, D=D, T=T, h0=h0)


def _mixed_lens(rng, n, T):
    return np.where(rng.random(n) < 0.3, 0, rng.integers(1, T + 1, n))


def _draw(rng, m, T):
    """ids 50 .. I_ROWS - 1 of one cluster per user: in range, never 0"""
    taste = rng.integers(0, S.N_TASTES, (m, 1))
    return rng.integers(0, S.U_ROWS, m), taste + S.N_TASTES * rng.integers(1, S.I_ROWS // S.N_TASTES, (m, T))


def tail_inputs(g=G_NOMINAL):
    return make_inputs("pass-tail", 2 * g + 1, lens="mod")


def position_inputs(g=G_NOMINAL):
    return make_inputs("pass-position", 4 * g)


POS_PASSES = (0, 1, 3)  # of the case's four passes: the first, one in the middle, the last


def position_lens(k, g, pas, pos, length):
    """Position pos of pass pas gets `length`; the others keep theirs."""
    hlen = k["hlen"].copy()
    hlen[pas * g + pos] = length
    return hlen


def boundary_inputs(D, h0):
    return make_inputs(f"pass-boundary-D{D}-h{h0}", S.N_GRID, D=D, h0=h0, T=33 if D == 16 else T_MAIN, lens="mod")


@functools.lru_cache(maxsize=None)
def loop_inputs(g=G_NOMINAL, cus=S.NOMINAL_CUS):
    """n users over SAMPLE_CASE's tables and layers; the case's own rows, in
    order, sit at "sample": seeded positions that are never the first or the
    last user.  The other rows are drawn as in make_inputs."""
    k0 = S.make_case(SAMPLE_CASE)
    n, T = loop_n(g, cus), SAMPLE_CASE.T
    rng = np.random.default_rng(zlib.crc32(b"pass-loop"))
    hlen = _mixed_lens(rng, n, T)
    uid, hist = _draw(rng, n, T)
    sample = np.sort(rng.choice(np.arange(1, n - 1), N_SAMPLE, replace=False))
    uid[sample], hist[sample], hlen[sample] = k0["uid"], k0["hist"], k0["hlen"]
    return dict(ue=k0["ue"], ie=k0["ie"], uid=uid, hist=hist, hlen=hlen, layers=k0["layers"], n=n, D=SAMPLE_CASE.D,
                T=T, h0=SAMPLE_CASE.widths[0], sample=sample)


def loop_lens(k, ends):
    hlen = k["hlen"].copy()
    hlen[[0, -1]] = ends
    return hlen


def dead_inputs(g=G_NOMINAL):
    """n = 8 G + 3 users, W1 <= 0 and b1 >= 1: a row lives while |W1| y0 stays
    under b1, as it does for table rows of about 0.01.  dead: user 1 + p G of
    every whole pass p points at user-table row 0 = 100, which drives y0 into
    the hundreds and every last pre-activation far below zero: its output row
    is exactly zero.  nan_user: one user whose user-table row holds a NaN."""
    k = dict(make_inputs("pass-dead", 8 * g + 3))
    n = k["n"]
    (w0, b0), (w1, b1) = k["layers"]
    w1, b1 = -np.abs(w1), (1.0 + np.abs(b1)).astype(np.float32)
    ue, uid = k["ue"].copy(), k["uid"].copy()
    dead = 1 + g * np.arange(n // g)
    nan_user = 2 * g + 2
    ue[0] = 100.0
    ue[1, 5] = np.nan
    uid[uid < 2] = 2
    uid[dead] = 0
    uid[nan_user] = 1
    k.update(ue=ue, uid=uid, layers=((w0, b0), (w1, b1)), dead=dead, nan_user=nan_user)
    return k


# ------------------------------------------------------------------ GPU side --
@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


class _Run:
    """Device copies of one input set; two(hlen) / deep(hlen) run the two kernels."""

    def __init__(self, ops, k):
        self.ops, self.k = ops, k
        self.tabs = (_dev(k["ue"]), _dev(k["ie"]))
        self.uid, self.hist = _dev(k["uid"], torch.int32), _dev(k["hist"], torch.int32)
        self.layers = [(_dev(w), _dev(b)) for w, b in k["layers"]]
        self.hlen = _dev(k["hlen"], torch.int32)

    def _idx(self, hlen, sl):
        hl = self.hlen if hlen is None else _dev(hlen, torch.int32)
        return tuple(t[sl].contiguous() for t in (self.uid, self.hist, hl))

    def two(self, hlen=None, sl=slice(None), out=None):
        (w0, b0), (w1, b1) = self.layers
        return self.ops.tt_user_fwd(*self.tabs, *self._idx(hlen, sl), w0, b0, w1, b1, out=out)

    def deep(self, hlen=None, sl=slice(None)):
        return self.ops.tt_user_fwd_layers(*self.tabs, *self._idx(hlen, sl), self.layers)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_tail_passes(ops):
    g = ops.tt_user_pass_users(32, 64)
    assert g >= 1
    r = _Run(ops, tail_inputs(g))
    ref = r.deep()
    for n in range(1, 2 * g + 2):
        buf = torch.full((n + 8, 32), SENTINEL, device="cuda")
        out = r.two(sl=slice(0, n), out=buf[:n])
        assert out.data_ptr() == buf.data_ptr()
        assert _same_bits(buf[:n], ref[:n]), n
        assert bool((buf[n:] == SENTINEL).all()), n


def test_position_in_a_pass(ops):
    g = ops.tt_user_pass_users(32, 64)
    k = position_inputs(g)
    r = _Run(ops, k)
    base = r.two()
    assert _same_bits(base, r.deep())
    for pas, pos, length in ((a, b, c) for a in POS_PASSES for b in range(g) for c in POS_LENS):
        hlen = position_lens(k, g, pas, pos, length)
        got = r.two(hlen)
        assert _same_bits(got, r.deep(hlen)), (pas, pos, length)
        others = torch.arange(k["n"], device="cuda") != pas * g + pos
        assert _same_bits(got[others], base[others]), (pas, pos, length)  # the neighbours never see it


@pytest.mark.parametrize("D,h0", BOUNDARY)
def test_dispatch_boundary(ops, D, h0):
    g = ops.tt_user_pass_users(D, h0)
    assert (g == 0) == (h0 > 64), (D, h0, g)
    k = boundary_inputs(D, h0)
    assert len(np.unique(k["uid"])) < k["n"] and not np.array_equal(k["uid"], np.arange(k["n"]))
    r = _Run(ops, k)
    got = r.two()
    assert _same_bits(got, r.deep()), (D, h0)
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("ends", [0, T_MAIN])
def test_wave_loop(ops, ends):
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    g = ops.tt_user_pass_users(32, 64)
    k = loop_inputs(g, cus)
    assert k["n"] == 3 * g * 32 * cus + 7
    r = _wave_loop_run(ops, g, cus)
    hlen = loop_lens(k, ends)
    got = r.two(hlen)
    assert _same_bits(got, r.deep(hlen)), ends
    sample = k["sample"]  # SAMPLE_CASE's rows; never the first or the last user, so the same for both ends
    err = S.max_err(got[torch.from_numpy(sample).cuda()].cpu().numpy(), S.ref64(SAMPLE_CASE))
    print(f"wave loop, ends {ends}: max |gpu - f64| over {len(sample)} rows = {err:.3e} (bar {S.BAR_USER:.1e})")
    assert err <= S.BAR_USER, err


@functools.lru_cache(maxsize=1)
def _wave_loop_run(ops, g, cus):
    return _Run(ops, loop_inputs(g, cus))


def test_dead_and_non_finite_rows(ops):
    g = ops.tt_user_pass_users(32, 64)
    k = dead_inputs(g)
    r = _Run(ops, k)
    got, ref = r.two(), r.deep()
    assert _same_bits(got, ref)
    got = got.cpu().numpy()
    assert not got[k["dead"]].any()  # exactly zero, every one of them
    assert np.array_equal(np.isnan(got), np.isnan(ref.cpu().numpy()))
    live = np.ones(k["n"], bool)
    live[k["dead"]] = False
    live[k["nan_user"]] = False
    assert np.isfinite(got[live]).all() and got[live].any(1).all()  # the NaN stays with its user
