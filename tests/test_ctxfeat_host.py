"""Context-feature checks that need no GPU (csrc/ctxfeat.hip).

1. The kernel's pairwise-sum plan (pw_plan) and leaf arithmetic
   (coop_word_diff_n: 8 strided accumulators, the tree
   ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the tail in order, the shape combine)
   restated in plain numpy float64 operations, against
   np.linalg.norm(a.astype(f32) - h[None], axis=1) for every content width in
   1..256, bit for bit.  This pins what the GPU tests rest on: numpy on this
   host sums the way the kernel copies.  If a GPU word_diff test fails and
   this one passes, the kernel is wrong; if this one fails, numpy moved.
   For widths up to 256 only shapes 0, 1 and 3 are reachable: shapes 2 and 4
   of pw_plan need a first half above 128 and cannot happen.
   tie_history_row builds the rows on which that order survives the float32
   the kernel returns (the GPU tests add them to every world).
2. Every refusal of nrk_ctx_features' host wrapper, each before any launch
   (the library loads and answers on a host without a GPU).
"""
import ctypes

import numpy as np
import pytest

from nrk import _lib
from nrk.features import CtxSpecC, CtxTablesC


def pw_plan(n):
    """pw_plan of csrc/ctxfeat.hip: (shape, [(begin, length) per leaf])."""
    if n <= 128:
        return 0, [(0, n)]
    n2 = n // 2 - (n // 2) % 8
    r1 = n - n2
    m0 = n2 // 2 - (n2 // 2) % 8
    m1 = r1 // 2 - (r1 // 2) % 8
    s0, s1 = n2 > 128, r1 > 128
    if not s0 and not s1:
        return 1, [(0, n2), (n2, r1)]
    if s0 and not s1:
        return 2, [(0, m0), (m0, n2 - m0), (n2, r1)]
    if not s0 and s1:
        return 3, [(0, n2), (n2, m1), (n2 + m1, r1 - m1)]
    return 4, [(0, m0), (m0, n2 - m0), (n2, m1), (n2 + m1, r1 - m1)]


def pw_leaf(sq, b, n):
    """One leaf over the float64 squares sq[:, b:b+n] (every row at once)."""
    if n < 8:
        acc = sq[:, b].copy()
        for e in range(1, n):
            acc = acc + sq[:, b + e]
        return acc
    r = [sq[:, b + j].copy() for j in range(8)]
    full = n - n % 8
    for i in range(8, full, 8):
        for j in range(8):
            r[j] = r[j] + sq[:, b + i + j]
    acc = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for e in range(full, n):
        acc = acc + sq[:, b + e]
    return acc


def pw_word_diff(a, h):
    """The kernel's word_diff of rows a [R, dc] (float64 table rows) against
    the history row h [dc] (float64), before the final float32 rounding."""
    return np.sqrt(pw_sumsq(a, h))


def seq_sumsq(a, h):
    """the same squares summed left to right (NOT what numpy or the kernel do)."""
    d = a.astype(np.float32).astype(np.float64) - h[None]
    s = np.zeros(len(a))
    for e in range(a.shape[1]):
        s = s + d[:, e] * d[:, e]
    return s


def tie_history_row(dc, p, side, rng):
    """A history content row h [dc] whose distance from the item row
    e0 = (1, 0, ..., 0) the final float32 rounding does not hide.

    word_diff leaves the kernel as a float32, which swallows the last ~29 bits
    of the float64 sum: on ordinary rows no summation order is observable.
    Here the sum of squares sits |side| * (1 or 2) ulps above (side = +1) or
    below (-1) T = t^2, t the midpoint of two adjacent float32 values in
    (1.45, 1.95): there one ulp of the sum moves the double sqrt off t and
    decides the float32.  One square (element p) is ~T; every other is a
    fraction of an ulp of T, absorbed or counted depending on where the order
    of summation meets it.  Returns (h, float32 word_diff)."""
    lo = np.float32(rng.uniform(1.45, 1.95))
    t = (float(lo) + float(np.nextafter(lo, np.float32(2)))) / 2
    T, ulp = t * t, 2.0 ** -51
    assert 2 < T < 4 and np.sqrt(T) == t
    a = np.zeros((1, dc))
    a[0, 0] = 1.0
    small = np.sqrt(rng.uniform(0.3, 0.49, dc) * ulp) * rng.choice([-1.0, 1.0], dc)
    h = -small
    h[0] = 1.0 - small[0]
    j0 = -int((small * small).sum() / ulp / t)  # B^2 moves by t ulps of T per ulp of B
    for j in sorted(range(-40, 41), key=abs):
        B = t + (j0 + j) * 2.0 ** -52
        h[p] = 1.0 - B if p == 0 else -B
        m = (pw_sumsq(a, h)[0] - T) / ulp
        if side * m in (1.0, 2.0):
            wd = np.float32(np.sqrt(pw_sumsq(a, h)[0]))
            assert wd == (np.nextafter(lo, np.float32(2)) if side > 0 else lo)
            return h, wd
    raise AssertionError("no tie row found")


def pw_sumsq(a, h):
    """the float64 sum of squares under the square root of pw_word_diff."""
    d = a.astype(np.float32).astype(np.float64) - h[None]
    sq = d * d
    shape, leaves = pw_plan(a.shape[1])
    v = [pw_leaf(sq, b, n) for b, n in leaves]
    if shape == 0:
        s = v[0]
    elif shape == 1:
        s = v[0] + v[1]
    elif shape == 2:
        s = (v[0] + v[1]) + v[2]
    elif shape == 3:
        s = v[0] + (v[1] + v[2])
    else:
        s = (v[0] + v[1]) + (v[2] + v[3])
    return s


def test_reachable_plan_shapes():
    for dc in range(1, 257):
        shape, leaves = pw_plan(dc)
        want = 0 if dc <= 128 else 3 if 249 <= dc <= 255 else 1
        assert shape == want, dc
        assert len(leaves) == (1, 2, None, 3)[shape], dc
        # the leaves tile [0, dc) in order, none above numpy's block of 128,
        # at most 4 (the half-wave has 4 groups of 8 lanes)
        assert leaves[0][0] == 0 and sum(n for _, n in leaves) == dc, dc
        assert all(leaves[k][0] + leaves[k][1] == leaves[k + 1][0] for k in range(len(leaves) - 1)), dc
        assert all(1 <= n <= 128 for _, n in leaves), dc
    assert pw_plan(129)[1] == [(0, 64), (64, 65)]
    assert pw_plan(248)[1] == [(0, 120), (120, 128)]
    assert pw_plan(249)[1] == [(0, 120), (120, 64), (184, 65)]
    assert pw_plan(250)[1] == [(0, 120), (120, 64), (184, 66)]
    assert pw_plan(255)[1] == [(0, 120), (120, 64), (184, 71)]
    assert pw_plan(256)[1] == [(0, 128), (128, 128)]


@pytest.mark.parametrize("rows", [1, 65])
def test_restated_plan_is_numpys_pairwise_norm(rows):
    rng = np.random.default_rng(7 + rows)
    for dc in range(1, 257):
        a = rng.standard_normal((rows, dc)) * np.exp(rng.standard_normal((rows, dc)))
        h = rng.standard_normal(dc) * np.exp(rng.standard_normal(dc))
        want = np.linalg.norm(a.astype(np.float32) - h[None], axis=1)
        got = pw_word_diff(a, h)
        assert want.dtype == np.float64
        assert np.array_equal(got, want), (dc, np.flatnonzero(got != want)[:4].tolist())


def test_a_sequential_sum_is_not_the_pairwise_sum():
    """the float64 comparison above tells summation orders apart (a plain
    left-to-right sum differs on ordinary rows), the float32 the kernel
    returns does not -- except on the tie rows the GPU tests add."""
    rng = np.random.default_rng(11)
    for dc in (16, 40, 250):
        a = rng.standard_normal((65, dc)) * np.exp(rng.standard_normal((65, dc)))
        h = rng.standard_normal(dc) * np.exp(rng.standard_normal(dc))
        want = np.linalg.norm(a.astype(np.float32) - h[None], axis=1)
        assert (np.sqrt(seq_sumsq(a, h)) != want).any(), dc
        assert np.array_equal(np.sqrt(seq_sumsq(a, h)).astype(np.float32), want.astype(np.float32)), dc


@pytest.mark.parametrize("dc", [2, 5, 8, 9, 16, 40, 128, 129, 200, 248, 249, 250, 255, 256])
def test_tie_rows_show_the_summation_order_in_float32(dc):
    rng = np.random.default_rng(dc)
    a = np.zeros((1, dc))
    a[0, 0] = 1.0
    seen = 0
    for p in sorted({0, min(3, dc - 1), dc // 2, dc - 1}):
        for side in (1, -1):
            h, wd = tie_history_row(dc, p, side, rng)
            want = np.linalg.norm(a.astype(np.float32) - h[None], axis=1)
            assert want[0] == pw_word_diff(a, h)[0] and np.float32(want[0]) == wd
            seen += int(np.float32(np.sqrt(seq_sumsq(a, h)[0])) != wd)
    if dc >= 16:
        assert seen >= 2  # a left-to-right sum lands on the other float32


# --- host refusals of nrk_ctx_features -------------------------------------

_PTRS = ("group_off", "group_user", "pair_item", "pair_score", "hist_last", "hist_n", "ucat_off", "ucat", "w2v",
         "w2v_ok", "content", "content_flags", "created", "category")
_YT = ("user_yt", "user_yt_ok", "item_yt", "item_yt_ok")
_BUF = ctypes.create_string_buffer(64)  # a non-null address; no refused call reads it


def _tables(**over):
    """A CtxTablesC that passes every check (it would launch); ``over``
    replaces fields."""
    t = CtxTablesC()
    t.n_groups, t.last_n, t.code_stride, t.n_items = 1, 3, 16, 1
    t.dw, t.dc, t.dy = 64, 250, 64
    for f in _PTRS + _YT:
        setattr(t, f, ctypes.addressof(_BUF))
    for k, v in over.items():
        setattr(t, k, v)
    return t


def _call(t, spec=True, raw=True, codes=False):
    sp = (CtxSpecC * 16)()
    out = ctypes.addressof(_BUF)
    _lib.call("nrk_ctx_features", ctypes.c_void_p(ctypes.addressof(t)) if t is not None else None,
              ctypes.c_void_p(ctypes.addressof(sp)) if spec else None, ctypes.c_void_p(out) if raw else None,
              ctypes.c_void_p(out) if codes else None, None)


@pytest.mark.parametrize("over, kw, msg", [
    (dict(last_n=0), {}, "last_n must be in [1, 4]"),
    (dict(last_n=5, code_stride=22), {}, "last_n must be in [1, 4]"),
    (dict(dc=0), {}, "content dim must be in [1, 256]"),
    (dict(dc=257), {}, "content dim must be in [1, 256]"),
    (dict(dw=0), {}, "w2v dim must be in [1, 128]"),
    (dict(dw=129), {}, "w2v dim must be in [1, 128]"),
    (dict(n_groups=-1), {}, "n_groups must be >= 0"),
    (dict(), dict(raw=False, codes=False), "no output"),
    (dict(), dict(spec=False, codes=True), "codes need a spec and a stride"),
    (dict(code_stride=15), dict(codes=True), "codes need a spec and a stride"),
    (dict(last_n=4, code_stride=18), dict(raw=False, codes=True), "codes need a spec and a stride"),
    (dict(user_yt_ok=None), {}, "yt tables incomplete"),
    (dict(item_yt=None), {}, "yt tables incomplete"),
    (dict(item_yt_ok=None), {}, "yt tables incomplete"),
    (dict(dy=0), {}, "yt tables incomplete"),
] + [({f: None}, {}, "null table pointer") for f in _PTRS])
def test_refusals(over, kw, msg):
    with pytest.raises(ValueError) as e:
        _call(_tables(**over), **kw)
    assert str(e.value) == f"nrk_ctx_features: nrk_ctx_features: {msg}"


def test_null_tables_refused():
    with pytest.raises(ValueError, match="null tables"):
        _call(None)


def test_no_groups_is_ok():
    """n_groups = 0 with valid dimensions returns NRK_OK before the pointer
    checks (an empty chunk of the fused pipeline), with or without codes."""
    none = {f: None for f in _PTRS + _YT}
    _call(_tables(n_groups=0, **none))
    _call(_tables(n_groups=0, **none), codes=True)
    _call(_tables(n_groups=0, last_n=1, dc=1, dw=1, code_stride=10, **none), raw=False, codes=True)
    _call(_tables(n_groups=0, last_n=4, dc=256, dw=128, code_stride=19, **none), codes=True)
    # and the dimensions are still checked first
    with pytest.raises(ValueError, match="content dim"):
        _call(_tables(n_groups=0, dc=257, **none))
