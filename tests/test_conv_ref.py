"""The references and bounds of tests/_conv_ref.py, checked on the CPU: the reference arithmetic
alone (numpy emulations of the three-term split, the one-term mode and a float32 F(2x2, 3x3))
stays within its bound on every input family, the 2^-25 B' term is needed where the magnitudes
are small, and six locally wrong references all break the elementwise bound.  The range guard of
the Winograd transform is stated here as well: an emulation of wino_f16 with its range check in
either place flags an overflowed V with the check in front of the activation, and stores zeros
with a clear flag under a ReLU with the check behind it (the seventh mutation).  The figures the
module docstring and DESIGN.md quote are printed here (pytest -s)."""
import numpy as np
import pytest
import torch

import _conv_ref as cr

# (cin, cout, ks, h, w): the nets' odd output widths, an odd chunk count (24, 40), one chunk pair,
# planes that are no multiple of anything
SHAPES = [(16, 26, 1, 9, 13), (24, 19, 3, 9, 13), (40, 52, 3, 7, 11), (16, 22, 7, 9, 9), (64, 38, 3, 6, 7)]
IDS = ["c%d-%d-k%d-%dx%d" % s for s in SHAPES]


def _case(shape, family, seed=7):
    cin, cout, ks, h, w = shape
    rng = np.random.default_rng(seed)
    x = cr.make_x(family, (2, cin, h, w), rng)
    wt, b, s = cr.make_layer(cin, cout, ks, rng, bias=family != "small")
    if family == "nearrange":                      # one output at 0.9 x 65504, as the GPU range-guard test has it
        wt = cr.peak_weights(x, wt, b, 0.9 * cr.F16_MAX)
        assert abs(cr.ref64(x, wt, b)[-1, -1, -1, -1] / (0.9 * cr.F16_MAX) - 1) < 1e-6
    return x, wt, b, s


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_three_term_emulation_within_bound(shape, family):
    x, wt, b, s = _case(shape, family)
    for act in cr.ACTS:
        ref = cr.ref64(x, wt, b, s, shape[2], act)
        r, at = cr.worst(cr.emu_x3(x, wt, b, s, act), ref, cr.bound_x3(x, wt, b, s, act))
        print("x3 %s %s: worst |d| / bound %.4f at %s" % (family, act, r, at))
        assert r <= 1.0


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_term_emulation_within_bound(shape, family):
    x, wt, b, s = _case(shape, family)
    xr, wr = cr.f16(x), cr.round_w_f16(wt)
    ref = cr.ref64(xr, wr, b, s, shape[2], "prelu")
    bound = cr.bound_f16(xr, wr, b, s, "prelu")
    y = cr.emu_x3(x, wt, b, s, "prelu", terms=1)
    r, at = cr.worst(y, ref, bound)
    print("f16 %s: worst |d| / bound %.4f at %s" % (family, r, at))
    assert r <= 1.0
    # fp16 storage: the stored rounding of the same values
    r16, _ = cr.worst(cr.f16(y), ref, cr.bound_act16(bound, ref))
    assert r16 <= 1.0
    # ... and the mode is no fp32-accurate one: against the unrounded operands it breaks the
    # three-term bound where K is small (the worst-case bound grows with K, the roundings'
    # random walk with sqrt(K): at K = 784 the one-term sum sits inside it)
    if family == "uniform" and shape[2] == 1:
        assert cr.worst(y, cr.ref64(x, wt, b, s, shape[2], "prelu"), cr.bound_x3(x, wt, b, s, "prelu"))[0] > 1.0


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] == 3], ids=[i for i, s in zip(IDS, SHAPES) if s[2] == 3])
def test_winograd_restatement_within_bound(shape, family):
    x, wt, b, s = _case(shape, family)
    ref = cr.ref64(x, wt, b, s, 3, "prelu")
    r, at = cr.worst(cr.emu_wino32(x, wt, b, s, "prelu"), ref, cr.bound_wino(x, wt, b, s, "prelu"))
    print("wino %s: worst |d| / bound %.4f at %s" % (family, r, at))
    assert r <= 1.0
    # the split arithmetic is within the Winograd kernel's three-term bound as well
    assert cr.worst(cr.emu_x3(x, wt, b, s, "prelu"), ref, cr.bound_wino2(x, wt, b, s, "prelu"))[0] <= 1.0


def test_winograd_sums_dominate_the_plain_ones():
    """A_wino >= |ref| everywhere (it bounds the Winograd evaluation of the same number)."""
    x, wt, b, s = _case(SHAPES[1], "uniform")
    Aw, Aw2, Bw, Xw, _ = cr.wino_sums(x, wt, b)
    assert np.all(Aw * (1 + 1e-12) >= np.abs(cr.ref64(x, wt, b))) and np.all(Aw2 * (1 + 1e-12) >= Aw - np.abs(b)[None, :, None, None])


def test_small_magnitudes_need_the_absolute_term():
    """Activations of 1e-5 .. 1e-3: the lo halves (below 6.1e-5 the hi halves) are fp16
    subnormals, each off by up to 2^-25 whatever |x|.  The emulation passes the bound and breaks
    it once the 2^-25 B' term is taken out."""
    x, wt, b, s = _case(SHAPES[0], "small")
    ref = cr.ref64(x, wt, b)
    y = cr.emu_x3(x, wt, b)
    full = cr.worst(y, ref, cr.bound_x3(x, wt, b))[0]
    bare = cr.worst(y, ref, cr.bound_x3(x, wt, b, abs_term=False))[0]
    print("small magnitudes: worst |d| / bound %.3f with the term, %.1f without" % (full, bare))
    assert full <= 1.0 < bare


def test_operand_rounding_matches_the_pack():
    """round_w_f16 is pack_x3's hi half: max |w| 2^s in [2^13, 2^14), fp16 RNE, exact 2^-s."""
    w = np.array([0.3, -0.0007, 1e-13, 0.29999], np.float32)
    s = cr.pack_exp(w)
    assert 2 ** 13 <= 0.3 * 2.0 ** s < 2 ** 14
    wr = cr.round_w_f16(w)
    assert np.all(np.abs(wr[:2] - w[:2]) <= 2.0 ** -11 * np.abs(w[:2])) and wr[2] == 0.0
    assert cr.half_ulp16(1.0) == 2.0 ** -11 and cr.half_ulp16(1e-6) == 2.0 ** -25 and cr.half_ulp16(1.5) == 2.0 ** -11


# Which of the six mutations the whole-net bar (max |d| / max |ref| < 1e-4) sees when it is put on
# the one layer's output -- computed by the test below, which fails if this table goes stale.  On a
# single layer's output every one of them is gross enough for it; what that bar cannot do is see
# them ten layers later, and nothing but the per-layer entry puts a check on the layer itself.
OLD_BAR_SEES = {m: True for m in cr.MUTATIONS}


@pytest.mark.parametrize("kind", cr.MUTATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mutation_breaks_the_elementwise_bound(shape, kind):
    x, wt, b, s = _case(shape, "uniform")
    ref = cr.ref64(x, wt, b, s, shape[2], "prelu")
    y = cr.mutate(kind, x, wt, b, s, "prelu")
    r, at = cr.worst(y, ref, cr.bound_x3(x, wt, b, s, "prelu"))
    old = cr.old_bar(y, ref)
    print("%s: worst |d| / bound %.3g at %s; max |d| / max |ref| %.3g" % (kind, r, at, old))
    assert r > 1.0
    assert (old >= 1e-4) == OLD_BAR_SEES[kind]


# (computed, as OLD_BAR_SEES: the wrong slope turns the quiet frame's negative values over)
QUIET_STILL_SEEN = ("slope_neighbour",)


@pytest.mark.parametrize("kind", cr.MUTATIONS)
def test_mutation_in_a_quiet_region_escapes_the_old_bar(kind):
    """The same mutations where the layer's output is small against the tensor's maximum (one
    loud frame beside a quiet one, as a bright and a dark crop in one batch): the elementwise bound
    still breaks; the max-normalised bar sees the error against the loud frame's maximum."""
    shape = SHAPES[1]
    x, wt, b, s = _case(shape, "uniform")
    b = np.zeros_like(b) if kind != "bias_last" else b * 1e-3
    x[0] *= 3e3                                    # the loud frame; the mutations that name a frame hit the last
    x[1] *= 0.3
    if kind in ("chunk_pair", "swap_channels", "tile_tail", "bias_last", "slope_neighbour"):
        # frame-blind mutations: mutate the quiet frame alone
        ref = cr.ref64(x, wt, b, s, 3, "prelu")
        y = ref.copy()
        y[1:] = cr.mutate(kind, x[1:], wt, b, s, "prelu")
    else:
        ref = cr.ref64(x, wt, b, s, 3, "prelu")
        y = cr.mutate(kind, x, wt, b, s, "prelu")
    r, _ = cr.worst(y, ref, cr.bound_x3(x, wt, b, s, "prelu"))
    old = cr.old_bar(y, ref)
    print("%s (quiet frame): worst |d| / bound %.3g; max |d| / max |ref| %.3g" % (kind, r, old))
    assert r > 1.0
    assert (old >= 1e-4) == (kind in QUIET_STILL_SEEN)


# ---- the range guard of the Winograd transform ----------------------------------------------
# V = B^T d B reaches 4 x the input: a 2x2 plateau of P on the inner pixels of one tile gives
# V[1][1] = 4 P while every input and every true output stays below 65504.  (cin, cout, h, w):
# odd x odd (half-empty edge tiles on both sides), the GPU test's 19 x 65, even x even.
PLATEAU_SHAPES = [(24, 19, 9, 13), (16, 8, 19, 65), (16, 12, 8, 12)]
PLATEAU_IDS = ["c%d-%d-%dx%d" % s for s in PLATEAU_SHAPES]


def _plateau(shape, P, where, seed=11):
    cin, cout, h, w = shape
    rng = np.random.default_rng(seed)
    x = cr.make_x("plateau", (2, cin, h, w), rng, P=P, where=where)
    wt, b, s = cr.make_layer(cin, cout, 3, rng)
    f, c, ty, tx = cr.plateau_tile(x.shape, where)
    tile = (f, slice(None), slice(2 * ty, 2 * ty + 2), slice(2 * tx, 2 * tx + 2))
    assert float(np.max(np.abs(x))) < cr.F16_MAX and float(x[f, c, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2].sum()) == 4.0 * P
    assert float(np.max(np.abs(cr.ref64(x, wt, b)))) < cr.F16_MAX            # only V leaves the range
    return x, wt, b, s, tile


@pytest.mark.parametrize("where", cr.PLATEAU_WHERE)
@pytest.mark.parametrize("shape", PLATEAU_SHAPES, ids=PLATEAU_IDS)
def test_transform_overflow_raises_the_flag(shape, where):
    """P = 16384: V = 65536 splits to hi = inf, lo = -inf.  The kernel's check (before and after
    the activation) flags it for every activation and both term counts."""
    x, wt, b, s, tile = _plateau(shape, 16384.0, where)
    for act in cr.ACTS:
        for terms in (3, 1):
            y, flag = cr.emu_wino2(x, wt, b, s, act, terms=terms)
            assert flag == 1, (act, terms)
            if terms == 3:                      # inf - inf: every output of the tile, every channel
                assert np.all(y[tile] == 0) if act == "relu" else np.all(np.isnan(y[tile])), act
            else:                               # one term: +-inf by the sign of U (NaN for a zero U)
                assert not np.any(np.isfinite(y[tile]) & (y[tile] != 0)), act


@pytest.mark.parametrize("kind", cr.GUARD_MUTATIONS)
@pytest.mark.parametrize("where", cr.PLATEAU_WHERE)
@pytest.mark.parametrize("shape", PLATEAU_SHAPES, ids=PLATEAU_IDS)
def test_guard_mutation_escapes_with_relu(shape, where, kind):
    """The check behind the activation alone: with a ReLU and three terms the overflowed tile is
    stored as zeros and the flag stays clear, although the values break the bound by orders of
    magnitude.  What tests/test_gpu_conv_layers.py::test_range_guard_transform must catch."""
    x, wt, b, s, tile = _plateau(shape, 16384.0, where)
    y, flag = cr.emu_wino2(x, wt, b, s, "relu", terms=3, check=kind)
    ref = cr.ref64(x, wt, b, s, 3, "relu")
    r, at = cr.worst(y, ref, cr.bound_wino2(x, wt, b, s, "relu"))
    print("%s %s: flag %d, worst |d| / bound %.3g at %s, max |d| / max |ref| %.3g" % (kind, where, flag, r, at, cr.old_bar(y, ref)))
    assert flag == 0 and np.all(y[tile] == 0) and y[tile].size > 0
    assert r > 1.0 and np.all(np.isfinite(y))
    assert cr.emu_wino2(x, wt, b, s, "relu", terms=3)[1] == 1          # the kernel's check sees it
    # without the ReLU the NaN is stored, and the stored-value check alone is enough
    for act in ("none", "prelu"):
        assert cr.emu_wino2(x, wt, b, s, act, terms=3, check=kind)[1] == 1


@pytest.mark.parametrize("where", cr.PLATEAU_WHERE)
@pytest.mark.parametrize("shape", PLATEAU_SHAPES, ids=PLATEAU_IDS)
def test_plateau_in_range_within_bound(shape, where):
    """P = 16000: V = 64000 splits finitely.  No flag, and every element within bound_wino2."""
    x, wt, b, s, _ = _plateau(shape, 16000.0, where)
    for act in cr.ACTS:
        y, flag = cr.emu_wino2(x, wt, b, s, act)
        r, at = cr.worst(y, cr.ref64(x, wt, b, s, 3, act), cr.bound_wino2(x, wt, b, s, act))
        print("wino2 plateau 16000 %s %s: flag %d, worst |d| / bound %.4f at %s" % (where, act, flag, r, at))
        assert flag == 0 and r <= 1.0
        assert cr.emu_wino2(x, wt, b, s, act, check="stored_only")[1] == 0


@pytest.mark.parametrize("where", cr.PLATEAU_WHERE)
def test_split_boundary(where):
    """V = 65504 (P = 16376) is the largest fp16 number and splits exactly; V = 65520 (P = 16380)
    is the tie that rounds to even, to infinity."""
    with np.errstate(over="ignore"):
        assert cr.f16(65504.0) == 65504.0 and np.isinf(cr.f16(65520.0)) and np.isfinite(cr.f16(np.nextafter(np.float32(65520.0), np.float32(0))))
    for P, tripped in ((16376.0, 0), (16380.0, 1)):
        x, wt, b, s, _ = _plateau(PLATEAU_SHAPES[0], P, where)
        for act in cr.ACTS:
            y, flag = cr.emu_wino2(x, wt, b, s, act)
            assert flag == tripped, (P, act)
            if not tripped:
                assert cr.worst(y, cr.ref64(x, wt, b, s, 3, act), cr.bound_wino2(x, wt, b, s, act))[0] <= 1.0


def test_winograd_emulation_within_bound_on_the_families():
    """emu_wino2 on the plain input families stays within bound_wino2 with a clear flag."""
    for family in ("uniform", "postact", "small"):
        x, wt, b, s = _case(SHAPES[1], family)
        y, flag = cr.emu_wino2(x, wt, b, s, "prelu")
        assert flag == 0 and cr.worst(y, cr.ref64(x, wt, b, s, 3, "prelu"), cr.bound_wino2(x, wt, b, s, "prelu"))[0] <= 1.0


def test_headroom_of_native_fp32():
    """How far a plain fp32 convolution (torch CPU, float32) sits below the bounds, uniform(-1, 1):
    the figures of the module docstring and DESIGN.md."""
    for shape, lo, hi in ((SHAPES[0], 1e-3, 0.2), (SHAPES[1], 1e-4, 0.05), (SHAPES[4], 1e-4, 0.02)):
        x, wt, b, s = _case(shape, "uniform")
        y32 = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b),
                                         padding=shape[2] // 2).numpy()
        ref = cr.ref64(x, wt, b)
        r3 = cr.worst(y32, ref, cr.bound_x3(x, wt, b))[0]
        rd = cr.worst(y32, ref, cr.bound_direct(x, wt, b))[0]
        print("native fp32 c%d k%d: %.5f of bound_x3 (1/%.0f), %.5f of bound_direct (1/%.0f)" % (
            shape[0], shape[2], r3, 1 / r3, rd, 1 / rd))
        assert lo < r3 < hi and rd <= 1.0
