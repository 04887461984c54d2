"""The references and bounds of tests/_conv_ref.py, checked on the CPU: the reference arithmetic
alone (numpy emulations of the three-term split, the one-term mode and a float32 F(2x2, 3x3))
stays within its bound on every input family, the 2^-25 B' term is needed where the magnitudes
are small, and six locally wrong references all break the elementwise bound.  The range guard of
the Winograd transform is stated here as well: an emulation of wino_f16 with its range check in
either place flags an overflowed V with the check in front of the activation, and stores zeros
with a clear flag under a ReLU with the check behind it (the seventh mutation).  The last part
is the sharp statistic cr.nerr_rms at the depths the nets run (K 512 .. 4608): fair to every
honest arithmetic, sharp on every lost or mixed-up lo product, and the blind spot of the
elementwise bound and the whole-net bar there, pinned.  The figures the module docstring and
DESIGN.md quote are printed here (pytest -s)."""
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


# ---- the sharp statistic at the depths the nets run ------------------------------------------
# worst() against a bound that carries gamma(3 K) goes blind with K: honest rounding grows like
# sqrt(K), the bound like K, and a lost lo product shrinks like 1 / sqrt(K) against A.  From
# K ~ 1000 a kernel that drops one of its three products passes the elementwise bound and the
# whole-net bar.  cr.nerr_rms -- the rms over (frame, 32 output channels) of |d| / A -- is flat in
# K for the honest arithmetic, and the bar is 3 E with E the same figure of the emulation itself
# (cr.yardstick).  Below: fair (every honest arithmetic at most 0.5 of the bar), sharp (every
# named mutant at least 2 x the bar) at each depth tests/test_gpu_conv_layers.py asserts (g) at,
# and the blind spot of the old checks, pinned.  One frame of 11 x 23 and 64 output channels (two
# groups); the figures are printed (pytest -s) and quoted in DESIGN.md.

# (kernel, cin, ks): the five deep Winograd cases, union-k2304, pairs2-k512, and the g2 depth
DEEP = [("wino2", 128, 3), ("wino2", 180, 3), ("wino2", 256, 3), ("wino2", 384, 3), ("wino2", 512, 3),
        ("x3", 180, 3), ("x3", 256, 3), ("x3", 512, 1)]
DEEP_IDS = ["%s-c%d-k%d" % d for d in DEEP]
_DEEP = {}


class _Deep:
    """One depth's inputs, float64 reference, A, old bound and E, made once and never written to."""

    def __init__(self, kernel, cin, ks, cout=64, h=11, w=23):
        rng = np.random.default_rng(1000 * cin + ks)
        self.kernel, self.cin, self.ks, self.act = kernel, cin, ks, "prelu"
        self.x = cr.make_x("uniform", (1, cin, h, w), rng)
        self.w, self.b, self.s = cr.make_layer(cin, cout, ks, rng)
        self.ref = cr.ref64(self.x, self.w, self.b, self.s, ks, self.act)
        self.fac = cr.act_factor(self.s, self.act)
        if kernel == "wino2":
            sums = cr.wino_sums(self.x, self.w, self.b)
            self.A, self.bound = sums[0], cr.bound_wino2(self.x, self.w, self.b, self.s, self.act, sums=sums)
            assert np.array_equal(self.A, cr.wino_absum(self.x, self.w, self.b))
        else:
            self.A = cr.absum(self.x, self.w, self.b)
            self.bound = cr.bound_x3(self.x, self.w, self.b, self.s, self.act, A=self.A)
        self.E = cr.yardstick(kernel, self.x, self.w, self.b, self.s, self.act)
        self.bar = cr.NERR_FACTOR * self.E

    def emu(self, **kw):
        if self.kernel == "wino2":
            return cr.emu_wino2(self.x, self.w, self.b, self.s, self.act, **kw)[0]
        return cr.emu_x3(self.x, self.w, self.b, self.s, self.act, **kw)

    def groups(self, y):
        return cr.nerr_rms(y, self.ref, self.A, self.fac)

    def last_pair(self):
        return (self.cin - 1) // 16 * 16, self.cin


def _deep(d):
    if d not in _DEEP:
        _DEEP[d] = _Deep(*d)
    return _DEEP[d]


def test_nerr_rms_is_what_it_says():
    """float64 throughout; per (frame, 32 channels); A == 0 elements left out and held to d == 0;
    a NaN in y is infinite; groups=None pools the tensor."""
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((2, 40, 3, 4))
    A = np.abs(ref) + 1.0
    d = rng.standard_normal(ref.shape) * 1e-7
    y = ref + d
    g = cr.nerr_rms(y, ref, A)
    assert g.shape == (2, 2) and g.dtype == np.float64
    want = np.sqrt(np.mean((d[1, 32:] / A[1, 32:]) ** 2))
    assert abs(g[1, 1] / want - 1) < 1e-6                      # (y - ref recovers d to 1e-16 of |ref|)
    pooled = cr.nerr_rms(y, ref, A, 1.0, None)
    assert isinstance(pooled, float) and abs(pooled / np.sqrt(np.mean(((y - ref) / A) ** 2)) - 1) < 1e-12
    fac = np.full((1, 40, 1, 1), 2.0)
    assert np.allclose(cr.nerr_rms(y, ref, A, fac), g / 2, rtol=1e-12)
    # a float32 result is compared in float64: its own rounding is what is measured
    y32 = ref.astype(np.float32)
    assert 1e-9 < cr.nerr_rms(y32, ref, A, 1.0, None) < 1e-7
    # A == 0: out of the mean, and d must be 0 there
    A0 = A.copy()
    A0[0, 0] = 0.0
    y0 = y.copy()
    y0[0, 0] = ref[0, 0]
    g0 = cr.nerr_rms(y0, ref, A0)
    assert abs(g0[0, 0] / np.sqrt(np.mean((d[0, 1:32] / A[0, 1:32]) ** 2)) - 1) < 1e-6 and g0[1, 1] == g[1, 1]
    g1 = cr.nerr_rms(y, ref, A0)                               # d != 0 where A == 0
    assert np.isinf(g1[0, 0]) and np.all(np.isfinite(g1.ravel()[1:]))
    assert cr.nerr_rms(ref, ref, np.zeros_like(A)).max() == 0.0
    yn = y.copy()
    yn[1, 39, 2, 3] = np.nan
    gn = cr.nerr_rms(yn, ref, A)
    assert np.isinf(gn[1, 1]) and np.all(np.isfinite(gn.ravel()[:3])) and np.isinf(cr.nerr_rms(yn, ref, A, 1.0, None))
    assert list(cr.yardstick_channels(64)) == list(range(16)) + list(range(48, 64))
    assert list(cr.yardstick_channels(19)) == list(range(19)) and list(cr.yardstick_channels(1)) == [0]


def test_mutant_seam_leaves_the_emulations_alone():
    """The default path of both emulations is the order they always had (x3: shuffled by seed;
    wino2: the channels' own), a mutant restricted to output channels changes no bit elsewhere,
    and every mutant kind changes something where it applies."""
    x, wt, b, s = _case(SHAPES[2], "uniform")                  # cin 40: two whole chunk pairs and a half
    y3 = cr.emu_x3(x, wt, b, s, "prelu")
    assert np.array_equal(y3.view(np.uint32), cr.emu_x3(x, wt, b, s, "prelu", order="shuffled", seed=0, mutant=None).view(np.uint32))
    yw = cr.emu_wino2(x, wt, b, s, "prelu")[0]
    assert np.array_equal(yw.view(np.uint32), cr.emu_wino2(x, wt, b, s, "prelu", order="inorder", mutant=None)[0].view(np.uint32))
    sel = np.r_[0:16, 36:52]
    assert np.array_equal(cr.emu_x3(x, wt[sel], b[sel], s[sel], "prelu", s=cr.pack_exp(wt)).view(np.uint32), y3[:, sel].view(np.uint32))
    assert np.array_equal(cr.emu_wino2(x, wt[sel], b[sel], s[sel], "prelu", s=cr.wino_exp(wt))[0].view(np.uint32), yw[:, sel].view(np.uint32))
    for kind in cr.MUTANT_KINDS:
        for emu, y, inner in ((lambda **k: cr.emu_x3(x, wt, b, s, "prelu", **k), y3, dict(tap=8)),
                              (lambda **k: cr.emu_wino2(x, wt, b, s, "prelu", **k)[0], yw, dict(xi=5))):
            m = emu(mutant=cr.lo_mutant(kind, co=(32, 52), ci=(16, 40), **inner))
            assert np.array_equal(m[:, :32].view(np.uint32), y[:, :32].view(np.uint32)), kind
            assert not np.array_equal(m[:, 32:], y[:, 32:]), kind


def test_honest_figure_is_flat_in_depth():
    """E per kernel over the depths: within 15 % of one another (3 x 3 Winograd cin 128 .. 512;
    the direct form K 512 .. 2304), where gamma(3 K) moves by 4.5 x."""
    for kernel in ("wino2", "x3"):
        Es = [_deep(d).E for d in DEEP if d[0] == kernel]
        print("%s: E over the depths %s" % (kernel, " ".join("%.3e" % e for e in Es)))
        assert max(Es) / min(Es) < 1.15


@pytest.mark.parametrize("d", DEEP, ids=DEEP_IDS)
def test_statistic_is_fair(d):
    """Every honest arithmetic sits at or below 0.5 of the bar in every group: the emulation in
    three summation orders (in order, shuffled, a pairwise tree per 16 channels) and a plain
    float32 torch convolution."""
    D = _deep(d)
    rows = [(o, D.emu(order=o)) for o in cr.ORDERS]
    y32 = torch.nn.functional.conv2d(torch.from_numpy(D.x), torch.from_numpy(D.w), torch.from_numpy(D.b), padding=D.ks // 2).numpy()
    rows.append(("native fp32", np.where(y32 >= 0, y32, y32 * D.s[None, :, None, None]).astype(np.float32)))
    for name, y in rows:
        g = float(D.groups(y).max())
        print("%s cin %d k%d: %-11s largest group %.3e = %.3f E = %.3f of the bar (E %.3e)" % (
            D.kernel, D.cin, D.ks, name, g, g / D.E, g / D.bar, D.E))
        assert g <= 0.5 * D.bar
        assert cr.worst(y, D.ref, D.bound)[0] <= 1.0


def _mutants(D):
    """name -> lo_mutant, the mutants of the issue that exist for this arithmetic."""
    last = D.last_pair()
    m = {"drop hi.lo": cr.lo_mutant("drop_hl"), "drop lo.hi": cr.lo_mutant("drop_lh"),
         "drop hi.lo, last pair": cr.lo_mutant("drop_hl", ci=last), "drop lo.hi, last pair": cr.lo_mutant("drop_lh", ci=last),
         "stale lo of pair k - 1": cr.lo_mutant("stale_lo"),
         "one term, channels 32..63": cr.lo_mutant("one_term", co=(32, 64))}
    if D.kernel == "wino2":
        m.update({"drop hi.lo, GEMM 5": cr.lo_mutant("drop_hl", xi=5), "drop lo.hi, GEMM 5": cr.lo_mutant("drop_lh", xi=5),
                  "drop hi.lo, GEMM 5, last pair": cr.lo_mutant("drop_hl", xi=5, ci=last),
                  "drop lo.hi, GEMM 5, last pair": cr.lo_mutant("drop_lh", xi=5, ci=last)})
    elif D.ks == 3:
        m.update({"drop hi.lo, tap 4 of 9": cr.lo_mutant("drop_hl", tap=4), "drop lo.hi, tap 0 of 9": cr.lo_mutant("drop_lh", tap=0)})
    return m


@pytest.mark.parametrize("d", DEEP, ids=DEEP_IDS)
def test_statistic_is_sharp(d):
    """Every named mutant exceeds 2 x the bar in its worst group -- and (printed) where it stands
    against the elementwise bound and the whole-net bar, which most of them pass."""
    D = _deep(d)
    for name, m in _mutants(D).items():
        y = D.emu(mutant=m)
        g = float(D.groups(y).max())
        print("%s cin %d k%d: %-30s %7.1f E = %6.1f x the bar; worst |d| / bound %.3f, max |d| / max |ref| %.2e" % (
            D.kernel, D.cin, D.ks, name, g / D.E, g / D.bar, cr.worst(y, D.ref, D.bound)[0], cr.old_bar(y, D.ref)))
        assert g > 2 * D.bar, name
    # the one-group mutant is seen in its group alone
    g = D.groups(D.emu(mutant=cr.lo_mutant("one_term", co=(32, 64))))
    assert g[0, 1] > 2 * D.bar and g[0, 0] <= 0.5 * D.bar


def test_deep_k_blind_spot_of_the_old_checks():
    """The gap, recorded as test_mutation_in_a_quiet_region_escapes_the_old_bar records its own.
    "Drop Uh Vl in GEMM 5" at cin 512: within the elementwise bound (0.061) and under the whole-net
    bar on the layer's own output (9.1e-5 < 1e-4), at 29 x the new bar.  "Drop wh xl" everywhere
    at K 1620: within the elementwise bound (0.107); the whole-net bar reads 1.8e-4 on the mutated
    layer's own output -- there it still sees it -- and 1.8e-5 once a frame ten times as loud
    shares the tensor (the bar is put on net outputs, ten layers on, over a batch); the new bar is
    missed 56 times over in the mutated frame's groups and kept by the loud frame's."""
    W = _deep(("wino2", 512, 3))
    y = W.emu(mutant=cr.lo_mutant("drop_hl", xi=5))
    r, old, g = cr.worst(y, W.ref, W.bound)[0], cr.old_bar(y, W.ref), float(W.groups(y).max())
    print("wino2 cin 512, drop Uh.Vl in GEMM 5: worst |d| / bound %.3f, max |d| / max |ref| %.2e, %.1f x the new bar" % (r, old, g / W.bar))
    assert r <= 1.0 and old < 1e-4 and g > 2 * W.bar
    X = _deep(("x3", 180, 3))
    y = X.emu(mutant=cr.lo_mutant("drop_hl"))
    r, old, g = cr.worst(y, X.ref, X.bound)[0], cr.old_bar(y, X.ref), float(X.groups(y).max())
    loud = 10.0 * X.x                                           # exact in fp32 and in the fp16 splits
    y2 = np.concatenate([cr.emu_x3(loud, X.w, X.b, X.s, X.act), y])
    x2 = np.concatenate([loud, X.x])
    ref2 = cr.ref64(x2, X.w, X.b, X.s, 3, X.act)
    A2 = cr.absum(x2, X.w, X.b)
    r2 = cr.worst(y2, ref2, cr.bound_x3(x2, X.w, X.b, X.s, X.act, A=A2))[0]
    old2, g2 = cr.old_bar(y2, ref2), cr.nerr_rms(y2, ref2, A2, X.fac)
    print("x3 K 1620, drop wh.xl: worst |d| / bound %.3f, max |d| / max |ref| %.2e on its own output, %.2e beside a loud frame; "
          "%.1f x the new bar" % (r, old, old2, g / X.bar))
    assert r <= 1.0 and r2 <= 1.0 and old >= 1e-4 > old2
    assert g > 2 * X.bar and g2[1].min() > 2 * X.bar and g2[0].max() <= 0.5 * X.bar


# (depth, the product dropped everywhere, whether the elementwise bound still sees it)
BLIND_WITH_K = [(("x3", 24, 3), "drop_hl", True), (("x3", 180, 3), "drop_hl", False), (("x3", 512, 3), "drop_lh", False),
                (("wino2", 40, 3), "drop_hl", True), (("wino2", 256, 3), "drop_hl", False), (("wino2", 384, 3), "drop_hl", False),
                (("wino2", 512, 3), "drop_hl", False)]


def test_elementwise_bound_goes_blind_with_k():
    """One product lost everywhere against the elementwise bound: caught at cin 24 and 40 (the
    depths tests/test_gpu_conv_layers.py had), passed from K ~ 1000 on, the ratio falling like
    1 / sqrt(K).  The new statistic sees every row."""
    for d, kind, caught in BLIND_WITH_K:
        D = _deep(d)
        y = D.emu(mutant=cr.lo_mutant(kind))
        r, g = cr.worst(y, D.ref, D.bound)[0], float(D.groups(y).max())
        print("%s cin %d (K %d) %s everywhere: worst |d| / bound %.3f (%s), %.0f x the new bar" % (
            D.kernel, D.cin, D.cin * D.ks ** 2, kind, r, "caught" if r > 1 else "passes", g / D.bar))
        assert (r > 1.0) == caught and g > 2 * D.bar
