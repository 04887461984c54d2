"""Float64 references, per-element error bounds and numpy emulations of the conv kernels, for
tests/test_conv_ref.py (CPU) and tests/test_gpu_conv_layers.py (one layer through
rt.debug_conv on an MI355X).

Notation.  u = 2^-24 is the fp32 unit round-off, gamma(n) = n u / (1 - n u) the bound of n
accumulated roundings (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).
K = cin * ks^2 is the number of products of one output.  Per output element, all in float64:

  A  = sum |x| |w| + |b|                absum(): the convolution of the absolute values
  B  = sum |w| over the taps inside the image                                   wsum()
  X1 = sum |x| over those taps                                                  xsum()

Summation.  A sum of n fp32 terms taken in ANY order (a chain, a tree, the canonical K ranges,
split-K partial sums added by x3_splitk_reduce) passes every term through at most n - 1 rounded
additions, so its error is at most gamma(n - 1) sum |terms|.  The matrix cores' internal order
is not documented; the bound does not need it.

Three-term conv_x3 (csrc/conv_x3.hip lines 1-22, pack_x3 in csrc/pack.cpp).
  x = xh + xl + rx with xh = fp16(x), xl = fp16(x - xh) (the subtraction is exact in fp32).
  fp16 carries 11 bits: |x - xh| <= 2^-11 |x| while xh is a normal number, and
  |rx| <= 2^-11 |x - xh| <= 2^-22 |x| while xl is one.  An fp16 subnormal is a multiple of 2^-24,
  so below the normal range a rounding errs by at most 2^-25 absolutely -- the "absolute error
  <= 2^-25" of line 18.  In every case |rx| <= 2^-22 |x| + 2^-25.
  w' = w 2^s (exact; max |w'| in [2^13, 2^14)) = wh + wl + rw in the same way:
  |rw| <= 2^-22 |w'| + 2^-25, i.e. 2^-22 |w| + 2^-25 2^-s after the epilogue's exact 2^-s.
  The kernel sums xh wh + xh wl + xl wh (each product exact in fp32: 11 x 11 bits).  Against
  x w' that misses  xl wl + rx w' + (xh + xl) rw, at most
      3 * 2^-22 |x| |w'| + 2^-25 |w'| + 2^-25 |x|,
  times 1 + 2^-10 for the second-order terms (|xl| <= 2^-11 |x| (1 + 2^-11), ...).  Hence
      c_s = 1.5 (1 + 2^-10)        on 2^-21 A     (the dropped lo*lo term and both residuals)
      c_u = 1 + 2^-10              on 2^-25 B'    B' = B + 2^-s X1: the subnormal lo halves of
                                                   the activations (B) and of the filters (X1)
  The 3K products, the bias and the activation's multiply make 3K - 1 + 2 roundings of terms
  whose absolute sum is at most (1 + 2^-9) A (|xh| <= (1 + 2^-11) |x|, |wl| <= 2^-11 |w'|):
      c_K = 3, c_0 = 2:   gamma(3K + 2) (1 + 2^-9) A
  bound_x3 = act * [gamma(3K + 2)(1 + 2^-9) A + c_s 2^-21 A + c_u 2^-25 B'].
  act = max(1, |slope|) for PReLU, 1 otherwise: where y and ref have one sign the activation
  scales the error by 1 or |slope|; where they differ |ref| <= |y - ref| and the same factor holds.

conv_x3_rgb is the same arithmetic with K = 27.

One-term (ISL_PREC_FP16, include/islpose.h): the operands are rounded once, x to fp16(x) and w to
fp16(w 2^s) 2^-s, the products are exact in fp32, the accumulation is fp32.  Against ref64 of the
ROUNDED operands only the summation remains:  bound_f16 = act * gamma(K + 2) A(rounded operands).

direct (csrc/conv.hip, fp32 matrix cores): fp32 operands are exact; K products and K - 1 + 2
additions round:  bound_direct = act * gamma(2K + 2) A.

wino (csrc/wino.hip, F(2x2, 3x3) in fp32): U = G g G^T in float64 rounded once to fp32, V = B^T d B
in fp32 (two additions per entry), M = sum_ci U V (cin products, cin - 1 additions), Y = A^T M A
(four additions), bias, activation: 2 cin + 9 roundings.  The cancellation in B^T d B makes A the
wrong yardstick; the Winograd-domain absolute sum is
      A_wino  = |A^T| (sum_ci |U| . |V|) |A| + |b|,       V = B^T d B in float64,
and the two roundings of V act on |B^T| |d| |B| >= |V|, which needs the companion
      A_wino2 = |A^T| (sum_ci |U| . (|B^T| |d| |B|)) |A|:
  bound_wino = act * [gamma(2 cin + 7) A_wino + gamma(2) (1 + 2^-10) A_wino2].

wino2 (csrc/wino_f16.hip): the same transforms with the three-term split of U 2^s and V:
  bound_wino2 = act * [gamma(3 cin + 7)(1 + 2^-9) A_wino + c_s 2^-21 A_wino
                       + gamma(2)(1 + 2^-10) A_wino2 + c_u 2^-25 (B_wino + 2^-s X_wino)],
  B_wino = |A^T| (sum_ci |U|) |A|, X_wino = |A^T| (sum_ci |V|) |A|.

  Range of the transform (emu_wino2, the plateau family).  V sums four inputs, so inputs below 65504
  give |V| up to 4 x 65504.  The split's hi = fp16(V) is finite up to |V| < 65520 (65504 is the
  largest fp16 number, 65520 the tie that rounds to even: to infinity); from there hi = +-inf,
  lo = fp16(V - hi) = -+inf, and hi Uh + lo Uh + hi Ul is inf - inf: NaN in every output of the tile,
  in every channel.  A 2x2 plateau P on a tile's inner pixels makes V[1][1] = 4 P exactly (fp32 adds
  of equal powers-of-two multiples are exact here): P = 16376 -> 65504 (clean), 16380 -> 65520 and
  16384 -> 65536 (overflow), 16000 -> 64000 (in range: the bound above holds unchanged, since
  |rv| <= 2^-22 |V| + 2^-25 needs only a normal, finite hi).  The kernel must raise the range flag
  for the overflow whatever the activation stores; a ReLU stores that NaN as 0.

fp16 storage (ISL_ACT_FP16): the epilogue stores RNE(v) of a value v within the bound E of ref:
  |y - ref| <= E + half an fp16 ulp at |ref| + E   (bound_act16).

Headroom (test_conv_ref.py::test_headroom_of_native_fp32, uniform(-1, 1) inputs): a plain native
fp32 convolution (torch CPU, float32) has max |y - ref| / bound_x3 of 0.042 (1x1, 16 channels: 1/24),
0.0025 (3x3, 24 channels: 1/397) and 0.0008 (3x3, 64 channels: 1/1250); against bound_direct 0.078,
0.0039 and 0.0012.  The worst-case bound grows with K, the roundings' random walk with sqrt(K).  On
the MI355X the three-term kernels sit at 0.0001 .. 0.09 of bound_x3 (the same ratios as native fp32),
the one-term kernels at 0.0003 .. 0.17 of bound_f16, and the fp16-storage forms at 0.47 .. 0.999 of
bound_act16, which the half ulp of the stored rounding leads: a truncation instead of the rounding
to nearest, or a double rounding, would break it.  On small magnitudes (1e-5 .. 1e-3, K = 16) the
emulation reaches 0.62 of the bound and 59.6 times the bound without its 2^-25 B' term.

The sharp statistic (nerr_rms, yardstick).  The headroom above is the bounds' blind
spot: gamma(3 K + 2) A grows like K, the honest error like sqrt(K), and the error of a lost lo
product (2^-12 relative per term, signs at random) shrinks like 1 / sqrt(K) against A.  At K = 216
"drop wh xl everywhere" is 1.8 x bound_x3; at K = 1620 it is 0.11, at K = 2304 0.06; for wino2,
"drop Uh Vl in one of the 16 GEMMs" at cin 512 is 0.06 of bound_wino2.  The rms over a tensor of
d / A (d / A_wino) does not have that slope: 1.15e-8 .. 1.18e-8 for emu_wino2 at cin 128 .. 512 and
3.0e-8 .. 3.2e-8 for emu_x3 at K 512 .. 2304, whatever the order of the sum; a float32 convolution
and a pairwise sum per 16 channels sit at 0.1 .. 0.4 of it.  So a kernel's output is held, per
(frame, 32 output channels), to NERR_FACTOR = 3 times E, the same figure of the emulation on the
case's own inputs -- the reference arithmetic is the yardstick, never the kernel.  Every mutant of
lo_mutant() tried is at 15 E or more at every depth (test_conv_ref.py::test_statistic_is_sharp).

The bound is not vacuous for being loose in the sum: it is per element and normalised by A there,
where the whole-net bar max |d| / max |ref| < 1e-4 is one number per tensor.  The mutation checks of
test_conv_ref.py (a dropped corner tap, a skipped chunk pair of one channel, two channels swapped,
a tile-tail pixel from the next row, a missing bias, a neighbour's PReLU slope) break the
elementwise bound by factors of 55 to 370000 at every shape tried.  Put on the same one-layer
output the old bar sees all six as well (0.012 .. 1.5 against 1e-4: on one layer's own output they
are gross); what it cannot see is the same mistake in a quiet part of the tensor.  With a loud
frame (x 3000) beside the mutated quiet one, five of the six stay under 1e-4 of the tensor's maximum
(1.5e-5 .. 7.9e-5; the missing bias 7e-9) while the elementwise ratio is 1.56 .. 10600; only the
neighbour's slope still shows (1.2e-4).  Ten more layers and a max over the map dilute further.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
C_S = 1.5 * (1 + 2.0 ** -10)
C_U = 1 + 2.0 ** -10
F16_MAX = 65504.0

ACTS = ("none", "relu", "prelu")


def gamma(n):
    return n * U32 / (1.0 - n * U32)


# ---- references -----------------------------------------------------------------------------

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def activate(t, slope, act):
    """The activation of a float64 tensor [n, cout, h, w] (numpy in, numpy out)."""
    if act == "relu":
        return np.maximum(t, 0.0)
    if act == "prelu":
        return np.where(t >= 0, t, t * np.asarray(slope, np.float64)[None, :, None, None])
    return t


def conv64(x, w, b):
    ks = w.shape[2]
    return torch.nn.functional.conv2d(_t(x), _t(w), None if b is None else _t(b), padding=ks // 2).numpy()


def ref64(x, w, b, slope=None, ks=None, act="none"):
    """torch-CPU conv2d in float64 (stride 1, 'same' padding), bias, activation."""
    assert ks is None or ks == w.shape[2]
    return activate(conv64(x, w, b), slope, act)


def hpool(y):
    """Max of horizontal pixel pairs (even width): the pair-max map of ConvLaunch::hpool."""
    return np.maximum(y[..., 0::2], y[..., 1::2])


def pool2(y):
    """MaxPool2d(2, 2), floor mode."""
    h, w = y.shape[2] // 2 * 2, y.shape[3] // 2 * 2
    y = y[:, :, :h, :w]
    return np.maximum(np.maximum(y[:, :, 0::2, 0::2], y[:, :, 0::2, 1::2]),
                      np.maximum(y[:, :, 1::2, 0::2], y[:, :, 1::2, 1::2]))


def absum(x, w, b):
    """A: the same convolution of |x|, |w|, |b| in float64."""
    return conv64(np.abs(x), np.abs(w), np.abs(b))


def wsum(w, h, wd):
    """B: per element, sum |w| over the taps that fall inside the image; [1, cout, h, w]."""
    return conv64(np.ones((1, w.shape[1], h, wd)), np.abs(w), None)


def xsum(x, ks):
    """X1: per pixel, sum |x| over the window's taps inside the image; [n, 1, h, w]."""
    return conv64(np.abs(x), np.ones((1, x.shape[1], ks, ks)), None)


# ---- operand roundings ----------------------------------------------------------------------

def pack_exp(w):
    """pack_x3's s: max |w| 2^s in [2^13, 2^14) (0 for an all-zero filter)."""
    mx = float(np.max(np.abs(np.asarray(w, np.float32)))) if np.size(w) else 0.0
    if mx == 0.0:
        return 0
    _, e = np.frexp(np.float32(mx))
    return 14 - int(e)


def f16(a):
    """Round to nearest even to fp16, returned as float32."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def round_w_f16(w, s=None):
    """The one-term filters: fp16(w 2^s) 2^-s."""
    s = pack_exp(w) if s is None else s
    return np.ldexp(f16(np.ldexp(np.asarray(w, np.float32), s)), -s).astype(np.float32)


def half_ulp16(m):
    """Half an fp16 ulp at magnitude m (2^-25 below the normal range)."""
    m = np.maximum(np.asarray(m, np.float64), 2.0 ** -14)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 11)


# ---- bounds ---------------------------------------------------------------------------------

def act_factor(slope, act):
    if act == "prelu":
        return np.maximum(1.0, np.abs(np.asarray(slope, np.float64)))[None, :, None, None]
    return 1.0


def bound_x3(x, w, b, slope=None, act="none", abs_term=True, A=None):
    """Three-term conv_x3 / conv_x3_rgb against ref64(x, w, b).  abs_term=False drops the
    2^-25 B' term (the small-magnitude test shows it is needed).  A: absum(x, w, b) where the
    caller has it."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    A = absum(x, w, b) if A is None else A
    e = gamma(3 * K + 2) * (1 + 2.0 ** -9) * A + C_S * 2.0 ** -21 * A
    if abs_term:
        Bp = wsum(w, x.shape[2], x.shape[3]) + np.ldexp(1.0, -pack_exp(w)) * xsum(x, w.shape[2])
        e = e + C_U * 2.0 ** -25 * Bp
    return act_factor(slope, act) * e


def bound_f16(xr, wr, b, slope=None, act="none"):
    """One-term kernels against ref64 of the rounded operands xr = f16(x), wr = round_w_f16(w)."""
    K = wr.shape[1] * wr.shape[2] * wr.shape[3]
    return act_factor(slope, act) * gamma(K + 2) * absum(xr, wr, b)


def bound_direct(x, w, b, slope=None, act="none"):
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return act_factor(slope, act) * gamma(2 * K + 2) * absum(x, w, b)


def bound_act16(bound, ref):
    return bound + half_ulp16(np.abs(ref) + bound)


# Winograd F(2x2, 3x3)
_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def _tiles(x, dtype=np.float64):
    """The 4x4 input tiles d [n, cin, th, tw, 4, 4] of the zero-padded map (pad 1, odd sizes
    padded to whole tiles)."""
    n, c, h, w = x.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = np.zeros((n, c, 2 * th + 2, 2 * tw + 2), dtype)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    d = np.empty((n, c, th, tw, 4, 4), dtype)
    for i in range(4):
        for j in range(4):
            d[..., i, j] = xp[:, :, i:i + 2 * th:2, j:j + 2 * tw:2]
    return d


def _untile(y, h, w):
    """[n, cout, th, tw, 2, 2] -> [n, cout, h, w]."""
    n, c, th, tw = y.shape[:4]
    return y.transpose(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * th, 2 * tw)[:, :, :h, :w]


def wino_sums(x, w, b):
    """(A_wino, A_wino2, B_wino, X_wino, s) of the module docstring, each [n, cout, h, w]
    (B_wino: [1, ...]); s = pack_wino_f16's exponent (max |U| 2^s in [2^13, 2^14))."""
    h, wd = x.shape[2], x.shape[3]
    U = np.einsum("ik,ockl,jl->ocij", _G, np.asarray(w, np.float64), _G)
    d = _tiles(np.asarray(x, np.float64))
    V = np.einsum("ik,ncabkl,jl->ncabij", _BT, d, _BT)
    V2 = np.einsum("ik,ncabkl,jl->ncabij", np.abs(_BT), np.abs(d), np.abs(_BT))
    aA = np.abs(_AT)

    def back(M):
        return _untile(np.einsum("ik,noabkl,jl->noabij", aA, M, aA), h, wd)
    aU = np.abs(U)
    Aw = back(np.einsum("ocij,ncabij->noabij", aU, np.abs(V))) + np.abs(np.asarray(b, np.float64))[None, :, None, None]
    Aw2 = back(np.einsum("ocij,ncabij->noabij", aU, V2))
    ones = np.ones((1,) + V.shape[1:])
    Bw = back(np.einsum("ocij,ncabij->noabij", aU, ones))
    Xw = back(np.einsum("ocij,ncabij->noabij", np.ones_like(aU), np.abs(V)))
    mx = float(np.max(np.abs(U)))
    s = 0 if mx == 0.0 else 14 - int(np.frexp(mx)[1])
    return Aw, Aw2, Bw, Xw, s


def wino_absum(x, w, b):
    """A_wino alone (wino_sums()[0]): the yardstick of nerr_rms for the Winograd kernels."""
    U = np.abs(np.einsum("ik,ockl,jl->ocij", _G, np.asarray(w, np.float64), _G))
    V = np.abs(np.einsum("ik,ncabkl,jl->ncabij", _BT, _tiles(np.asarray(x, np.float64)), _BT))
    aA = np.abs(_AT)
    M = np.einsum("ik,noabkl,jl->noabij", aA, np.einsum("ocij,ncabij->noabij", U, V), aA)
    return _untile(M, x.shape[2], x.shape[3]) + np.abs(np.asarray(b, np.float64))[None, :, None, None]


def wino_exp(w):
    """pack_wino_f16's s: max |U| 2^s in [2^13, 2^14) (0 for an all-zero filter)."""
    mx = float(np.max(np.abs(np.einsum("ik,ockl,jl->ocij", _G, np.asarray(w, np.float64), _G))))
    return 0 if mx == 0.0 else 14 - int(np.frexp(mx)[1])


def bound_wino(x, w, b, slope=None, act="none"):
    cin = w.shape[1]
    Aw, Aw2, _, _, _ = wino_sums(x, w, b)
    return act_factor(slope, act) * (gamma(2 * cin + 7) * Aw + gamma(2) * (1 + 2.0 ** -10) * Aw2)


def bound_wino2(x, w, b, slope=None, act="none", sums=None):
    """sums: wino_sums(x, w, b) where the caller has it."""
    cin = w.shape[1]
    Aw, Aw2, Bw, Xw, s = wino_sums(x, w, b) if sums is None else sums
    e = (gamma(3 * cin + 7) * (1 + 2.0 ** -9) * Aw + C_S * 2.0 ** -21 * Aw + gamma(2) * (1 + 2.0 ** -10) * Aw2 +
         C_U * 2.0 ** -25 * (Bw + np.ldexp(1.0, -s) * Xw))
    return act_factor(slope, act) * e


# ---- emulations (the reference arithmetic alone must pass its own bound) --------------------

def _im2col(x, ks):
    """[n, cin, h, w] -> [cin * ks * ks, n * h * w] float32, k = (ci, ky, kx) as OIHW filters."""
    x = np.asarray(x, np.float32)
    n, c, h, w = x.shape
    p = ks // 2
    xp = np.zeros((n, c, h + 2 * p, w + 2 * p), np.float32)
    xp[:, :, p:p + h, p:p + w] = x
    cols = np.empty((c, ks, ks, n, h, w), np.float32)
    for ky in range(ks):
        for kx in range(ks):
            cols[:, ky, kx] = xp[:, :, ky:ky + h, kx:kx + w].transpose(1, 0, 2, 3)
    return cols.reshape(c * ks * ks, n * h * w)


def _epilogue(acc, scale_inv, b, slope, act, shape):
    n, cout, h, w = shape
    v = (acc * np.float32(scale_inv) + np.asarray(b, np.float32)[:, None]).astype(np.float32)
    v = v.reshape(cout, n, h, w).transpose(1, 0, 2, 3)
    if act == "relu":
        v = np.maximum(v, np.float32(0))
    elif act == "prelu":
        v = np.where(v >= 0, v, v * np.asarray(slope, np.float32)[None, :, None, None]).astype(np.float32)
    return np.ascontiguousarray(v, np.float32)


# A mutant of the emulations: the arithmetic with one lo product removed or altered in one place,
# as a K-loop rewrite loses or mixes up a fragment.  "hi lo" is (filter hi) x (activation lo):
# wh xl, Uh Vl; "lo hi" is wl xh, Ul Vh.
#   drop_hl / drop_lh   the product is left out
#   one_term            both lo products are left out (what is left there is the one-term sum)
#   stale_lo            the filters' lo fragment of chunk pair k (16 channels) is that of pair k - 1
#                       (a filter register set that was not reloaded); pair 0 keeps its own
# restricted to the input channels ci = (from, to), the output channels co = (from, to), one
# Winograd GEMM xi = 4 i + j (emu_wino2) or one filter tap = ky ks + kx (emu_x3); None: everywhere.
MUTANT_KINDS = ("drop_hl", "drop_lh", "one_term", "stale_lo")
ORDERS = ("inorder", "shuffled", "tree16")


def lo_mutant(kind, ci=None, co=None, xi=None, tap=None):
    assert kind in MUTANT_KINDS
    return dict(kind=kind, ci=ci, co=co, xi=xi, tap=tap)


def _mutant_filters(m, Fh, Fl, inner):
    """(the hi filters of the hi lo product, the lo filters of the lo hi product) of a mutant;
    Fh, Fl [cout, cin, a, a], inner the (i, j) the mutant is restricted to or None."""
    hit = np.zeros(Fh.shape, bool)
    co = slice(None) if m["co"] is None else slice(*m["co"])
    ci = slice(None) if m["ci"] is None else slice(*m["ci"])
    hit[(co, ci) + ((slice(None), slice(None)) if inner is None else inner)] = True
    assert hit.any()
    zero = np.float32(0)
    Fh_hl = np.where(hit, zero, Fh) if m["kind"] in ("drop_hl", "one_term") else Fh
    Fl_lh = np.where(hit, zero, Fl) if m["kind"] in ("drop_lh", "one_term") else Fl
    if m["kind"] == "stale_lo":
        stale = Fl.copy()
        stale[:, 16:] = Fl[:, :-16]
        Fl_lh = np.where(hit, stale, Fl)
    return Fh_hl, Fl_lh


def _tree(P):
    """The pairwise sum over axis 0 in float32 (an odd one out moves up a level unchanged)."""
    while P.shape[0] > 1:
        half = P.shape[0] // 2
        head = P[0:2 * half:2] + P[1:2 * half:2]
        P = head if P.shape[0] % 2 == 0 else np.concatenate([head, P[-1:]])
    return P[0]


def emu_x3(x, w, b, slope=None, act="none", seed=0, terms=3, mutant=None, order="shuffled", s=None):
    """The split arithmetic in numpy: fp16 hi / lo of x, fp16 hi / lo of w 2^s, the three exact
    products of every (tap, channel) added one by one into a float32 accumulator in a shuffled
    order, the epilogue's 2^-s, bias and activation in float32.  terms=1: the one-term mode.
    mutant: a lo_mutant() (three terms).  order: "shuffled" (by seed), "inorder" (k = (ci, ky, kx),
    hi hi, lo hi, hi lo of each), "tree16" (the products of 16 channels summed pairwise, the
    blocks' sums added in order: a matrix core's step).  s: the filters' exponent where it is not
    that of w (a subset of a layer's output channels)."""
    assert order in ORDERS and (mutant is None or terms == 3)
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    n, cin, h, wd = x.shape
    cout, ks = w.shape[0], w.shape[2]
    s = pack_exp(w) if s is None else s
    ws = np.ldexp(w, s).astype(np.float32).reshape(cout, -1)
    wh = f16(ws)
    wl = f16(ws - wh)
    X = _im2col(x, ks)
    xh = f16(X)
    xl = f16(X - xh)
    wh_hl, wl_lh = wh, wl
    if mutant is not None:
        tap = None if mutant["tap"] is None else divmod(mutant["tap"], ks)
        wh_hl, wl_lh = (f.reshape(cout, -1) for f in _mutant_filters(
            mutant, wh.reshape(w.shape), wl.reshape(w.shape), tap))
    ops = [(wh, xh)] if terms == 1 else [(wh, xh), (wl_lh, xh), (wh_hl, xl)]
    acc = np.zeros((cout, X.shape[1]), np.float32)
    if order == "tree16":
        kk = ks * ks
        for c0 in range(0, cin, 16):
            ksel = range(c0 * kk, min(c0 + 16, cin) * kk)
            acc += _tree(np.stack([a[:, k, None] * v[None, k, :] for k in ksel for a, v in ops]))
        return _epilogue(acc, np.ldexp(1.0, -s), b, slope, act, (n, cout, h, wd))
    seq = [(k, t) for k in range(X.shape[0]) for t in range(len(ops))]
    if order == "shuffled":
        np.random.default_rng(seed).shuffle(seq)
    for k, t in seq:
        a, v = ops[t]
        acc += a[:, k, None] * v[None, k, :]      # the product is exact in fp32, the += rounds
    return _epilogue(acc, np.ldexp(1.0, -s), b, slope, act, (n, cout, h, wd))


def emu_wino32(x, w, b, slope=None, act="none"):
    """F(2x2, 3x3) restated in float32: U from float64 rounded once, V, M and Y in float32."""
    x = np.asarray(x, np.float32)
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    U = np.einsum("ik,ockl,jl->ocij", _G, np.asarray(w, np.float64), _G).astype(np.float32)
    d = _tiles(x, np.float32)
    bt = _BT.astype(np.float32)
    t = np.zeros(d.shape, np.float32)
    for i in range(4):                                   # rows of B^T have two nonzeros
        (r0, r1) = np.nonzero(bt[i])[0]
        t[..., i, :] = bt[i, r0] * d[..., r0, :] + bt[i, r1] * d[..., r1, :]
    V = np.zeros(d.shape, np.float32)
    for j in range(4):
        (r0, r1) = np.nonzero(bt[j])[0]
        V[..., j] = bt[j, r0] * t[..., r0] + bt[j, r1] * t[..., r1]
    M = np.zeros((n, cout) + d.shape[2:], np.float32)
    for c in range(cin):
        M += U[None, :, c, None, None] * V[:, None, c]
    at = _AT.astype(np.float32)
    t2 = np.zeros(M.shape[:4] + (2, 4), np.float32)
    for i in range(2):
        t2[..., i, :] = ((at[i, 0] * M[..., 0, :] + at[i, 1] * M[..., 1, :]) + at[i, 2] * M[..., 2, :]) + at[i, 3] * M[..., 3, :]
    Y = np.zeros(M.shape[:4] + (2, 2), np.float32)
    for j in range(2):
        Y[..., j] = ((at[j, 0] * t2[..., 0] + at[j, 1] * t2[..., 1]) + at[j, 2] * t2[..., 2]) + at[j, 3] * t2[..., 3]
    y = _untile(Y, h, wd)
    acc = y.transpose(1, 0, 2, 3).reshape(cout, -1)
    return _epilogue(acc, 1.0, b, slope, act, (n, cout, h, wd))


GUARD_CHECKS = ("pre_and_stored", "stored_only")


def emu_wino2(x, w, b, slope=None, act="none", terms=3, check="pre_and_stored", mutant=None, order="inorder", seed=0,
              s=None):
    """csrc/wino_f16.hip in numpy, returning (y, flag).  U = G g G^T in float64, x 2^s, rounded to
    fp32, hi = fp16(U), lo = fp16(U - hi) (pack_wino_f16).  V = B^T d B in fp32, rows then columns,
    then split as split_dw does: hi = fp16(V) by RNE, which overflows to +-inf from |V| >= 65520, and
    lo = fp16(V - fp32(hi)), -+inf then.  M = sum_ci of the exact products Uh Vh + Uh Vl + Ul Vh
    (terms=1: Uh Vh alone) accumulated in fp32, Y = A^T M A in the epilogue's order, x 2^-s, + bias,
    the activation as the kernel writes it (v > 0 ? v : 0 -- a NaN becomes 0).
    check: where the range test sits.  "pre_and_stored": a non-finite value before the activation
    or a stored |v| outside [0, 65504) raises the flag (the kernel); "stored_only": the stored
    value alone (the kernel before the ReLU hole was closed: GUARD_MUTATIONS).
    mutant, order, seed, s: as emu_x3 has them; the default order is the channels' own, with
    Uh Vh, Uh Vl, Ul Vh of each."""
    assert check in GUARD_CHECKS and terms in (1, 3) and order in ORDERS and (mutant is None or terms == 3)
    x = np.asarray(x, np.float32)
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    U = np.einsum("ik,ockl,jl->ocij", _G, np.asarray(w, np.float64), _G)
    mx = float(np.max(np.abs(U)))
    if s is None:
        s = 0 if mx == 0.0 else 14 - int(np.frexp(mx)[1])
    Us = np.ldexp(U, s).astype(np.float32)
    Uh = f16(Us)
    Ul = f16(Us - Uh)
    Uh_hl, Ul_lh = Uh, Ul
    if mutant is not None:
        Uh_hl, Ul_lh = _mutant_filters(mutant, Uh, Ul, None if mutant["xi"] is None else divmod(mutant["xi"], 4))
    d = _tiles(x, np.float32)
    bt = _BT.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.zeros(d.shape, np.float32)
        for i in range(4):
            (r0, r1) = np.nonzero(bt[i])[0]
            t[..., i, :] = bt[i, r0] * d[..., r0, :] + bt[i, r1] * d[..., r1, :]
        V = np.zeros(d.shape, np.float32)
        for j in range(4):
            (r0, r1) = np.nonzero(bt[j])[0]
            V[..., j] = bt[j, r0] * t[..., r0] + bt[j, r1] * t[..., r1]
        Vh = f16(V)                                      # +-inf from |V| >= 65520
        Vl = f16(V - Vh)                                 # -+inf beside an infinite hi
        M = np.zeros((n, cout) + d.shape[2:], np.float32)
        ops = [(Uh, Vh)] if terms == 1 else [(Uh, Vh), (Uh_hl, Vl), (Ul_lh, Vh)]
        if order == "tree16":
            for c0 in range(0, cin, 16):
                M += _tree(np.stack([a[None, :, c, None, None] * v[:, None, c]
                                     for c in range(c0, min(c0 + 16, cin)) for a, v in ops]))
        else:
            seq = [(c, t) for c in range(cin) for t in range(len(ops))]
            if order == "shuffled":
                np.random.default_rng(seed).shuffle(seq)
            for c, t in seq:
                a, v = ops[t]
                M += a[None, :, c, None, None] * v[:, None, c]
        R0 = (M[..., 0, :] + M[..., 1, :]) + M[..., 2, :]
        R1 = (M[..., 1, :] - M[..., 2, :]) - M[..., 3, :]
        Y = np.empty(M.shape[:4] + (2, 2), np.float32)
        for i, R in enumerate((R0, R1)):
            Y[..., i, 0] = (R[..., 0] + R[..., 1]) + R[..., 2]
            Y[..., i, 1] = (R[..., 1] - R[..., 2]) - R[..., 3]
        pre = (_untile(Y, h, wd) * np.float32(np.ldexp(1.0, -s))).astype(np.float32)
        pre = (pre + np.asarray(b, np.float32)[None, :, None, None]).astype(np.float32)
        if act == "relu":
            y = np.where(pre > 0, pre, np.float32(0))
        elif act == "prelu":
            y = np.where(pre >= 0, pre, pre * np.asarray(slope, np.float32)[None, :, None, None])
        else:
            y = pre
        y = np.ascontiguousarray(y, np.float32)
        flag = not bool(np.all(np.abs(y) < F16_MAX))
        if check == "pre_and_stored":
            flag = flag or not bool(np.all(np.isfinite(pre)))
    return y, int(flag)


# ---- inputs ---------------------------------------------------------------------------------

FAMILIES = ("uniform", "postact", "small", "nearrange")
NEAR_SPIKE = 16384.0
PLATEAU_WHERE = ("interior", "row_end", "last")


def plateau_tile(shape, where):
    """(frame, channel, ty, tx) of the Winograd tile a plateau sits in.  interior: the middle tile of
    frame 0; row_end: the last tile of a middle tile row (W odd: the half-empty edge tile, whose
    second inner column is outside the image); last: in the last frame, the last tile in row-major
    order whose inner 2x2 has at least two pixels inside the image (H and W odd: the corner tile
    holds one pixel, which alone cannot carry an overflowing V below 65504)."""
    n, c, h, w = shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    if where == "interior":
        return 0, c // 2, th // 2, tw // 2
    if where == "row_end":
        return 0, c // 2, th // 2, tw - 1
    if where == "last":
        tx = tw - 2 if (h % 2 and w % 2) else tw - 1
        return n - 1, c - 1, th - 1, tx
    raise ValueError(where)


def make_x(family, shape, rng, P=None, where=None):
    """The input families: uniform(-1, 1); post-activation-like (non-negative, sparse, one whole
    channel zero, signed zeros); small magnitudes (1e-5 .. 1e-3, either sign), where the fp16 lo
    halves -- below 6.1e-5 the hi halves too -- are subnormal; near the range: uniform(-1, 1) with
    one activation of 16384 at the last pixel of the last channel of the last frame, which
    peak_weights() turns into one output near +-65504.
    plateau(P, where): uniform(-1, 1) with the inner 2x2 of one Winograd tile (image rows 2 ty,
    2 ty + 1, columns 2 tx, 2 tx + 1 of one channel; plateau_tile) set so that the tile's
    V[1][1] = d11 + d12 + d21 + d22 is 4 P exactly: P on each of the four pixels, and where the
    image's edge clips the patch to two pixels (a half-empty edge tile), 2 P on each.  Every input
    stays below 65504; only V = 4 P can leave the fp16 range."""
    if family == "plateau":
        x = rng.uniform(-1, 1, shape).astype(np.float32)
        f, c, ty, tx = plateau_tile(shape, where)
        patch = x[f, c, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2]          # a view, clipped by the image
        assert patch.size in (2, 4) and 4.0 * P / patch.size < F16_MAX
        patch[...] = np.float32(4.0 * P / patch.size)
        return x
    if family == "uniform":
        return rng.uniform(-1, 1, shape).astype(np.float32)
    if family == "postact":
        x = np.maximum(rng.standard_normal(shape), 0) * (rng.uniform(size=shape) < 0.6)
        x = x.astype(np.float32)
        x[:, shape[1] // 2] = 0.0
        x[x == 0] = np.where(rng.uniform(size=int((x == 0).sum())) < 0.5, -0.0, 0.0).astype(np.float32)
        return x
    if family == "nearrange":
        x = rng.uniform(-1, 1, shape).astype(np.float32)
        x[-1, -1, -1, -1] = NEAR_SPIKE
        return x
    if family == "small":
        return (10.0 ** rng.uniform(-5, -3, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    raise ValueError(family)


def make_layer(cin, cout, ks, rng, bias=True):
    """Filters ~ N(0, 1 / K), bias uniform(-0.1, 0.1), PReLU slopes with negative, zero and > 1
    entries."""
    w = (rng.standard_normal((cout, cin, ks, ks)) / np.sqrt(cin * ks * ks)).astype(np.float32)
    b = (rng.uniform(-0.1, 0.1, cout) if bias else np.zeros(cout)).astype(np.float32)
    s = rng.uniform(0.05, 0.25, cout).astype(np.float32)
    s[0] = -0.5
    if cout > 1:
        s[cout - 1] = 0.0
    if cout > 2:
        s[cout // 2] = 1.75
    return w, b, s


def peak_weights(x, w, b, peak):
    """The filters with the centre tap of (last output channel, last input channel) set so that the
    last pixel of the last frame's last channel is `peak` before the activation (x carries
    NEAR_SPIKE there: the near-range family); every other output stays far below 65504."""
    w = np.array(w, np.float32)
    co, ci, p = w.shape[0] - 1, w.shape[1] - 1, w.shape[2] // 2
    w[co, ci, p, p] = 0.0
    base = conv64(x[-1:], w[co:co + 1], b[co:co + 1])[0, 0, -1, -1]
    w[co, ci, p, p] = (peak - base) / float(x[-1, ci, -1, -1])
    return w


def old_bar(y, ref):
    """The whole-net comparison: max |d| / max |ref|, one number per tensor (bar: < 1e-4)."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(y - ref)) / max(float(np.max(np.abs(ref))), 1e-30))


def worst(y, ref, bound):
    """max |y - ref| / bound over the elements (<= 1 passes), and where it is."""
    d = np.abs(np.asarray(y, np.float64) - ref)
    bound = np.broadcast_to(bound, d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)             # a NaN in y is no pass
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(v) for v in i)


# ---- the sharp statistic: the rms of the normalised error ------------------------------------
# worst() against a gamma(3 K) bound grows blind with K (the docstring of test_conv_ref.py's
# deep-K tests has the figures); the rms over a tensor of d / A is flat in K for the honest
# arithmetic and moves 15 to 1000 times when one lo product is lost.

NERR_GROUP = 32       # output channels per group: wino_f16's epilogue round, conv_x3's narrowest tile
NERR_FACTOR = 3.0     # the bar is NERR_FACTOR x the emulation's own pooled figure (yardstick)


def nerr_rms(y, ref, A, act_fac=1.0, groups=NERR_GROUP):
    """The root mean square of |y - ref| / (act_fac A), in float64, per (frame, `groups`
    consecutive output channels): [n, ceil(cout / groups)].  groups=None: one number for the
    whole tensor.  A is absum() for the direct-form kernels and A_wino (wino_absum) for the
    Winograd ones.  Elements with A == 0 are left out of the mean and must have d == 0; one that
    has not, or a NaN in y, makes its group infinite."""
    y = np.asarray(y, np.float64)
    d = np.abs(y - ref)
    A = np.broadcast_to(np.asarray(A, np.float64), d.shape)
    fac = np.broadcast_to(np.asarray(act_fac, np.float64), d.shape)
    live = A > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(live, d / (fac * A), 0.0) ** 2
    bad = np.isnan(y) | (~live & (d != 0))

    def rms(sl):
        if bool(bad[sl].any()) or not bool(np.all(np.isfinite(q[sl]))):
            return np.inf
        return float(np.sqrt(q[sl].sum() / max(int(live[sl].sum()), 1)))
    if groups is None:
        return rms(np.s_[:])
    n, c = d.shape[:2]
    return np.array([[rms(np.s_[f, g:g + groups]) for g in range(0, c, groups)] for f in range(n)])


def yardstick_channels(cout):
    """The output channels the yardstick is computed on: the first 16 and the last 16."""
    return np.unique(np.r_[0:min(16, cout), max(0, cout - 16):cout])


def yardstick(kernel, x, w, b, slope=None, act="none"):
    """E: the pooled nerr_rms of the reference arithmetic itself -- emu_wino2 for "wino2", emu_x3
    for "x3" and "rgb" -- on the first frame and yardstick_channels() of a case's inputs, with the
    whole layer's filter exponent.  Every group of a kernel's output is held to NERR_FACTOR x E."""
    sel = yardstick_channels(w.shape[0])
    x1, ws, bs = x[:1], w[sel], np.asarray(b)[sel]
    ss = None if slope is None else np.asarray(slope)[sel]
    if kernel == "wino2":
        y, A = emu_wino2(x1, ws, bs, ss, act, s=wino_exp(w))[0], wino_absum(x1, ws, bs)
    else:
        y, A = emu_x3(x1, ws, bs, ss, act, s=pack_exp(w)), absum(x1, ws, bs)
    return nerr_rms(y, ref64(x1, ws, bs, ss, None, act), A, act_factor(ss, act), None)


# ---- mutations: references that are wrong in one local way ----------------------------------

def mutate(kind, x, w, b, slope, act, tile=128):
    """A float64 result computed wrongly in one local way, as a kernel bug would."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, cin, h, wd = x.shape
    cout, ks = w.shape[0], w.shape[2]
    p = ks // 2
    pre = conv64(x, w, b)
    if kind == "corner_tap":            # one tap dropped at one corner pixel of the last frame
        pre[n - 1, :, h - 1, wd - 1] -= w64[:, :, p, p] @ x64[n - 1, :, h - 1, wd - 1]
    elif kind == "chunk_pair":          # the last chunk pair (16 channels) skipped for one channel
        c0 = max(0, (cin - 1) // 16 * 16)
        co = cout // 2
        pre[:, co] -= conv64(x[:, c0:], w[co:co + 1, c0:], None)[:, 0]
    elif kind == "swap_channels":       # two channels of an 8-chunk swapped
        a, c = min(1, cout - 1), min(5, cout - 1) if cout > 1 else 0
        pre[:, [a, c]] = pre[:, [c, a]]
    elif kind == "tile_tail":           # the last pixel of the first tile taken from the next row
        m = min(tile, h * wd) - 1
        yy, xx = divmod(m, wd)
        pre[:, :, yy, xx] = pre[:, :, min(yy + 1, h - 1), xx] if yy + 1 < h else pre[:, :, yy - 1, xx]
    elif kind == "bias_last":           # bias missing on channel cout - 1
        pre[:, cout - 1] -= np.float64(b[cout - 1])
    elif kind == "slope_neighbour":     # PReLU slope of the neighbouring channel
        assert act == "prelu"
        return activate(pre, np.roll(np.asarray(slope, np.float64), 1), act)
    else:
        raise ValueError(kind)
    return activate(pre, slope, act)


MUTATIONS = ("corner_tap", "chunk_pair", "swap_channels", "tile_tail", "bias_last", "slope_neighbour")

# The seventh mutation is one of the range guard, not of the values: emu_wino2's check put behind
# the activation alone ("stored_only").  With a ReLU an overflowed V (NaN in every output of its
# tile) is stored as 0 and the flag stays clear: the layer is wrong and says nothing.
GUARD_MUTATIONS = ("stored_only",)
