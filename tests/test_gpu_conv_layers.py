"""Every conv kernel, one layer at a time, through rt.debug_conv (isl_debug_conv): each case is
built to reach one variant of the dispatch and is held to
  a) the elementwise float64 bound of tests/_conv_ref.py,
  b) no write outside (frame interior) x [out_coff, out_coff + cout) -- the output buffer is filled
     with a canary, the input's foreign chunks with NaN,
  c) the same bits run to run,
  d) the last frame alone giving the bits it has in the batch, where the source promises it
     (canonical K ranges, kernels with one order at every batch size),
  e) the variant code the case was built to reach (dispatch depends on the 256 CUs),
  f) the range guard: a layer is within its bound or raises the flag -- at an output
     (test_range_guard), at an intermediate while every input and output is in range
     (test_range_guard_transform: the Winograd input transform), and on in-contract inputs of
     large magnitude for one case per kernel family (test_flag_or_bound),
  g) the sharp statistic, for the three-term form of every x3, rgb and wino2 case: the rms of
     |d| / A (A_wino for wino2) over each (frame, 32 output channels) is at most 3 E, E being the
     same figure of the numpy emulation of that arithmetic on the case's own inputs
     (cr.yardstick).  The bound of (a) carries gamma(3 K) and goes blind with K: a kernel that
     loses one of its three products passes it from K ~ 1000 on.  This one is flat in K (CPU proof:
     tests/test_conv_ref.py); the deep cases (wino2-c128 .. c512, union-k2304, pairs2-k512) put
     it at the depths the nets run.  The one-term and fp16-storage forms are exempt (their
     references isolate the summation already), direct and wino are the fp32 controls.
Runs on an MI355X only (-m gpu)."""
import contextlib
import os

import numpy as np
import pytest

import _conv_ref as cr
from islpose import runtime as rt

pytestmark = pytest.mark.gpu

C180 = [(0, 0, 52), (56, 52, 128)]                    # 52 PAF channels in a 56-channel slot + 128 features
COCO = [(0, 0, 38), (40, 38, 19), (64, 57, 128)]      # 38 PAF + 19 heat + 128 features: c185 in 192
HAND = [(0, 0, 22), (24, 22, 128)]                    # 22 heat + 128 features: c150 in 152


def vname(code):
    """A variant code as a name: kernel size, tile pixels and channels, then the variant bits."""
    d = rt.decode_variant(code)
    if not d:
        return "none"
    var = d["var"]
    bits = [("union", d["union"]), ("ranged", d["ranged"]), ("split", d["split"]), ("pairs2", d["pairs2"]),
            ("vin", d["vin"]), ("sib", d["sib"]), ("g2", d["g2"]), ("half", bool(var & 256)), ("deep", bool(var & 128)),
            ("wr", d["wave_ranges"]), ("rgb", d["rgb"]), ("w2", d["wino2"]), ("f16", d["f16"]), ("a16", d["act16"])]
    return ".".join(["k%d" % d["ks"], "p%d" % d["bpx"], "c%d" % d["bco"]] + [n for n, on in bits if on])


def case(name, variant, ks, cin, cout, n, h, w, *, kernel="x3", act="prelu", family="uniform", lone=False, env=None,
         forms=("",), data=None, **kw):
    """data: the case whose inputs this one shares (the other side of a switch)."""
    return dict(name=name, variant=variant, ks=ks, cin=cin, cout=cout, n=n, h=h, w=w, kernel=kernel, act=act,
                family=family, lone=lone, env=env or {}, forms=forms, data=data or name, kw=kw)


ALL3 = ("", "f16", "a16")
# name, the variant it is built to reach (three-term name), ks, cin, cout, n, h, w.  Grids: 256 CUs.
CASES = [
    # -- the 512-pixel family: n * ceil(hw / 512) * channel tiles >= 256
    case("union-c128", "k3.p512.c128.union", 3, 16, 128, 128, 33, 31, forms=ALL3),        # 1023 px: a 511-pixel tail tile
    case("big-c96", "k3.p512.c96", 3, 24, 96, 64, 8, 200, act="relu", forms=ALL3),                    # rows too long for the union run
    case("big-k1-c32", "k1.p512.c32", 1, 16, 26, 128, 23, 41, act="none", in_pad=3, out_pad=3, forms=ALL3),
    case("half64", "k3.p256.c64", 3, 16, 64, 37, 8, 200, forms=ALL3),                     # 7 tiles x 37 = 259 blocks
    case("wide1-pairs2", "k1.p256.c256.pairs2", 1, 32, 256, 128, 16, 17, forms=ALL3),     # 272 px: 2 tiles
    # two rounds of blocks: the last round on 256-pixel tail tiles (x3_tail_plan)
    case("tail-k1", "k1.p512.c32", 1, 16, 26, 64, 40, 65, act="relu", forms=ALL3),
    case("tail-union-c19", "k3.p512.c32.union", 3, 16, 19, 64, 40, 65, forms=ALL3),
    # -- the 128-pixel family, plain loops: small grids, no K ranges
    case("s-k1-c26", "k1.p128.c32", 1, 16, 26, 2, 9, 13, forms=ALL3, lone=True, family="postact"),
    case("s-k1-small", "k1.p128.c32", 1, 16, 26, 2, 9, 13, lone=True, family="small", act="none"),   # K = 16: the 2^-25 B' term leads
    case("s-k1-c52-hand", "k1.p128.c64", 1, 150, 52, 2, 9, 13, segs=HAND, lone=True, forms=ALL3),
    case("s-k1-c96", "k1.p128.c96", 1, 24, 96, 2, 9, 13, lone=True, in_coff=8, in_cs=48, act="relu", forms=ALL3),
    case("s-k1-c128", "k1.p128.c128", 1, 8, 128, 3, 8, 16, lone=True, forms=ALL3),                      # one chunk; 128 px: a full tile
    case("s-k3-c38", "k3.p128.c64", 3, 40, 38, 2, 9, 13, forms=ALL3, lone=True, out_coff=16, out_cs=64, in_pad=3),
    case("s-k3-c19", "k3.p128.c32", 3, 24, 19, 2, 7, 11, lone=True, out_coff=40, out_cs=64, out_pad=3, family="small"),
    case("s-k3-c1", "k3.p128.c32", 3, 16, 1, 2, 9, 13, lone=True, act="none", forms=ALL3),
    case("s-k3-w1", "k3.p128.c32", 3, 16, 22, 2, 37, 1, lone=True),                       # W = 1: tile_pixels shrinks the tile
    case("s-k3-w5", "k3.p128.c64", 3, 16, 52, 2, 27, 5, lone=True),                       # W < 8; 135 px: one above a tile
    case("s-k7-c22", "k7.p128.c32", 7, 16, 22, 2, 9, 9, forms=ALL3, lone=True, family="postact"),
    case("s-k7-w3", "k7.p128.c32", 7, 8, 22, 2, 43, 3, lone=True, act="relu"),            # 129 px: one above a tile
    # -- its other loops
    case("halfsmall", "k3.p128.c64.half", 3, 16, 128, 1, 9, 13, forms=ALL3),
    case("halfsmall-off-deep", "k3.p128.c128.deep", 3, 16, 128, 1, 9, 13, env={"ISLPOSE_X3_HALFSMALL": "0"}, forms=ALL3, data="halfsmall"),
    case("halfsmall-off-plain", "k3.p128.c128", 3, 16, 128, 1, 9, 13,
         env={"ISLPOSE_X3_HALFSMALL": "0", "ISLPOSE_X3_DEEP": "0"}, data="halfsmall", forms=ALL3),
    case("deep-c96", "k3.p128.c96.deep", 3, 24, 96, 2, 9, 13, lone=True, forms=ALL3),
    # -- canonical K ranges (allow_split, <= 1024 px): in one block on big grids, across blocks on small
    case("g2", "k3.p128.c128.ranged.g2", 3, 180, 128, 32, 23, 41, segs=C180, allow_split=True, lone=True, forms=ALL3),
    case("g2-off-deep", "k3.p128.c128.ranged.deep", 3, 180, 128, 32, 23, 41, segs=C180, allow_split=True, lone=True,
         env={"ISLPOSE_X3_G2": "0"}, data="g2", forms=ALL3),
    case("g2-off-plain", "k3.p128.c128.ranged", 3, 180, 128, 32, 23, 41, segs=C180, allow_split=True, lone=True,
         env={"ISLPOSE_X3_G2": "0", "ISLPOSE_X3_DEEP": "0"}, data="g2", forms=ALL3),
    case("ranged-k1-c96", "k1.p128.c96.ranged", 1, 128, 96, 32, 23, 41, allow_split=True, lone=True, forms=ALL3),
    case("hw1024-ranged", "k3.p128.c64.ranged", 3, 64, 52, 32, 32, 32, allow_split=True, lone=True, forms=ALL3),   # at the threshold
    case("hw1025-unranged", "k3.p512.c64.union", 3, 64, 52, 86, 25, 41, allow_split=True, in_pad=3, forms=ALL3),   # one above it
    case("wr", "k3.p32.c32.ranged.wr", 3, 64, 26, 2, 9, 13, allow_split=True, lone=True, forms=("", "f16"), in_coff=8, in_cs=80,
         out_coff=8, out_cs=48),
    case("wr-k1", "k1.p32.c32.ranged.wr", 1, 128, 38, 1, 23, 41, allow_split=True, forms=("", "f16")),
    case("split-c64", "k3.p128.c64.split", 3, 160, 52, 2, 9, 13, allow_split=True, lone=True, forms=("", "f16"), in_pad=3,
         out_pad=3),
    case("split-halfco", "k3.p64.c64.split.half", 3, 180, 128, 1, 23, 41, segs=C180, allow_split=True, forms=("", "f16")),
    case("split-halfco-px128", "k3.p128.c64.split.half", 3, 180, 128, 1, 23, 41, segs=C180, allow_split=True,
         env={"ISLPOSE_X3_PX64": "0"}, data="split-halfco", forms=("", "f16")),
    case("split-px64-c96", "k3.p64.c96.split", 3, 64, 96, 2, 9, 13, allow_split=True, env={"ISLPOSE_X3_WR": "0"}, lone=True,
         forms=("", "f16")),
    case("split-px128-c96", "k3.p128.c96.split", 3, 64, 96, 2, 9, 13, allow_split=True,
         env={"ISLPOSE_X3_WR": "0", "ISLPOSE_X3_PX64": "0"}, lone=True, data="split-px64-c96", forms=("", "f16")),
    # -- 7x7 with 128-channel tiles: the tile by grid quantisation, the small forms by grid and switch
    case("k7-p128", "k7.p128.c128", 7, 8, 128, 16, 16, 128, act="relu", forms=ALL3),
    case("k7-p256", "k7.p256.c128", 7, 8, 128, 16, 20, 128, forms=ALL3),
    case("k7-p384", "k7.p384.c128.sib", 7, 8, 128, 16, 48, 96, act="relu", forms=ALL3),
    case("small7-deep", "k7.p64.c64.half.deep", 7, 16, 128, 2, 9, 9, forms=ALL3),
    case("small7-plain", "k7.p64.c64.half", 7, 16, 128, 2, 9, 9, env={"ISLPOSE_X3_SMALL7": "1"}, forms=ALL3, data="small7-deep"),
    case("small7-off", "k7.p128.c128", 7, 16, 128, 2, 9, 9, env={"ISLPOSE_X3_SMALL7": "0"}, data="small7-deep", forms=ALL3),
    case("small7-96", "k7.p96.c64.half.deep", 7, 8, 128, 1, 92, 92, forms=("", "f16")),
    case("small7-96-off", "k7.p64.c64.half", 7, 8, 128, 1, 92, 92, env={"ISLPOSE_X3_S7W96": "0"}, data="small7-96", forms=ALL3),
    case("k7-split-coco", "k7.p64.c64.split.half.deep", 7, 185, 128, 1, 9, 9, segs=COCO, allow_split=True, forms=("", "f16")),
    # -- the other kernels
    case("rgb", "k3.p256.c64.rgb", 3, 3, 64, 2, 17, 19, kernel="rgb", act="relu", lone=True, forms=ALL3),
    case("rgb-c26", "k3.p256.c64.rgb", 3, 3, 26, 1, 16, 16, kernel="rgb", out_coff=8, out_cs=48),
    case("wino2-17x63", "k3.p128.c64.w2", 3, 24, 64, 2, 17, 63, kernel="wino2", lone=True),
    case("wino2-19x65", "k3.p128.c64.w2", 3, 40, 128, 2, 19, 65, kernel="wino2", lone=True, out_coff=8, out_cs=144, out_pad=3,
         family="postact"),
    case("wino2-small", "k3.p128.c64.w2", 3, 16, 64, 1, 17, 63, kernel="wino2", family="small", act="none"),
    # -- the depths the nets run (assertion g): the smallest planes launch_wino_f16 takes
    case("wino2-c128", "k3.p128.c64.w2", 3, 128, 256, 2, 17, 63, kernel="wino2", lone=True),   # 4 channel blocks; 288 tiles: a half-full last block
    case("wino2-c180", "k3.p128.c64.w2", 3, 180, 128, 2, 19, 65, kernel="wino2", act="relu", segs=C180),   # 23 chunks: no odd chunk in the last pair; TW = 33
    case("wino2-c256", "k3.p128.c64.w2", 3, 256, 128, 3, 20, 64, kernel="wino2", act="none", out_pad=3),   # whole tiles, bands and blocks: the control
    case("wino2-c384", "k3.p128.c64.w2", 3, 384, 128, 1, 18, 64, kernel="wino2", in_coff=8, in_cs=400, out_coff=128, out_cs=384),   # a slice into a slot; 9 tile rows
    case("wino2-c512", "k3.p128.c64.w2", 3, 512, 192, 1, 17, 63, kernel="wino2", family="postact"),   # 32 pairs; 3 channel blocks
    # ... and of the 512-pixel family: 128 x 2 tiles = 256 blocks, the smallest batch with these planes
    case("union-k2304", "k3.p512.c128.union", 3, 256, 128, 128, 27, 19),                  # 513 px: a one-pixel tail tile
    case("pairs2-k512", "k1.p256.c256.pairs2", 1, 512, 256, 128, 9, 29, act="relu"),      # 261 px: a five-pixel tail tile
    case("direct-k1", "none", 1, 24, 26, 2, 9, 13, kernel="direct"),
    case("direct-k3", "none", 3, 180, 52, 2, 9, 13, kernel="direct", segs=C180, in_coff=16, out_coff=8, out_cs=72),
    case("direct-k7", "none", 7, 16, 128, 2, 9, 9, kernel="direct", act="relu"),
    case("wino-c64", "none", 3, 24, 64, 2, 9, 13, kernel="wino"),
    case("wino-c96", "none", 3, 40, 96, 2, 17, 63, kernel="wino", act="relu", in_pad=3),
]
RUNS = [(c, f) for c in CASES for f in c["forms"]]
RUN_IDS = ["%s%s" % (c["name"], "-" + f if f else "") for c, f in RUNS]


def form_name(variant, form):
    return variant + {"": "", "f16": ".f16", "a16": ".f16.a16"}[form] if variant != "none" else variant


# Every variant of the dispatch this file must keep reaching (the coverage guard), by vname():
# k = kernel size, p = tile pixels, c = tile channels, then union (row union), ranged (in-block K
# ranges), split (split-K + x3_splitk_reduce), pairs2 (two pairs per step), vin (pooled input), sib (one
# input buffer: the 384-pixel 7x7 tiles), g2 (two K groups), half (half-channel blocks), deep (prefetch
# two steps ahead), wr (conv_x3_wr), rgb, w2 (wino_f16), f16 (one-term), a16 (fp16 storage).
COVERED = [
    "k1.p128.c128", "k1.p128.c128.f16", "k1.p128.c128.f16.a16", "k1.p128.c32", "k1.p128.c32.f16",
    "k1.p128.c32.f16.a16", "k1.p128.c64", "k1.p128.c64.f16", "k1.p128.c64.f16.a16", "k1.p128.c96",
    "k1.p128.c96.f16", "k1.p128.c96.f16.a16", "k1.p128.c96.ranged", "k1.p128.c96.ranged.f16",
    "k1.p128.c96.ranged.f16.a16", "k1.p256.c256.pairs2", "k1.p256.c256.pairs2.f16",
    "k1.p256.c256.pairs2.f16.a16", "k1.p32.c32.ranged.wr", "k1.p32.c32.ranged.wr.f16", "k1.p512.c32",
    "k1.p512.c32.f16", "k1.p512.c32.f16.a16", "k3.p128.c128", "k3.p128.c128.deep", "k3.p128.c128.deep.f16",
    "k3.p128.c128.deep.f16.a16", "k3.p128.c128.f16", "k3.p128.c128.f16.a16", "k3.p128.c128.ranged",
    "k3.p128.c128.ranged.deep", "k3.p128.c128.ranged.deep.f16", "k3.p128.c128.ranged.deep.f16.a16",
    "k3.p128.c128.ranged.f16", "k3.p128.c128.ranged.f16.a16", "k3.p128.c128.ranged.g2",
    "k3.p128.c128.ranged.g2.f16", "k3.p128.c128.ranged.g2.f16.a16", "k3.p128.c32", "k3.p128.c32.f16",
    "k3.p128.c32.f16.a16", "k3.p128.c64", "k3.p128.c64.f16", "k3.p128.c64.f16.a16", "k3.p128.c64.half",
    "k3.p128.c64.half.f16", "k3.p128.c64.half.f16.a16", "k3.p128.c64.ranged", "k3.p128.c64.ranged.f16",
    "k3.p128.c64.ranged.f16.a16", "k3.p128.c64.split", "k3.p128.c64.split.f16", "k3.p128.c64.split.half",
    "k3.p128.c64.split.half.f16", "k3.p128.c64.w2", "k3.p128.c96.deep", "k3.p128.c96.deep.f16",
    "k3.p128.c96.deep.f16.a16", "k3.p128.c96.split", "k3.p128.c96.split.f16", "k3.p256.c64", "k3.p256.c64.f16",
    "k3.p256.c64.f16.a16", "k3.p256.c64.rgb", "k3.p256.c64.rgb.f16", "k3.p256.c64.rgb.f16.a16",
    "k3.p256.c64.vin", "k3.p256.c64.vin.f16", "k3.p256.c64.vin.f16.a16", "k3.p32.c32.ranged.wr",
    "k3.p32.c32.ranged.wr.f16", "k3.p512.c128.union", "k3.p512.c128.union.f16", "k3.p512.c128.union.f16.a16",
    "k3.p512.c128.union.vin", "k3.p512.c32.union", "k3.p512.c32.union.f16", "k3.p512.c32.union.f16.a16",
    "k3.p512.c64.union", "k3.p512.c64.union.f16", "k3.p512.c64.union.f16.a16", "k3.p512.c96", "k3.p512.c96.f16",
    "k3.p512.c96.f16.a16", "k3.p64.c64.split.half", "k3.p64.c64.split.half.f16", "k3.p64.c96.split",
    "k3.p64.c96.split.f16", "k7.p128.c128", "k7.p128.c128.f16", "k7.p128.c128.f16.a16", "k7.p128.c32",
    "k7.p128.c32.f16", "k7.p128.c32.f16.a16", "k7.p256.c128", "k7.p256.c128.f16", "k7.p256.c128.f16.a16",
    "k7.p384.c128.sib", "k7.p384.c128.sib.f16", "k7.p384.c128.sib.f16.a16", "k7.p64.c64.half",
    "k7.p64.c64.half.deep", "k7.p64.c64.half.deep.f16", "k7.p64.c64.half.deep.f16.a16", "k7.p64.c64.half.f16",
    "k7.p64.c64.half.f16.a16", "k7.p64.c64.split.half.deep", "k7.p64.c64.split.half.deep.f16",
    "k7.p96.c64.half.deep", "k7.p96.c64.half.deep.f16"]


@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def inputs(c):
    rng = np.random.default_rng(sum(map(ord, c["data"])))
    x = cr.make_x(c["family"], (c["n"], c["cin"], c["h"], c["w"]), rng)
    wt, b, s = cr.make_layer(c["cin"], c["cout"], c["ks"], rng, bias=c["family"] != "small")
    return x, wt, b, s


SHARP = ("x3", "rgb", "wino2")     # the kernels whose three-term form assertion (g) holds to 3 E


def reference(c, form, x, wt, b, s, sharp=None):
    """(ref, bound) of a case in one of its forms.  sharp: a dict that receives what assertion
    (g) needs of a three-term x3, rgb or wino2 case: A (absum, or A_wino for wino2) and the
    yardstick E of the reference arithmetic (cr.yardstick)."""
    k, act = c["kernel"], c["act"]
    if form:                                        # one-term: ref64 of the rounded operands
        xr, wr = cr.f16(x), cr.round_w_f16(wt)
        ref, bound = cr.ref64(xr, wr, b, s, c["ks"], act), cr.bound_f16(xr, wr, b, s, act)
        return (ref, cr.bound_act16(bound, ref)) if form == "a16" else (ref, bound)
    ref = cr.ref64(x, wt, b, s, c["ks"], act)
    if k == "wino2":
        sums = cr.wino_sums(x, wt, b)
        A, bound = sums[0], cr.bound_wino2(x, wt, b, s, act, sums=sums)
    elif k in ("x3", "rgb"):
        A = cr.absum(x, wt, b)
        bound = cr.bound_x3(x, wt, b, s, act, A=A)
    else:
        A, bound = None, {"direct": cr.bound_direct, "wino": cr.bound_wino}[k](x, wt, b, s, act)
    if sharp is not None and k in SHARP:
        sharp.update(A=A, E=cr.yardstick(k, x, wt, b, s if act == "prelu" else None, act))
    return ref, bound


def launch(c, form, x, wt, b, s, **more):
    kw = dict(c["kw"])
    kw.update(more)
    with switches(c["env"]):
        try:
            return rt.debug_conv(x, wt, b, s if c["act"] == "prelu" else None, act=c["act"], kernel=c["kernel"],
                                 f16=bool(form), act16=form == "a16", **kw)
        except rt.IslError as e:
            if "(%d)" % rt.ISL_E_HIP in str(e):      # a HIP error: nothing more of this file runs on the device
                pytest.exit("HIP error in %s: %s" % (c["name"], e), returncode=3)
            raise


REACHED = set()       # the variant names the tests of this file launched
KEPT = {}             # three-term results other tests compare against: name -> DebugConvResult


def case_reference(c, form, x, wt, b, s):
    """(ref, bound, sharp) of a case's form, computed once for the cases that share its inputs
    (the two sides of a switch): the float64 reference is each case's host time."""
    def make():
        sharp = {}
        return reference(c, form, x, wt, b, s, sharp) + (sharp,)
    if sum(o["data"] == c["data"] for o in CASES) == 1:          # nobody to share with: nothing kept
        return make()
    return shared(("layer", c["data"], form, c["kernel"], c["act"]), make)


def run(c, form):
    """A case's runs: the layer twice, the last frame alone, reference and bound."""
    x, wt, b, s = inputs(c)
    a = launch(c, form, x, wt, b, s)
    again = launch(c, form, x, wt, b, s)
    # (K ranges across blocks have no fp16-storage form: the lone frame of such a case runs the
    # one-term form, whose values the fp16-storage form stores rounded)
    lone_form = "f16" if form == "a16" and c["kw"].get("allow_split") else form
    last = launch(c, lone_form, x[-1:], wt, b, s) if c["lone"] and c["n"] > 1 else None
    ref, bound, sharp = case_reference(c, form, x, wt, b, s)
    REACHED.add(vname(a.variant))
    return dict(a=a, again=again, last=last, ref=ref, bound=bound, sharp=sharp, fac=cr.act_factor(s, c["act"]))


def kept(name):
    """The three-term result of a case: what test_layer kept of it, or one launch."""
    if name not in KEPT:
        c = next(c for c in CASES if c["name"] == name)
        KEPT[name] = launch(c, "", *inputs(c))
    return KEPT[name]


def clean(r):
    assert r.stray_writes == 0, "stray writes: %d, the first at %s" % (r.stray_writes, r.stray)
    assert r.unwritten == 0, "%d elements of the footprint never written" % r.unwritten


@pytest.mark.parametrize("c,form", RUNS, ids=RUN_IDS)
def test_layer(c, form):
    r = run(c, form)
    a = r["a"]
    if not form and any(c["name"] in pair for pair in SAME_BITS):
        KEPT[c["name"]] = a
    worst, at = cr.worst(a.y, r["ref"], r["bound"])
    print("%s: variant %s, worst |d| / bound %.4f at %s, max |d| / max |ref| %.3g, stray %d" % (
        c["name"], vname(a.variant), worst, at, cr.old_bar(a.y, r["ref"]), a.stray_writes))
    assert vname(a.variant) == form_name(c["variant"], form)                       # e
    clean(a)                                                                       # b
    assert a.range_flag == 0
    assert worst <= 1.0                                                            # a
    assert np.array_equal(a.y.view(np.uint32), r["again"].y.view(np.uint32))       # c
    if r["last"] is not None:                                                      # d
        clean(r["last"])
        last = cr.f16(r["last"].y) if form == "a16" and not rt.decode_variant(r["last"].variant)["act16"] else r["last"].y
        assert np.array_equal(a.y[-1:].view(np.uint32), last.view(np.uint32))
    if r["sharp"]:                                                                 # g
        E = r["sharp"]["E"]
        groups = cr.nerr_rms(a.y, r["ref"], r["sharp"]["A"], r["fac"])
        f, g = (int(v) for v in np.unravel_index(int(np.argmax(groups)), groups.shape))
        print("%s: largest group nerr_rms %.3e = %.3f of the bar 3 E (E %.3e), frame %d channels %d..%d" % (
            c["name"], groups[f, g], groups[f, g] / max(cr.NERR_FACTOR * E, 1e-300), E, f, cr.NERR_GROUP * g,
            min(cr.NERR_GROUP * (g + 1), c["cout"]) - 1))
        assert np.all(groups <= cr.NERR_FACTOR * E)


# "Same bits" the source states between two sides of a per-launch switch (csrc/conv_x3.hip: the
# half-channel blocks, the 64-pixel tiles, the small 7x7 forms; canonical ranges in one block or
# across blocks, one K group or two).
SAME_BITS = [("halfsmall", "halfsmall-off-plain"), ("g2", "g2-off-plain"), ("g2", "g2-off-deep"),
             ("split-halfco", "split-halfco-px128"), ("split-px64-c96", "split-px128-c96"),
             ("small7-deep", "small7-off"), ("small7-plain", "small7-off"), ("small7-96", "small7-96-off")]


@pytest.mark.parametrize("one,other", SAME_BITS, ids=["%s=%s" % p for p in SAME_BITS])
def test_same_bits_across_switch(one, other):
    a, b = kept(one), kept(other)
    assert a.variant != b.variant
    assert np.array_equal(a.y.view(np.uint32), b.y.view(np.uint32))


def test_canonical_ranges_frame_alone_runs_across_blocks():
    """The g2 case's last frame alone has 8 blocks: its ranges run across blocks (the wave-range
    kernel or split-K), and test_layer held its bits to the in-block sums of the batch."""
    c = next(c for c in CASES if c["name"] == "g2")
    x, wt, b, s = inputs(c)
    d = rt.decode_variant(launch(c, "", x[-1:], wt, b, s).variant)
    assert d["wave_ranges"] or d["split"]


# ---- pools ----------------------------------------------------------------------------------

POOLS = [("pool-half64", 3, 16, 64, 37, 8, 200, "k3.p256.c64"), ("pool-small-oddh", 3, 24, 38, 2, 9, 12, "k3.p128.c64"),
         ("pool-k1", 1, 16, 26, 2, 7, 10, "k1.p128.c32")]


@pytest.mark.parametrize("form", ALL3, ids=["x3", "f16", "a16"])
@pytest.mark.parametrize("p", POOLS, ids=[p[0] for p in POOLS])
def test_fused_pool(p, form):
    """hpool + vpool2 against the pooled reference; and conv -> pool = fused, bit for bit (the
    pair-max epilogue takes the maximum of the values the plain epilogue stores)."""
    name, ks, cin, cout, n, h, w, variant = p
    c = case(name, variant, ks, cin, cout, n, h, w, act="prelu")
    x, wt, b, s = inputs(c)
    ref, bound = reference(c, form, x, wt, b, s)
    plain = launch(c, form, x, wt, b, s)
    fused = launch(c, form, x, wt, b, s, hpool=True)
    again = launch(c, form, x, wt, b, s, hpool=True)
    REACHED.add(vname(fused.variant))
    assert vname(fused.variant) == form_name(variant, form) == vname(plain.variant)
    clean(plain)
    clean(fused)
    wh, _ = cr.worst(fused.y, cr.hpool(ref), cr.hpool(bound))       # a maximum moves by at most its inputs' largest error
    wp, _ = cr.worst(fused.pooled, cr.pool2(ref), cr.pool2(bound))
    print("%s %s: pair-max %.4f, pooled %.4f of the bound" % (name, form or "x3", wh, wp))
    assert wh <= 1.0 and wp <= 1.0
    assert np.array_equal(fused.y.view(np.uint32), cr.hpool(plain.y).view(np.uint32))
    assert np.array_equal(fused.pooled.view(np.uint32), cr.pool2(plain.y).view(np.uint32))
    assert np.array_equal(fused.pooled.view(np.uint32), again.pooled.view(np.uint32))


VINS = [("vin-half64", 16, 64, 37, 8, 200, "k3.p256.c64", ALL3), ("vin-union", 16, 128, 128, 32, 32, "k3.p512.c128.union", ("",))]


def vin_case(v):
    name, cin, cout, n, h, w, variant, _ = v
    return case(name, variant, 3, cin, cout, n, 2 * h, 2 * w, act="prelu", family="postact")


@pytest.mark.parametrize("v,form", [(v, f) for v in VINS for f in v[7]], ids=["%s%s" % (v[0], "-" + f if f else "") for v in VINS for f in v[7]])
def test_pooled_input(v, form):
    """vin: the conv stages from the pool's pair-max buffer.  Against the reference on the pooled
    map, and bit for bit the plain launch on that map (only the staging differs)."""
    name, cin, cout, n, h, w, variant, _ = v
    c = vin_case(v)
    x, wt, b, s = inputs(c)                                         # the pre-pool map
    xp = cr.pool2(x)
    cp = dict(c, h=h, w=w)
    ref, bound = reference(cp, form, xp, wt, b, s)
    got = launch(c, form, x, wt, b, s, vin=True)
    plain = launch(cp, form, xp, wt, b, s)
    REACHED.add(vname(got.variant))
    assert vname(got.variant) == form_name(variant + ".vin", form)
    assert vname(plain.variant) == form_name(variant, form)
    clean(got)
    worst, at = cr.worst(got.y, ref, bound)
    print("%s %s: worst |d| / bound %.4f at %s" % (name, form or "x3", worst, at))
    assert worst <= 1.0
    assert np.array_equal(got.y.view(np.uint32), plain.y.view(np.uint32))


def test_pool_forms_refused_where_the_dispatch_has_none():
    x = np.zeros((1, 16, 10, 11), np.float32)
    wt = np.zeros((26, 16, 3, 3), np.float32)
    b = np.zeros(26, np.float32)
    with pytest.raises(rt.IslError):
        rt.debug_conv(x, wt, b, hpool=True)                          # odd width
    with pytest.raises(rt.IslError):
        rt.debug_conv(np.zeros((1, 16, 20, 20), np.float32), wt, b, vin=True)   # a small grid: x3_vin_ok says no
    with pytest.raises(rt.IslError):
        rt.debug_conv(x, wt, b, f16=True, kernel="wino2")            # the Winograd kernel has no one-term form


# ---- the range guard, per layer -------------------------------------------------------------

RANGE = [("union-c128", ""), ("union-c128", "f16"), ("s-k3-c38", ""), ("s-k3-c38", "a16"), ("wr", ""), ("split-c64", "f16"),
         ("g2", ""), ("small7-deep", ""), ("rgb", ""), ("wino2-17x63", "")]


@pytest.mark.parametrize("name,form", RANGE, ids=["%s%s" % (n, "-" + f if f else "") for n, f in RANGE])
def test_range_guard(name, form):
    """One output -- last frame, last pixel, last channel: the last channel of the last tile --
    at 1.1 x 65504 raises the flag (ISL_E_RANGE when asked for); the same layer peaking at 0.9 x
    65504 does not and is within its bound."""
    c = dict(next(c for c in CASES if c["name"] == name), act="relu")
    c = dict(c, family="nearrange")                  # uniform(-1, 1) with one activation of 16384
    x, w0, b, s = inputs(c)
    for peak, tripped in ((1.1 * cr.F16_MAX, True), (0.9 * cr.F16_MAX, False)):
        wt = cr.peak_weights(x, w0, b, peak)
        ref, bound = reference(c, form, x, wt, b, s)
        assert int((np.abs(ref) >= cr.F16_MAX).sum()) == int(tripped) and abs(ref[-1, -1, -1, -1] / peak - 1) < 1e-2
        r = launch(c, form, x, wt, b, s)
        assert vname(r.variant) == form_name(c["variant"], form)
        assert r.range_flag == int(tripped)
        clean(r)
        if tripped:
            with pytest.raises(rt.IslError, match="fp16 split range"):
                launch(c, form, x, wt, b, s, range_error=True)
        else:
            worst, at = cr.worst(r.y, ref, bound)
            print("%s %s near the range: worst |d| / bound %.4f at %s" % (name, form or "x3", worst, at))
            assert worst <= 1.0


# ---- the range guard inside a layer: the Winograd transform ----------------------------------

def by_name(name):
    return next(c for c in CASES if c["name"] == name)


SHARED = {}           # references shared by the parameters of one test: key -> tuple, never written to


def shared(key, make):
    if key not in SHARED:
        SHARED[key] = make()
    return SHARED[key]


def pre_and_bound(c, x, wt, b, s):
    """(float64 reference before the activation, three-term bound without the activation's
    factor): every bound of _conv_ref is act_factor(slope, act) times the latter."""
    return reference(dict(c, act="none"), "", x, wt, b, s)


# the smallest shapes launch_wino_f16 takes (32 tiles per row, > 1024 pixels); 19 x 65 has the
# half-empty edge tiles.  The entry has one form of this kernel: three terms (asserted below).
TRANSFORM_CASES = ("wino2-17x63", "wino2-19x65")
PLATEAU_OVER, PLATEAU_IN = 16384.0, 16000.0           # V = 4 P = 65536: hi = inf; 64000: a finite split


def plateau_inputs(name, where, n, P):
    c = by_name(name)

    def make():
        rng = np.random.default_rng(sum(map(ord, name + where)) + n)
        x = cr.make_x("plateau", (n, c["cin"], c["h"], c["w"]), rng, P=P, where=where)
        wt, b, s = cr.make_layer(c["cin"], c["cout"], 3, rng)
        return (x, wt, b, s) + pre_and_bound(c, x, wt, b, s)
    return shared(("plateau", name, where, n, P), make)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("where", cr.PLATEAU_WHERE)
@pytest.mark.parametrize("act", cr.ACTS)
@pytest.mark.parametrize("name", TRANSFORM_CASES)
def test_range_guard_transform(name, act, where, n):
    """An intermediate out of range while every input and every true output is in range: a 2x2
    plateau on the inner pixels of one tile makes V[1][1] = 4 P.  P = 16384: V = 65536 splits to
    hi = inf, lo = -inf, every output of the tile is NaN, and the layer must raise the flag --
    with a ReLU too, which stores that NaN as 0.  P = 16000: V = 64000 splits finitely, no flag,
    every element within bound_wino2."""
    c = dict(by_name(name), act=act)
    with pytest.raises(rt.IslError):                 # no one-term form of this kernel to cross with
        rt.debug_conv(np.zeros((1, 8, 17, 63), np.float32), np.zeros((64, 8, 3, 3), np.float32), np.zeros(64, np.float32),
                      f16=True, kernel="wino2")
    for P, tripped in ((PLATEAU_OVER, True), (PLATEAU_IN, False)):
        x, wt, b, s, pre, e = plateau_inputs(name, where, n, P)
        ref, bound = cr.activate(pre, s, act), cr.act_factor(s, act) * e
        assert float(np.max(np.abs(x))) < cr.F16_MAX and float(np.max(np.abs(ref))) < cr.F16_MAX   # only V overflows
        r = launch(c, "", x, wt, b, s)
        REACHED.add(vname(r.variant))
        assert vname(r.variant) == c["variant"]
        worst, at = cr.worst(r.y, ref, bound)
        print("%s %s %s n=%d P=%g: flag %d, worst |d| / bound %.4g at %s, stray %d, unwritten %d" % (
            name, act, where, n, P, r.range_flag, worst, at, r.stray_writes, r.unwritten))
        assert r.range_flag == int(tripped)
        clean(r)
        if tripped:
            with pytest.raises(rt.IslError, match="fp16 split range"):
                launch(c, "", x, wt, b, s, range_error=True)
        else:
            assert worst <= 1.0


# ---- flag or bound: in-contract inputs of large magnitude -----------------------------------

# one case per kernel family, and what the family promises about the flag: the x3 kernels have no
# intermediate above their inputs, so an in-range layer must not flag; the Winograd transform may
# leave the range (V reaches 4 x the input) and then must flag; direct is the fp32 control.
FLAG_OR_BOUND = [("union-c128", "union"), ("s-k3-c38", "plain p128"), ("g2", "ranged g2"), ("wr", "wave ranges"),
                 ("split-c64", "split-K"), ("small7-deep", "small 7x7"), ("rgb", "rgb"), ("wino2-19x65", "wino2"),
                 ("direct-k3", "direct")]


def large_inputs(name):
    """uniform(-1, 1), post-activation-like sparsity (0.6 kept, one channel zero), scaled to
    max |x| = 0.9 x 65504; the filters scaled so that the float64 reference peaks at 0.5 x 65504
    before the activation (a PReLU slope of 1.75 takes that to 0.875 x 65504 at most)."""
    c = by_name(name)

    def make():
        rng = np.random.default_rng(sum(map(ord, "large" + name)))
        shape = (c["n"], c["cin"], c["h"], c["w"])
        x = rng.uniform(-1, 1, shape) * (rng.uniform(size=shape) < 0.6)
        x[:, c["cin"] // 2] = 0.0
        x = (x * (0.9 * cr.F16_MAX / np.max(np.abs(x)))).astype(np.float32)
        wt, b, s = cr.make_layer(c["cin"], c["cout"], c["ks"], rng)
        wt = (wt * (0.5 * cr.F16_MAX / np.max(np.abs(cr.conv64(x, wt, None))))).astype(np.float32)
        return (x, wt, b, s) + pre_and_bound(c, x, wt, b, s)
    return shared(("large", name), make)


@pytest.mark.parametrize("act", ["relu", "prelu"])
@pytest.mark.parametrize("name,family", FLAG_OR_BOUND, ids=[n for n, _ in FLAG_OR_BOUND])
def test_flag_or_bound(name, family, act):
    """The promise every layer test relies on: a layer either stays within its float64 bound or
    raises the range flag -- never flag clear and wrong."""
    c = dict(by_name(name), act=act)
    x, wt, b, s, pre, e = large_inputs(name)
    ref, bound = cr.activate(pre, s, act), cr.act_factor(s, act) * e
    peak = float(np.max(np.abs(pre)))
    assert abs(float(np.max(np.abs(x))) / (0.9 * cr.F16_MAX) - 1) < 1e-6 and abs(peak / (0.5 * cr.F16_MAX) - 1) < 1e-3
    assert float(np.max(np.abs(ref))) < cr.F16_MAX
    r = launch(c, "", x, wt, b, s)
    REACHED.add(vname(r.variant))
    assert vname(r.variant) == c["variant"]
    worst, at = cr.worst(r.y, ref, bound)
    print("%s (%s) %s: flag %d, worst |d| / bound %.4g at %s" % (name, family, act, r.range_flag, worst, at))
    clean(r)
    assert r.range_flag != 0 or worst <= 1.0
    if c["kernel"] != "wino2":
        assert r.range_flag == 0 and worst <= 1.0


# ---- the coverage guard (last in the file: it reads what the tests above reached) ----------

def test_coverage_of_the_dispatch():
    """The variants this file reaches contain the committed list: a dispatcher change that
    quietly stops a kernel from being covered fails here.  (Run on its own, it launches each
    listed variant's case once itself.)"""
    where = {form_name(c["variant"], f): (c, f, {}) for c, f in RUNS}
    where.update({form_name(v[6] + ".vin", f): (vin_case(v), f, dict(vin=True)) for v in VINS for f in v[7]})
    assert set(COVERED) <= set(where)
    # the range-guard tests above: their cases exist, are built for a listed variant (direct, the
    # control, has no variant code), and name every kernel family once
    for name in TRANSFORM_CASES + tuple(n for n, _ in FLAG_OR_BOUND):
        assert by_name(name)["variant"] == "none" or by_name(name)["variant"] in COVERED, name
    assert all(by_name(n)["kernel"] == "wino2" for n in TRANSFORM_CASES)
    tag = {"union": ".union", "plain p128": "k3.p128.c64", "ranged g2": ".ranged.g2", "wave ranges": ".wr", "split-K": ".split",
           "small 7x7": "k7.p64", "rgb": ".rgb", "wino2": ".w2", "direct": "none"}
    assert [f for _, f in FLAG_OR_BOUND] == list(tag)
    for name, family in FLAG_OR_BOUND:
        v = by_name(name)["variant"]
        assert v == tag[family] if family in ("plain p128", "direct") else tag[family] in v, (name, family)
    for name in COVERED:
        if name not in REACHED:
            c, f, more = where[name]
            REACHED.add(vname(launch(c, f, *inputs(c), **more).variant))
    print("reached: %s" % ", ".join(sorted(REACHED)))
    assert not sorted(set(COVERED) - REACHED)
