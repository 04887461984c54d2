"""The opt-in fp16 precision mode on the GPU (rt.Net.set_precision('fp16'): one fp16 product per
multiply-add, fp32 accumulate) against the fp64 oracle.

The mode cannot be held to a CPU emulation bit for bit -- one flipped fp16 rounding in an early
layer is amplified downstream, and two emulations that differ only in accumulation order are as
far from each other as from the oracle -- so every net case is held to the oracle at a margin over
the emulations' own error.  Per frame, E = the largest max-normalised error against the fp64
oracle over two CPU emulations (activations and weights of every conv rounded to fp16; fp32 and
fp64 accumulate) and all output tensors; the GPU's error must be <= 3 E (its accumulation order
is a third sample of that spread, with a max statistic over ~1e5 values; a structural fault -- a
dropped chunk, a wrong tap, lo planes read as hi -- moves the result by orders of magnitude
more), and E < 2e-2 so that the bar cannot go slack.  The bar is computed on the CPU from the
oracle alone, never from the code under test.  Every net case also checks, from op_variants(),
that every conv ran a one-term kernel: without that the cases pass on the three-term kernels.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from islpose import synth
from islpose import runtime as rt
from islpose.body import BodyEstimator

import _tame

pytestmark = pytest.mark.gpu
TOL32 = 1e-4     # the project's fp32 bar (test_gpu_body.TOL)
MARGIN, E_CAP = 3.0, 2e-2
KINDS = {"body25": rt.ISL_BODY25, "coco": rt.ISL_COCO, "hand": rt.ISL_HAND}
WSEED = {"body25": 0, "coco": 1, "hand": 2}


class _P64(cpu_ref._Params):
    """The fp64 oracle: the reference network in double precision."""

    def __init__(self, weights):
        self.t = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in weights.items()}


class _EmuF16(cpu_ref._Params):
    """fp16-operand emulation: every conv's activations and weights rounded with .half(),
    products accumulated in `acc` (torch.float32 or torch.float64), fp32 between layers."""

    def __init__(self, weights, acc):
        super().__init__(weights)
        self.acc = acc

    def conv(self, x, name, act):
        w = self.t[name + ".weight"].half().to(self.acc)
        y = F.conv2d(x.half().to(self.acc), w, self.t[name + ".bias"].to(self.acc), stride=1,
                     padding=w.shape[-1] // 2).float()
        if act == "relu":
            return F.relu(y)
        if act is None:
            return y
        return F.prelu(y, self.t[act + ".weight"])


def _tup(o):
    return tuple(t.numpy() for t in (o if isinstance(o, tuple) else (o,)))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


@functools.lru_cache(maxsize=None)
def _weights(model):
    return synth.synth_weights(WSEED[model])


def _inputs(n, h, w, seed):
    f = synth.synth_frames(n, h, w, seed=seed)
    return np.ascontiguousarray(np.transpose(f.astype(np.float32), (0, 3, 1, 2)) / 256 - 0.5)


@functools.lru_cache(maxsize=None)
def _frame_bar(model, h, w, seed, index):
    """(input [1,3,h,w], fp64 oracle outputs, E) of frame `index` of _inputs(index + 1, h, w, seed);
    computed once per frame and shared."""
    x = _inputs(index + 1, h, w, seed)[index:index + 1]
    fwd, wts = cpu_ref.FORWARDS[model], _weights(model)
    with torch.no_grad():
        ref = _tup(fwd(_P64(wts), torch.from_numpy(x).double()))
        errs = []
        for acc in (torch.float32, torch.float64):
            emu = _tup(fwd(_EmuF16(wts, acc), torch.from_numpy(x)))
            errs.append([_rel(e, r) for e, r in zip(emu, ref)])
    E = max(max(e) for e in errs)
    print("%s %dx%d: emulation errors vs fp64 (fp32 acc, fp64 acc) %s -> E = %.3e, bar %.3e"
          % (model, h, w, errs, E, MARGIN * E))
    return x, ref, E


@functools.lru_cache(maxsize=None)
def _net16(model):
    net = rt.Net(KINDS[model])
    net.load_weights(_weights(model))
    net.set_precision("fp16")
    return net


def _assert_one_term(net):
    """Every conv op of the last run carries the f16 bit (or ran inside another launch /
    was a folded pool), and none ran the Winograd kernel."""
    ops = net.op_variants()
    convs = [(name, rt.decode_variant(code)) for name, code in ops if name != "maxpool2"]
    assert len(convs) >= 40
    for name, d in convs:
        assert d.get("f16") or d.get("pool_fused") or d.get("fused_into_prev"), (name, d)
        assert not d.get("wino2"), (name, d)
    return convs


def _check_frame(model, outs, frame, ref, E):
    errs = [_rel(o[frame].cpu().numpy(), r[0]) for o, r in zip(outs, ref)]
    print("%s: GPU fp16-mode errors vs fp64 %s (bar %.3e)" % (model, ["%.3e" % e for e in errs], MARGIN * E))
    assert E < E_CAP, E
    assert all(e <= MARGIN * E for e in errs), (errs, E)
    return errs


def _forward(net, x):
    out = net.forward(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    return out if isinstance(out, tuple) else (out,)


def test_body25_bench_shape():
    """2 x 368x656, the bench shape at a small batch: conv1_1, the c128 / c384 stage layers on the
    128-pixel family (the chip-filling forms of the same frame: test_chip_filling_batches)."""
    x0, ref, E = _frame_bar("body25", 368, 656, 11, 0)
    x = _inputs(2, 368, 656, 11)
    assert np.array_equal(x[:1], x0)
    net = _net16("body25")
    outs = _forward(net, x)
    convs = _assert_one_term(net)
    assert any(d.get("rgb") for _, d in convs)
    _check_frame("body25 2x368x656", outs, 0, ref, E)


@pytest.mark.parametrize("model,n,h,w,seed", [("body25", 16, 368, 656, 11), ("hand", 16, 368, 368, 14)])
def test_chip_filling_batches(model, n, h, w, seed):
    """The same frames (and bars) as the cases above at the head of a batch that fills the chip,
    where the plan picks the 512-pixel family: the row union, pooled-input staging, two pairs per
    step and tail tiles (body), the 256-pixel 7x7 tiles (hand)."""
    x0, ref, E = _frame_bar(model, h, w, seed, 0)
    x = _inputs(n, h, w, seed)
    assert np.array_equal(x[:1], x0)
    net = _net16(model)
    outs = _forward(net, x)
    convs = _assert_one_term(net)
    if model == "body25":
        assert any(d.get("union") for _, d in convs) and any(d.get("vin") for _, d in convs)
        assert any(d.get("pairs2") for _, d in convs)
    else:
        assert any(d.get("ks") == 7 and d["bpx"] >= 256 for _, d in convs)
    _check_frame("%s %dx%dx%d" % (model, n, h, w), outs, 0, ref, E)


def test_body25_odd_planes():
    """1 x 376x664: 47x83 planes -- odd rows and columns, tail tiles."""
    x, ref, E = _frame_bar("body25", 376, 664, 12, 0)
    net = _net16("body25")
    outs = _forward(net, x)
    _assert_one_term(net)
    _check_frame("body25 1x376x664", outs, 0, ref, E)


def test_body25_small_grids_batch_invariant():
    """1 x 184x328 and 3 x 184x328 (Mode R): the wave-range kernel, split-K reduce and canonical
    ranges; the frame alone against the bar, and bit-identical at position 2 of a batch of 3."""
    x1, ref, E = _frame_bar("body25", 184, 328, 13, 2)
    x3 = _inputs(3, 184, 328, 13)
    assert np.array_equal(x3[2:3], x1)
    net = _net16("body25")
    one = _forward(net, x1)
    convs1 = _assert_one_term(net)
    assert any(d.get("wave_ranges") for _, d in convs1) or any(d.get("split") for _, d in convs1)
    three = _forward(net, x3)
    _assert_one_term(net)
    _check_frame("body25 1x184x328", one, 0, ref, E)
    for a, b in zip(one, three):
        assert torch.equal(a[0], b[2])


@pytest.mark.parametrize("model,h,w", [("hand", 184, 184), ("hand", 368, 368), ("coco", 184, 328)])
def test_hand_and_coco(model, h, w):
    """The 7x7 layers on small and mid grids (hand), the 7x7 stages and the heat-ReLU quirk (coco)."""
    x, ref, E = _frame_bar(model, h, w, 14, 0)
    net = _net16(model)
    outs = _forward(net, x)
    convs = _assert_one_term(net)
    assert any(d["ks"] == 7 for _, d in convs if "ks" in d)
    _check_frame("%s 1x%dx%d" % (model, h, w), outs, 0, ref, E)


def test_graph_replay_bit_identical(monkeypatch):
    monkeypatch.delenv("ISLPOSE_NET_GRAPH", raising=False)
    x = _inputs(2, 184, 328, 15)
    net = rt.Net(rt.ISL_BODY25)
    net.load_weights(_weights("body25"))
    net.set_precision("fp16")
    eager = _forward(net, x)
    _assert_one_term(net)
    var0 = net.op_variants()
    net.set_graph(True)
    try:
        for k in range(3):
            g = _forward(net, x)
            assert all(torch.equal(a, b) for a, b in zip(eager, g)), k
            assert net.op_variants() == var0, k
    finally:
        net.set_graph(False)


def test_round_trip_and_env(monkeypatch):
    """fp32 -> fp16 -> fp32 on one net: the fp32 bits come back (and are a fresh net's, within
    1e-4 of the oracle, with no f16 variant); a net created under ISLPOSE_PRECISION=fp16 reports
    fp16 and gives the bits of the set_precision net."""
    monkeypatch.delenv("ISLPOSE_PRECISION", raising=False)
    w = _weights("body25")
    x = _inputs(2, 184, 328, 16)
    net = rt.Net(rt.ISL_BODY25)
    net.load_weights(w)
    assert net.precision == "fp32"
    paf0, heat0 = _forward(net, x)
    net.set_precision("fp16")
    paf16, heat16 = _forward(net, x)
    _assert_one_term(net)
    assert not torch.equal(paf16, paf0)
    net.set_precision("fp32")
    paf1, heat1 = _forward(net, x)
    assert not any(rt.decode_variant(c).get("f16") for _, c in net.op_variants())
    assert torch.equal(paf1, paf0) and torch.equal(heat1, heat0)
    fresh = rt.Net(rt.ISL_BODY25)
    fresh.load_weights(w)
    paf2, heat2 = _forward(fresh, x)
    assert torch.equal(paf2, paf0) and torch.equal(heat2, heat0)
    rp, rh = cpu_ref.make_net_fn("body25", w)(x)
    assert _rel(paf1.cpu().numpy(), rp) < TOL32 and _rel(heat1.cpu().numpy(), rh) < TOL32
    net.set_precision("fp16")                 # back again: the kept hi-only pack, the same bits
    paf3, heat3 = _forward(net, x)
    assert torch.equal(paf3, paf16) and torch.equal(heat3, heat16)
    monkeypatch.setenv("ISLPOSE_PRECISION", "fp16")
    env = rt.Net(rt.ISL_BODY25)
    env.load_weights(w)
    assert env.precision == "fp16"
    paf4, heat4 = _forward(env, x)
    _assert_one_term(env)
    assert torch.equal(paf4, paf16) and torch.equal(heat4, heat16)


def test_range_guard_in_fp16_mode():
    """The recipe of test_gpu_body.py::test_x3_range_guard_falls_back_to_fp32 in fp16 mode: the
    raw run raises the flag, the guarded seam recomputes on the fp32 kernels, the net keeps
    both its algorithm and its precision."""
    w = dict(_weights("body25"))
    w["conv1_1.weight"] = w["conv1_1.weight"] * np.float32(2.0 ** 20)
    w["conv1_1.bias"] = w["conv1_1.bias"] * np.float32(2.0 ** 20)
    net = rt.Net(rt.ISL_BODY25)
    net.load_weights(w)
    net.set_precision("fp16")
    x = _inputs(1, 64, 96, seed=21)
    xt = torch.from_numpy(x).cuda()
    o0 = torch.empty((1, 52, 8, 12), device="cuda")
    o1 = torch.empty((1, 26, 8, 12), device="cuda")
    rt.check(rt.lib().isl_net_forward(net.h, rt.ptr(xt), 1, 64, 96, rt.ptr(o0), rt.ptr(o1), rt.stream_handle()))
    assert not net.range_ok()
    assert net.range_ok()
    paf, heat = net.forward(xt)
    rp, rh = cpu_ref.make_net_fn("body25", w)(x)
    assert _rel(paf.cpu().numpy(), rp) < TOL32 and _rel(heat.cpu().numpy(), rh) < TOL32
    assert net.precision == "fp16" and net.algo == "x3"


def test_frame_seam_peaks():
    """BodyEstimator(precision='fp16').estimate on a tamed 368x656 frame against the fp32
    oracle's body_call: at most 5 % of the oracle's peaks (at least 100 of them) without an
    fp16-mode peak within 1 px in x and y.  (On the CPU the two emulations left 1.5 % and 0.4 %
    of 265 oracle peaks unmatched at this seed and gain.)  Person counts are not compared: the
    synthetic nets' near-threshold peaks make them differ between the emulations themselves."""
    frame = synth.synth_frames(1, 368, 656, seed=41)[0]
    w = _tame.tame_body(_weights("body25"), frame, scale=0.5, gain=0.05)
    est = BodyEstimator(w, "body25", precision="fp16")
    assert est.net.precision == "fp16"
    cand, _ = est.estimate(frame)
    _assert_one_term(est.net)
    ref, _ = cpu_ref.body_call(frame, cpu_ref.make_net_fn("body25", w), "body25", (0.5,))
    ref, cand = np.asarray(ref).reshape(-1, 4), np.asarray(cand).reshape(-1, 4)
    assert len(ref) >= 100, len(ref)
    missed = 0
    for px, py in ref[:, :2]:
        near = (np.abs(cand[:, 0] - px) <= 1) & (np.abs(cand[:, 1] - py) <= 1) if len(cand) else np.zeros(0, bool)
        missed += not near.any()
    print("frame seam: %d oracle peaks, %d fp16-mode peaks, %d unmatched (%.2f %%)"
          % (len(ref), len(cand), missed, 100.0 * missed / len(ref)))
    assert missed <= 0.05 * len(ref), (missed, len(ref))


def test_state_key_differs_between_precisions():
    """ISLSignPos.state_key() over the same weights: fp32 and fp16 estimators differ, so the
    translator's cached feature rows are dropped on a switch."""
    from src.ISL_Model_parameter import ISLSignPos
    from src.body import Body
    from src.hand import Hand
    tw = lambda k: {n: torch.from_numpy(v) for n, v in synth.synth_weights(k).items()}  # noqa: E731
    body, hand = Body(tw(0), "body25", precision="fp32"), Hand(tw(2), precision="fp32")
    isl = ISLSignPos(body.model, hand.model)
    b, h = isl._estimators()
    assert b.net.precision == "fp32" and h.net.precision == "fp32"
    k32 = isl.state_key()
    body.model.set_precision("fp16")
    hand.model.set_precision("fp16")
    b, h = isl._estimators()
    assert b.net.precision == "fp16" and h.net.precision == "fp16"
    k16 = isl.state_key()
    assert k16 != k32
    body.model.set_precision("fp32")
    hand.model.set_precision("fp32")
    assert isl.state_key() == k32
