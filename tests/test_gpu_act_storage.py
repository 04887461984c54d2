"""The opt-in fp16 activation storage on the GPU (rt.Net.set_act_storage('fp16') under precision
'fp16'): the arena buffers between the convs hold the fp16 roundings the one-term kernels make
anyway, so every result must be the SAME BITS as the fp16 mode with fp32 storage on the same net.

That yardstick -- precision 'fp16', storage 'fp32' -- is unchanged by this feature and is held to the
fp64 oracle by test_gpu_fp16.py.  Every comparison here is torch.equal / np.array_equal: there is
no tolerance.  Every case also reads the plan back (op_variants): without the act16 bit on every
conv the cases would pass on the fp32-storage kernels.
"""
import functools

import numpy as np
import pytest
import torch

from islpose import synth
from islpose import runtime as rt
from islpose.body import BodyEstimator
from islpose.hand import HandEstimator

import _tame

pytestmark = pytest.mark.gpu
KINDS = {"body25": rt.ISL_BODY25, "coco": rt.ISL_COCO, "hand": rt.ISL_HAND}
WSEED = {"body25": 0, "coco": 1, "hand": 2}


@functools.lru_cache(maxsize=None)
def _weights(model):
    return synth.synth_weights(WSEED[model])


def _inputs(n, h, w, seed):
    f = synth.synth_frames(n, h, w, seed=seed)
    return np.ascontiguousarray(np.transpose(f.astype(np.float32), (0, 3, 1, 2)) / 256 - 0.5)


def _net(model, storage="fp32", precision="fp16", weights=None):
    net = rt.Net(KINDS[model])
    net.load_weights(weights if weights is not None else _weights(model))
    net.set_precision(precision)
    net.set_act_storage(storage)
    return net


@functools.lru_cache(maxsize=None)
def _pair(model):
    """(fp32-storage net, fp16-storage net), both precision 'fp16', one pair per model."""
    return _net(model, "fp32"), _net(model, "fp16")


def _forward(net, x):
    out = net.forward(torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x)
    torch.cuda.synchronize()
    return out if isinstance(out, tuple) else (out,)


def _convs(net):
    return [(name, code, rt.decode_variant(code)) for name, code in net.op_variants() if name != "maxpool2"]


def _assert_plan(net32, net16):
    """After the same forward on both: every conv of the fp16-storage run carries act16 (or ran
    inside another launch / was a folded pool), none of the fp32-storage run does, and apart
    from that bit the variant codes are equal op by op -- same plan, same tiles, same K order."""
    v32, v16 = net32.op_variants(), net16.op_variants()
    assert [n for n, _ in v32] == [n for n, _ in v16]
    convs = _convs(net16)
    assert len(convs) >= 40
    for name, code, d in convs:
        assert d.get("act16") or d.get("pool_fused") or d.get("fused_into_prev"), (name, d)
        assert d.get("f16") or d.get("pool_fused") or d.get("fused_into_prev"), (name, d)
    for (name, c32), (_, c16) in zip(v32, v16):
        if c32 > 0:
            assert not (c32 & 1), (name, c32)
            assert c16 == c32 | 1, (name, c32, c16)
        else:
            assert c16 == c32, (name, c32, c16)
    return [d for _, _, d in convs]


def _same_bits(model, n, h, w, seed):
    net32, net16 = _pair(model)
    x = torch.from_numpy(_inputs(n, h, w, seed)).cuda()
    ref = _forward(net32, x)
    assert net32.act_storage_active is False
    got = _forward(net16, x)
    assert net16.act_storage_active is True, "the plan fell back to fp32 storage"
    assert net16.precision == "fp16" and net16.act_storage == "fp16"
    for a, b in zip(ref, got):
        assert a.shape == b.shape and torch.equal(a, b), float((a - b).abs().max())
    return _assert_plan(net32, net16)


def _tail_tiles(n, hw, co_tiles, tpx, cus):
    """conv_x3.hip's x3_tail_plan: the tail tile size (0: one tiling) of a launch of the 256- / 512-
    pixel families without K ranges, from the grid alone."""
    per = n * co_tiles
    px_tiles = -(-hw // tpx)
    r0 = -(-per * px_tiles // cus)
    rf = per * (hw // tpx) // cus
    if rf < 1 or r0 < 2:
        return 0
    full = rf * cus // per
    if full < 1 or (per * full) % 8:
        return 0
    rem, best, ttpx = hw - full * tpx, r0 - 0.25, 0
    for t in range(128, tpx, 128):
        nt = per * -(-rem // t)
        est = per * full / cus + -(-nt // cus) * (0.3 + 0.7 * t / tpx)
        if est < best:
            best, ttpx = est, t
    return ttpx


def test_body25_bench_shape():
    """2 x 368x656: conv1_1's 3-channel kernel (fp32 in, fp16 out), the 128-pixel family with its
    deep-prefetch loop, the final PAF stored twice (fp32 output + the fp16 slice the heat stages read)."""
    ds = _same_bits("body25", 2, 368, 656, 11)
    assert any(d.get("rgb") for d in ds)
    assert any(d.get("bpx") == 128 for d in ds)
    assert any(d.get("var", 0) & 128 for d in ds)


def test_body25_chip_filling_batch():
    """16 x 368x656: the 512-pixel family -- row union, pooled-input staging (packed fp16 row-pair
    max), two pairs per step, and tail tiles: the variant code does not carry them, so the test
    repeats the launch's tail plan for conv2_2 (184x328 planes, 128 channels, 512-pixel tiles)
    and requires that it splits the frame into full and tail tiles."""
    ds = _same_bits("body25", 16, 368, 656, 11)
    assert any(d.get("union") for d in ds) and any(d.get("vin") for d in ds)
    assert any(d.get("pairs2") for d in ds)
    d22 = dict((name, d) for name, _, d in _convs(_pair("body25")[1]))["conv2_2"]
    assert d22["bpx"] == 512 and d22["bco"] == 128 and not d22["ranged"], d22
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _tail_tiles(16, 184 * 328, 1, 512, cus) in (128, 256, 384), cus


def test_body25_odd_planes():
    """1 x 376x664: 47x83 planes -- odd rows and columns, masked tiles."""
    _same_bits("body25", 1, 376, 664, 12)


def test_body25_ranged_small_planes():
    """32 x 184x328 (Mode R at batch 32): 23x41 stage planes with canonical K ranges kept in one
    block, two K groups where the plan picks them."""
    ds = _same_bits("body25", 32, 184, 328, 13)
    assert any(d.get("ranged") for d in ds)
    print("two K groups in the plan:", any(d.get("g2") for d in ds))
    assert all(d.get("ranged") for d in ds if d.get("g2"))
    assert not any(d.get("split") or d.get("wave_ranges") for d in ds)


def test_hand_wide_7x7():
    """hand 16 x 368x368: the 7x7 layers on 256- / 384-pixel tiles (one input buffer)."""
    ds = _same_bits("hand", 16, 368, 368, 14)
    assert any(d.get("ks") == 7 and d["bpx"] >= 256 for d in ds)


def test_coco():
    """coco 2 x 368x656: the heat-ReLU quirk, the 7x7 stages, two outputs in slices of one buffer."""
    ds = _same_bits("coco", 2, 368, 656, 15)
    assert any(d.get("ks") == 7 for d in ds)


@pytest.mark.parametrize("model,n,h,w,seed", [("body25", 16, 368, 656, 11)])
def test_dma_staging_switch(monkeypatch, model, n, h, w, seed):
    """ISLPOSE_A16_DMA (read per launch): the row union's plain input runs copied into LDS by
    LDS-DMA (the default) or staged through registers (=0, the A/B form) -- the same plan, the
    same bits."""
    monkeypatch.setenv("ISLPOSE_A16_DMA", "0")
    ds = _same_bits(model, n, h, w, seed)
    assert any(d.get("union") and not d.get("vin") for d in ds)
    monkeypatch.setenv("ISLPOSE_A16_DMA", "1")
    _same_bits(model, n, h, w, seed)


def test_fallback_on_uncovered_plan():
    """body25 1 x 184x328 with storage fp16 requested: its 23x41 layers split their K ranges
    across blocks (split-K / the wave-range kernel), which have no fp16-storage form, so the whole
    run keeps fp32 buffers: not active, no act16 bit, the bits and the plan of the fp32-storage run."""
    net32, net16 = _pair("body25")
    x = torch.from_numpy(_inputs(1, 184, 328, 13)).cuda()
    ref = _forward(net32, x)
    got = _forward(net16, x)
    assert net16.act_storage == "fp16" and net16.act_storage_active is False
    assert all(torch.equal(a, b) for a, b in zip(ref, got))
    assert net16.op_variants() == net32.op_variants()
    ds = [d for _, _, d in _convs(net16)]
    assert not any(d.get("act16") for d in ds)
    assert any(d.get("wave_ranges") or d.get("split") for d in ds)
    assert all(d.get("f16") or d.get("pool_fused") or d.get("fused_into_prev") for d in ds)


def test_inert_under_fp32_precision():
    """precision fp32 with storage fp16: the bits and the plan of a default net, no act16 / f16 bit."""
    x = torch.from_numpy(_inputs(2, 368, 656, 11)).cuda()
    default = rt.Net(rt.ISL_BODY25)
    default.load_weights(_weights("body25"))
    net = _net("body25", "fp16", precision="fp32")
    ref, got = _forward(default, x), _forward(net, x)
    assert net.act_storage == "fp16" and net.act_storage_active is False
    assert all(torch.equal(a, b) for a, b in zip(ref, got))
    assert net.op_variants() == default.op_variants()
    for _, code, d in _convs(net):
        assert not d.get("act16") and not d.get("f16"), d


def test_frame_seam_body():
    """BodyEstimator.estimate on two tamed 368x656 frames at scale 1 (net input 368x656: the
    reference's 0.5 gives 23x41 planes, whose K ranges across blocks keep fp32 buffers): preprocess
    -> conv1_1, the PAF stored twice, the post kernels reading the fp32 outputs -- the same
    candidate and subset.  (The heat layer is tamed at that scale, so that the synthetic net gives
    hundreds of peaks, not thousands.)"""
    frames = synth.synth_frames(2, 368, 656, seed=41)
    w = _tame.tame_body(_weights("body25"), frames[0], scale=1.0, gain=0.05)
    ref = BodyEstimator(w, "body25", scale_search=(1.0,), precision="fp16").estimate(frames)
    est = BodyEstimator(w, "body25", scale_search=(1.0,), precision="fp16", act_storage="fp16")
    assert est.net.act_storage == "fp16"
    got = est.estimate(frames)
    assert est.net.act_storage_active is True
    assert all(d.get("act16") or d.get("pool_fused") for _, _, d in _convs(est.net))
    assert len(ref) == len(got) == 2
    npk = sum(len(np.asarray(c).reshape(-1, 4)) for c, _ in ref)
    print("frame seam: %d peaks, %d persons in the two frames" % (npk, sum(len(s) for _, s in ref)))
    assert npk >= 20, npk
    for (c0, s0), (c1, s1) in zip(ref, got):
        assert np.array_equal(c0, c1) and np.array_equal(s0, s1)


def test_frame_seam_hand_crops():
    """HandEstimator.estimate_crops on 8 crops: the same peaks; the small scales may keep fp32
    buffers (K ranges across blocks), the 736 px scale must run on fp16 buffers."""
    frames = synth.synth_frames(2, 368, 656, seed=42)
    boxes = [(i % 2, 16 + 40 * i, 8 + 20 * i, 150 + 6 * (i % 3)) for i in range(8)]
    w = _weights("hand")
    ref = HandEstimator(w, precision="fp16").estimate_crops(frames, boxes)
    est = HandEstimator(w, precision="fp16", act_storage="fp16")
    got = est.estimate_crops(frames, boxes)
    assert ref.shape == (8, 21, 2) and np.array_equal(ref, got)
    # one scale again, to read its plan: 8 crops at 2 x 368 px
    t = torch.as_tensor(frames).cuda()
    crops = [(f, x, y, s, s) for (f, x, y, s) in boxes]
    gh, gw = est.net.preprocess_crops(t, crops, 2.0 * 368)
    assert (gh, gw) == (736, 736)
    est.net.run(torch.empty((8, 22, 92, 92), device="cuda"))
    torch.cuda.synchronize()
    assert est.net.act_storage_active is True
    assert all(d.get("act16") or d.get("pool_fused") for _, _, d in _convs(est.net))


def test_range_guard():
    """conv1_1 scaled by 2^20 at 2 x 368x656: the raw run raises the flag (checked on the fp32
    value, before anything is rounded), Net.forward recomputes on the fp32 kernels (an fp32 arena)
    and returns the bits of the fp32-storage net's own fallback; the net keeps its settings."""
    w = dict(_weights("body25"))
    w["conv1_1.weight"] = w["conv1_1.weight"] * np.float32(2.0 ** 20)
    w["conv1_1.bias"] = w["conv1_1.bias"] * np.float32(2.0 ** 20)
    x = torch.from_numpy(_inputs(2, 368, 656, 21)).cuda()
    net32, net16 = _net("body25", "fp32", weights=w), _net("body25", "fp16", weights=w)
    o0 = torch.empty((2, 52, 46, 82), device="cuda")
    o1 = torch.empty((2, 26, 46, 82), device="cuda")
    rt.check(rt.lib().isl_net_forward(net16.h, rt.ptr(x), 2, 368, 656, rt.ptr(o0), rt.ptr(o1), rt.stream_handle()))
    assert net16.act_storage_active is True
    assert not net16.range_ok()
    assert net16.range_ok()
    ref = _forward(net32, x)
    got = _forward(net16, x)
    assert all(torch.equal(a, b) for a, b in zip(ref, got))
    assert all(bool(torch.isfinite(a).all()) for a in got)
    assert net16.precision == "fp16" and net16.algo == "x3" and net16.act_storage == "fp16"
    assert net32.range_trips() >= 1 and net16.range_trips() >= 2


def test_graph_replay_and_switching(monkeypatch):
    """Eager, then three replays: equal bits and variants.  Then fp16 -> fp32 -> fp16 storage on
    the one net: each mode's bits come back, and the size then has two arenas."""
    monkeypatch.delenv("ISLPOSE_NET_GRAPH", raising=False)
    x = torch.from_numpy(_inputs(2, 368, 656, 16)).cuda()
    net = _net("body25", "fp16")
    eager = _forward(net, x)
    assert net.act_storage_active is True and net.arena_info()[1] == 1
    var16 = net.op_variants()
    assert all(c & 1 for _, c in var16 if c > 0)
    net.set_graph(True)
    try:
        for k in range(3):
            g = _forward(net, x)
            assert all(torch.equal(a, b) for a, b in zip(eager, g)), k
            assert net.op_variants() == var16 and net.act_storage_active is True, k
        net.set_act_storage("fp32")
        for k in range(3):                      # eager, capture, replay on the other arena
            f32 = _forward(net, x)
            assert net.act_storage_active is False, k
            assert all(torch.equal(a, b) for a, b in zip(eager, f32)), k
            assert [(n, c | 1 if c > 0 else c) for n, c in net.op_variants()] == var16, k
            assert not any(c & 1 for _, c in net.op_variants() if c > 0), k
        assert net.arena_info()[1] == 2
        net.set_act_storage("fp16")
        back = _forward(net, x)
        assert net.act_storage_active is True and net.op_variants() == var16
        assert all(torch.equal(a, b) for a, b in zip(eager, back))
        assert net.arena_info()[1] == 2
    finally:
        net.set_graph(False)


def test_arena_memory_halves():
    """Fresh nets at 2 x 368x656: only the 8-channel net input and the output maps stay fp32, so
    the fp16-storage arena is just above half the fp32-storage one; the bar is 0.6."""
    x = torch.from_numpy(_inputs(2, 368, 656, 11)).cuda()
    net32, net16 = _net("body25", "fp32"), _net("body25", "fp16")
    _forward(net32, x)
    _forward(net16, x)
    assert net16.act_storage_active is True
    (b32, k32), (b16, k16) = net32.arena_info(), net16.arena_info()
    ratio = b16 / b32
    print("arena bytes at 2x368x656: fp32 storage %d, fp16 storage %d, ratio %.4f" % (b32, b16, ratio))
    assert k32 == k16 == 1
    assert 0.5 < ratio < 0.6, ratio
