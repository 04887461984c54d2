"""The fp16 precision mode's two fused launches on the GPU: conv1_1 -> conv1_2 -> pool in one launch
(conv_c12.hip's one-term form, taken by default wherever the fp32 plan takes it) and the fused 1x1
pair (conv_x3 VAR 16 | 2, opt-in through ISLPOSE_X3_FUSE67 because its Mconv7 K order is the
permuted one).

Bits: the c12 launch must change no bit of the fp16 mode (torch.equal against ISLPOSE_C12=0, whose
launches test_gpu_fp16.py holds to the oracle); the fused pair must equal its permuted two-launch
form (=3) bit for bit, and is held to the fp64 oracle at test_gpu_fp16.py's bar (3 E, E from that
file's CPU emulations).  Under fp16 activation storage both must give the bits of the fp32-storage
run.  Every case reads the plan back (op_variants): without that the cases pass on the unfused
launches.  All nets run precision 'fp16'."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from islpose import runtime as rt

from test_gpu_fp16 import TOL32, _check_frame, _frame_bar, _inputs, _rel, _weights
from test_gpu_act_storage import _net

pytestmark = pytest.mark.gpu
KINDS = {"body25": rt.ISL_BODY25, "hand": rt.ISL_HAND}


@functools.lru_cache(maxsize=None)
def _nets(model):
    """(fp32-storage net, fp16-storage net), precision 'fp16', one pair per model for this file."""
    return _net(model, "fp32"), _net(model, "fp16")


def _run(net, x):
    out = net.forward(x)
    torch.cuda.synchronize()
    out = out if isinstance(out, tuple) else (out,)
    return [t.clone() for t in out], net.op_variants()


def _equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _dec(var):
    return [(name, code, rt.decode_variant(code)) for name, code in var]


def _assert_c12(var, pooled, act16):
    """conv1_1's launch is the fused conv1 variant with f16 (and act16), conv1_2 ran inside it, the
    pool ran inside it (pooled) or left its row-pair max to conv2_1's staging / vpool2."""
    d = _dec(var)
    names = [n for n, _, _ in d]
    i = names.index("conv1_1")
    assert names[i + 1] == "conv1_2" and names[i + 2] == "maxpool2", names[i:i + 3]
    d11, d12, dpl = d[i][2], d[i + 1][2], d[i + 2][2]
    assert d11.get("c12") and d11.get("f16") and d11.get("ks") == 3 and d11.get("bco") == 64, d11
    assert bool(d11.get("act16")) == act16, d11
    assert d12.get("fused_into_prev") or d12.get("pool_fused"), d12
    if pooled:
        assert dpl.get("fused_into_prev") or dpl.get("pool_fused"), dpl
        assert not d[i + 3][2].get("vin"), d[i + 3]
    else:
        assert not dpl.get("fused_into_prev"), dpl


def _assert_no_c12(var):
    d = _dec(var)
    assert not any(x.get("c12") for _, _, x in d)
    d11 = dict((n, x) for n, _, x in d)["conv1_1"]
    assert d11.get("rgb") and d11.get("f16"), d11
    assert dict((n, x) for n, _, x in d)["conv1_2"].get("f16")


def _fused_ops(var):
    return [k for k, (_, c) in enumerate(var) if rt.decode_variant(c).get("fused67")]


def _assert_pairs_fused(var, n_pairs, act16):
    ks = _fused_ops(var)
    assert len(ks) == n_pairs, [var[k][0] for k in ks]
    for k in ks:
        d = rt.decode_variant(var[k][1])
        assert d["f16"] and d["ks"] == 1 and d["bco"] in (128, 256, 512), (var[k], d)
        assert bool(d["act16"]) == act16, (var[k], d)
        assert var[k + 1][1] == -2, var[k + 1]          # the second layer ran inside the first
    return ks


# ---- 1. the c12 launch is taken by default and changes no bit ----------------------------------
@pytest.mark.parametrize("model,n,h,w", [("body25", 1, 184, 328), ("body25", 2, 368, 656), ("hand", 2, 184, 184),
                                         ("body25", 1, 376, 664)])
def test_c12_taken_and_bit_identical(model, n, h, w, monkeypatch):
    """(1 x 376x664: a partial 32-column tile at the right edge.)"""
    monkeypatch.delenv("ISLPOSE_X3_FUSE67", raising=False)
    net = _nets(model)[0]
    x = torch.from_numpy(_inputs(n, h, w, 3 * h + w + n)).cuda()
    monkeypatch.delenv("ISLPOSE_C12", raising=False)
    o1, v1 = _run(net, x)
    monkeypatch.setenv("ISLPOSE_C12", "0")
    o0, v0 = _run(net, x)
    monkeypatch.setenv("ISLPOSE_C12", "2")
    o2, v2 = _run(net, x)
    _assert_c12(v1, True, False)
    _assert_c12(v2, False, False)
    _assert_no_c12(v0)
    assert _equal(o0, o1) and _equal(o0, o2)
    assert all(bool(torch.isfinite(t).all()) for t in o1)


# ---- 2. ... and under fp16 storage -------------------------------------------------------------
@pytest.mark.parametrize("model,n,h,w", [("body25", 2, 368, 656), ("hand", 2, 368, 368)])
def test_c12_fp16_storage(model, n, h, w, monkeypatch):
    monkeypatch.delenv("ISLPOSE_X3_FUSE67", raising=False)
    net32, net16 = _nets(model)
    x = torch.from_numpy(_inputs(n, h, w, 3 * h + w + n)).cuda()
    monkeypatch.setenv("ISLPOSE_C12", "0")
    ref, _ = _run(net32, x)
    for mode, pooled in ((None, True), ("2", False), ("0", None)):
        if mode is None:
            monkeypatch.delenv("ISLPOSE_C12")
        else:
            monkeypatch.setenv("ISLPOSE_C12", mode)
        got, var = _run(net16, x)
        assert net16.act_storage_active is True, mode
        if pooled is None:
            _assert_no_c12(var)
        else:
            _assert_c12(var, pooled, True)
        assert _equal(ref, got), mode
    monkeypatch.delenv("ISLPOSE_C12")
    o32, v32 = _run(net32, x)
    assert net32.act_storage_active is False
    _assert_c12(v32, True, False)
    assert _equal(ref, o32)


# ---- 3. the pair: fused == permuted two launches, opt-in ---------------------------------------
@pytest.mark.parametrize("model,n,h,w", [("body25", 2, 368, 656), ("body25", 1, 184, 328), ("hand", 2, 368, 368),
                                         ("hand", 1, 184, 184)])
def test_pair_fused_equals_permuted_and_is_opt_in(model, n, h, w, monkeypatch):
    """(body25 1 x 184x328 and hand 1 x 184x184: Mconv7 / conv6_2 with K ranges, where =3 really
    runs the two launches.)"""
    net = _nets(model)[0]
    x = torch.from_numpy(_inputs(n, h, w, 7 * h + w + n)).cuda()
    monkeypatch.setenv("ISLPOSE_X3_FUSE67", "2")
    o2, v2 = _run(net, x)
    ks = _assert_pairs_fused(v2, 6, False)
    if model == "hand":
        assert "conv6_1_CPM" in [v2[k][0] for k in ks]
    monkeypatch.setenv("ISLPOSE_X3_FUSE67", "3")
    o3, v3 = _run(net, x)
    ranged7 = [rt.decode_variant(v3[k + 1][1]) for k in ks if not rt.decode_variant(v3[k][1]).get("fused67")]
    print("%s %dx%dx%d: =3 runs %d of 6 pairs as the permuted two launches" % (model, n, h, w, len(ranged7)))
    assert all(d.get("f16") and (d.get("ranged") or d.get("split") or d.get("wave_ranges")) for d in ranged7), ranged7
    if h == 184:                      # Mconv7 with K ranges: the two-launch form really runs
        assert len(ranged7) == 6 if model == "body25" else len(ranged7) >= 1, len(ranged7)
    assert _equal(o2, o3)
    # =1 selects by grid as the fp32 plan's default does: the same ops fused as an fp32 net's run
    fp32 = rt.Net(KINDS[model])
    fp32.load_weights(_weights(model))
    monkeypatch.delenv("ISLPOSE_X3_FUSE67")
    _, vf = _run(fp32, x)
    monkeypatch.setenv("ISLPOSE_X3_FUSE67", "1")
    o1, v1 = _run(net, x)
    assert _fused_ops(v1) == _fused_ops(vf), (_fused_ops(v1), _fused_ops(vf))
    _assert_pairs_fused(v1, len(_fused_ops(vf)), False)
    assert _equal(o1, o2)
    # unset: today's plan and bits
    monkeypatch.delenv("ISLPOSE_X3_FUSE67")
    od, vd = _run(net, x)
    monkeypatch.setenv("ISLPOSE_X3_FUSE67", "0")
    o0, v0 = _run(net, x)
    assert _equal(od, o0) and vd == v0
    assert not _fused_ops(vd) and not any(c == -2 for (n_, c) in vd if n_ != "maxpool2")
    assert all(rt.decode_variant(c).get("f16") for name, c in vd if name.startswith(("Mconv6", "Mconv7")))


# ---- 4. the pair under fp16 storage (the dual store) -------------------------------------------
@pytest.mark.parametrize("model,n,h,w", [("body25", 2, 368, 656), ("hand", 2, 368, 368)])
def test_pair_fp16_storage(model, n, h, w, monkeypatch):
    net32, net16 = _nets(model)
    x = torch.from_numpy(_inputs(n, h, w, 7 * h + w + n)).cuda()
    monkeypatch.setenv("ISLPOSE_X3_FUSE67", "2")
    ref, v32 = _run(net32, x)
    _assert_pairs_fused(v32, 6, False)
    got, v16 = _run(net16, x)
    assert net16.act_storage_active is True
    _assert_pairs_fused(v16, 6, True)
    assert [(nm, c | 1 if c > 0 else c) for nm, c in v32] == v16
    assert _equal(ref, got)


# ---- 5. accuracy of the fused pair --------------------------------------------------------------
@pytest.mark.parametrize("model,h,w,seed,index", [("body25", 184, 328, 13, 2), ("hand", 184, 184, 14, 0)])
def test_pair_accuracy(model, h, w, seed, index, monkeypatch):
    """test_gpu_fp16.py's frames, oracle and bar (3 E, E from the CPU emulations alone)."""
    x, ref, E = _frame_bar(model, h, w, seed, index)
    net = _nets(model)[0]
    monkeypatch.setenv("ISLPOSE_X3_FUSE67", "2")
    outs, var = _run(net, torch.from_numpy(x).cuda())
    _assert_pairs_fused(var, 6, False)
    _check_frame("%s 1x%dx%d fused pairs" % (model, h, w), outs, 0, ref, E)


# ---- 6. batch invariance ------------------------------------------------------------------------
def test_pair_batch_invariant(monkeypatch):
    monkeypatch.setenv("ISLPOSE_X3_FUSE67", "1")
    net = _nets("body25")[0]
    x = torch.from_numpy(_inputs(2, 184, 328, 404)).cuda()
    ob, _ = _run(net, x)
    for i in (0, 1):
        o1, _ = _run(net, x[i:i + 1].contiguous())
        assert all(torch.equal(a, b[i:i + 1]) for a, b in zip(o1, ob)), i


# ---- 7. the range guard through both fusions ----------------------------------------------------
def _guard(w, env, monkeypatch, expect):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = rt.Net(rt.ISL_BODY25)
    net.load_weights(w)
    net.set_precision("fp16")
    x = _inputs(1, 64, 96, seed=21)
    xt = torch.from_numpy(x).cuda()
    o0 = torch.empty((1, 52, 8, 12), device="cuda")
    o1 = torch.empty((1, 26, 8, 12), device="cuda")
    rt.check(rt.lib().isl_net_forward(net.h, rt.ptr(xt), 1, 64, 96, rt.ptr(o0), rt.ptr(o1), rt.stream_handle()))
    expect(net.op_variants())
    assert not net.range_ok()
    assert net.range_ok()
    paf, heat = net.forward(xt)
    rp, rh = cpu_ref.make_net_fn("body25", w)(x)
    assert _rel(paf.cpu().numpy(), rp) < TOL32 and _rel(heat.cpu().numpy(), rh) < TOL32
    assert net.precision == "fp16" and net.algo == "x3"


def test_range_guard_conv1_1_inside_c12(monkeypatch):
    """conv1_1's outputs reach >= 65504 inside the c12 launch, where they never leave LDS: the
    check on the fp32 value before the rounding is the only place the overflow can be seen."""
    monkeypatch.delenv("ISLPOSE_C12", raising=False)
    w = dict(_weights("body25"))
    w["conv1_1.weight"] = w["conv1_1.weight"] * np.float32(2.0 ** 20)
    w["conv1_1.bias"] = w["conv1_1.bias"] * np.float32(2.0 ** 20)
    _guard(w, {}, monkeypatch, lambda var: _assert_c12(var, True, False))


def test_range_guard_mconv6_inside_fused_pair(monkeypatch):
    w = dict(_weights("body25"))
    for k in list(w):
        if k.startswith("Mconv6_stage0_L2") and k.endswith(".bias"):
            w[k] = w[k] + np.float32(1e5)
    _guard(w, {"ISLPOSE_X3_FUSE67": "2"}, monkeypatch, lambda var: _assert_pairs_fused(var, 6, False))


# ---- 8. graph replay and switching --------------------------------------------------------------
def test_graph_replay_and_switching(monkeypatch):
    monkeypatch.delenv("ISLPOSE_NET_GRAPH", raising=False)
    monkeypatch.delenv("ISLPOSE_X3_FUSE67", raising=False)
    x = torch.from_numpy(_inputs(2, 184, 328, 15)).cuda()
    net = rt.Net(rt.ISL_BODY25)
    net.load_weights(_weights("body25"))
    # the ungraphed bits and variants of the four states
    want = {}
    for prec in ("fp32", "fp16"):
        net.set_precision(prec)
        for f67 in (None, "2"):
            if f67 is None:
                monkeypatch.delenv("ISLPOSE_X3_FUSE67", raising=False)
            else:
                monkeypatch.setenv("ISLPOSE_X3_FUSE67", f67)
            want[prec, f67] = _run(net, x)
    assert len(_fused_ops(want["fp16", "2"][1])) == 6 and not _fused_ops(want["fp16", None][1])
    assert all(rt.decode_variant(want["fp16", "2"][1][k][1])["f16"] for k in _fused_ops(want["fp16", "2"][1]))
    assert not _equal(want["fp16", "2"][0], want["fp32", "2"][0])
    net.set_graph(True)
    try:
        for rnd in range(3):                    # eager, capture, replay of every key, interleaved
            for prec, f67 in (("fp16", "2"), ("fp32", None), ("fp16", None), ("fp32", "2")):
                net.set_precision(prec)
                if f67 is None:
                    monkeypatch.delenv("ISLPOSE_X3_FUSE67", raising=False)
                else:
                    monkeypatch.setenv("ISLPOSE_X3_FUSE67", f67)
                out, var = _run(net, x)
                assert _equal(out, want[prec, f67][0]), (rnd, prec, f67)
                assert var == want[prec, f67][1], (rnd, prec, f67)
    finally:
        net.set_graph(False)
