"""The fp16-storage decision and the run read one launch plan (runtime.cpp plan_steps), so they
cannot disagree: whatever the switches, a net with storage 'fp16' requested either runs every conv
on an fp16-storage form or keeps the plan of the fp32-storage run -- never an error in the middle
of a run, never other bits.

Each case takes the fp32-storage and the fp16-storage net of one model (both precision 'fp16') over
one input, under the default switches and then one switch at a time.  Every comparison is
torch.equal or equality of the variant codes: there is no tolerance.
"""
import pytest
import torch

from islpose import runtime as rt

from test_gpu_act_storage import _assert_plan, _forward, _inputs, _pair

pytestmark = pytest.mark.gpu

# (environment, split-K mode); the first entry is the default plan
SETTINGS = [({}, 1)] + [({name: value}, 1) for name, value in [
    ("ISLPOSE_FUSED_POOL", "0"), ("ISLPOSE_POOL_INPUT", "0"), ("ISLPOSE_C12", "0"), ("ISLPOSE_C12", "2"),
    ("ISLPOSE_RGB_CONV", "0"), ("ISLPOSE_X3_FUSE67", "1"), ("ISLPOSE_X3_FUSE67", "2"), ("ISLPOSE_X3_FUSE67", "3"),
    ("ISLPOSE_X3_WR", "0"), ("ISLPOSE_X3_WR", "2")]] + [({}, 2)]
SWITCHES = sorted({name for env, _ in SETTINGS for name in env})

# what the default plan must decide (held by test_gpu_act_storage.py too): without these the file
# could pass with every case on one side of the decision
ACTIVE_BY_DEFAULT = {("body25", 2, 368, 656): True, ("body25", 1, 184, 328): False}

SHAPES = [
    ("body25", 1, 64, 96),       # the smoke shape
    ("body25", 1, 184, 328),     # 23x41 planes: K ranges across blocks
    ("body25", 2, 368, 656),
    ("body25", 1, 376, 664),     # odd planes: the pool that cannot defer
    ("body25", 16, 368, 656),    # a chip-filling grid: row union, pooled-input staging
    ("hand", 2, 184, 184),
    ("hand", 16, 368, 368),
    ("coco", 2, 368, 656),
]


@pytest.mark.parametrize("model,n,h,w", SHAPES, ids=["%s-%dx%dx%d" % s for s in SHAPES])
def test_storage_decision_agrees_with_run(monkeypatch, model, n, h, w):
    net32, net16 = _pair(model)
    x = torch.from_numpy(_inputs(n, h, w, 31)).cuda()
    seen, split_k0 = [], (net32.split_k, net16.split_k)
    try:
        for env, split_k in SETTINGS:
            for name in SWITCHES:
                monkeypatch.delenv(name, raising=False)
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            net32.set_split_k(split_k)
            net16.set_split_k(split_k)
            what = (env, split_k)
            ref = _forward(net32, x)
            got = _forward(net16, x)
            assert net32.act_storage_active is False, what
            for a, b in zip(ref, got):
                assert a.shape == b.shape and torch.equal(a, b), what
            active = net16.act_storage_active
            if active:
                _assert_plan(net32, net16)
            else:
                assert net16.op_variants() == net32.op_variants(), what
                assert not any(rt.decode_variant(c).get("act16") for name, c in net16.op_variants()
                               if name != "maxpool2"), what
            seen.append(active)
    finally:
        net32.set_split_k(split_k0[0])
        net16.set_split_k(split_k0[1])
    print("%s %dx%dx%d fp16 storage active per setting:" % (model, n, h, w), seen)
    if (model, n, h, w) in ACTIVE_BY_DEFAULT:
        assert seen[0] is ACTIVE_BY_DEFAULT[(model, n, h, w)]
