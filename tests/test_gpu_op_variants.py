"""What every op of a run becomes (Net.op_variants()), held to golden/op_variants.json: the codes
the commit before csrc/x3_select.cpp reported, when its launchers still left them behind after the
launch.  Now they come from the launch plan (plan_steps: x3_choose), before anything runs.

The eight shapes of test_gpu_plan_agreement.py -- the smallest that still reach the row union,
pooled-input staging, across-block K ranges and the wave-range kernel -- at the three precision /
storage settings and split-K modes 1 and 2, under the default switches.  Equality of integers.
The golden holds each distinct list of codes once ("plans") and the case that runs it ("cases").
"""
import json
import os

import pytest
import torch

from test_gpu_act_storage import _inputs, _net
from test_gpu_plan_agreement import SHAPES

pytestmark = pytest.mark.gpu
FORMS = [("fp32", "fp32"), ("fp16", "fp32"), ("fp16", "fp16")]

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_variants.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize("model,n,h,w", SHAPES, ids=["%s-%dx%dx%d" % s for s in SHAPES])
def test_op_variants_equal_the_recorded_plan(monkeypatch, model, n, h, w):
    for name in list(os.environ):
        if name.startswith("ISLPOSE_X3_") or name in ("ISLPOSE_C12", "ISLPOSE_RGB_CONV", "ISLPOSE_FUSED_POOL",
                                                      "ISLPOSE_POOL_INPUT", "ISLPOSE_A16_DMA"):
            monkeypatch.delenv(name)
    net = _net(model, "fp32", "fp32")
    x = torch.from_numpy(_inputs(n, h, w, 31)).cuda()
    for prec, store in FORMS:
        net.set_precision(prec)
        net.set_act_storage(store)
        for split_k in (1, 2):
            net.set_split_k(split_k)
            net.forward(x)
            torch.cuda.synchronize()
            key = "%s-%dx%dx%d/%s/%s/%d" % (model, n, h, w, prec, store, split_k)
            ops = net.op_variants()
            want = GOLDEN["plans"][GOLDEN["cases"][key]]   # the code of every op, in order
            diff = [(name, w_, int(g)) for (name, g), w_ in zip(ops, want) if w_ != int(g)]
            assert not diff and len(ops) == len(want), (key, diff[:3])
