"""The K loop of the split-fp16 Winograd kernel (csrc/wino_f16.hip) with its raw pixels read one
channel quad ahead behind hand-placed waits: every path of the loop on the smallest frames that
reach it, against conv_x3 (ISLPOSE_X3_W2=0) and the oracle, and for equal bits from run to run
(a wait placed in front of its data shows as bits that change).  Runs on an MI355X only (-m gpu).

Eligibility needs >= 32 tiles per row and > 1024 pixels per level-3 plane, so:
  (1, 136, 504)  level 3 is 17x63: TW = 32 exactly (every block is one whole band), 9 tile rows
                 (the last band is half empty), odd columns
  (2, 152, 520)  level 3 is 19x65: TW = 33 (blocks straddle two bands); a 38x130 level for
                 conv3_2 / conv3_3; a second frame
Both run c180->128 (23 input chunks: the last pair has no odd chunk), c384->128 (24 pairs) and
c512->512 (32 pairs).  A loop of one or two K steps is not reachable from either net (the fewest
are the 8 pairs of a 128-channel layer), so there is no case for it."""
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from islpose import synth
from islpose import runtime as rt

pytestmark = pytest.mark.gpu
TOL_X3 = 2e-5    # test_gpu_wino2.py: against conv_x3
TOL = 1e-4       # north_star: heatmap/PAF tensors within 1e-4 relative (max|d| / max|ref|) in fp32
FRAMES = [(1, 136, 504), (2, 152, 520)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _inputs(n, h, w, seed):
    f = synth.synth_frames(n, h, w, seed=seed)
    return np.ascontiguousarray(np.transpose(f.astype(np.float32), (0, 3, 1, 2)) / 256 - 0.5)


def _w2_layers(net):
    return [name for name, v in net.op_variants() if rt.decode_variant(v).get("wino2")]


@pytest.fixture(scope="module")
def runs():
    """Per frame, computed once: the Winograd forward twice, the last frame of the batch alone,
    the conv_x3 forward and the oracle's first frame."""
    w25 = synth.synth_weights(rt.ISL_BODY25)
    net = rt.Net(rt.ISL_BODY25)
    net.load_weights(w25)
    ref = cpu_ref.make_net_fn("body25", w25)
    old = os.environ.get("ISLPOSE_X3_W2")
    out = {}
    try:
        for n, h, w in FRAMES:
            x = _inputs(n, h, w, seed=h + 3 * w)
            xt = torch.from_numpy(x).cuda()
            os.environ["ISLPOSE_X3_W2"] = "1"   # every eligible layer on the Winograd kernel
            a = [t.clone() for t in net.forward(xt)]
            torch.cuda.synchronize()
            used = _w2_layers(net)
            b = [t.clone() for t in net.forward(xt)]
            last = [t.clone() for t in net.forward(xt[n - 1:n].contiguous())]
            os.environ["ISLPOSE_X3_W2"] = "0"
            x3 = [t.clone() for t in net.forward(xt)]
            torch.cuda.synchronize()
            used_x3 = _w2_layers(net)
            out[(n, h, w)] = dict(a=a, b=b, last=last, x3=x3, used=used, used_x3=used_x3, ref=ref(x[:1]))
    finally:
        if old is None:
            os.environ.pop("ISLPOSE_X3_W2", None)
        else:
            os.environ["ISLPOSE_X3_W2"] = old
    return out


@pytest.mark.parametrize("n,h,w", FRAMES)
def test_loop_layers_on_winograd(runs, n, h, w):
    r = runs[(n, h, w)]
    used = set(r["used"])
    # c512 -> 512, c180 -> 128 (23 chunks), c384 -> 128, a 128-channel layer (8 pairs)
    assert {"conv4_2", "Mconv1_stage1_L2_0", "Mconv2_stage1_L2_0", "Mconv2_stage1_L2_1"} <= used, used
    if (h // 4) * (w // 4) > 1024 and (w // 4 + 1) // 2 >= 32:
        assert {"conv3_2", "conv3_3"} <= used, used
    assert not r["used_x3"], r["used_x3"]


@pytest.mark.parametrize("n,h,w", FRAMES)
def test_loop_vs_x3_and_oracle(runs, n, h, w):
    r = runs[(n, h, w)]
    ep, eh = (_rel(r["a"][i].cpu().numpy(), r["x3"][i].cpu().numpy()) for i in (0, 1))
    print("wino2 vs x3: paf %.3g heat %.3g (%d layers)" % (ep, eh, len(r["used"])))
    assert ep < TOL_X3 and eh < TOL_X3, (ep, eh)
    op, oh = (_rel(r["a"][i][:1].cpu().numpy(), r["ref"][i]) for i in (0, 1))
    print("wino2 vs oracle: paf %.3g heat %.3g" % (op, oh))
    assert op < TOL and oh < TOL, (op, oh)


@pytest.mark.parametrize("n,h,w", FRAMES)
def test_loop_same_bits_twice(runs, n, h, w):
    r = runs[(n, h, w)]
    assert torch.equal(r["a"][0], r["b"][0]) and torch.equal(r["a"][1], r["b"][1])


@pytest.mark.parametrize("n,h,w", FRAMES)
def test_loop_frame_alone_equals_frame_in_batch(runs, n, h, w):
    r = runs[(n, h, w)]
    assert torch.equal(r["a"][0][n - 1:n], r["last"][0]) and torch.equal(r["a"][1][n - 1:n], r["last"][1])
