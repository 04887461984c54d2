"""The ends of the Winograd K loop (csrc/wino_f16.hip) with its filter loads and DMA pieces issued
inside the step: loops of 1, 2, 3 and 5 chunk pairs (16, 32, 48 and 80 input channels), where the
loads past the last pair repeat it and the counted waits meet the prologue's queue.  No graph has
such a layer, so the cases run one layer through isl_debug_conv3x3, on the planes of
test_gpu_wino2_loop.py: 17x63 (exactly 32 tiles per row) and 19x65 (blocks over two bands), batch 2,
64 and 128 output channels.  Each against conv_x3 and the oracle (torch-CPU conv2d in float64)
within that file's tolerances, for equal bits from run to run (a wait in front of its data shows
as bits that change) and for frame 1 alone against frame 1 in the batch.  Runs on an MI355X only
(-m gpu)."""
import os

import numpy as np
import pytest
import torch

from islpose import runtime as rt

pytestmark = pytest.mark.gpu
TOL_X3 = 2e-5    # test_gpu_wino2_loop.py: against conv_x3
TOL = 1e-4       # ... and against the oracle (max|d| / max|ref|)
PLANES = [(17, 63), (19, 65)]
CASES = [(cin, cout, h, w) for cin in (16, 32, 48, 80) for cout in (64, 128) for h, w in PLANES]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _layer(cin, cout, h, w):
    g = np.random.default_rng(1000 * cin + 10 * cout + h)
    x = g.uniform(-1, 1, (2, cin, h, w)).astype(np.float32)
    wt = (g.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = g.uniform(-0.1, 0.1, cout).astype(np.float32)
    s = g.uniform(0.05, 0.25, cout).astype(np.float32)
    return x, wt, b, s


def _oracle(x, wt, b, s):
    t = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(),
                                   torch.from_numpy(b).double(), padding=1)
    return torch.where(t >= 0, t, t * torch.from_numpy(s).double()[None, :, None, None]).numpy()


@pytest.fixture(scope="module")
def runs():
    """Per case, computed once: the Winograd layer twice, frame 1 alone, conv_x3 and the oracle."""
    old = os.environ.get("ISLPOSE_X3_W2")
    os.environ["ISLPOSE_X3_W2"] = "1"
    out = {}
    try:
        for case in CASES:
            x, wt, b, s = _layer(*case)
            out[case] = dict(a=rt.debug_conv3x3(x, wt, b, s, "wino2"), b=rt.debug_conv3x3(x, wt, b, s, "wino2"),
                             last=rt.debug_conv3x3(x[1:2], wt, b, s, "wino2"),
                             x3=rt.debug_conv3x3(x, wt, b, s, "x3"), ref=_oracle(x, wt, b, s))
    finally:
        if old is None:
            os.environ.pop("ISLPOSE_X3_W2", None)
        else:
            os.environ["ISLPOSE_X3_W2"] = old
    return out


@pytest.mark.parametrize("cin,cout,h,w", CASES)
def test_issue_vs_x3_and_oracle(runs, cin, cout, h, w):
    r = runs[(cin, cout, h, w)]
    e3, eo = _rel(r["a"], r["x3"]), _rel(r["a"], r["ref"])
    print("c%d->%d %dx%d (%d pairs): vs x3 %.3g, vs oracle %.3g" % (cin, cout, h, w, cin // 16, e3, eo))
    assert e3 < TOL_X3, e3
    assert eo < TOL, eo


@pytest.mark.parametrize("cin,cout,h,w", CASES)
def test_issue_same_bits_twice(runs, cin, cout, h, w):
    r = runs[(cin, cout, h, w)]
    assert np.array_equal(r["a"].view(np.uint32), r["b"].view(np.uint32))


@pytest.mark.parametrize("cin,cout,h,w", CASES)
def test_issue_frame_alone_equals_frame_in_batch(runs, cin, cout, h, w):
    r = runs[(cin, cout, h, w)]
    assert np.array_equal(r["a"][1:2].view(np.uint32), r["last"].view(np.uint32))


def test_debug_conv3x3_rejects_ineligible_shape():
    x, wt, b, s = _layer(16, 64, 17, 63)
    with pytest.raises(rt.IslError):
        rt.debug_conv3x3(x[:, :, :, :31], wt, b, s, "wino2")   # 16 tiles per row
