"""The hand-path options (hand_scales, flip_left, hand_info / flip, return_scores), CPU side: the
validation at every constructor, util.hand_boxes against handDetect's goldens, and the CPU
seam's statement of the mirror and score rules on designed maps."""
import os
import re

import numpy as np
import pytest
import torch

from islpose import cpu
from islpose import runtime as rt
from islpose import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAN, INF = float("nan"), float("inf")
EIGHT = (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)
BAD_SCALES = [(), EIGHT + (2.25,), (0,), (1.0, 0), (-1.0,), (NAN,), (INF,), (1e-3,)]


def _torch_weights(kind):
    return {k: torch.from_numpy(v) for k, v in synth.synth_weights(kind).items()}


def test_symbols_declared_and_exported():
    text = open(os.path.join(REPO, "include", "islpose.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(isl_\w+)\s*\(", text, re.M))
    new = {"isl_net_preprocess_crops_flip", "isl_hand_post_ex", "isl_hand_post_crops_ex"}
    assert new <= declared and new <= set(rt.EXPORTS)
    assert re.search(r"#define\s+ISL_ABI_VERSION\s+1\b", text)          # additions only


def test_check_hand_opts():
    assert rt.check_hand_opts() == {"hand_scales": (0.5, 1.0, 1.5, 2.0), "flip_left": False}
    assert rt.check_hand_opts(None, False) == rt.check_hand_opts()
    assert rt.check_hand_opts((1.0,)) == {"hand_scales": (1.0,), "flip_left": False}
    assert rt.check_hand_opts([1, 1.5], True) == {"hand_scales": (1.0, 1.5), "flip_left": True}
    assert rt.check_hand_opts(EIGHT)["hand_scales"] == EIGHT and len(EIGHT) == rt.MAX_HAND_SCALES
    assert rt.check_hand_opts((8 / 368,))["hand_scales"] == (8 / 368,)      # round(s * 368) == 8: the smallest
    for bad in BAD_SCALES + [1.0, "x", (None,)]:
        with pytest.raises(ValueError):
            rt.check_hand_opts(bad)
    with pytest.raises(ValueError):
        rt.check_hand_opts(None, 1)


def test_constructors_validate():
    """ValueError at construction, GPU or not (before the feature: TypeError, no such keyword)."""
    from islpose.hand import HandEstimator
    from src.ISL_Model_parameter import ISLSignPos, ISLSignPosTranslator
    from src.body import Body
    from src.hand import Hand
    wb, wh = _torch_weights(0), _torch_weights(2)
    body, hand = Body(wb, "body25"), Hand(wh)
    for bad in BAD_SCALES:
        with pytest.raises(ValueError):
            Hand(wh, scales=bad)
        with pytest.raises(ValueError):
            HandEstimator(scale_search=bad)
        with pytest.raises(ValueError):
            ISLSignPos(body.model, hand.model, hand_scales=bad)
        with pytest.raises(ValueError):
            ISLSignPosTranslator(body.model, hand.model, None, hand_scales=bad)
    assert Hand(wh).scales == (0.5, 1.0, 1.5, 2.0) and Hand(wh, scales=(1.0,)).scales == (1.0,)
    assert Hand(wh, scales=EIGHT).scales == EIGHT
    isl = ISLSignPos(body.model, hand.model)
    assert isl.hand_opts == rt.check_hand_opts() and isl.hand_info is False
    isl = ISLSignPosTranslator(body.model, hand.model, None, hand_scales=(1.0,), flip_left=True, hand_info=True)
    assert isl.hand_opts == {"hand_scales": (1.0,), "flip_left": True} and isl.hand_info is True
    with pytest.raises(TypeError):          # the reference's positional signature is untouched
        Hand(wh, (1.0,))


def test_state_key_follows_each_option():
    from src.ISL_Model_parameter import ISLSignPos
    from src.body import Body
    from src.hand import Hand
    body, hand = Body(_torch_weights(0), "body25"), Hand(_torch_weights(2))
    k0 = ISLSignPos(body.model, hand.model).state_key()
    assert ISLSignPos(body.model, hand.model, hand_scales=(0.5, 1.0, 1.5, 2.0), flip_left=False,
                      hand_info=False).state_key() == k0
    keys = {k0}
    for kw in (dict(hand_scales=(1.0,)), dict(hand_scales=(0.5, 1.0, 1.5)), dict(flip_left=True), dict(hand_info=True),
               dict(flip_left=True, hand_info=True), dict(hand_scales=(1.0,), flip_left=True)):
        keys.add(ISLSignPos(body.model, hand.model, **kw).state_key())
    assert len(keys) == 7


def test_hand_boxes_golden():
    """hand_boxes == handDetect in its first four fields and order on the G5 cases, and
    person_row is the subset row whose arm gives that box (handDetect on that row alone)."""
    from src import util
    z = np.load(os.path.join(GOLDEN, "g5_hand_detect.npz"))
    n_boxes, rows_seen = 0, set()
    for c in sorted({k.split("/")[0] for k in z.files}):
        cand, subset = z[c + "/candidate"], z[c + "/subset"]
        img = np.zeros(tuple(z[c + "/img_hw"]) + (3,))
        got = util.hand_boxes(cand, subset, img)
        assert all(len(b) == 5 for b in got)
        four = np.array([[x, y, w, int(l)] for x, y, w, l, _ in got], np.int64).reshape(-1, 4)
        assert np.array_equal(four, z[c + "/result"]), c
        assert [b[:4] for b in got] == util.handDetect(cand, subset, img)
        rows = [b[4] for b in got]
        assert rows == sorted(rows) and all(isinstance(r, int) and 0 <= r < len(subset) for r in rows)
        for r in set(rows):
            alone = util.handDetect(cand, subset[r:r + 1], img)
            assert alone == [b[:4] for b in got if b[4] == r], (c, r)
        n_boxes += len(got)
        rows_seen |= set(rows)
    assert n_boxes > 0 and len(rows_seen) > 1


def _designed(seed=7):
    """Low-res maps of a 57 x 57 image at one scale (net 184 -> 23 x 23): part 3 all zero,
    part 5 a single peak in the corner pixel, the others designed blobs."""
    m = synth.designed_hand_maps(23, 23, seed=seed, n_blobs=3).copy()
    m[3] = 0
    m[5] = 0
    m[5, 0, 0], m[5, 0, 1], m[5, 1, 0] = 0.9, 0.5, 0.5
    return m


def test_cpu_hand_call_flip_and_scores():
    """cpu.hand_call(flip=True, return_scores=True) on an image == the call on img[:, ::-1] with
    the detected x mirrored back and the same scores; an all-zero part is [0, 0] with score 0.0;
    the corner part is found at x = W - 1 with a positive score, not taken for 'nothing found'.
    The stub net answers from the image it is given, so a wrong or missing mirror shows."""
    W = 57
    img = synth.synth_frames(1, W, W, seed=3)[0]
    a, b = _designed(7), _designed(8)
    seen = []

    def net_fn(im):
        # the sign of the input's left-right moment tells the image from its mirror
        assert im.shape[1] == 3
        t = float((im[0].astype(np.float64) * np.linspace(-1, 1, im.shape[3])).sum())
        seen.append(t)
        return (a if t > 0 else b)[None]

    scales = (0.5,)
    plain, sc_plain = cpu.hand_call(img, net_fn, scales, return_scores=True)
    assert np.array_equal(plain, cpu.hand_call(img, net_fn, scales))            # the peaks are the old result
    mir, sc_mir = cpu.hand_call(np.ascontiguousarray(img[:, ::-1]), net_fn, scales, return_scores=True)
    got, sc = cpu.hand_call(img, net_fn, scales, flip=True, return_scores=True)
    assert sc.dtype == np.float64 and sc.shape == (21,) and got.shape == (21, 2)
    assert np.array_equal(sc, sc_mir)
    found = sc_mir > 0
    want = mir.copy()
    want[found, 0] = W - 1 - mir[found, 0]
    assert np.array_equal(got, want)
    assert np.array_equal(cpu.hand_call(img, net_fn, scales, flip=True), want)
    assert not np.array_equal(sc_plain, sc_mir)             # the two images gave different maps
    for peaks, s, x0 in ((plain, sc_plain, 0), (mir, sc_mir, 0), (got, sc, W - 1)):
        assert list(peaks[3]) == [0, 0] and s[3] == 0.0                          # nothing found
        assert list(peaks[5]) == [x0, 0] and s[5] > 0                            # found in the corner
    assert found.sum() >= 15 and not found[3]
    assert min(abs(t) for t in seen) > 1.0 and {t > 0 for t in seen} == {True, False}
