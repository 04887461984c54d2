"""Augmented extraction on the GPU: isl_augment against the numpy restatement of the variant
definition (tests/_augment.py) byte for byte, its refusals, ISLSignPos.call_augmented against
call_batch on host-built variants, and KeypointExtractor(transforms=...) on the overlapped path."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _augment as ref
import _tame
from islpose import augment, pipeline, synth
from islpose import runtime as rt

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 96), (61, 98), (120, 160), (1, 7), (5, 1)]
ANGLES = [0, 17.3, -30, 45, 180, 30, -29]
SRC = [2, 0, 0, 1, 2]


def _items(a, b):
    """Five items from three frames: a plain copy, two rotations, a solarize, both."""
    return [augment.Item(SRC[0], None, 256), augment.Item(SRC[1], a, 256), augment.Item(SRC[2], b, 256),
            augment.Item(SRC[3], None, 192), augment.Item(SRC[4], a, 100)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_isl_augment_equals_the_definition(h, w):
    fr = np.random.default_rng(h * 1000 + w).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    t = torch.from_numpy(fr).cuda()
    side = torch.cuda.Stream()
    angles = ANGLES + ([90] if h % 2 and w % 2 else [])
    for k, a in enumerate(angles):
        items = _items(a, angles[(k + 1) % len(angles)])
        for swap in (False, True):
            want = ref.variants(fr, items, swap_rb=swap)
            got = augment.apply(t, items, swap_rb=swap)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (5, h, w, 3)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (h, w, a, swap)
        # a non-default stream
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = augment.apply(t, items, swap_rb=True)
        side.synchronize()
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (h, w, a, "stream")


def test_unaligned_item_bases_and_many_items():
    """61 x 98 x 3 = 17934 bytes per item: item k starts at every 16-byte phase in turn (the
    scalar head and tail of the wide stores), and more items than the table ring has slots in
    back-to-back calls."""
    fr = np.random.default_rng(5).integers(0, 256, (3, 61, 98, 3), dtype=np.uint8)
    t = torch.from_numpy(fr).cuda()
    items = [augment.Item(k % 3, [None, 17.3, -29.0][k % 3], [256, 192][k % 2]) for k in range(16)]
    want = torch.from_numpy(ref.variants(fr, items, swap_rb=True))
    outs = [augment.apply(t, items, swap_rb=True) for _ in range(12)]
    torch.cuda.synchronize()
    assert all(torch.equal(o.cpu(), want) for o in outs)


def test_refusals_and_the_empty_call():
    L = rt.lib()
    h, w = 8, 10
    frame = h * w * 3
    buf = torch.full((8 * frame,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((2, h, w, 3), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = rt.stream_handle()

    def call(src_ptr, n_src, dst_ptr, items, m=None):
        arr = (rt.IslAugItem * max(len(items), 1))(*items)
        rc = L.isl_augment(ctypes.c_void_p(src_ptr), n_src, h, w, ctypes.c_void_p(dst_ptr), arr,
                           len(items) if m is None else m, st)
        return rc, L.isl_last_error().decode()

    ok = rt.IslAugItem(1.0, 0.0, 0, 0, 256, 0)
    src = buf.data_ptr()
    # d_dst inside d_src, d_src inside d_dst, and ranges one byte apart
    for s_ptr, n_src, d_ptr, m in ((src, 3, src + 2 * frame, 2), (src + frame, 2, src, 2), (src, 3, src + 1, 1)):
        rc, msg = call(s_ptr, n_src, d_ptr, [ok] * m)
        assert rc == rt.ISL_E_ARG and "overlaps" in msg, msg
    rc, msg = call(src, 3, dst.data_ptr(), [ok, rt.IslAugItem(1.0, 0.0, 3, 0, 256, 0)])
    assert rc == rt.ISL_E_ARG and "src index 3" in msg and "item 1" in msg, msg
    rc, msg = call(src, 3, dst.data_ptr(), [rt.IslAugItem(1.0, 0.0, -1, 0, 256, 0)])
    assert rc == rt.ISL_E_ARG and "src index -1" in msg, msg
    for thr in (257, -1):
        rc, msg = call(src, 3, dst.data_ptr(), [ok, rt.IslAugItem(1.0, 0.0, 0, 0, thr, 0)])
        assert rc == rt.ISL_E_ARG and "threshold %d" % thr in msg, msg
    rc, msg = call(src, 3, dst.data_ptr(), [ok], m=-1)
    assert rc == rt.ISL_E_ARG and "m = -1" in msg, msg
    rc, msg = call(src, 3, dst.data_ptr(), [ok], m=65536)
    assert rc == rt.ISL_E_ARG and "65536" in msg, msg
    rc, msg = call(src, 3, dst.data_ptr(), [rt.IslAugItem(math.nan, 0.0, 0, 1, 256, 0)])
    assert rc == rt.ISL_E_ARG and "finite" in msg, msg
    assert call(src, 3, dst.data_ptr(), [ok], m=0)[0] == rt.ISL_OK          # the empty call
    assert call(0, 0, 0, [ok], m=0)[0] == rt.ISL_OK
    torch.cuda.synchronize()
    assert bool((dst == 9).all()) and bool((buf == 7).all())               # nothing was launched
    # touching but disjoint ranges are accepted
    rc, msg = call(src, 3, src + 3 * frame, [ok, ok])
    assert rc == rt.ISL_OK, msg
    torch.cuda.synchronize()
    assert bool((buf == 7).all())
    # the Python layer's errors
    t = buf[:3 * frame].view(3, h, w, 3)
    with pytest.raises(ValueError, match="5"):
        augment.apply(t, [augment.Item(5, None, 256)])
    with pytest.raises(ValueError, match="999"):
        augment.apply(t, [augment.Item(0, None, 999)])
    with pytest.raises(ValueError):
        augment.apply(t.cpu(), [augment.Item(0, None, 256)])
    assert tuple(augment.apply(t, []).shape) == (0, h, w, 3)


@pytest.fixture(scope="module")
def isl_model():
    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPos
    frames = synth.synth_frames(3, 240, 320, seed=31)
    wb = _tame.tame_body(synth.synth_weights(0), frames[0], scale=0.5 * 368 / 240, gain=0.05)
    tw = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    body, hand = Body(tw(wb), "body25"), Hand(tw(synth.synth_weights(2)))
    return ISLSignPos(body.model, hand.model), frames


def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb) == 3
        for x, y in zip(ra[:2], rb[:2]):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert len(ra[2]) == len(rb[2])
        for x, y in zip(ra[2], rb[2]):
            assert np.array_equal(x, y) and x.dtype == y.dtype


def test_call_augmented_equals_call_batch_on_host_variants(isl_model):
    isl, frames = isl_model
    bgr = np.ascontiguousarray(frames[:2, ..., ::-1])
    ts = [augment.Rotate(17.3), augment.Solarize(192)]
    host = np.concatenate([bgr, np.stack([ref.variant(f, 17.3) for f in bgr]),
                           np.stack([ref.variant(f, None, 192) for f in bgr])])
    want = isl.call_batch(host)
    assert sum(len(r[0]) for r in want[:2]) >= 1          # the originals give candidates
    got = isl.call_augmented(bgr, ts)
    assert list(got) == ["original", "Rotate", "Solarize"]
    for j, name in enumerate(got):
        _same(got[name], want[2 * j:2 * j + 2])
    # device frames in, the same results
    dev = isl.call_augmented(torch.from_numpy(bgr).cuda(), ts)
    for name in got:
        _same(dev[name], got[name])
    with pytest.raises(ValueError):
        isl.call_augmented(bgr, [augment.Rotate(1), augment.Rotate(2)])
    with pytest.raises(ValueError):
        isl.call_augmented(bgr, ts, keys=[("v", 0)])


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".json"):
                p = os.path.join(d, f)
                out[os.path.relpath(p, root)] = open(p).read()
    return out


def test_extractor_overlapped_with_random_transforms(isl_model, tmp_path):
    isl, frames = isl_model
    base = tmp_path / "data"
    os.makedirs(base)
    np.save(base / "clip.npy", frames)
    rows = [{"Filepath": "clip.npy", "type": "T", "expression": "x"}]
    ts = [augment.RandomRotation(30, seed=3), augment.RandomSolarize(192, 0.5, seed=3)]
    out = str(tmp_path / "aug")
    feats, ex = pipeline.extract_dataset(rows, pipeline.npy_decoder(str(base)), isl, out, batch=9, export=False,
                                         overlap=True, transforms=ts)
    assert ex.frames_done == 9 and len(feats) == 9
    # the same nine units built on the host, in the extractor's order, through call_batch
    bgr = np.ascontiguousarray(frames[..., ::-1])
    units, host = [], []
    for i in range(3):
        units.append((i, "original"))
        host.append(bgr[i])
        for k, t in enumerate(ts):
            p = augment.params_for(t, "clip.npy", i, k)
            units.append((i, t.name))
            host.append(ref.variant(bgr[i], p.angle, p.threshold))
    want = isl.call_batch(np.stack(host))
    assert [(f["frame_no"], f["transform"]) for f in feats] == units
    for f, res in zip(feats, want):
        assert f["filepath"] == pipeline.json_path(out, "T", "x", "clip.npy", f["frame_no"], f["transform"])
        assert open(f["filepath"]).read() == pipeline.frame_json(*res)
    # the -original files are those of a run without transforms
    plain = str(tmp_path / "plain")
    pipeline.extract_dataset(rows, pipeline.npy_decoder(str(base)), isl, plain, batch=9, export=False, overlap=True)
    tree = _tree(out)
    assert len(tree) == 9 and {p: v for p, v in tree.items() if "-original" in p} == _tree(plain)
    # a second run computes nothing
    feats2, ex2 = pipeline.extract_dataset(rows, pipeline.npy_decoder(str(base)), isl, out, batch=9, export=False,
                                           overlap=True, transforms=ts)
    assert feats2 == [] and ex2.frames_done == 0 and ex2.frames_skipped == 9
