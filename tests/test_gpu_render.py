"""Stick-model overlays on the GPU: isl_draw against the scalar statement of the drawing
definition (tests/_render.py) byte for byte -- in place, out of place and on the blank canvas --
its guard bands and refusals, and ISLSignPos.render against islpose.render.apply_numpy."""
import ctypes

import numpy as np
import pytest
import torch

import _render as ref
import _tame
from islpose import render, synth
from islpose import runtime as rt

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _guarded(frames, offset):
    """A copy of `frames` at byte `offset` of a canary-filled flat buffer, as (buffer, view)."""
    size = frames.size
    buf = torch.full((size + 2 * 4096,), CANARY, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + size].view(frames.shape)
    view.copy_(torch.from_numpy(np.array(frames)))
    return buf, view


def _guards_intact(buf, offset, size):
    return bool((buf[:offset] == CANARY).all()) and bool((buf[offset + size:] == CANARY).all())


@pytest.mark.parametrize("name", list(ref.CASES))
def test_isl_draw_equals_the_definition(name):
    frames, lists, want, blank = ref.case(name)
    assert not np.array_equal(want, frames)
    src = torch.from_numpy(np.array(frames)).cuda()
    # out of place, into a new tensor; the source stays
    got = render.apply(src, lists)
    assert got.dtype == torch.uint8 and got.shape == src.shape and got.data_ptr() != src.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(src.cpu().numpy(), frames)
    # in place equals out of place
    work = src.clone()
    assert render.apply(work, lists, out=work) is work
    assert np.array_equal(work.cpu().numpy(), want)
    # the blank canvas, into a destination full of something else
    dst = torch.full_like(src, 77)
    render.apply(None, lists, out=dst)
    assert np.array_equal(dst.cpu().numpy(), blank)
    assert np.array_equal(render.apply(None, lists, shape=frames.shape).cpu().numpy(), blank)
    # no primitives: out of place the source, on the blank canvas zeros
    none = [[] for _ in lists]
    assert np.array_equal(render.apply(src, none).cpu().numpy(), frames)
    assert not render.apply(None, none, out=torch.full_like(src, 77)).any()
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = render.apply(src, lists)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["wide", "odd", "tiles", "many"])
@pytest.mark.parametrize("src_off,dst_off", [(4096, 4096), (4096, 4096 + 1), (4096 + 3, 4096 + 2),
                                             (4096 + 2, 4096)])
def test_odd_byte_offsets_and_guard_bands(name, src_off, dst_off):
    """Source and destination at byte offsets of every phase inside canary-filled buffers:
    the bytes before and after the destination stay, out of place, in place and blank."""
    frames, lists, want, blank = ref.case(name)
    sbuf, sview = _guarded(frames, src_off)
    dbuf, dview = _guarded(np.full_like(frames, 77), dst_off)
    render.apply(sview, lists, out=dview)
    assert np.array_equal(dview.cpu().numpy(), want)
    assert _guards_intact(dbuf, dst_off, frames.size) and _guards_intact(sbuf, src_off, frames.size)
    assert np.array_equal(sview.cpu().numpy(), frames)
    render.apply(None, lists, out=dview)
    assert np.array_equal(dview.cpu().numpy(), blank)
    assert _guards_intact(dbuf, dst_off, frames.size)
    render.apply(sview, lists, out=sview)
    assert np.array_equal(sview.cpu().numpy(), want)
    assert _guards_intact(sbuf, src_off, frames.size)


def test_order_is_part_of_the_result():
    frames, lists, want, _ = ref.case("odd")
    rev = [list(reversed(ref.ORDERED)) + lists[0][len(ref.ORDERED):]] + lists[1:]
    want_rev, _ = ref.draw(frames[:1], rev[:1])
    assert not np.array_equal(want_rev, want[:1])
    got = render.apply(torch.from_numpy(np.array(frames)).cuda(), rev).cpu().numpy()
    assert np.array_equal(got[:1], want_rev) and np.array_equal(got[1:], want[1:])


def test_in_place_leaves_untouched_tiles_unwritten_and_empty_calls_alone():
    """In place with nothing to draw, and n = 0, launch nothing (an unsynchronised canary
    stays); a list whose primitives all lie off the frame changes no byte."""
    frames, lists, _, _ = ref.case("gap")
    t = torch.from_numpy(np.array(frames)).cuda()
    render.apply(t, [[], [], []], out=t)
    off = [[ref.disc(-50, -50, 16, (1, 2, 3)), ref.stick(500, 500, 20, 4, 30, (4, 5, 6))]] * 3
    render.apply(t, off, out=t)
    assert np.array_equal(t.cpu().numpy(), frames)
    empty = torch.empty((0, 20, 40, 3), dtype=torch.uint8, device="cuda")
    assert tuple(render.apply(empty, []).shape) == (0, 20, 40, 3)


def test_refusals_touch_nothing():
    L = rt.lib()
    h, w = 8, 10
    frame = h * w * 3
    buf = torch.full((8 * frame,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((2, h, w, 3), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = rt.stream_handle()
    P = rt.IslDrawPrim

    def call(src_ptr, dst_ptr, n, prims, first, hh=h, ww=w, null_prims=False, null_first=False):
        arr = (P * max(len(prims), 1))(*prims)
        fst = (ctypes.c_int32 * len(first))(*first)
        rc = L.isl_draw(ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), n, hh, ww,
                        None if null_prims else arr, None if null_first else fst, st)
        return rc, L.isl_last_error().decode()

    ok = P(1, (3, 3, 0, 0), 0, 0, 16, (1, 2, 3), 0, 0)
    src, d = buf.data_ptr(), dst.data_ptr()
    rc, msg = call(src, 0, 2, [ok], [0, 1, 1])
    assert rc == rt.ISL_E_ARG and "d_dst" in msg, msg
    # partial overlaps: shifted by a frame, by a byte, either way round
    for s_ptr, d_ptr in ((src, src + frame), (src + frame, src), (src, src + 1), (src + 1, src)):
        rc, msg = call(s_ptr, d_ptr, 2, [ok], [0, 1, 1])
        assert rc == rt.ISL_E_ARG and "overlaps" in msg, msg
    for n, hh, ww in ((-1, h, w), (2, 0, w), (2, h, 0), (2, 16385, 1), (2, 1, 16385), (2, 16384 * 2, 16384 + 1),
                      (1, 16384, 16384 * 2 + 1)):
        rc, msg = call(src, d, n, [ok], [0, 1, 1], hh, ww)
        assert rc == rt.ISL_E_ARG and ("shape" in msg or "negative" in msg), msg
    rc, msg = call(src, d, 2, [ok], [1, 1, 1])
    assert rc == rt.ISL_E_ARG and "first[0]" in msg, msg
    rc, msg = call(src, d, 2, [ok, ok], [0, 2, 1])
    assert rc == rt.ISL_E_ARG and "decreases" in msg, msg
    rc, msg = call(src, d, 2, [ok], [0, 1, (1 << 20) + 1])
    assert rc == rt.ISL_E_ARG and "2^20" in msg, msg
    rc, msg = call(src, d, 2, [ok], [0, 1, 1], null_prims=True)
    assert rc == rt.ISL_E_ARG and "prims" in msg, msg
    rc, msg = call(src, d, 2, [ok], [0, 1, 1], null_first=True)
    assert rc == rt.ISL_E_ARG and "first" in msg, msg
    bad = {
        "kind": [P(3, (3, 3, 0, 0), 0, 0, 16, (1, 2, 3), 0, 0), P(-1, (3, 3, 0, 0), 0, 0, 16, (1, 2, 3), 0, 0)],
        "blend": [P(1, (3, 3, 0, 0), 0, 0, 16, (1, 2, 3), 2, 0)],
        "reserved": [P(1, (3, 3, 0, 0), 0, 0, 16, (1, 2, 3), 0, 1)],
        "coordinate": [P(1, (16385, 3, 0, 0), 0, 0, 16, (1, 2, 3), 0, 0), P(1, (3, -16385, 0, 0), 0, 0, 16, (1, 2, 3), 0, 0),
                       P(2, (3, 3, 16385, 0), 0, 0, 2, (1, 2, 3), 0, 0), P(2, (3, 3, 0, -16385), 0, 0, 2, (1, 2, 3), 0, 0),
                       P(0, (-16385, 3, 5, 4), 16384, 0, 0, (1, 2, 3), 1, 0)],
        "half axes": [P(0, (3, 3, 0, 4), 16384, 0, 0, (1, 2, 3), 1, 0), P(0, (3, 3, 4097, 4), 16384, 0, 0, (1, 2, 3), 1, 0),
                      P(0, (3, 3, 5, 0), 16384, 0, 0, (1, 2, 3), 1, 0), P(0, (3, 3, 5, 17), 16384, 0, 0, (1, 2, 3), 1, 0)],
        "c, s": [P(0, (3, 3, 5, 4), 16385, 0, 0, (1, 2, 3), 1, 0), P(0, (3, 3, 5, 4), 0, -16385, 0, (1, 2, 3), 1, 0)],
        "r2": [P(1, (3, 3, 0, 0), 0, 0, -1, (1, 2, 3), 0, 0), P(1, (3, 3, 0, 0), 0, 0, 4097, (1, 2, 3), 0, 0),
               P(2, (3, 3, 5, 5), 0, 0, 4097, (1, 2, 3), 0, 0)],
    }
    for word, prims in bad.items():
        for q in prims:
            for s_ptr in (src, d, 0):                     # out of place, in place, blank
                rc, msg = call(s_ptr, d, 2, [ok, q], [0, 1, 2])
                assert rc == rt.ISL_E_ARG and word in msg and "primitive 1" in msg, (word, msg)
    torch.cuda.synchronize()
    assert bool((dst == 9).all()) and bool((buf == 7).all())        # nothing was launched
    # n = 0 and the in-place call without primitives are no-ops
    assert call(src, d, 0, [ok], [0])[0] == rt.ISL_OK
    assert call(d, d, 2, [ok], [0, 0, 0], null_prims=True)[0] == rt.ISL_OK
    torch.cuda.synchronize()
    assert bool((dst == 9).all())
    # touching but disjoint ranges are accepted
    rc, msg = call(src, src + 2 * frame, 2, [ok], [0, 1, 1])
    assert rc == rt.ISL_OK, msg
    torch.cuda.synchronize()
    assert bool((buf[:2 * frame] == 7).all()) and bool((buf[4 * frame:] == 7).all())
    # the Python layer
    t = buf[:2 * frame].view(2, h, w, 3)
    with pytest.raises(ValueError):
        render.apply(t.cpu(), [[], []])
    with pytest.raises(ValueError, match="lists"):
        render.apply(t, [[]])
    with pytest.raises(ValueError, match="out"):
        render.apply(t, [[], []], out=torch.empty((2, h, w + 1, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="kind"):
        render.apply(t, [[(5, (0, 0, 0, 0), 0, 0, 0, (0, 0, 0), 0)], []])
    with pytest.raises(rt.IslError, match="overlaps"):
        render.apply(t, [[], []], out=buf[frame:3 * frame].view(2, h, w, 3))


@pytest.fixture(scope="module")
def isl_model():
    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPos
    frames = synth.synth_frames(2, 184, 328, seed=31)
    wb = _tame.tame_body(synth.synth_weights(0), frames[0], scale=1.0, gain=0.05)
    tw = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    body, hand = Body(tw(wb), "body25"), Hand(tw(synth.synth_weights(2)))
    return ISLSignPos(body.model, hand.model), frames


def test_islsignpos_render_equals_apply_numpy(isl_model):
    isl, frames = isl_model
    bgr = np.ascontiguousarray(frames[..., ::-1])
    results = isl.call_batch(bgr)
    lists = isl.render_primitives(results)
    assert sum(len(lst) for lst in lists) >= 1            # something is drawn
    want = render.apply_numpy(bgr, lists)
    assert not np.array_equal(want, bgr)
    got = isl.render(bgr, results)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    dev = isl.render(torch.from_numpy(bgr).cuda(), results)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    assert np.array_equal(isl.render(bgr, results, blank=True), render.apply_numpy(None, lists, shape=bgr.shape))
    body_only = [render.body_primitives(r[0], r[1]) for r in results]
    assert np.array_equal(isl.render(bgr, results, hands=False), render.apply_numpy(bgr, body_only))


def test_extractor_overlapped_writes_the_pictures(isl_model, tmp_path):
    """KeypointExtractor(write_jpg=True) on the overlapped path: the JSON files are those of a
    run without pictures, and each JPEG is the RGB frame with its result drawn (up to the
    JPEG's loss: nearer to the drawing than to the frame where the two differ)."""
    Image = pytest.importorskip("PIL.Image")
    import os
    from islpose import pipeline
    isl, frames = isl_model
    base = tmp_path / "data"
    os.makedirs(base)
    np.save(base / "clip.npy", frames)
    rows = [{"Filepath": "clip.npy", "type": "T", "expression": "x"}]
    dec = pipeline.npy_decoder(str(base))
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    f0, _ = pipeline.extract_dataset(rows, dec, isl, plain, batch=1, export=False, overlap=True)
    f1, ex = pipeline.extract_dataset(rows, dec, isl, out, batch=1, export=False, overlap=True, write_jpg=True,
                                      jpg_workers=2, jpg_quality=95)
    assert ex.frames_done == 2 and [f["candidate"] for f in f1] == [f["candidate"] for f in f0]
    results = isl.call_batch(np.ascontiguousarray(frames[..., ::-1]))
    drawn = render.apply_numpy(frames, isl.render_primitives(results))
    for i in range(2):
        assert open(pipeline.json_path(out, "T", "x", "clip.npy", i)).read() == \
            open(pipeline.json_path(plain, "T", "x", "clip.npy", i)).read()
        im = Image.open(pipeline.jpg_path(out, "T", "x", "clip.npy", i))
        assert im.size == (328, 184) and im.mode == "RGB"
        got = np.asarray(im).astype(np.int64)
        changed = np.any(drawn[i] != frames[i], axis=2)
        assert changed.sum() > 20
        assert np.abs(got - drawn[i])[changed].mean() < np.abs(got - frames[i])[changed].mean()
    f2, ex2 = pipeline.extract_dataset(rows, dec, isl, out, batch=1, export=False, overlap=True, write_jpg=True)
    assert f2 == [] and ex2.frames_skipped == 2
