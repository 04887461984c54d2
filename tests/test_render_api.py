"""Stick-model overlays without a GPU: the C ABI's declaration, the host form of the drawing
definition (islpose.render.apply_numpy) against the scalar statement of tests/_render.py on the
GPU tests' inputs, the blend identity, the primitive builders, the Python layer's refusals, and
KeypointExtractor(write_jpg=True) with a stub model."""
import colorsys
import ctypes
import os
import re

import numpy as np
import pytest

import _render as ref
from islpose import pipeline, render
from islpose import runtime as rt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_and_abi_stays_1():
    text = open(os.path.join(REPO, "include", "islpose.h")).read()
    assert re.search(r"^#define ISL_ABI_VERSION 1$", text, re.M)
    assert re.search(r"^int isl_draw\(const uint8_t\* d_src, uint8_t\* d_dst, int n, int H, int W,\s*"
                     r"const isl_draw_prim\* prims, const int32_t\* first, void\* stream\);", text, re.M)
    struct = re.search(r"typedef struct \{([^}]*)\} isl_draw_prim;", text)
    assert struct
    for field in ("int32_t kind, p[4], c, s, r2;", "uint8_t color[3], blend;", "int32_t reserved;"):
        assert field in struct.group(1), field
    assert "isl_draw" in rt.EXPORTS
    assert ctypes.sizeof(rt.IslDrawPrim) == 40
    assert rt.IslDrawPrim.color.offset == 32 and rt.IslDrawPrim.blend.offset == 35
    src = open(os.path.join(REPO, "Makefile")).read()
    assert "$(CSRC)/draw.hip" in src


@pytest.mark.parametrize("name", list(ref.CASES))
def test_apply_numpy_equals_the_scalar_statement(name):
    frames, lists, want, blank = ref.case(name)
    got = render.apply_numpy(frames, lists)
    assert got.dtype == np.uint8 and got.shape == frames.shape and got is not frames
    assert np.array_equal(got, want)
    assert np.array_equal(render.apply_numpy(None, lists, shape=frames.shape), blank)
    assert np.array_equal(render.apply_numpy(frames, [[] for _ in lists]), frames)
    assert not render.apply_numpy(None, [[] for _ in lists], shape=frames.shape).any()


def test_order_is_part_of_the_result():
    frames, lists, want, _ = ref.case("odd")
    rev = [list(reversed(ref.ORDERED)) + lists[0][len(ref.ORDERED):]]
    got = render.apply_numpy(frames[:1], rev)
    assert np.array_equal(got, ref.draw(frames[:1], rev)[0])
    assert not np.array_equal(got, want[:1])


def test_blend_identity_over_all_pairs():
    c, k = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = (4 * c + 6 * k + 5) // 10
    for dt in (np.float32, np.float64):
        got = np.rint(dt(0.4) * c.astype(dt) + dt(0.6) * k.astype(dt))
        assert np.array_equal(got.astype(np.int64), want), dt
    assert want.min() == 0 and want.max() == 255
    assert all(ref.colour(int(a), int(b), 1) == int(w) for a, b, w in zip(c[::17, ::13].ravel(), k[::17, ::13].ravel(),
                                                                         want[::17, ::13].ravel()))


def test_builders_make_the_records():
    q = render.stick(10, -3, 7, 4, -135, (1, 2, 3))
    assert q == render.Prim(0, (10, -3, 7, 4), *ref.cs(-135), 0, (1, 2, 3), 1) == ref.stick(10, -3, 7, 4, -135, (1, 2, 3))
    assert render.cos_sin(0) == (16384, 0) and render.cos_sin(90) == (0, 16384) and render.cos_sin(179)[0] == -16382
    assert render.disc(5, 6, (9, 8, 7)) == (1, (5, 6, 0, 0), 0, 0, 16, (9, 8, 7), 0) == ref.disc(5, 6, 16, (9, 8, 7))
    assert render.segment(1, 2, 3, 4, (0, 0, 255)) == (2, (1, 2, 3, 4), 0, 0, 2, (0, 0, 255), 0)
    assert render.segment(1, 2, 3, 4, (0, 0, 255), r2=9, blend=1) == ref.segment(1, 2, 3, 4, 9, (0, 0, 255), 1)
    # numpy integers are taken, and come out as plain ints
    q = render.disc(np.int64(5), np.int32(6), np.array([1, 2, 3], dtype=np.uint8), r2=np.int64(4))
    assert q == (1, (5, 6, 0, 0), 0, 0, 4, (1, 2, 3), 0) and all(type(v) is int for v in q.p + q.color + (q.r2,))


def _two_persons():
    """Person 0: joints 0, 1, 2, 5 (limbs 1-0, 1-2, 1-5); person 1: joints 1 and 8 (limb 1-8),
    so close together that its stick's half length rounds to 0."""
    cand = np.array([[100.0, 50.0, 0.9, 0], [100.0, 90.0, 0.9, 1], [60.5, 95.0, 0.9, 2], [140.0, 95.0, 0.9, 3],
                     [200.0, 80.0, 0.9, 4], [200.0, 81.4, 0.9, 5]])
    subset = np.full((2, 27), -1.0)
    subset[0, [0, 1, 2, 5]] = [0, 1, 2, 3]
    subset[1, [1, 8]] = [4, 5]
    return cand, subset


def test_body_primitives_order_colour_by_type_and_half_length():
    from src import util
    cand, subset = _two_persons()
    prims = render.body_primitives(cand, subset, "body25")
    circles, tuples = util.get_bodypose(cand, subset, "body25")
    assert len(tuples) == 4 and len(circles) == 6 and len(prims) == 10
    sticks, joints = prims[:4], prims[4:]
    assert all(q.kind == render.STICK and q.blend == 1 and q.p[3] == 4 for q in sticks)
    assert all(q.kind == render.DISC and q.blend == 0 and q.r2 == 16 for q in joints)
    # limb types in get_bodypose's order: 0 (1-0), 1 (1-2), 4 (1-5) of person 0, 7 (1-8) of person 1
    assert [q.color for q in sticks] == [render.BODY_COLORS[i] for i in (0, 1, 4, 7)]
    # ... not drawStickmodel's list positions 0, 1, 2, 3
    assert [q.color for q in sticks] != [render.BODY_COLORS[i] for i in range(4)]
    for q, (mx, my, angle, length) in zip(sticks, tuples):
        assert q.p[:2] == (int(mx), int(my)) and q.p[2] == max(int(length / 2), 1)
        assert (q.c, q.s) == ref.cs(int(angle))
    assert sticks[0].p == (100, 70, 20, 4) and (sticks[0].c, sticks[0].s) == ref.cs(90)
    assert sticks[1].p[:3] == (80, 92, 19)                      # int(80.25), int(92.5), int(39.8 / 2)
    assert sticks[3].p == (200, 80, 1, 4)                       # int(1.4 / 2) = 0 -> a = 1
    # joints by type: joint 0, then joint 1 of both persons, 2, 5, 8
    assert [q.color for q in joints] == [render.BODY_COLORS[i] for i in (0, 1, 1, 2, 5, 8)]
    assert [q.p[:2] for q in joints] == [(100, 50), (100, 90), (200, 80), (60, 95), (140, 95), (200, 81)]
    assert render.body_primitives(cand, subset, "body25", order="joints_first") == joints + sticks
    assert render.body_primitives(cand, np.zeros((0, 27))) == []
    with pytest.raises(ValueError):
        render.body_primitives(cand, subset, order="sideways")
    with pytest.raises(ValueError):
        render.body_primitives(cand, subset, "body18")


def test_hand_primitives_skip_missing_peaks_and_their_edges():
    pk = np.zeros((21, 2), dtype=np.int64)
    pk[[0, 1, 2, 5, 9, 10]] = [[50, 60], [55, 58], [60, 55], [52, 40], [0, 7], [3, 0]]
    prims = render.hand_primitives([pk, np.zeros((21, 2), dtype=np.int64)])
    segs = [q for q in prims if q.kind == render.SEGMENT]
    discs = [q for q in prims if q.kind == render.DISC]
    assert prims == segs + discs                                # edges, then peaks
    # edges 0 (0-1), 1 (1-2), 4 (0-5), 8 (0-9), 9 (9-10): an end with one zero coordinate is a peak
    assert [q.p for q in segs] == [(50, 60, 55, 58), (55, 58, 60, 55), (50, 60, 52, 40), (50, 60, 0, 7), (0, 7, 3, 0)]
    for q, ie in zip(segs, (0, 1, 4, 8, 9)):
        assert q.color == tuple(int(round(255 * v)) for v in colorsys.hsv_to_rgb(ie / 20, 1, 1))
        assert q.r2 == 2 and q.blend == 0
    assert segs[0].color == (255, 0, 0) and segs[2].color == (204, 255, 0)
    assert [q.p[:2] for q in discs] == [(50, 60), (55, 58), (60, 55), (52, 40), (0, 7), (3, 0)]
    assert all(q.color == (255, 0, 0) and q.r2 == 16 and q.blend == 0 for q in discs)
    assert render.hand_primitives([pk], dot=(0, 0, 255))[-1].color == (0, 0, 255)
    assert render.hand_primitives([]) == []
    with pytest.raises(ValueError):
        render.hand_primitives([np.zeros((20, 2))])


def test_the_python_layer_refuses():
    ok = (1, 2, 3)
    for bad in (lambda: render.stick(0, 0, 0, 4, 0, ok), lambda: render.stick(0, 0, 4097, 4, 0, ok),
                lambda: render.stick(0, 0, 5, 0, 0, ok), lambda: render.stick(0, 0, 5, 17, 0, ok),
                lambda: render.stick(0, 0, 5, 4, 30.5, ok), lambda: render.stick(0.5, 0, 5, 4, 30, ok),
                lambda: render.stick(16385, 0, 5, 4, 30, ok), lambda: render.stick(0, 0, 5, 4, 30, ok, blend=2),
                lambda: render.stick(0, 0, 5, 4, 30, ok, blend=True),
                lambda: render.disc(0, -16385, ok), lambda: render.disc(0, 0, ok, r2=-1),
                lambda: render.disc(0, 0, ok, r2=4097), lambda: render.disc(0, 0, ok, r2=1.0),
                lambda: render.disc(0, 0, (1, 2)), lambda: render.disc(0, 0, (1, 2, 256)),
                lambda: render.disc(0, 0, (1, 2, -1)), lambda: render.disc(0, 0, 7), lambda: render.disc(0, 0, (1, 2, 3.0)),
                lambda: render.segment(0, 0, 16385, 0, ok), lambda: render.segment(0, 0, 0, -16385, ok),
                lambda: render.segment(0, 0, 1, 1, ok, r2=4097),
                lambda: render.check_prim((3, (0, 0, 0, 0), 0, 0, 0, ok, 0)),
                lambda: render.check_prim((0, (0, 0, 5, 4), 16385, 0, 0, ok, 1)),
                lambda: render.check_prim((0, (0, 0, 5, 4), 0, -16385, 0, ok, 1)),
                lambda: render.check_prim((1, (0, 0, 0), 0, 0, 0, ok, 0)),
                lambda: render.check_prim("disc"), lambda: render.check_prim((1, 2, 3))):
        with pytest.raises(ValueError):
            bad()
    fr = np.zeros((2, 4, 5, 3), np.uint8)
    one = [render.disc(1, 1, ok)]
    for bad in (lambda: render.apply_numpy(fr, [one]), lambda: render.apply_numpy(fr, [one, one, one]),
                lambda: render.apply_numpy(fr.astype(np.int32), [one, one]),
                lambda: render.apply_numpy(fr[0], [one]), lambda: render.apply_numpy(fr[..., :2], [one, one]),
                lambda: render.apply_numpy(None, [one]), lambda: render.apply_numpy(None, [one], shape=(1, 4, 5)),
                lambda: render.apply_numpy(None, [one], shape=(1, 0, 5, 3)),
                lambda: render.apply_numpy(None, [one], shape=(1, 16385, 1, 3)),
                lambda: render.apply_numpy(fr, [one, [(7, (0, 0, 0, 0), 0, 0, 0, ok, 0)]]),
                lambda: render.apply(fr, [one, one])):
        with pytest.raises(ValueError):
            bad()
    # the limits themselves are taken
    render.stick(-16384, 16384, 4096, 16, -180, (0, 0, 0), blend=0)
    render.disc(16384, -16384, (255, 255, 255), r2=4096)
    render.check_prim((0, (0, 0, 1, 1), 0, 0, 0, ok, 1))          # c = s = 0: every pixel
    assert render.apply_numpy(fr, [[(0, (0, 0, 1, 1), 0, 0, 0, ok, 0)], []])[0].tolist() == \
        np.broadcast_to(np.array(ok, np.uint8), (4, 5, 3)).tolist()


class StubModel:
    """Stand-in for ISLSignPos.call_batch: one person with a limb and one hand, placed by the
    frame's content, so the picture differs from the frame and between frames."""

    def __init__(self):
        self.calls = 0

    def call_batch(self, frames_bgr):
        out = []
        for f in np.asarray(frames_bgr):
            self.calls += 1
            x = 8.0 + float(f[0, 0, 0] % 8)
            cand = np.array([[x, 6.0, 0.9, 0.0], [x + 10.0, 14.0, 0.9, 1.0]])
            subset = np.full((1, 27), -1.0)
            subset[0, [0, 1]], subset[0, -2], subset[0, -1] = [0, 1], 1.5, 2
            hand = np.zeros((21, 2), dtype=np.int64)
            hand[[0, 1]] = [[20, 5], [26, 9]]
            out.append((cand, subset, [hand]))
        return out


def _tree(root, ext=None):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if ext is None or f.endswith(ext):
                p = os.path.join(d, f)
                out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_extractor_writes_the_pictures_and_resumes_on_both_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from islpose import augment
    base = tmp_path / "data"
    os.makedirs(base)
    frames = np.random.default_rng(21).integers(0, 256, (3, 24, 40, 3), dtype=np.uint8)
    np.save(base / "clip.npy", frames)
    rows = [{"Filepath": "clip.npy", "type": "T", "expression": "x"}]
    dec = pipeline.npy_decoder(str(base))
    # off: the file tree is today's -- JSON only, byte for byte what the run with pictures writes
    plain = str(tmp_path / "plain")
    f0, _ = pipeline.extract_dataset(rows, dec, StubModel(), plain, batch=2, overlap=False)
    assert len(_tree(plain)) == 3 and all(p.endswith(".json") for p in _tree(plain))
    out = str(tmp_path / "out")
    f1, ex = pipeline.extract_dataset(rows, dec, StubModel(), out, batch=2, overlap=False, write_jpg=True,
                                      jpg_workers=2, jpg_quality=95)
    assert ex.frames_done == 3 and [f["frame_no"] for f in f1] == [0, 1, 2]
    assert _tree(out, ".json") == _tree(plain)
    assert [{k: v for k, v in f.items() if k != "filepath"} for f in f1] == \
        [{k: v for k, v in f.items() if k != "filepath"} for f in f0]
    d = os.path.join(out, "transforms", "T", "x", "clip-original")
    assert sorted(os.listdir(d)) == sorted(["clip.npy-%d.json" % i for i in range(3)] + ["clip-%d.jpg" % i for i in range(3)])
    for i in range(3):
        assert pipeline.jpg_path(out, "T", "x", "clip.npy", i) == os.path.join(d, "clip-%d.jpg" % i)
        im = Image.open(os.path.join(d, "clip-%d.jpg" % i))
        assert im.format == "JPEG" and im.size == (40, 24) and im.mode == "RGB"
        # the picture is the drawn RGB frame, up to the JPEG's loss: nearer to it than to the frame
        drawn = render.apply_numpy(frames[i:i + 1], KeypointPrims(frames[i]))[0].astype(np.int64)
        got = np.asarray(im).astype(np.int64)
        changed = np.any(drawn != frames[i], axis=2)
        assert changed.sum() > 20
        assert np.abs(got - drawn)[changed].mean() < np.abs(got - frames[i])[changed].mean()
    # resume: both files present -> nothing to do
    m = StubModel()
    f2, ex2 = pipeline.extract_dataset(rows, dec, m, out, batch=2, overlap=False, write_jpg=True)
    assert f2 == [] and ex2.frames_skipped == 3 and m.calls == 0
    # a missing picture, or a missing JSON, makes the unit due again; without write_jpg the JSON decides
    os.remove(os.path.join(d, "clip-1.jpg"))
    os.remove(os.path.join(d, "clip.npy-2.json"))
    m = StubModel()
    f3, ex3 = pipeline.extract_dataset(rows, dec, m, out, batch=2, overlap=False)
    assert [f["frame_no"] for f in f3] == [2] and not os.path.exists(os.path.join(d, "clip-1.jpg"))
    os.remove(os.path.join(d, "clip.npy-2.json"))
    m = StubModel()
    f4, ex4 = pipeline.extract_dataset(rows, dec, m, out, batch=2, overlap=False, write_jpg=True)
    assert [f["frame_no"] for f in f4] == [1, 2] and ex4.frames_skipped == 1 and m.calls == 2
    assert len(_tree(out, ".jpg")) == 3 and _tree(out, ".json") == _tree(plain)
    # the augmented variants' pictures go to their own folders
    aug = str(tmp_path / "aug")
    f5, ex5 = pipeline.extract_dataset(rows, dec, StubModel(), aug, batch=4, overlap=False, write_jpg=True,
                                       transforms=[augment.Solarize(192)])
    assert ex5.frames_done == 6
    for name in ("original", "Solarize"):
        dd = os.path.join(aug, "transforms", "T", "x", "clip-%s" % name)
        assert sorted(f for f in os.listdir(dd) if f.endswith(".jpg")) == ["clip-%d.jpg" % i for i in range(3)]
    a = np.asarray(Image.open(os.path.join(aug, "transforms", "T", "x", "clip-Solarize", "clip-0.jpg"))).astype(np.int64)
    sol = augment.apply_numpy(frames[:1], [augment.Item(0, None, 192)])[0].astype(np.int64)
    assert np.abs(a - sol).mean() < np.abs(a - frames[0]).mean()
    with pytest.raises(ValueError):
        pipeline.KeypointExtractor(StubModel(), out, write_jpg=True, jpg_workers=0)
    with pytest.raises(ValueError):
        pipeline.KeypointExtractor(StubModel(), out, write_jpg=True, jpg_quality=101)


def KeypointPrims(rgb_frame):
    """The primitive list the extractor draws for one RGB frame of the stub model."""
    res = StubModel().call_batch(rgb_frame[None, ..., ::-1])
    return [render.body_primitives(res[0][0], res[0][1], "body25") + render.hand_primitives(res[0][2])]


def test_write_jpg_without_pillow_is_a_clear_import_error(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(ImportError, match="Pillow"):
        pipeline.KeypointExtractor(StubModel(), "unused", write_jpg=True)
    pipeline.KeypointExtractor(StubModel(), "unused")             # off: Pillow is never asked for
