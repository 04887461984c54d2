"""Augmented extraction without a GPU: the C ABI's declaration, the host form of the variant
definition (islpose.augment.apply_numpy) against the independent restatement of tests/_augment.py
and against torchvision's fp32 route, the per-frame draws, validation, and KeypointExtractor's
units, folders, rows and resume with a stub model."""
import json
import os
import re

import numpy as np
import pytest

import _augment as ref
from islpose import augment, pipeline
from islpose import runtime as rt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(37, 53), (64, 96), (61, 98), (1, 7), (5, 1)]
ANGLES = [0, 17.3, -30, 45, 180]


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _cases():
    for h, w in SHAPES:
        for a in ANGLES + ([90] if h % 2 and w % 2 else []):
            yield h, w, a


def test_header_declares_the_entry_and_abi_stays_1():
    text = open(os.path.join(REPO, "include", "islpose.h")).read()
    assert re.search(r"^#define ISL_ABI_VERSION 1$", text, re.M)
    assert re.search(r"^int isl_augment\(const uint8_t\* d_src, int n_src, int H, int W, uint8_t\* d_dst,\s*"
                     r"const isl_aug_item\* items, int m, void\* stream\);", text, re.M)
    struct = re.search(r"typedef struct \{([^}]*)\} isl_aug_item;", text)
    assert struct
    for field in ("double c, s;", "int32_t src;", "int32_t rotate;", "int32_t threshold;", "int32_t swap_rb;",
                  "int32_t reserved[2];"):
        assert field in struct.group(1), field
    assert "isl_augment" in rt.EXPORTS
    import ctypes
    assert ctypes.sizeof(rt.IslAugItem) == 40
    assert [f[0] for f in rt.IslAugItem._fields_] == ["c", "s", "src", "rotate", "threshold", "swap_rb", "reserved"]


@pytest.mark.parametrize("h,w,angle", list(_cases()))
def test_apply_numpy_rotation_equals_helper(h, w, angle):
    fr = _frames(2, h, w, seed=h * 100 + w)
    for swap in (False, True):
        got = augment.apply_numpy(fr, [augment.Item(1, angle, 256), augment.Item(0, angle, 192)], swap_rb=swap)
        assert got.dtype == np.uint8 and got.shape == (2, h, w, 3)
        assert np.array_equal(got[0], ref.variant(fr[1], angle, 256, swap))
        assert np.array_equal(got[1], ref.variant(fr[0], angle, 192, swap))


def test_rotation_by_180_and_90_are_the_exact_flips():
    """Sanity of the shared definition itself: 180 degrees is both flips on any size, +90 (odd
    square, counter-clockwise) is np.rot90."""
    fr = _frames(1, 37, 53, 1)[0]
    assert np.array_equal(ref.variant(fr, 180), fr[::-1, ::-1])
    sq = _frames(1, 31, 31, 2)[0]
    assert np.array_equal(ref.variant(sq, 90), np.rot90(sq, 1))
    assert np.array_equal(augment.apply_numpy(sq[None], [augment.Item(0, 90, 256)])[0], np.rot90(sq, 1))


@pytest.mark.parametrize("t", [0, 192, 255, 256])
def test_solarize_thresholds(t):
    fr = _frames(1, 37, 53, 7)
    fr[0, 0, :3] = [[0, 191, 192], [193, 254, 255], [1, 2, 3]]
    got = augment.apply_numpy(fr, [augment.Item(0, None, t)])[0]
    v = fr[0].astype(np.int64)
    assert np.array_equal(got, np.where(v >= t, 255 - v, v).astype(np.uint8))
    assert np.array_equal(got, ref.variant(fr[0], None, t))
    if t == 256:
        assert np.array_equal(got, fr[0])


def test_rotation_then_solarize_fills_255_at_threshold_0_and_swap_rb():
    fr = _frames(1, 37, 53, 9)
    got = augment.apply_numpy(fr, [augment.Item(0, 45, 0)])[0]
    assert np.array_equal(got, ref.variant(fr[0], 45, 0))
    assert np.array_equal(got[0, 0], [255, 255, 255]) and np.array_equal(got[-1, -1], [255, 255, 255])
    plain = augment.apply_numpy(fr, [augment.Item(0, 45, 256)])[0]
    assert np.array_equal(plain[0, 0], [0, 0, 0])
    assert np.array_equal(got, 255 - plain)
    # swap_rb commutes with both transforms
    for it in (augment.Item(0, None, 256), augment.Item(0, 17.3, 192)):
        sw = augment.apply_numpy(fr, [it], swap_rb=True)[0]
        assert np.array_equal(sw, augment.apply_numpy(fr, [it])[0][..., ::-1])
        assert np.array_equal(sw, augment.apply_numpy(np.ascontiguousarray(fr[..., ::-1]), [it])[0])


def test_fp64_definition_against_torchvisions_fp32_route_1080p():
    """The fp64 definition and torchvision's fp32 route may differ only where a source
    coordinate sits on a rounding tie: every differing pixel has an fp64 source coordinate
    within 2^-10 px of a half-integer, and they are at most 1e-3 of the pixels."""
    H, W, angle = 1080, 1920, 17.3
    fr = _frames(1, H, W, 11)[0]
    got = augment.apply_numpy(fr[None], [augment.Item(0, angle, 256)])[0]
    tv = ref.tv_rotate_fp32(fr, angle)
    diff = np.any(got != tv, axis=2)
    share = diff.mean()
    xs, ys = ref.source_coords(H, W, angle)
    tie = lambda v: np.abs(np.abs(v - np.floor(v)) - 0.5)     # noqa: E731  distance to a half-integer
    dist = np.minimum(tie(xs), tie(ys))[diff]
    print("differing pixels %d (share %.3g), largest distance to a tie %.3g"
          % (diff.sum(), share, dist.max() if dist.size else 0.0))
    assert share <= 1e-3
    assert np.all(dist <= 2.0 ** -10)


def test_params_for():
    rot, sol = augment.RandomRotation(30, seed=3), augment.RandomSolarize(192, 0.5, seed=3)
    draws = [augment.params_for(rot, "MVI_1.MOV", i, 0) for i in range(64)]
    assert draws == [augment.params_for(rot, "MVI_1.MOV", i, 0) for i in range(64)]     # deterministic
    angles = [d.angle for d in draws]
    assert all(-30 <= a <= 30 for a in angles) and all(d.threshold == 256 for d in draws)
    assert len(set(angles)) == 64                                                      # differs across frames
    assert min(angles) < -15 and max(angles) > 15                                      # uses the range
    other = [augment.params_for(augment.RandomRotation(30, seed=4), "MVI_1.MOV", i, 0).angle for i in range(64)]
    assert all(a != b for a, b in zip(angles, other))                                  # ... and across seeds
    assert augment.params_for(rot, "MVI_2.MOV", 0, 0) != draws[0]                      # ... videos
    assert augment.params_for(rot, "MVI_1.MOV", 0, 1) != draws[0]                      # ... list positions
    fired = [augment.params_for(sol, "MVI_1.MOV", i, 1) for i in range(200)]
    assert {d.threshold for d in fired} == {192, 256} and all(d.angle is None for d in fired)
    assert 60 <= sum(d.threshold == 192 for d in fired) <= 140
    assert augment.params_for(augment.RandomSolarize(192, 1.0), "v", 0, 0).threshold == 192
    assert augment.params_for(augment.RandomSolarize(192, 0.0), "v", 0, 0).threshold == 256
    assert augment.params_for(augment.Rotate(17.3), "v", 5, 0) == augment.Params(17.3, 256)
    assert augment.params_for(augment.Solarize(), "v", 5, 1) == augment.Params(None, 192)


def test_names_and_validation():
    assert augment.Rotate(5).name == "Rotate" and augment.Solarize().name == "Solarize"
    assert augment.RandomRotation().name == "RandomRotation" and augment.RandomSolarize().name == "RandomSolarize"
    assert augment.RandomRotation().degrees == 30 and augment.RandomSolarize().threshold == 192
    assert augment.RandomSolarize().p == 0.5
    for bad in (lambda: augment.Rotate(float("nan")), lambda: augment.Rotate("3"), lambda: augment.Solarize(-1),
                lambda: augment.Solarize(257), lambda: augment.Solarize(191.5), lambda: augment.RandomRotation(-1),
                lambda: augment.RandomRotation(float("inf")), lambda: augment.RandomRotation(30, seed=-1),
                lambda: augment.RandomSolarize(192, 1.5), lambda: augment.RandomSolarize(300),
                lambda: augment.RandomSolarize(192, 0.5, seed=1.5),
                lambda: augment.params_for(object(), "v", 0, 0), lambda: augment.params_for(augment.Rotate(1), "v", -1, 0),
                lambda: augment.check_transforms([augment.Rotate(1), augment.Rotate(2)]),
                lambda: augment.check_transforms(["rotation"]),
                lambda: augment.parse_spec("rotation"), lambda: augment.parse_spec("blur:3"),
                lambda: augment.parse_spec("rotation:30,rotation:10")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="257"):
        augment.Solarize(257)
    fr = _frames(2, 5, 7, 0)
    with pytest.raises(ValueError, match="2"):
        augment.apply_numpy(fr, [augment.Item(2, None, 256)])
    with pytest.raises(ValueError, match="300"):
        augment.apply_numpy(fr, [augment.Item(0, None, 300)])
    with pytest.raises(ValueError):
        augment.apply_numpy(fr, [augment.Item(0, float("inf"), 256)])
    with pytest.raises(ValueError):
        augment.apply_numpy(fr.astype(np.float32), [augment.Item(0, None, 256)])
    with pytest.raises(ValueError):
        augment.apply_numpy(fr[0], [augment.Item(0, None, 256)])
    assert augment.apply_numpy(fr, []).shape == (0, 5, 7, 3)
    ts = augment.parse_spec("rotation:30,solarize:192", seed=5)
    assert [t.name for t in ts] == ["RandomRotation", "RandomSolarize"] and ts[0].degrees == 30 and ts[1].seed == 5
    assert augment.parse_spec("solarize:100:1")[0].p == 1.0 and augment.parse_spec("") is None


class StubModel:
    """Stand-in for ISLSignPos.call_batch that keeps every BGR frame it is given and answers
    with a result that depends on it."""

    def __init__(self):
        self.seen = []

    def call_batch(self, frames_bgr):
        out = []
        for f in np.asarray(frames_bgr):
            self.seen.append(f.copy())
            cand = np.array([[float(f[..., 0].sum()), float(f[..., 2].sum()), 0.5, 0.0]])
            subset = np.full((1, 27), -1.0)
            subset[0, 0], subset[0, -2], subset[0, -1] = 0, 1.5, 1
            out.append((cand, subset, []))
        return out


def _video(tmp_path, T=3):
    base = tmp_path / "data"
    os.makedirs(base, exist_ok=True)
    np.save(base / "clip.npy", _frames(T, 12, 16, 21))
    return str(base), [{"Filepath": "clip.npy", "type": "T", "expression": "x"}]


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".json"):
                p = os.path.join(d, f)
                out[os.path.relpath(p, root)] = open(p).read()
    return out


def test_extractor_units_folders_rows_and_resume(tmp_path):
    base, rows = _video(tmp_path)
    frames = np.load(os.path.join(base, "clip.npy"))
    ts = [augment.RandomRotation(30, seed=3), augment.RandomSolarize(192, 0.5, seed=3)]
    out = str(tmp_path / "out")
    model = StubModel()
    feats, ex = pipeline.extract_dataset(rows, pipeline.npy_decoder(base), model, out, batch=4, overlap=False,
                                         transforms=ts)
    names = ["original", "RandomRotation", "RandomSolarize"]
    assert ex.frames_done == 9 and len(feats) == 9
    assert [(f["frame_no"], f["transform"]) for f in feats] == [(i, n) for i in range(3) for n in names]
    # the reference's row columns, nothing added (no angle column)
    assert sorted(feats[0]) == sorted(pipeline.feature_row("p", 0, "T", "x", StubModel().call_batch(frames[:1])[0]))
    # the stub saw exactly the BGR variants, unit by unit
    want = []
    for i in range(3):
        want.append(ref.variant(frames[i], swap_rb=True))
        for k, t in enumerate(ts):
            p = augment.params_for(t, "clip.npy", i, k)
            want.append(ref.variant(frames[i], p.angle, p.threshold, swap_rb=True))
    assert len(model.seen) == 9 and all(np.array_equal(a, b) for a, b in zip(model.seen, want))
    for f in feats:
        assert f["filepath"] == os.path.join(out, "transforms", "T", "x", "clip-%s" % f["transform"],
                                             "clip.npy-%d.json" % f["frame_no"])
        assert json.load(open(f["filepath"]))["candidate"] == f["candidate"]
    assert len(_tree(out)) == 9
    # resume skips per unit
    m2 = StubModel()
    feats2, ex2 = pipeline.extract_dataset(rows, pipeline.npy_decoder(base), m2, out, batch=4, overlap=False,
                                           transforms=ts)
    assert feats2 == [] and ex2.frames_skipped == 9 and m2.seen == []
    # deleting one variant's JSON recomputes only it
    before = _tree(out)
    os.remove(feats[4]["filepath"])                      # frame 1, RandomRotation
    m3 = StubModel()
    feats3, ex3 = pipeline.extract_dataset(rows, pipeline.npy_decoder(base), m3, out, batch=4, overlap=False,
                                           transforms=ts)
    assert [(f["frame_no"], f["transform"]) for f in feats3] == [(1, "RandomRotation")]
    assert ex3.frames_skipped == 8 and len(m3.seen) == 1 and np.array_equal(m3.seen[0], want[4])
    assert _tree(out) == before


def test_extractor_without_transforms_is_unchanged(tmp_path):
    """transforms=None writes the files of a run made without passing the argument, and the
    -original files of an augmented run are those files too."""
    base, rows = _video(tmp_path)
    outs = {}
    for name, kw in (("plain", {}), ("none", {"transforms": None}),
                     ("aug", {"transforms": [augment.Rotate(17.3), augment.Solarize(192)]})):
        feats, _ = pipeline.extract_dataset(rows, pipeline.npy_decoder(base), StubModel(), str(tmp_path / name),
                                            batch=2, overlap=False, **kw)
        outs[name] = (_tree(str(tmp_path / name)),
                      [{k: v for k, v in f.items() if k != "filepath"} for f in feats])
    assert outs["none"] == outs["plain"] and len(outs["plain"][0]) == 3
    assert all("-original" in p for p in outs["plain"][0])
    assert {p: t for p, t in outs["aug"][0].items() if "-original" in p} == outs["plain"][0]
    assert len(outs["aug"][0]) == 9
    assert [r for r in outs["aug"][1] if r["transform"] == "original"] == outs["plain"][1]
