"""Augmented copies of frames: rotation and solarize.

The reference's dataset extractor runs the model on augmented copies of every frame
(extract_featuressingle.py:49-52: ``transformations = [v2.RandomRotation(degrees=30),
v2.RandomSolarize(threshold=192.0)]``, applied at :116-120) and files each beside the original
under ``<stem>-<TransformClassName>/``.  Here a variant is built on the GPU from frames that
are already resident: one launch (``isl_augment``, csrc/augment.hip) writes the originals and
the variants of a batch into one ``[m, H, W, 3]`` tensor.

The definition (the kernel, ``apply_numpy`` and the tests share it)
-------------------------------------------------------------------
A variant of a ``uint8 [H, W, 3]`` frame is the rotation first, then the solarize; either may
be off.  Both follow torchvision v2's tensor path.  That parity is **unpinned**, as
``cv2.resize``'s is: torchvision is absent here, so nothing in the tests runs it.

* Rotation by ``angle`` degrees: counter-clockwise for positive angles, about the image
  centre, nearest neighbour, same output size, fill 0.  All coordinate arithmetic is fp64, in
  this order, with no fused multiply-add: ``r = radians(-angle)``, ``c = cos(r)``,
  ``s = sin(r)`` (Python's ``math`` on the host, passed as doubles); ``cx = (W-1)*0.5``,
  ``cy = (H-1)*0.5``; for output pixel (row j, column i) ``dx = i - cx``, ``dy = j - cy``,
  ``xs = (c*dx + s*dy) + cx``, ``ys = ((-s)*dx + c*dy) + cy``, ``xi = rint(xs)``,
  ``yi = rint(ys)`` (half to even); the output is ``src[yi, xi, :]`` if ``0 <= xi < W`` and
  ``0 <= yi < H``, else 0.  Every pixel is computed from the formula, never incrementally.
* Solarize with threshold ``t``: a byte ``v`` becomes ``255 - v`` where ``v >= t``; ``t`` is an
  integer in [0, 256] and 256 means off.  Filled pixels go through it too.
* ``swap_rb``: output channel k is source channel 2 - k, applied at the load, so it commutes
  with both transforms.

The random transforms draw per frame from ``np.random.default_rng([seed, crc32(filename),
frame_idx, position_in_list])``, so a variant does not depend on the batch, the rank or a
resumed run.  The reference draws from torch's global RNG in whatever order its workers reach
the frames; its draws cannot be reproduced, only their distributions.
"""
from __future__ import annotations

import collections
import math
import zlib

import numpy as np

SOLARIZE_OFF = 256

# one entry of a launch: source frame index, rotation angle in degrees (None: no rotation),
# solarize threshold (256: off)
Item = collections.namedtuple("Item", "src angle threshold")
# a transform's draw for one frame
Params = collections.namedtuple("Params", "angle threshold")


def _number(name, v, lo=None, hi=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) \
            or not math.isfinite(v) or (lo is not None and v < lo) or (hi is not None and v > hi):
        rng = "" if lo is None and hi is None else " in [%s, %s]" % ("-inf" if lo is None else lo, "inf" if hi is None else hi)
        raise ValueError("%s must be a finite number%s, got %r" % (name, rng, v))
    return v


def check_threshold(t):
    """A solarize threshold as an int in [0, 256] (256: off), else ValueError."""
    _number("threshold", t, 0, SOLARIZE_OFF)
    if int(t) != t:
        raise ValueError("threshold must be an integer in [0, 256], got %r" % (t,))
    return int(t)


def _seed(seed):
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("seed must be an integer >= 0, got %r" % (seed,))
    return int(seed)


class Rotate:
    """Rotation by a fixed angle in degrees (counter-clockwise for positive angles)."""
    name = "Rotate"

    def __init__(self, angle):
        self.angle = float(_number("angle", angle))

    def params(self, rng):
        return Params(self.angle, SOLARIZE_OFF)


class Solarize:
    """Solarize with a fixed threshold: v -> 255 - v where v >= threshold."""
    name = "Solarize"

    def __init__(self, threshold=192):
        self.threshold = check_threshold(threshold)

    def params(self, rng):
        return Params(None, self.threshold)


class RandomRotation:
    """v2.RandomRotation(degrees): an angle uniform in [-degrees, degrees] per frame."""
    name = "RandomRotation"

    def __init__(self, degrees=30, seed=0):
        self.degrees = float(_number("degrees", degrees, 0))
        self.seed = _seed(seed)

    def params(self, rng):
        return Params(float(rng.uniform(-self.degrees, self.degrees)), SOLARIZE_OFF)


class RandomSolarize:
    """v2.RandomSolarize(threshold, p): the solarize with probability p per frame."""
    name = "RandomSolarize"

    def __init__(self, threshold=192, p=0.5, seed=0):
        self.threshold = check_threshold(threshold)
        self.p = float(_number("p", p, 0, 1))
        self.seed = _seed(seed)

    def params(self, rng):
        return Params(None, self.threshold if rng.random() < self.p else SOLARIZE_OFF)


def params_for(transform, filename, idx, k):
    """The draw of `transform`, at position k of the transform list, for frame idx of video
    `filename`: Params(angle in degrees or None, solarize threshold or 256).  The generator is
    np.random.default_rng([seed, crc32(filename), idx, k]) (seed 0 for the fixed transforms,
    which do not draw), so the result depends on nothing else."""
    if not hasattr(transform, "params") or not hasattr(transform, "name"):
        raise ValueError("not a transform: %r" % (transform,))
    if isinstance(idx, (bool, np.bool_)) or int(idx) != idx or idx < 0 or int(k) != k or k < 0:
        raise ValueError("frame index and list position must be integers >= 0, got %r, %r" % (idx, k))
    key = [getattr(transform, "seed", 0), zlib.crc32(str(filename).encode()), int(idx), int(k)]
    return transform.params(np.random.default_rng(key))


def check_transforms(transforms):
    """A transform list as a tuple; ValueError for an entry that is no transform, a name used
    twice (the names are the output folders) or the name 'original'."""
    ts = tuple(transforms)
    names = []
    for t in ts:
        if not hasattr(t, "params") or not isinstance(getattr(t, "name", None), str):
            raise ValueError("not a transform: %r" % (t,))
        if t.name == "original" or t.name in names:
            raise ValueError("transform name %r is taken (one output folder per name)" % (t.name,))
        names.append(t.name)
    return ts


def item(src, params=None):
    """Item for source frame `src` with a transform's Params (None: a plain copy)."""
    return Item(int(src), None, SOLARIZE_OFF) if params is None else Item(int(src), params.angle, params.threshold)


def cos_sin(angle):
    """(c, s) of the definition: cos and sin of radians(-angle), Python's math."""
    r = math.radians(-angle)
    return math.cos(r), math.sin(r)


def _check_items(items, n_src):
    out = []
    for it in items:
        src, angle, thr = it
        if isinstance(src, (bool, np.bool_)) or int(src) != src or not 0 <= src < n_src:
            raise ValueError("item source index %r outside [0, %d)" % (src, n_src))
        if angle is not None:
            angle = float(_number("angle", angle))
        out.append(Item(int(src), angle, check_threshold(thr)))
    return out


def _check_frames_shape(shape):
    if len(shape) != 4 or shape[3] != 3 or shape[1] < 1 or shape[2] < 1:
        raise ValueError("frames: uint8 [n, H, W, 3] expected, got shape %r" % (tuple(shape),))


def apply(frames_t, items, swap_rb=False, stream=None):
    """frames_t cuda uint8 [n, H, W, 3]; items [Item] -> cuda uint8 [len(items), H, W, 3], item
    k's variant of frame items[k].src, in one launch (isl_augment) on the current stream.
    swap_rb reverses the channels of every item (RGB -> BGR) on the way."""
    import torch
    from . import runtime as rt
    if not (isinstance(frames_t, torch.Tensor) and frames_t.is_cuda and frames_t.dtype == torch.uint8):
        raise ValueError("frames: a cuda uint8 tensor expected, got %r" % (type(frames_t),))
    _check_frames_shape(frames_t.shape)
    its = _check_items(items, frames_t.shape[0])
    if len(its) > 65535:
        raise ValueError("at most 65535 items per launch, got %d" % len(its))
    recs = []
    for it in its:
        c, s = cos_sin(it.angle) if it.angle is not None else (1.0, 0.0)
        recs.append(rt.IslAugItem(c, s, it.src, int(it.angle is not None), it.threshold, int(bool(swap_rb))))
    return rt.augment(frames_t.contiguous(), recs, stream=stream)


def apply_numpy(frames, items, swap_rb=False):
    """The GPU-less form of the same definition: frames uint8 [n, H, W, 3] (array-like);
    items [Item] -> uint8 [len(items), H, W, 3], byte for byte what `apply` gives."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise ValueError("frames: uint8 expected, got %s" % frames.dtype)
    _check_frames_shape(frames.shape)
    n, H, W, _ = frames.shape
    its = _check_items(items, n)
    out = np.empty((len(its), H, W, 3), np.uint8)
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    dx = np.arange(W, dtype=np.float64)[None, :] - cx
    dy = np.arange(H, dtype=np.float64)[:, None] - cy
    for k, it in enumerate(its):
        src = frames[it.src]
        if swap_rb:
            src = src[..., ::-1]
        if it.angle is None:
            v = np.array(src, dtype=np.uint8)
        else:
            c, s = cos_sin(it.angle)
            # separate numpy operations: every product and sum rounds on its own (no FMA)
            xi = np.rint((c * dx + s * dy) + cx)
            yi = np.rint(((-s) * dx + c * dy) + cy)
            inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            xg = np.where(inside, xi, 0).astype(np.int64)
            yg = np.where(inside, yi, 0).astype(np.int64)
            v = np.where(inside[..., None], src[yg, xg], np.uint8(0))
        if it.threshold < SOLARIZE_OFF:
            v = np.where(v >= it.threshold, 255 - v, v).astype(np.uint8)
        out[k] = v
    return out


def parse_spec(spec, seed=0):
    """The tools' --augment syntax -> a transform list: comma-separated 'rotation:DEGREES'
    (RandomRotation) and 'solarize:THRESHOLD[:P]' (RandomSolarize), e.g.
    'rotation:30,solarize:192'.  An empty spec gives None."""
    if not spec:
        return None
    out = []
    for part in spec.split(","):
        f = part.strip().split(":")
        try:
            if f[0] == "rotation" and len(f) == 2:
                out.append(RandomRotation(float(f[1]), seed=seed))
                continue
            if f[0] == "solarize" and len(f) in (2, 3):
                out.append(RandomSolarize(float(f[1]), *([float(f[2])] if len(f) == 3 else []), seed=seed))
                continue
        except ValueError as e:
            raise ValueError("--augment %r: %s" % (part, e))
        raise ValueError("--augment %r: expected rotation:DEGREES or solarize:THRESHOLD[:P]" % (part,))
    return list(check_transforms(out))
