"""Keypoint-space augmentation of the sign classifier's windows.

The classifier never sees pixels: on the 156-d rows of ``populate_features`` a rotation, scaling or
shift of the frame is an affine map of the (x, y) pairs, and a speed change, temporal shift or
dropped frame is a choice of source rows.  ``WindowAugment`` draws those per window and per step
from counter-based hashes and builds a batch of augmented windows from resident rows in one launch
(``isl_sign_augment``, csrc/sign_augment.hip); ``apply_numpy`` gives the same bits without a GPU.

The definition (the kernel, ``apply_numpy`` and tests/_sign_augment.py share it)
-------------------------------------------------------------------------------
* A row has ``F = 2*n_body + n_slots*3*n_hand`` features: n_body x, n_body y, then per hand slot
  n_hand x, n_hand y, n_hand labels; the default layout (15, 2, 21) is populate_features' 156.  A
  pair (x, y) is absent iff both values are exactly 0.  The row carries no part identities, so a
  horizontal mirror is not definable on it and there is none.
* An item (``ITEM_DTYPE``, the C struct isl_sign_aug_item) views the rows
  ``[row0, row0 + nrows)`` of a store.  Output frame t of T reads source row
  ``r = ((2t - (T-1))*q + 16*(T-1) + 16) // 32 + start``; r outside [0, nrows) gives an all-zero
  frame.  ``kw = sm(sm(seed ^ step) ^ id)`` with section 4.2k's ``sm``; frame t is dropped (all
  zero) iff ``sm(kw ^ (16<<32 | t)) >> 40 < floor(drop*2^24 + 0.5)``.
* A present pair of a live frame, fp64 in this order without fused multiply-adds:
  ``X = (m0*x + m1*y) + m2``, ``Y = (m3*x + m4*y) + m5``; with jitter > 0,
  ``X = X + jitter*(u*2^-23 - 1)``, ``u = sm(kw ^ (17<<32 | (t*512 + 2p))) >> 40``, p the pair's
  index in the row (body pairs, then the slots' pairs), and Y with index ``t*512 + 2p + 1``; both
  rounded once to fp32; if both are then 0, x is stored as 2^-10.  Absent pairs are stored as
  (0, 0); labels are copied, and are 0 on zeroed frames.  Points are not clipped to the frame.
* Per item, on the host only (``items``): ``u_j = (sm(kw ^ (32<<32 | j)) >> 11) * 2^-53`` and
  ``d_j = 2*u_j - 1``; angle = ``d_0*rotation`` degrees; s = ``1 + d_1*scale``;
  tx = ``(d_2*shift)*W``, ty = ``(d_3*shift)*H``; q = ``clip(16 + rint((d_4*speed)*16), 8, 32)``;
  start = ``base + rint(d_5*tshift)``; with ``c, s_ = cos, sin(radians(angle))`` (Python's math, as
  in islpose/augment.py) and ``(cx, cy) = ((W-1)/2, (H-1)/2)``: ``m0 = s*c``, ``m1 = -(s*s_)``,
  ``m2 = (cx + tx) - (m0*cx + m1*cy)``, ``m3 = s*s_``, ``m4 = s*c``,
  ``m5 = (cy + ty) - (m3*cx + m4*cy)``, and 0.0 is added to each so that a zero is +0.  All
  magnitudes 0 give the identity item exactly.

drop and jitter are fp32 numbers (the C struct's): their fp32 values enter the arithmetic above.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from .augment import _number

MAX_WINDOW, MAX_FEATURES, MAX_ITEMS = 32, 256, 65535
MAX_DROP = 0.9
SITE_DROP, SITE_JITTER, SITE_HOST = 16, 17, 32

# isl_sign_aug_item, 80 bytes
ITEM_DTYPE = np.dtype([("row0", "<i8"), ("nrows", "<i4"), ("start", "<i4"), ("q", "<i4"), ("reserved", "<i4"),
                       ("id", "<u8"), ("m", "<f8", (6,))])
assert ITEM_DTYPE.itemsize == 80

_SPEC_KEYS = {"rot": "rotation", "scale": "scale", "shift": "shift", "speed": "speed", "tshift": "tshift",
              "drop": "drop", "jitter": "jitter"}


def sm(z):
    """The splitmix64 finaliser of section 4.2k on a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def window_key(seed, step, ids):
    """kw = sm(sm(seed ^ step) ^ id) for every id, uint64."""
    k0 = sm(np.array([int(seed) ^ int(step)], np.uint64))
    return sm(k0 ^ np.asarray(ids, np.uint64))


def site_draw(kw, site, index):
    """sm(kw ^ (site << 32 | index)), broadcast over kw and index (uint64)."""
    return sm(np.asarray(kw, np.uint64) ^ (np.uint64(site << 32) | np.asarray(index, np.uint64)))


def drop_threshold(drop):
    """floor(drop * 2^24 + 0.5) of the fp32 rate (the product is exact in fp64; halves round up)."""
    return int(np.floor(np.float64(np.float32(drop)) * 2.0 ** 24 + 0.5))


def check_layout(layout, n_features=None):
    """(n_body, n_slots, n_hand) as ints; ValueError for a negative or non-integer count, a row
    longer than 256 features, or a size that is not n_features."""
    try:
        lay = tuple(layout)
    except TypeError:
        lay = ()
    if len(lay) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0 for v in lay):
        raise ValueError("layout must be three integers >= 0 (n_body, n_slots, n_hand), got %r" % (layout,))
    lay = tuple(int(v) for v in lay)
    F = 2 * lay[0] + lay[1] * 3 * lay[2]
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError("layout %r has %d features, outside [1, %d]" % (lay, F, MAX_FEATURES))
    if n_features is not None and F != n_features:
        raise ValueError("layout %r has %d features, the rows have %d" % (lay, F, n_features))
    return lay


def identity_layout(n_features):
    """A layout of n_features >= 2 for items that change no value (the identity map gives every
    pair its own bits, whichever entries are paired)."""
    F = int(n_features)
    if not 2 <= F <= MAX_FEATURES:
        raise ValueError("n_features must be in [2, %d], got %r" % (MAX_FEATURES, n_features))
    return (F // 2, 0, 0) if F % 2 == 0 else ((F - 3) // 2, 1, 1)


def layout_index(layout):
    """(x index [P], y index [P], label index [L]) of a layout's pairs and labels in the row."""
    nb, ns, nh = layout
    xs = list(range(nb)) + [2 * nb + s * 3 * nh + o for s in range(ns) for o in range(nh)]
    ys = list(range(nb, 2 * nb)) + [2 * nb + s * 3 * nh + nh + o for s in range(ns) for o in range(nh)]
    labs = [2 * nb + s * 3 * nh + 2 * nh + o for s in range(ns) for o in range(nh)]
    return np.array(xs, np.int64), np.array(ys, np.int64), np.array(labs, np.int64)


def check_window(window):
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, np.integer)) or not 1 <= window <= MAX_WINDOW:
        raise ValueError("window must be an integer in [1, %d], got %r" % (MAX_WINDOW, window))
    return int(window)


def _uint64(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2 ** 64:
        raise ValueError("%s must be an integer in [0, 2^64), got %r" % (name, v))
    return int(v)


def check_items(items, n_rows):
    """Items as a contiguous ITEM_DTYPE array; ValueError unless every item has nrows >= 1, q in
    [8, 32], reserved 0, a finite m, and rows inside [0, n_rows)."""
    it = np.asarray(items)
    if it.dtype != ITEM_DTYPE or it.ndim != 1:
        raise ValueError("items must be a 1-d array of sign_augment.ITEM_DTYPE (WindowAugment.items)")
    if len(it) > MAX_ITEMS:
        raise ValueError("at most %d items per launch, got %d" % (MAX_ITEMS, len(it)))
    if np.any(it["nrows"] < 1):
        raise ValueError("item nrows must be >= 1")
    if np.any((it["q"] < 8) | (it["q"] > 32)):
        raise ValueError("item q must be in [8, 32]")
    if np.any(it["reserved"] != 0):
        raise ValueError("item reserved field must be 0")
    if not np.all(np.isfinite(it["m"])):
        raise ValueError("item m must be finite")
    if np.any(it["row0"] < 0) or np.any(it["row0"] > int(n_rows) - it["nrows"].astype(np.int64)):
        raise ValueError("an item's rows leave the store of %d rows" % int(n_rows))
    return np.ascontiguousarray(it)


def source_rows(window, q, start):
    """r [n, window] of the definition for per-item q and start (int64)."""
    T = int(window)
    t = np.arange(T, dtype=np.int64)[None, :]
    q = np.asarray(q, np.int64)[:, None]
    return ((2 * t - (T - 1)) * q + 16 * (T - 1) + 16) // 32 + np.asarray(start, np.int64)[:, None]


class WindowAugment:
    """Per-window, per-step augmentation of keypoint rows.

    rotation: degrees, in [0, 180]; scale, shift (a share of the frame), speed: in [0, 0.5]; tshift:
    frames, an integer in [0, 32]; drop: the share of frames zeroed, in [0, 0.9]; jitter: pixels,
    >= 0.  frame = (W, H) of the coordinates; layout = (n_body, n_slots, n_hand) of the rows; seed of
    the draws (the trainer passes its own)."""

    def __init__(self, rotation=0., scale=0., shift=0., speed=0., tshift=0, drop=0., jitter=0.,
                 frame=(1920, 1080), layout=(15, 2, 21), seed=0):
        self.rotation = float(_number("rotation", rotation, 0, 180))
        self.scale = float(_number("scale", scale, 0, 0.5))
        self.shift = float(_number("shift", shift, 0, 0.5))
        self.speed = float(_number("speed", speed, 0, 0.5))
        _number("tshift", tshift, 0, 32)
        if int(tshift) != tshift:
            raise ValueError("tshift must be an integer in [0, 32], got %r" % (tshift,))
        self.tshift = int(tshift)
        self.drop = float(_number("drop", drop, 0, MAX_DROP))
        if np.float32(self.drop) > np.float32(MAX_DROP):
            raise ValueError("drop must be in [0, %g], got %r" % (MAX_DROP, drop))
        self.jitter = float(_number("jitter", jitter, 0))
        if self.jitter > float(np.finfo(np.float32).max):
            raise ValueError("jitter must be finite in fp32, got %r" % (jitter,))
        try:
            W, H = frame
        except (TypeError, ValueError):
            raise ValueError("frame must be (W, H), got %r" % (frame,))
        self.frame = (float(_number("frame width", W, 0)), float(_number("frame height", H, 0)))
        self.layout = check_layout(layout)
        self.n_features = 2 * self.layout[0] + self.layout[1] * 3 * self.layout[2]
        self.seed = _uint64("seed", seed)

    @classmethod
    def parse(cls, spec, **kw):
        """The tools' --augment syntax -> a WindowAugment: comma-separated KEY:VALUE with the keys
        rot, scale, shift, speed, tshift, drop and jitter, e.g.
        'rot:15,scale:0.1,shift:0.05,speed:0.2,tshift:3,drop:0.1,jitter:2'.  An empty spec gives
        None.  kw: frame, layout, seed."""
        if not spec:
            return None
        args = {}
        for part in spec.split(","):
            f = part.strip().split(":")
            if len(f) != 2 or f[0] not in _SPEC_KEYS:
                raise ValueError("--augment %r: expected KEY:VALUE with KEY one of %s" % (part, ", ".join(_SPEC_KEYS)))
            name = _SPEC_KEYS[f[0]]
            if name in args:
                raise ValueError("--augment %r: %s given twice" % (part, f[0]))
            try:
                args[name] = int(f[1]) if name == "tshift" else float(f[1])
            except ValueError:
                raise ValueError("--augment %r: %r is not a number" % (part, f[1]))
        try:
            return cls(**args, **kw)
        except ValueError as e:
            raise ValueError("--augment %r: %s" % (spec, e))

    # ------------------------------------------------------------------ host: the items
    def items(self, ids, step, nrows, row0, base=0, seed=None):
        """The items of one step as an ITEM_DTYPE array: ids [n] (uint64 sample ids); nrows, row0
        and base per item or one value for all.  seed None: the augment's own."""
        ids = np.asarray(ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("ids must be a 1-d integer array, got %s %s" % (ids.dtype, ids.shape))
        ids = ids.astype(np.uint64)
        n = len(ids)
        seed = self.seed if seed is None else _uint64("seed", seed)
        step = _uint64("step", step)
        nrows, row0, base = (np.broadcast_to(np.asarray(v), (n,)) for v in (nrows, row0, base))
        for name, v in (("nrows", nrows), ("row0", row0), ("base", base)):
            if v.dtype.kind not in "iu":
                raise ValueError("%s must be integers, got %s" % (name, v.dtype))
        if n and (nrows.min() < 1 or nrows.max() >= 2 ** 31 or row0.min() < 0 or abs(base).max() >= 2 ** 30):
            raise ValueError("nrows must be in [1, 2^31), row0 >= 0 and |base| < 2^30")
        kw = window_key(seed, step, ids)
        k = site_draw(kw[:, None], SITE_HOST, np.arange(6, dtype=np.uint64)[None, :])
        u = (k >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        d = 2.0 * u - 1.0
        angle = d[:, 0] * self.rotation
        s = 1.0 + d[:, 1] * self.scale
        W, H = self.frame
        tx = (d[:, 2] * self.shift) * W
        ty = (d[:, 3] * self.shift) * H
        q = np.clip(16.0 + np.rint((d[:, 4] * self.speed) * 16.0), 8.0, 32.0)
        start = base.astype(np.float64) + np.rint(d[:, 5] * float(self.tshift))
        if self.rotation > 0:
            rad = [math.radians(a) for a in angle.tolist()]
            c = np.array([math.cos(r) for r in rad], np.float64)
            s_ = np.array([math.sin(r) for r in rad], np.float64)
        else:
            c, s_ = np.ones(n), np.zeros(n)
        cx, cy = (W - 1.0) / 2.0, (H - 1.0) / 2.0
        m0, m1, m3, m4 = s * c, -(s * s_), s * s_, s * c
        m2 = (cx + tx) - (m0 * cx + m1 * cy)
        m5 = (cy + ty) - (m3 * cx + m4 * cy)
        out = np.zeros(n, ITEM_DTYPE)
        out["row0"], out["nrows"], out["start"], out["q"], out["id"] = row0, nrows, start, q, ids
        out["m"] = np.stack([m0, m1, m2, m3, m4, m5], axis=1) + 0.0
        return out

    # ------------------------------------------------------------------ the transform
    def _check_rows_shape(self, shape):
        if len(shape) != 2 or not 1 <= shape[1] <= MAX_FEATURES:
            raise ValueError("rows must be [n_rows, F <= %d], got %s" % (MAX_FEATURES, tuple(shape)))
        check_layout(self.layout, shape[1])

    def apply_numpy(self, rows, items, window, step, seed=None, out=None):
        """The GPU-less form: rows fp32 [n_rows, F] (array-like), items from `items` -> fp32
        [n, window, F], bit for bit what `apply` gives.  out: the destination, which must not
        share memory with the rows."""
        rows = np.asarray(rows)
        if rows.dtype != np.float32:
            raise ValueError("rows: float32 expected, got %s" % rows.dtype)
        self._check_rows_shape(rows.shape)
        T = check_window(window)
        it = check_items(items, rows.shape[0])
        seed = self.seed if seed is None else _uint64("seed", seed)
        step = _uint64("step", step)
        n, F = len(it), rows.shape[1]
        if out is None:
            out = np.empty((n, T, F), np.float32)
        elif not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != (n, T, F) \
                or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous float32 [%d, %d, %d] array" % (n, T, F))
        elif np.shares_memory(out, rows):
            raise ValueError("out overlaps the rows")
        out[...] = 0
        if n == 0:
            return out
        kw = window_key(seed, step, it["id"])
        tt = np.arange(T, dtype=np.uint64)[None, :]
        r = source_rows(T, it["q"], it["start"])
        live = (r >= 0) & (r < it["nrows"].astype(np.int64)[:, None])
        thr = drop_threshold(self.drop)
        if thr:
            live &= (site_draw(kw[:, None], SITE_DROP, tt) >> np.uint64(40)) >= np.uint64(thr)
        src = rows[np.where(live, it["row0"][:, None] + r, 0)]          # [n, T, F]; junk where not live
        xi, yi, li = layout_index(self.layout)
        x, y = src[:, :, xi].astype(np.float64), src[:, :, yi].astype(np.float64)
        m = it["m"][:, None, :, None]                                   # [n, 1, 6, 1]
        # separate numpy operations: every product and sum rounds on its own (no FMA)
        X = (m[:, :, 0] * x + m[:, :, 1] * y) + m[:, :, 2]
        Y = (m[:, :, 3] * x + m[:, :, 4] * y) + m[:, :, 5]
        jit = np.float64(np.float32(self.jitter))
        if jit > 0:
            j = tt[:, :, None] * np.uint64(512) + np.uint64(2) * np.arange(len(xi), dtype=np.uint64)[None, None, :]
            ux = (site_draw(kw[:, None, None], SITE_JITTER, j) >> np.uint64(40)).astype(np.float64)
            uy = (site_draw(kw[:, None, None], SITE_JITTER, j + np.uint64(1)) >> np.uint64(40)).astype(np.float64)
            X = X + jit * (ux * 2.0 ** -23 - 1.0)
            Y = Y + jit * (uy * 2.0 ** -23 - 1.0)
        with np.errstate(over="ignore", invalid="ignore"):
            X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
        X32 = np.where((X32 == 0) & (Y32 == 0), np.float32(2.0 ** -10), X32)
        present = live[:, :, None] & ((src[:, :, xi] != 0) | (src[:, :, yi] != 0))
        out[:, :, xi] = np.where(present, X32, np.float32(0))
        out[:, :, yi] = np.where(present, Y32, np.float32(0))
        out[:, :, li] = np.where(live[:, :, None], src[:, :, li], np.float32(0))
        return out

    def apply(self, rows_t, items, window, step, seed=None, out=None, stream=None):
        """rows_t cuda fp32 [n_rows, F]; items from `items` -> cuda fp32 [n, window, F] in one launch
        (isl_sign_augment) on the current stream, without waiting for the device.  out: the
        destination, which must not overlap the rows."""
        import torch
        from . import runtime as rt
        if not (isinstance(rows_t, torch.Tensor) and rows_t.is_cuda and rows_t.dtype == torch.float32):
            raise ValueError("rows: a cuda float32 tensor expected, got %r" % (type(rows_t),))
        self._check_rows_shape(tuple(rows_t.shape))
        if not rows_t.is_contiguous():
            raise ValueError("rows must be contiguous")
        T = check_window(window)
        it = check_items(items, rows_t.shape[0])
        seed = self.seed if seed is None else _uint64("seed", seed)
        step = _uint64("step", step)
        n, F = len(it), rows_t.shape[1]
        if out is None:
            out = torch.empty((n, T, F), dtype=torch.float32, device=rows_t.device)
        else:
            if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == rows_t.device
                    and tuple(out.shape) == (n, T, F) and out.is_contiguous()):
                raise ValueError("out must be a contiguous cuda float32 [%d, %d, %d] tensor on the rows' device" % (n, T, F))
            check_no_overlap(rows_t.data_ptr(), rows_t.numel() * 4, out.data_ptr(), out.numel() * 4)
        if n == 0:
            return out
        # the records go through pinned memory, so the copy does not wait for the stream
        pin = torch.empty(n * ITEM_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
        pin.numpy()[:] = it.view(np.uint8).reshape(-1)
        with torch.cuda.device(rows_t.device), torch.cuda.stream(stream):
            items_t = pin.to(rows_t.device, non_blocking=True)
            opts = rt.IslSignAugOpts(self.drop, self.jitter, seed, step)
            rt.sign_augment(rows_t, self.layout, items_t, n, T, opts, out)
        return out


def check_no_overlap(a_ptr, a_bytes, b_ptr, b_bytes):
    """ValueError if the byte ranges [a_ptr, a_ptr + a_bytes) and [b_ptr, b_ptr + b_bytes) overlap."""
    if a_bytes and b_bytes and a_ptr < b_ptr + b_bytes and b_ptr < a_ptr + a_bytes:
        raise ValueError("out overlaps the rows")


def clip_items(lengths, window=20, stride=5):
    """The static windows of clips of `lengths` rows, enumerated as tools/train_sign.py's
    cut_windows cuts them: (clip index, base) per window, int64 arrays.  A clip shorter than the
    window gives one window at base 0, an empty clip none."""
    clip, base = [], []
    for k, n in enumerate(lengths):
        n = int(n)
        if n <= 0:
            continue
        starts = [0] if n < window else range(0, n - window + 1, stride)
        for s in starts:
            clip.append(k)
            base.append(s)
    return np.array(clip, np.int64), np.array(base, np.int64)
