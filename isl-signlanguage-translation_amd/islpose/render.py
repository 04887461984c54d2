"""Stick-model overlays of the keypoints.

The reference's extraction scripts write a picture beside every keypoint JSON:
``util.drawStickmodel`` on the frame (extract_features_mp.py:85-91), and its demos show
``util.draw_bodypose`` / ``util.draw_handpose``.  Those run cv2's polygon rasteriser and a
matplotlib figure on the host, one full-canvas copy and blend per limb.  Here a picture is a
list of primitives per frame, drawn onto frames that are already resident by one launch
(``isl_draw``, csrc/draw.hip); ``apply_numpy`` is the same definition on the host.

The definition (the kernel, ``apply_numpy`` and the tests share it, byte for byte)
--------------------------------------------------------------------------------
A frame is ``uint8 [H, W, 3]``; a colour goes to channels 0, 1, 2 as given.  A frame's
primitives are applied in list order (the blend does not commute).  All arithmetic is integer;
``(x, y)`` is the pixel, ``dx = x - cx``, ``dy = y - cy``.

* stick (kind 0): centre ``(cx, cy)``, half axes ``a`` in [1, 4096] and ``b`` in [1, 16],
  ``C = round(cos t * 16384)``, ``S = round(sin t * 16384)`` of the integer angle ``t`` in
  degrees.  ``u = dx*C + dy*S``, ``v = -dx*S + dy*C``; covered iff ``|u| <= a*2^14`` and
  ``|v| <= b*2^14`` and ``u^2*b^2 + v^2*a^2 <= a^2*b^2*2^28``.
* disc (kind 1): covered iff ``dx^2 + dy^2 <= r2``, ``r2`` in [0, 4096].
* segment (kind 2): ends ``P0``, ``P1``; ``d = P1 - P0``, ``L2 = d.d``, ``w = (x, y) - P0``,
  ``t = w.d``, ``cr = w.x*d.y - w.y*d.x``; covered iff ``L2 > 0 and 0 <= t <= L2 and cr^2 <= r2*L2``, or
  ``|w|^2 <= r2``, or ``|(x, y) - P1|^2 <= r2`` (``L2 = 0``: the disc).
* a covered channel value ``v`` under colour ``k`` becomes ``k`` (blend 0) or
  ``(4*v + 6*k + 5) // 10`` (blend 1) -- ``rint(0.4*v + 0.6*k)`` for all 65536 pairs, what
  ``cv2.addWeighted(canvas, 0.4, cur, 0.6, 0)`` leaves inside a limb.
* coordinates lie in [-16384, 16384], ``H, W <= 16384``, ``H*W <= 2^29``; what lies off the
  frame is clipped.

Parity with cv2's and matplotlib's pixels is **unpinned**: both are absent here.  Two
deviations from the reference are deliberate: body colours go by limb / joint type as
``draw_bodypose`` does (``drawStickmodel`` indexes them by list position, which breaks with two
persons), and hand peaks at ``[0, 0]`` ("not found") are skipped (the reference plots them at
the origin).
"""
from __future__ import annotations

import collections
import colorsys
import ctypes
import math

import numpy as np

STICK, DISC, SEGMENT = 0, 1, 2
COORD_MAX = 16384
SIZE_MAX = 16384
PIXELS_MAX = 1 << 29
PRIMS_MAX = 1 << 20

# one primitive: kind, p (cx, cy, a, b | cx, cy, 0, 0 | x0, y0, x1, y1), c, s, r2, color, blend
Prim = collections.namedtuple("Prim", "kind p c s r2 color blend")


class _Checked(Prim):
    """A Prim that check_prim made: immutable, so it need not be checked again."""
    __slots__ = ()

# util.py:64-67
BODY_COLORS = [(255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 255, 0), (170, 255, 0), (85, 255, 0), (0, 255, 0),
               (0, 255, 85), (0, 255, 170), (0, 255, 255), (0, 170, 255), (0, 85, 255), (0, 0, 255), (85, 0, 255),
               (170, 0, 255), (255, 0, 255), (255, 0, 170), (255, 0, 85), (255, 255, 0), (255, 255, 85),
               (255, 255, 170), (255, 255, 255), (170, 255, 255), (85, 255, 255), (0, 255, 255)]


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    return int(v)


def _color(color):
    try:
        c = tuple(color)
    except TypeError:
        raise ValueError("color: three integers in [0, 255] expected, got %r" % (color,))
    if len(c) != 3:
        raise ValueError("color: three integers in [0, 255] expected, got %r" % (color,))
    return tuple(_int("color", v, 0, 255) for v in c)


def cos_sin(angle):
    """(C, S) of the definition for an integer angle in degrees."""
    r = math.radians(angle)
    return int(round(math.cos(r) * 16384)), int(round(math.sin(r) * 16384))


def stick(cx, cy, a, b, angle, color, blend=1):
    """A filled ellipse with half axes a (along the angle, in integer degrees, image
    coordinates) and b, as ellipse2Poly + fillConvexPoly draw a limb."""
    angle = _int("angle", angle, -(1 << 30), 1 << 30)
    c, s = cos_sin(angle)
    return check_prim(Prim(STICK, (cx, cy, a, b), c, s, 0, _color(color), blend))


def disc(cx, cy, color, r2=16, blend=0):
    """The pixels within squared distance r2 of (cx, cy)."""
    return check_prim(Prim(DISC, (cx, cy, 0, 0), 0, 0, r2, _color(color), blend))


def segment(x0, y0, x1, y1, color, r2=2, blend=0):
    """The pixels within squared distance r2 of the segment (x0, y0) - (x1, y1)."""
    return check_prim(Prim(SEGMENT, (x0, y0, x1, y1), 0, 0, r2, _color(color), blend))


def check_prim(q):
    """A Prim with plain ints, or ValueError for anything isl_draw would refuse."""
    if type(q) is _Checked:
        return q
    try:
        kind, p, c, s, r2, color, blend = q
        p = tuple(p)
    except (TypeError, ValueError):
        raise ValueError("not a primitive: %r" % (q,))
    if isinstance(kind, (bool, np.bool_)) or kind not in (STICK, DISC, SEGMENT):
        raise ValueError("unknown primitive kind %r" % (kind,))
    if len(p) != 4:
        raise ValueError("a primitive has four parameters, got %r" % (p,))
    blend = _int("blend", blend, 0, 1)
    color = _color(color)
    x0, y0 = _int("coordinate", p[0], -COORD_MAX, COORD_MAX), _int("coordinate", p[1], -COORD_MAX, COORD_MAX)
    if kind == STICK:
        p = (x0, y0, _int("half axis a", p[2], 1, 4096), _int("half axis b", p[3], 1, 16))
        return _Checked(STICK, p, _int("c", c, -16384, 16384), _int("s", s, -16384, 16384), 0, color, blend)
    r2 = _int("r2", r2, 0, 4096)
    if kind == DISC:
        return _Checked(DISC, (x0, y0, 0, 0), 0, 0, r2, color, blend)
    p = (x0, y0, _int("coordinate", p[2], -COORD_MAX, COORD_MAX), _int("coordinate", p[3], -COORD_MAX, COORD_MAX))
    return _Checked(SEGMENT, p, 0, 0, r2, color, blend)


def body_primitives(candidate, subset, model_type="body25", order="sticks_first"):
    """The body's primitives from a Body result.  Sticks: src.util.get_bodypose's tuples as
    util.drawStickmodel reads them (util.py:318-323) -- centre (int(x mean), int(y mean)),
    a = max(int(length / 2), 1), b = 4, angle int(angle), blended; joints: a disc of r2 = 16 per
    present joint, overwriting (util.py:327-328).  Colours go by limb / joint type, as
    draw_bodypose's do (util.py:75,92).  order: 'sticks_first' (drawStickmodel) or
    'joints_first' (draw_bodypose)."""
    from src import util
    if order not in ("sticks_first", "joints_first"):
        raise ValueError("order is 'sticks_first' or 'joints_first', got %r" % (order,))
    if model_type not in ("body25", "coco"):
        raise ValueError("model_type is 'body25' or 'coco', got %r" % (model_type,))
    candidate, subset = np.asarray(candidate), np.asarray(subset)
    limbs, njoint = (util.BODY25_LIMBS, 25) if model_type == "body25" else (util.COCO_LIMBS, 18)
    circles, tuples = util.get_bodypose(candidate, subset, model_type)
    # the types, in get_bodypose's own iteration order
    joint_type = [i for i in range(njoint) for n in range(len(subset)) if int(subset[n][i]) != -1]
    limb_type = [i for i in range(njoint - 1) for n in range(len(subset)) if -1 not in subset[n][np.array(limbs[i])]]
    assert len(joint_type) == len(circles) and len(limb_type) == len(tuples)
    sticks = [stick(int(mx), int(my), max(int(length / 2), 1), 4, int(angle), BODY_COLORS[i])
              for i, (mx, my, angle, length) in zip(limb_type, tuples)]
    joints = [disc(int(x), int(y), BODY_COLORS[i]) for i, (x, y) in zip(joint_type, circles)]
    return sticks + joints if order == "sticks_first" else joints + sticks


def hand_primitives(all_hand_peaks, dot=(255, 0, 0)):
    """The hands' primitives (util.draw_handpose, util.py:154-185): per hand the 20 edges as
    segments of r2 = 2 in round(255 * hsv_to_rgb(ie / 20, 1, 1)), an edge only when neither end
    is [0, 0]; then a disc of r2 = 16 in `dot` per peak that is not [0, 0]."""
    from src import util
    dot = _color(dot)
    out = []
    for peaks in all_hand_peaks:
        pk = np.asarray(peaks)
        if pk.shape != (21, 2):
            raise ValueError("hand peaks: [21, 2] expected, got shape %r" % (pk.shape,))
        found = [bool(pk[i, 0] != 0 or pk[i, 1] != 0) for i in range(21)]
        for ie, (i, j) in enumerate(util.HAND_EDGES):
            if found[i] and found[j]:
                col = tuple(int(round(255 * v)) for v in colorsys.hsv_to_rgb(ie / 20.0, 1.0, 1.0))
                out.append(segment(int(pk[i, 0]), int(pk[i, 1]), int(pk[j, 0]), int(pk[j, 1]), col))
        out += [disc(int(pk[i, 0]), int(pk[i, 1]), dot) for i in range(21) if found[i]]
    return out


def _check_shape(shape):
    shape = tuple(shape)
    if len(shape) != 4 or shape[3] != 3 or shape[0] < 0 or not 1 <= shape[1] <= SIZE_MAX \
            or not 1 <= shape[2] <= SIZE_MAX or shape[1] * shape[2] > PIXELS_MAX:
        raise ValueError("frames: uint8 [n, H, W, 3] with H, W in [1, 16384] and H * W <= 2^29 expected, got "
                         "shape %r" % (shape,))
    return tuple(int(v) for v in shape)


def _check_lists(prim_lists, n):
    lists = [[check_prim(q) for q in lst] for lst in prim_lists]
    if len(lists) != n:
        raise ValueError("one primitive list per frame: %d lists for %d frames" % (len(lists), n))
    if sum(len(lst) for lst in lists) > PRIMS_MAX:
        raise ValueError("at most 2^20 primitives per call, got %d" % sum(len(lst) for lst in lists))
    return lists


def apply(frames_t, prim_lists, out=None, stream=None, shape=None, device=None):
    """frames_t cuda uint8 [n, H, W, 3] with frame f's list prim_lists[f] drawn, in one launch
    (isl_draw).  out=None: a new tensor; out=frames_t: in place; any other contiguous cuda
    uint8 tensor of the shape that does not overlap frames_t: the destination.  frames_t=None
    with shape=(n, H, W, 3) (and optionally device): the drawing on an all-zero canvas."""
    import torch
    from . import runtime as rt
    if frames_t is None:
        if shape is None and out is None:
            raise ValueError("frames=None needs a shape (n, H, W, 3) or an out tensor")
        shape = _check_shape(out.shape if shape is None else shape)
    else:
        if not (isinstance(frames_t, torch.Tensor) and frames_t.is_cuda and frames_t.dtype == torch.uint8):
            raise ValueError("frames: a cuda uint8 tensor expected, got %r" % (type(frames_t),))
        if not frames_t.is_contiguous():
            raise ValueError("frames: a contiguous tensor expected")
        if shape is not None and tuple(shape) != tuple(frames_t.shape):
            raise ValueError("shape %r does not match the frames' %r" % (tuple(shape), tuple(frames_t.shape)))
        shape = _check_shape(frames_t.shape)
        device = frames_t.device
    lists = _check_lists(prim_lists, shape[0])
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device="cuda" if device is None else device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
              and tuple(out.shape) == shape and (frames_t is None or out.device == frames_t.device)):
        raise ValueError("out: a contiguous cuda uint8 tensor of shape %r on the frames' device expected" % (shape,))
    if shape[0] == 0:
        return out                                   # (an empty tensor has no address to pass)
    first = [0]
    for lst in lists:
        first.append(first[-1] + len(lst))
    # the 40-byte records as rows of ten little-endian int32: color[3] and blend share the ninth
    rows = [(q.kind, q.p[0], q.p[1], q.p[2], q.p[3], q.c, q.s, q.r2,
             q.color[0] | q.color[1] << 8 | q.color[2] << 16 | q.blend << 24, 0) for lst in lists for q in lst]
    table = np.array(rows, dtype="<i4").reshape(-1, 10)
    arr = table.ctypes.data_as(ctypes.POINTER(rt.IslDrawPrim)) if rows else None
    return rt.draw(frames_t, out, arr, first, stream=stream)


def _covered(q, xs, ys):
    """The definition's coverage test of primitive q on int64 pixel coordinate arrays."""
    dx, dy = xs - q.p[0], ys - q.p[1]
    if q.kind == STICK:
        a, b = q.p[2], q.p[3]
        u, v = dx * q.c + dy * q.s, dy * q.c - dx * q.s
        box = (np.abs(u) <= a << 14) & (np.abs(v) <= b << 14)
        # the squares only where the box holds: elsewhere they may pass 2^63
        u, v = np.where(box, u, 0), np.where(box, v, 0)
        return box & (u * u * (b * b) + v * v * (a * a) <= (a * a * b * b) << 28)
    near = dx * dx + dy * dy <= q.r2
    if q.kind == DISC:
        return near
    ex, ey = xs - q.p[2], ys - q.p[3]
    ddx, ddy = q.p[2] - q.p[0], q.p[3] - q.p[1]
    L2 = ddx * ddx + ddy * ddy
    t, cr = dx * ddx + dy * ddy, dx * ddy - dy * ddx
    return near | (ex * ex + ey * ey <= q.r2) | ((t >= 0) & (t <= L2) & (cr * cr <= q.r2 * L2) & (L2 > 0))


def _reach(q, H, W):
    """A conservative inclusive pixel box (x0, y0, x1, y1) of q inside the frame, None if
    empty.  A covered pixel of a stick has (C^2 + S^2) * (dx^2 + dy^2) = u^2 + v^2
    <= (a^2 + b^2) * 2^28."""
    if q.kind == STICK:
        nn = q.c * q.c + q.s * q.s
        if nn == 0:
            return 0, 0, W - 1, H - 1
        r = math.isqrt(((q.p[2] ** 2 + q.p[3] ** 2) << 28) // nn) + 1
        box = [q.p[0] - r, q.p[1] - r, q.p[0] + r, q.p[1] + r]
    else:
        r = math.isqrt(q.r2) + 1
        xs, ys = ([q.p[0], q.p[2]], [q.p[1], q.p[3]]) if q.kind == SEGMENT else ([q.p[0]], [q.p[1]])
        box = [min(xs) - r, min(ys) - r, max(xs) + r, max(ys) + r]
    x0, y0, x1, y1 = max(box[0], 0), max(box[1], 0), min(box[2], W - 1), min(box[3], H - 1)
    return None if x0 > x1 or y0 > y1 else (x0, y0, x1, y1)


def apply_numpy(frames, prim_lists, shape=None):
    """The GPU-less form of the same definition: frames uint8 [n, H, W, 3] (array-like; None
    with shape=(n, H, W, 3): all-zero canvases), prim_lists one list of primitives per frame ->
    a new uint8 array, byte for byte what `apply` gives."""
    if frames is None:
        if shape is None:
            raise ValueError("frames=None needs a shape (n, H, W, 3)")
        out = np.zeros(_check_shape(shape), np.uint8)
    else:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8:
            raise ValueError("frames: uint8 expected, got %s" % frames.dtype)
        _check_shape(frames.shape)
        out = np.array(frames, dtype=np.uint8, order="C")
    n, H, W, _ = out.shape
    for f, lst in enumerate(_check_lists(prim_lists, n)):
        for q in lst:
            box = _reach(q, H, W)
            if box is None:
                continue
            x0, y0, x1, y1 = box
            xs = np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
            ys = np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
            m = _covered(q, xs, ys)
            if not m.any():
                continue
            view = out[f, y0:y1 + 1, x0:x1 + 1]
            k = np.array(q.color, dtype=np.int64)
            new = (4 * view.astype(np.int64) + 6 * k + 5) // 10 if q.blend else np.broadcast_to(k, view.shape)
            view[m] = new[m].astype(np.uint8)
    return out
