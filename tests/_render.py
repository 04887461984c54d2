"""The stick-model drawing definition stated with Python ints, one pixel
and one primitive at a time, and the inputs the render tests share.  Nothing here comes from
islpose/render.py: a primitive is the plain tuple (kind, (p0, p1, p2, p3), c, s, r2, (k0, k1, k2),
blend), which is also what islpose.render accepts."""
import functools
import math

import numpy as np

STICK, DISC, SEGMENT = 0, 1, 2


def cs(angle):
    r = math.radians(angle)
    return int(round(math.cos(r) * 16384)), int(round(math.sin(r) * 16384))


def stick(cx, cy, a, b, angle, color, blend=1):
    c, s = cs(angle)
    return (STICK, (cx, cy, a, b), c, s, 0, tuple(color), blend)


def disc(cx, cy, r2, color, blend=0):
    return (DISC, (cx, cy, 0, 0), 0, 0, r2, tuple(color), blend)


def segment(x0, y0, x1, y1, r2, color, blend=0):
    return (SEGMENT, (x0, y0, x1, y1), 0, 0, r2, tuple(color), blend)


def covers(q, x, y):
    kind, p, c, s, r2 = q[0], q[1], q[2], q[3], q[4]
    if kind == STICK:
        cx, cy, a, b = p
        dx, dy = x - cx, y - cy
        u = dx * c + dy * s
        v = -dx * s + dy * c
        if abs(u) > a * 2 ** 14 or abs(v) > b * 2 ** 14:
            return False
        return u * u * b * b + v * v * a * a <= a * a * b * b * 2 ** 28
    if kind == DISC:
        dx, dy = x - p[0], y - p[1]
        return dx * dx + dy * dy <= r2
    wx, wy = x - p[0], y - p[1]
    ddx, ddy = p[2] - p[0], p[3] - p[1]
    L2 = ddx * ddx + ddy * ddy
    t = wx * ddx + wy * ddy
    cr = wx * ddy - wy * ddx
    if L2 > 0 and 0 <= t <= L2 and cr * cr <= r2 * L2:      # L2 = 0: the disc
        return True
    if wx * wx + wy * wy <= r2:
        return True
    ex, ey = x - p[2], y - p[3]
    return ex * ex + ey * ey <= r2


def colour(v, k, blend):
    return (4 * v + 6 * k + 5) // 10 if blend else k


def draw(frames, lists):
    """(frames with the lists drawn, all-zero canvases with the lists drawn): the coverage of a
    pixel does not depend on the canvas, so both pictures come from one walk."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    out, blank = frames.copy(), np.zeros_like(frames)
    for f in range(n):
        for y in range(H):
            for x in range(W):
                for q in lists[f]:
                    if covers(q, x, y):
                        for ch in range(3):
                            out[f, y, x, ch] = colour(int(out[f, y, x, ch]), q[5][ch], q[6])
                            blank[f, y, x, ch] = colour(int(blank[f, y, x, ch]), q[5][ch], q[6])
    return out, blank


def _frames(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# three blended sticks that overlap around (26, 18): reversing them changes bytes
ORDERED = [stick(26, 18, 14, 4, 30, (255, 0, 0)), stick(27, 19, 12, 4, -45, (0, 255, 85)),
           stick(25, 17, 10, 3, 80, (85, 0, 255))]


def _case_odd():
    """3 x 37 x 53: 3*W = 159 is odd and a frame is 5883 bytes, so rows and frame bases fall on
    every byte phase.  Frame 0: the ordered sticks and an overwriting disc; frame 1: centres off
    and half off the frame; frame 2: a degenerate segment, r2 = 0, and the largest disc."""
    lists = [
        ORDERED + [disc(26, 18, 16, (255, 255, 255))],
        [disc(-3, 10, 16, (255, 85, 0)), disc(60, 40, 16, (1, 2, 3)), stick(52, 36, 9, 4, 20, (0, 170, 255)),
         segment(-10, -10, 20, 15, 2, (255, 0, 170)), stick(-100, -100, 30, 4, 45, (9, 9, 9)),
         disc(0, 0, 9, (0, 255, 0), 1), disc(52, 36, 4, (255, 255, 0)), segment(40, 50, 45, -6, 5, (7, 200, 90), 1),
         stick(26, -2, 20, 4, 0, (170, 0, 255)), disc(16384, -16384, 4096, (5, 5, 5))],
        [segment(10, 10, 10, 10, 9, (255, 0, 0)), segment(30, 5, 44, 9, 0, (0, 0, 255)), disc(5, 30, 0, (0, 255, 255)),
         segment(20, 30, 20, 30, 0, (255, 255, 85)), disc(20, 20, 4096, (10, 200, 30), 1),
         segment(0, 36, 52, 36, 1, (200, 10, 10))],
    ]
    return _frames(11, 3, 37, 53), lists


def _case_tiles():
    """2 x 70 x 200: primitives across the tile borders x = 128 and y = 16, 32, 48, 64."""
    lists = [
        [stick(128, 32, 60, 4, 10, (255, 0, 0)), stick(100, 35, 40, 4, 90, (0, 255, 0)),
         disc(128, 16, 16, (0, 0, 255)), disc(127, 47, 40, (255, 255, 0), 1), segment(5, 5, 195, 66, 2, (255, 0, 255)),
         segment(140, 69, 120, 0, 3, (0, 255, 255), 1), stick(160, 48, 30, 16, -30, (170, 255, 255))],
        [stick(100, 35, 150, 4, -160, (85, 255, 0)), disc(199, 69, 25, (255, 255, 255)), disc(0, 0, 25, (1, 1, 1)),
         segment(128, 0, 128, 69, 0, (9, 99, 199)), segment(0, 16, 199, 16, 0, (99, 9, 199), 1),
         stick(64, 64, 70, 2, 45, (255, 170, 0))],
    ]
    return _frames(12, 2, 70, 200), lists


def _case_gap():
    """A frame with an empty list between two drawn ones."""
    lists = [[disc(8, 8, 16, (255, 0, 0)), stick(20, 10, 12, 4, 15, (0, 255, 0))], [],
             [segment(2, 2, 37, 17, 2, (0, 0, 255)), disc(30, 5, 9, (255, 255, 0), 1)]]
    return _frames(13, 3, 20, 40), lists


def _case_many():
    """1 x 6 x 132: 700 primitives, more than one LDS chunk, nearly all on the first tile and
    most of them blended, so any slip in their order shows."""
    rng = np.random.default_rng(14)
    lst = []
    for k in range(700):
        col = tuple(int(v) for v in rng.integers(0, 256, 3))
        x, y = int(rng.integers(-2, 134)), int(rng.integers(-2, 8))
        if k % 3 == 0:
            lst.append(disc(x, y, int(rng.integers(0, 30)), col, int(k % 4 != 0)))
        elif k % 3 == 1:
            lst.append(segment(x, y, x + int(rng.integers(-9, 10)), y + int(rng.integers(-4, 5)),
                               int(rng.integers(0, 4)), col, int(k % 5 != 0)))
        else:
            lst.append(stick(x, y, int(rng.integers(1, 12)), int(rng.integers(1, 4)), int(rng.integers(-180, 181)),
                             col, int(k % 7 != 0)))
    return _frames(14, 1, 6, 132), [lst]


def _case_angles():
    """Stick angles 0, 90, -135, 179 with a = 1 and with a far larger than the frame."""
    lst = []
    for k, ang in enumerate((0, 90, -135, 179)):
        lst.append(stick(6 + 12 * k, 6, 1, 1 + k, ang, (255, 40 * k, 0)))
        lst.append(stick(8 + 11 * k, 20 + 3 * k, 4096, 2, ang, (0, 60 * k, 255)))
    return _frames(15, 1, 37, 53), [lst]


def _case_wide():
    """2 x 40 x 144: 3*W and a frame are multiples of 16 bytes, so from an aligned base every
    run takes the widest accesses; a whole-width tile column beside one of 16 pixels, and below
    two full tile rows one of 8 rows."""
    lists = [
        [stick(70, 20, 60, 4, 12, (255, 0, 0)), stick(127, 30, 20, 6, 80, (0, 255, 0)), disc(128, 16, 30, (0, 0, 255)),
         segment(3, 37, 140, 2, 2, (255, 255, 0), 1), disc(0, 39, 16, (0, 255, 255)), disc(143, 0, 16, (255, 0, 255), 1)],
        [segment(120, 35, 136, 33, 3, (9, 99, 199)), stick(64, 33, 10, 2, -20, (250, 120, 5))],
    ]
    return _frames(16, 2, 40, 144), lists


CASES = {"wide": _case_wide, "odd": _case_odd, "tiles": _case_tiles, "gap": _case_gap, "many": _case_many, "angles": _case_angles}


@functools.lru_cache(maxsize=None)
def case(name):
    """(frames, lists, the frames drawn, the blank canvases drawn); computed once per session and
    shared: treat all four as read-only."""
    frames, lists = CASES[name]()
    want, blank = draw(frames, lists)
    for a in (frames, want, blank):
        a.setflags(write=False)
    return frames, lists, want, blank
