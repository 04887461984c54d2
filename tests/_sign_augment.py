"""An independent scalar statement of the window augmentation, for the
tests of csrc/sign_augment.hip and islpose/sign_augment.py: plain Python loops, Python ints for the
hash, Python floats (fp64) for the arithmetic, one value at a time.  It shares no code with the
product's vectorised numpy form.  Also the cases the CPU and GPU tests share.
"""
import math

import numpy as np

M64 = (1 << 64) - 1


def sm(z):
    """splitmix64 finaliser on a Python int."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, step, sample_id):
    return sm(sm(seed ^ step) ^ sample_id)


def draw(kw, site, index):
    return sm(kw ^ (site << 32 | index))


def f32(v):
    """One rounding of a Python float to fp32, as a Python float."""
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def item(cfg, seed, step, sample_id, nrows, row0, base=0):
    """One item as a dict.  cfg: dict(rotation, scale, shift, speed, tshift, frame=(W, H))."""
    kw = key(seed, step, sample_id)
    d = [2.0 * ((draw(kw, 32, j) >> 11) * 2.0 ** -53) - 1.0 for j in range(6)]
    W, H = (float(v) for v in cfg["frame"])
    angle = d[0] * float(cfg["rotation"])
    s = 1.0 + d[1] * float(cfg["scale"])
    tx = (d[2] * float(cfg["shift"])) * W
    ty = (d[3] * float(cfg["shift"])) * H
    q = int(min(32.0, max(8.0, 16.0 + round((d[4] * float(cfg["speed"])) * 16.0))))   # round(): half to even
    start = int(base) + int(round(d[5] * float(cfg["tshift"])))
    c, s_ = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    cx, cy = (W - 1.0) / 2.0, (H - 1.0) / 2.0
    m0, m1, m3, m4 = s * c, -(s * s_), s * s_, s * c
    m2 = (cx + tx) - (m0 * cx + m1 * cy)
    m5 = (cy + ty) - (m3 * cx + m4 * cy)
    return {"row0": int(row0), "nrows": int(nrows), "start": start, "q": q, "reserved": 0, "id": int(sample_id),
            "m": [v + 0.0 for v in (m0, m1, m2, m3, m4, m5)]}


def pairs_of(layout):
    """[(x index, y index)] of a layout's pairs in pair order, and the label indices."""
    nb, ns, nh = layout
    pairs = [(j, nb + j) for j in range(nb)]
    labels = []
    for s in range(ns):
        o = 2 * nb + s * 3 * nh
        pairs += [(o + j, o + nh + j) for j in range(nh)]
        labels += [o + 2 * nh + j for j in range(nh)]
    return pairs, labels


def window(rows, layout, it, T, seed, step, drop, jitter):
    """One output window [T, F] (fp32 numpy) of item `it` (a dict, or a record of the product's
    ITEM_DTYPE) over rows [n_rows, F].  An item that leaves the store gives zeros."""
    rows = np.asarray(rows, np.float32)
    n_rows, F = rows.shape
    row0, nrows, start, q, sid = (int(it[k]) for k in ("row0", "nrows", "start", "q", "id"))
    m = [float(v) for v in it["m"]]
    out = np.zeros((T, F), np.float32)
    if nrows < 1 or q < 8 or q > 32 or row0 < 0 or row0 + nrows > n_rows:
        return out
    kw = key(seed, step, sid)
    thr = int(math.floor(float(np.float32(drop)) * 2.0 ** 24 + 0.5))
    jit = float(np.float32(jitter))
    pairs, labels = pairs_of(layout)
    for t in range(T):
        r = ((2 * t - (T - 1)) * q + 16 * (T - 1) + 16) // 32 + start
        if r < 0 or r >= nrows:
            continue
        if (draw(kw, 16, t) >> 40) < thr:
            continue
        src = rows[row0 + r]
        for e in labels:
            out[t, e] = src[e]
        for p, (ex, ey) in enumerate(pairs):
            x, y = float(src[ex]), float(src[ey])
            if x == 0.0 and y == 0.0:
                continue
            X = (m[0] * x + m[1] * y) + m[2]
            Y = (m[3] * x + m[4] * y) + m[5]
            if jit > 0.0:
                X = X + jit * ((draw(kw, 17, t * 512 + 2 * p) >> 40) * 2.0 ** -23 - 1.0)
                Y = Y + jit * ((draw(kw, 17, t * 512 + 2 * p + 1) >> 40) * 2.0 ** -23 - 1.0)
            X, Y = f32(X), f32(Y)
            if X == 0.0 and Y == 0.0:
                X = 2.0 ** -10
            out[t, ex], out[t, ey] = X, Y
    return out


def windows(rows, layout, items, T, seed, step, drop, jitter):
    return np.stack([window(rows, layout, it, T, seed, step, drop, jitter) for it in items]) if len(items) \
        else np.zeros((0, T, np.shape(rows)[1]), np.float32)


# ------------------------------------------------------------------ the shared cases
def layout_size(layout):
    return 2 * layout[0] + layout[1] * 3 * layout[2]


def make_rows(n_rows, layout, seed, absent=0.25, empty=0.1):
    """Pixel-scale rows: some pairs absent (0, 0), some with one coordinate exactly 0, some rows
    empty; labels 0 / 1."""
    rng = np.random.RandomState(seed)
    F = layout_size(layout)
    rows = rng.uniform(1, 1900, (n_rows, F)).astype(np.float32)
    pairs, labels = pairs_of(layout)
    for ex, ey in pairs:
        gone = rng.rand(n_rows) < absent
        rows[gone, ex] = 0
        rows[gone, ey] = 0
        rows[rng.rand(n_rows) < 0.05, ex] = 0          # x alone 0: still present
    for e in labels:
        rows[:, e] = (rng.rand(n_rows) < 0.5).astype(np.float32)
    rows[rng.rand(n_rows) < empty] = 0
    return rows


def record(it):
    """A dict item -> a tuple in the product's ITEM_DTYPE field order."""
    return (it["row0"], it["nrows"], it["start"], it["q"], it["reserved"], it["id"], tuple(it["m"]))


CFG_REAL = {"rotation": 20.0, "scale": 0.15, "shift": 0.05, "speed": 0.3, "tshift": 4, "frame": (1920, 1080)}
C_LENGTHS = (1, 5, 19, 20, 21, 40, 64)
C_SPEEDS = (8, 13, 16, 20, 32)


def case_a():
    """T 1, F 12, layout (3, 1, 2), one item over a one-row source."""
    layout, T = (3, 1, 2), 1
    rows = make_rows(1, layout, 21, absent=0.2, empty=0.0)
    its = [item(dict(CFG_REAL, speed=0.0, tshift=0), 5, 9, 77, 1, 0)]
    return {"name": "A", "layout": layout, "T": T, "rows": rows, "items": its, "seed": 5, "step": 9,
            "opts": [(0.0, 0.0), (0.0, 1.5)]}


def case_b():
    """T 32, F 256, layout (2, 4, 21): both ABI limits, three items."""
    layout, T = (2, 4, 21), 32
    rows = make_rows(70, layout, 22)
    its = [item(CFG_REAL, 3, 4, 1000 + k, n, r0, b) for k, (n, r0, b) in enumerate(((40, 0, 3), (30, 40, 0), (70, 0, 35)))]
    its[1]["q"], its[2]["q"] = 32, 8
    return {"name": "B", "layout": layout, "T": T, "rows": rows, "items": its, "seed": 3, "step": 4,
            "opts": [(0.0, 0.0), (0.3, 2.5)]}


def case_c():
    """T 20, F 156, 257 items over seven ragged clips; the last clip ends on the store's last row."""
    layout, T = (15, 2, 21), 20
    rows = make_rows(sum(C_LENGTHS), layout, 23)
    first = np.concatenate([[0], np.cumsum(C_LENGTHS)])[:-1]
    its = []
    for k in range(257):
        c = k % len(C_LENGTHS)
        n = C_LENGTHS[c]
        it = item(CFG_REAL, 11, 2, 5000 + 3 * k, n, int(first[c]), 0)
        it["q"] = C_SPEEDS[(k // len(C_LENGTHS)) % len(C_SPEEDS)]
        it["start"] = -25 + (k * 7) % (n + 31)            # -25 ... len + 5
        its.append(it)
    return {"name": "C", "layout": layout, "T": T, "rows": rows, "items": its, "seed": 11, "step": 2,
            "opts": [(0.0, 2.5), (0.3, 0.0), (0.9, 2.5)]}


CASES = {"A": case_a, "B": case_b, "C": case_c}
_expected = {}


def expected(name, drop, jitter):
    """The scalar statement's windows of a case, computed once per (case, drop, jitter)."""
    k = (name, drop, jitter)
    if k not in _expected:
        c = CASES[name]()
        _expected[k] = windows(c["rows"], c["layout"], c["items"], c["T"], c["seed"], c["step"], drop, jitter)
        _expected[k].setflags(write=False)
    return _expected[k]
