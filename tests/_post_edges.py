"""Test helper of the post kernels' edge cases (no GPU needed): builders of maps whose peaks sit
on the frame border and in the resize's scalar-tail column, hand fields sized in crop pixels,
lattices of exactly tied hand components, the case tables with the branch each row is meant to
reach, and the oracle's results on them (computed once per case and shared)."""
import functools

import numpy as np

from islpose import runtime as rt
from islpose import synth
from islpose.body import KINDS, scale_geometry
from islpose.hand import HAND_SCALES
from oracle import cpu_ref

NPARTS = {"body25": 25, "coco": 18}
CN = {"body25": 26, "coco": 19, "hand": 22}          # channels of the interleaved rows OpenCV resizes
LIMBS = {"body25": (synth.BODY25_LIMBS, synth.BODY25_MAPIDX), "coco": (synth.COCO_LIMBS, synth.COCO_MAPIDX)}
RS_MAXR = 40                                          # LDS source rows of the resize kernels (csrc/post.hip)


def tail_parts(W, kind):
    """The parts whose column W - 1 lies in the scalar tail of OpenCV's vertical cubic pass over
    rows of W * cn floats: element (W - 1) * cn + c >= rowlen - rowlen % 4."""
    cn = CN[kind]
    rowlen = W * cn
    return [c for c in range(NPARTS[kind]) if (W - 1) * cn + c >= rowlen - rowlen % 4]


def tail_limb(W, kind):
    """(limb index, part B) of the limb edge_maps lays along the right side: the first limb after
    limbs 0-2 whose part B is a tail part of width W, or whose B is the last part when the width
    has no tail part (body25 at even W: part 24)."""
    want = tail_parts(W, kind) or [NPARTS[kind] - 1]
    for li, (a, b) in enumerate(LIMBS[kind][0]):
        if li >= 3 and b in want:
            return li, b
    raise AssertionError("no limb ends in parts %s" % want)


def _lay_limb(paf, heat, kind, li, a_rc, b_rc):
    """Limb li from low-res pixel a_rc to b_rc (row, col), axis-aligned: single hot end points of
    0.9 (A) and 0.8 (B), the limb's two PAF channels the unit vector over the pixels between."""
    (a, b), (cx, cy) = LIMBS[kind][0][li], LIMBS[kind][1][li]
    heat[a][a_rc] = 0.9
    heat[b][b_rc] = 0.8
    dr, dc = b_rc[0] - a_rc[0], b_rc[1] - a_rc[1]
    assert (dr == 0) != (dc == 0)
    r0, r1 = sorted((a_rc[0], b_rc[0]))
    c0, c1 = sorted((a_rc[1], b_rc[1]))
    paf[cx, r0:r1 + 1, c0:c1 + 1] = np.sign(dc)
    paf[cy, r0:r1 + 1, c0:c1 + 1] = np.sign(dr)


def edge_maps(h8, w8, valid_h, valid_w, kind, seed, W=None):
    """designed_pose_maps(h8, w8, 2, seed, kind) plus four limbs along the four sides of the valid
    area: limb 0 along low-res row 0 and limb 1 along the last valid row (columns 1 to
    min(6, lx)), limb 2 down column 0 and tail_limb(W) down the last valid column (rows 1 to
    min(6, ly)).  W: the frame width the maps are resized to (default: valid_w)."""
    paf, heat = synth.designed_pose_maps(h8, w8, 2, seed, kind)
    paf, heat = paf.copy(), heat.copy()
    ly, lx = (valid_h - 1) // 8, (valid_w - 1) // 8
    cb, rb = min(6, lx), min(6, ly)
    _lay_limb(paf, heat, kind, 0, (0, 1), (0, cb))
    _lay_limb(paf, heat, kind, 1, (ly, 1), (ly, cb))
    _lay_limb(paf, heat, kind, 2, (1, 0), (rb, 0))
    _lay_limb(paf, heat, kind, tail_limb(valid_w if W is None else W, kind)[0], (1, lx), (rb, lx))
    return np.ascontiguousarray(paf), np.ascontiguousarray(heat)


def noise_maps(h8, w8, kind, seed):
    """One designed person plus the threshold noise of test_gpu_blur_filter._heat."""
    rng = np.random.RandomState(seed)
    pl, hl = synth.designed_pose_maps(h8, w8, 1, seed, kind)
    hl = hl + (rng.uniform(0.0, 0.16, hl.shape) * (rng.rand(*hl.shape) < 0.15)).astype(np.float32)
    return np.ascontiguousarray(pl), np.ascontiguousarray(hl)


def hand_geoms(h, w, scales=HAND_SCALES):
    return [g[1:] for g in scale_geometry(h, w, scales)]


HAND_BORDER = {20: "right", 5: "bottom", 9: "left", 13: "top", 17: "corner"}


def hand_field_maps(h, w, seed, scales=HAND_SCALES):
    """Per scale the low-res maps [22, h8, w8] of one continuous field over an h x w crop: every
    part a Gaussian of sigma 2.5 crop px and amplitude 0.4-1.0, sampled where low-res pixel (i, j)
    of the scale lies in the crop, ((j * 8 + 3.5) * w / valid_w, (i * 8 + 3.5) * h / valid_h).
    Parts 20, 5, 9, 13, 17 sit on the right, bottom, left and top border and in the far corner,
    part 0 in the (0, 0) corner, the rest at seeded interior points."""
    rng = np.random.RandomState(seed)
    amp = rng.uniform(0.4, 1.0, 21)
    cx = rng.uniform(0.2, 0.8, 21) * (w - 1)
    cy = rng.uniform(0.2, 0.8, 21) * (h - 1)
    fixed = {20: (w - 1, h / 2), 5: (w / 2, h - 1), 9: (0, h / 3), 13: (w / 3, 0), 17: (w - 1, h - 1), 0: (0, 0)}
    for p, (x, y) in fixed.items():
        cx[p], cy[p] = x, y
    per = []
    for (nh, nw, vh, vw) in hand_geoms(h, w, scales):
        ii, jj = np.mgrid[0:nh // 8, 0:nw // 8].astype(np.float64)
        x, y = (jj * 8 + 3.5) * w / vw, (ii * 8 + 3.5) * h / vh
        m = np.zeros((22, nh // 8, nw // 8), np.float64)
        for p in range(21):
            m[p] = amp[p] * np.exp(-((x - cx[p]) ** 2 + (y - cy[p]) ** 2) / (2 * 2.5 ** 2))
        m[21] = 1.0 - np.clip(m[:21].max(axis=0), 0, 1)
        per.append(m.astype(np.float32))
    return per


BOOST_PART = 11


def lattice_hand_maps(side8, start, step, count, amp):
    """[22, side8, side8]: every part has one hot low-res pixel of `amp` at (start + step * k,
    start + step * l), k, l < count -- count^2 components that are the same numbers, so their
    sums tie exactly and the first label wins; in BOOST_PART the last lattice point holds
    1.5 * amp instead, an outright winner that is not the first label."""
    at = start + step * np.arange(count)
    assert at[-1] + 2 < side8
    m = np.zeros((22, side8, side8), np.float32)
    m[:21][:, at[:, None], at[None, :]] = np.float32(amp)
    m[BOOST_PART, at[-1], at[-1]] = np.float32(1.5 * amp)
    m[21] = 1.0 - m[:21].max(axis=0)
    return m


# ---------------------------------------------------------------------------
# body cases
# ---------------------------------------------------------------------------
# key -> (kind, H, W, scales, blur branch, (peaks on the left / top / right / bottom border, peaks
# of the right-side limb's part B at x = W - 1, connections whose two end points both lie on a
# border)).  The counts are the oracle's on edge_maps (test_post_edges_ref.py holds it to them);
# every case assembles two persons.  They differ where the geometry does: on narrow frames the
# designed persons reach the right side themselves; at 1001 x 999 the x8 stage is blown up 5.4
# times again and the single-pixel end points of the top and left limbs blur below the threshold,
# those of the right limb move off the last column.  Where the width has tail parts (tail_parts)
# the right-side part is one, so its peak at x = W - 1 is computed by the scalar tail.
EDGE_SEED = 7
BODY_CASES = {
    "b120x160": ("body25", 120, 160, (0.5,), "DENSE", (2, 2, 2, 2, 1, 4)),
    "b97x131": ("body25", 97, 131, (0.5,), "DENSE", (2, 2, 2, 2, 1, 4)),
    "b64x48": ("body25", 64, 48, (0.5,), "DENSE", (2, 2, 7, 2, 0, 6)),
    "b185x329": ("body25", 185, 329, (0.5,), "DENSE", (2, 2, 2, 2, 1, 4)),
    "b240x320": ("body25", 240, 320, (0.5,), "DENSE", (2, 2, 2, 2, 1, 4)),
    "b369x657": ("body25", 369, 657, (0.5,), "BAND_LIVE", (2, 2, 2, 2, 1, 4)),
    "b369x657s1": ("body25", 369, 657, (1.0,), "DENSE", (2, 2, 2, 2, 1, 4)),
    "b336x132": ("body25", 336, 132, (0.5,), "BAND_LIVE", (2, 2, 11, 2, 1, 9)),
    "b201x121m2": ("body25", 201, 121, (0.5, 1.0), "MULTI_F64", (3, 3, 6, 3, 2, 5)),
    "b97x131m4": ("body25", 97, 131, (0.5, 1.0, 1.5, 2.0), "MULTI_F64", (3, 3, 2, 3, 1, 4)),
    "b1001x999": ("body25", 1001, 999, (0.5,), "FUSED_LIVE", (0, 0, 3, 7, 0, 2)),
    "c97x133": ("coco", 97, 133, (0.5,), "DENSE", (2, 2, 2, 2, 1, 4)),
    "c150x134": ("coco", 150, 134, (0.5,), "DENSE", (2, 2, 2, 2, 1, 4)),
}
# the oracle takes 4-5 s per frame on these: the CPU-only file leaves their noise frame to the GPU file
SLOW = ("b1001x999", "b97x131m4")


def body_geoms(key):
    kind, H, W, scales, _, _ = BODY_CASES[key]
    return [g[1:] for g in scale_geometry(H, W, scales)]


def body_plan(key, n=2):
    kind, H, W, _, _, _ = BODY_CASES[key]
    return rt.body_post_plan(KINDS[kind], n, H, W, body_geoms(key))


@functools.lru_cache(maxsize=None)
def body_maps(key, frame):
    """Per scale (paf, heat) of frame 0 (the edge maps) or frame 1 (one person and noise)."""
    kind, H, W, scales, _, _ = BODY_CASES[key]
    out = []
    for si, (nh, nw, vh, vw) in enumerate(body_geoms(key)):
        if frame == 0:
            out.append(edge_maps(nh // 8, nw // 8, vh, vw, kind, EDGE_SEED, W=W))
        else:
            out.append(noise_maps(nh // 8, nw // 8, kind, 77 + si))
    for a, b in out:
        a.setflags(write=False)
        b.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def body_oracle(key, frame=0):
    """(candidate, subset, all_peaks, connection_all) of cpu_ref.body_maps + body_post."""
    kind, H, W, scales, _, _ = BODY_CASES[key]
    it = iter([(p[None], h[None]) for p, h in body_maps(key, frame)])
    heat_avg, paf_avg = cpu_ref.body_maps(np.zeros((H, W, 3), np.uint8), lambda im: next(it), kind, scales)
    return cpu_ref.body_post(heat_avg, paf_avg, kind, H)


def body_properties(key, frame=0):
    """What the oracle finds on the case: peaks per border, tail-part peaks at x = W - 1,
    border-to-border connections, persons."""
    kind, H, W, _, _, _ = BODY_CASES[key]
    cand, subset, all_peaks, conns = body_oracle(key, frame)
    flat = [pk for part in all_peaks for pk in part]
    on = lambda pk: pk[0] == 0 or pk[1] == 0 or pk[0] == W - 1 or pk[1] == H - 1  # noqa: E731
    by_id = {pk[3]: pk for pk in flat}
    tails, part_b = tail_parts(W, kind), tail_limb(W, kind)[1]
    rows = [r for c in conns for r in np.asarray(c).reshape(-1, 5)]
    return {"L": int(sum(pk[0] == 0 for pk in flat)), "T": int(sum(pk[1] == 0 for pk in flat)),
            "R": int(sum(pk[0] == W - 1 for pk in flat)), "B": int(sum(pk[1] == H - 1 for pk in flat)),
            "right_b": int(sum(pk[0] == W - 1 for pk in all_peaks[part_b])),
            "tail": int(sum(pk[0] == W - 1 for p in tails for pk in all_peaks[p])),
            "b2b": int(sum(on(by_id[int(r[0])]) and on(by_id[int(r[1])]) for r in rows)),
            "persons": len(subset), "peaks": len(flat)}


# ---------------------------------------------------------------------------
# hand cases
# ---------------------------------------------------------------------------
HAND_SQUARE = (20, 21, 23, 29, 37, 51, 63, 185)      # crops whose field maps give 20 found parts
HAND_RECT = (45, 77)                                 # h x w
HAND_BATCH = (20, 37, 63, 185, 21)                   # one post_crops call


def _hand_result(h, w, per, scales):
    it = iter(per)
    avg = cpu_ref.hand_maps(np.zeros((h, w, 3), np.uint8), lambda im: next(it)[None], scales)
    found = tuple(bool((cpu_ref.gaussian_blur(avg[:, :, p]) > 0.05).any()) for p in range(21))
    peaks = cpu_ref.hand_post(avg)
    scores = np.array([avg[peaks[p, 1], peaks[p, 0], p] if found[p] else 0.0 for p in range(21)], np.float64)
    peaks.setflags(write=False)
    scores.setflags(write=False)
    return peaks, scores, found


@functools.lru_cache(maxsize=None)
def hand_field(h, w):
    per = hand_field_maps(h, w, seed=h * 1000 + w)
    for m in per:
        m.setflags(write=False)
    return tuple(per)


@functools.lru_cache(maxsize=None)
def hand_oracle(h, w):
    """(peaks int64 [21, 2], scores float64 [21], found) of hand_field(h, w), as
    tests/_hand_opts.oracle computes them."""
    return _hand_result(h, w, hand_field(h, w), HAND_SCALES)


# key -> (crop side, scales, start, step, count, amp): 8-px-aligned single-scale lattices
LATTICES = {
    "lat368n81": (368, (1.0,), 3, 5, 9, 0.25),
    "lat368n81hi": (368, (1.0,), 3, 5, 9, 0.5),
    "lat368n4": (368, (1.0,), 3, 5, 2, 0.25),
    "lat368n16": (368, (1.0,), 3, 5, 4, 0.25),
    "lat184n4": (184, (0.5,), 3, 5, 2, 0.25),
    "lat184n16": (184, (0.5,), 3, 5, 4, 0.25),
}


@functools.lru_cache(maxsize=None)
def lattice_maps(key):
    side, scales, start, step, count, amp = LATTICES[key]
    (nh, nw, vh, vw), = hand_geoms(side, side, scales)
    assert (nh, nw, vh, vw) == (side, side, side, side)
    m = lattice_hand_maps(side // 8, start, step, count, amp)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def lattice_oracle(key):
    """(peaks, component sums of part 0 in label order, component count of BOOST_PART)."""
    side, scales, _, _, _, _ = LATTICES[key]
    avg = cpu_ref.hand_maps(np.zeros((side, side, 3), np.uint8), lambda im: lattice_maps(key)[None], scales)
    sums = []
    for p in (0, BOOST_PART):
        lab, n = cpu_ref.label8(np.ascontiguousarray(cpu_ref.gaussian_blur(avg[:, :, p]) > 0.05, dtype=np.uint8))
        sums.append([np.sum(avg[:, :, p][lab == i]) for i in range(1, n + 1)])
    peaks = cpu_ref.hand_post(avg)
    peaks.setflags(write=False)
    return peaks, sums[0], sums[1]


# ---------------------------------------------------------------------------
# the host's tile sizing, restated
# ---------------------------------------------------------------------------
def tap_first(d, scale):
    """taps() of csrc/post.hip for an array of output indices d: the floor of the float32 value
    of (d + 0.5) * scale - 0.5 (computed in fp64, as the kernels do); the four source indices
    are this - 1 ... + 2, clamped to the source."""
    return np.floor(((np.asarray(d, np.float64) + 0.5) * scale - 0.5).astype(np.float32)).astype(np.int64)


def max_window(oh, src_h, ty, scale=None):
    """The most source rows any tile of ty output rows needs in a resize of src_h rows onto oh
    rows (scale as the host passes it: 1 / (oh / src_h) unless given): hi[3] - lo[0] + 1 of the
    tile's first and last row.  The kernels trap above RS_MAXR."""
    if scale is None:
        scale = 1.0 / (float(oh) / src_h)
    y0 = np.arange(0, oh, ty)
    y1 = np.minimum(y0 + ty, oh) - 1
    lo = np.clip(tap_first(y0, scale) - 1, 0, src_h - 1)
    hi = np.clip(tap_first(y1, scale) + 2, 0, src_h - 1)
    return int((hi - lo + 1).max())
