"""Designed inputs and the oracle's peaks and scores for the hand-option tests (no GPU needed)."""
import functools

import numpy as np

from islpose import synth
from islpose.body import scale_geometry
from islpose.hand import HAND_SCALES
from oracle import cpu_ref

# low-res blob positions of the tie input, in cells of the 0.5 scale's 23 x 23 map: 8 apart
TIE_PART = 9
TIE_AT = [(3, 7), (11, 7), (19, 7), (3, 15), (11, 15), (19, 15)]     # (x, y)


def geoms_of(h, w, scales=HAND_SCALES):
    return [g[1:] for g in scale_geometry(h, w, scales)]


def edit(m):
    """The two designed edits: part 3 nowhere, part 5 a lone peak in the map's corner cell."""
    m = m.copy()
    m[3] = 0
    m[5] = 0
    m[5, 0, 0], m[5, 0, 1], m[5, 1, 0] = 0.9, 0.5, 0.5
    return m


@functools.lru_cache(maxsize=None)
def designed(h, w, n=3, kind="blobs"):
    """Per scale the low-res maps [n, 22, h8, w8] of n crops of h x w: test_gpu_hand.py's designed
    batch ('blobs'), its dense maps ('dense'), or the blobs with part TIE_PART replaced by six
    identical blobs a multiple of 8 cells apart ('tie': for a crop whose size divides every
    scale's net size the six components are the same numbers, so their sums tie exactly)."""
    rng = np.random.RandomState(h + w)
    per = []
    for k, (nh, nw, vh, vw) in enumerate(geoms_of(h, w)):
        if kind == "dense":
            maps = [rng.uniform(0.02, 1.0, (22, nh // 8, nw // 8)).astype(np.float32) for _ in range(n)]
        else:
            maps = [synth.designed_hand_maps(nh // 8, nw // 8, seed=7 * i + nh, n_blobs=3) for i in range(n)]
        maps = [edit(m) for m in maps]
        if kind == "tie":
            f = k + 1                                    # cells of this scale per cell of the 0.5 scale
            yy, xx = np.mgrid[-2 * f:2 * f + 1, -2 * f:2 * f + 1].astype(np.float64)
            blob = (0.8 * np.exp(-(xx * xx + yy * yy) / (2.0 * (0.7 * f) ** 2))).astype(np.float32)
            for m in maps:
                m[TIE_PART] = 0
                for (x, y) in TIE_AT:
                    m[TIE_PART, y * f - 2 * f:y * f + 2 * f + 1, x * f - 2 * f:x * f + 2 * f + 1] = blob
        per.append(np.stack(maps))
    return per


@functools.lru_cache(maxsize=None)
def oracle(h, w, n=3, kind="blobs", i=0):
    """(peaks int64 [21, 2], scores float64 [21]) of crop i of designed(h, w, n, kind): the
    oracle's post, the score read from the heatmap_avg that hand_post masked in place
    (hand.py:70) at the returned pixel, 0.0 where the thresholded map is empty (hand.py:63)."""
    per = designed(h, w, n, kind)
    it = iter([p[i] for p in per])
    avg = cpu_ref.hand_maps(np.zeros((h, w, 3), np.uint8), lambda im: next(it)[None])
    found = [bool((cpu_ref.gaussian_blur(avg[:, :, p]) > 0.05).any()) for p in range(21)]
    peaks = cpu_ref.hand_post(avg)
    scores = np.array([avg[peaks[p, 1], peaks[p, 0], p] if found[p] else 0.0 for p in range(21)], np.float64)
    peaks.setflags(write=False)
    scores.setflags(write=False)
    return peaks, scores, tuple(found)


def mirrored(peaks, scores_or_found, w):
    """The peaks a mirrored crop reports: x -> w - 1 - x where the part was found."""
    out = np.array(peaks)
    f = np.asarray(scores_or_found) != 0
    out[f, 0] = w - 1 - out[f, 0]
    return out
