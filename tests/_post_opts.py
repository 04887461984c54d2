"""Test helper of the post-processing options (thre1, thre2, hand_thre, max_people): the
ramped designed maps, the oracle's results on them (computed once per value and shared), and
the person-cap rule stated in numpy."""
import functools

import numpy as np

from islpose import synth
from oracle import cpu_ref

THRE1 = (0.1, 0.2, 0.3, 0.5)
THRE2 = (0.05, 0.4)
RAMP = np.linspace(0.15, 1.0, 41, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def ramped_maps(seed=100):
    """designed_pose_maps(23, 41, 3) with both maps multiplied by a column ramp: the persons'
    peaks and PAF samples get different heights, so every threshold value cuts differently."""
    paf, heat = synth.designed_pose_maps(23, 41, 3, seed=seed)
    return np.ascontiguousarray(paf * RAMP), np.ascontiguousarray(heat * RAMP)


@functools.lru_cache(maxsize=None)
def oracle_maps(case, seed=100):
    """(heatmap_avg, paf_avg, H) of the oracle.  case 'fused': a 184 x 328 frame whose net input
    is the frame (multiplier 1.0); 'unfused': a 368 x 656 frame at multiplier 0.5 (two resizes);
    'large': designed_pose_maps(46, 82, 6) on a 368 x 656 frame at multiplier 1.0."""
    if case == "large":
        paf, heat = synth.designed_pose_maps(46, 82, 6, seed=seed)
        H, W, s = 368, 656, 1.0
    else:
        paf, heat = ramped_maps(seed)
        H, W, s = (184, 328, 0.5) if case == "fused" else (368, 656, 0.5)   # multiplier s * 368 / H
    heat_avg, paf_avg = cpu_ref.body_maps(np.zeros((H, W, 3), np.uint8), lambda im: (paf[None], heat[None]),
                                          "body25", (s,))
    return heat_avg, paf_avg, H


@functools.lru_cache(maxsize=None)
def oracle_peaks(case, thre1, seed=100):
    heat_avg, _, _ = oracle_maps(case, seed)
    return cpu_ref.find_peaks(heat_avg, 26, thre1)


@functools.lru_cache(maxsize=None)
def oracle_body(case, thre1, thre2, seed=100):
    """(candidate, subset, all_peaks, connection_all) of the oracle at (thre1, thre2)."""
    _, paf_avg, H = oracle_maps(case, seed)
    all_peaks = oracle_peaks(case, thre1, seed)
    conns, special_k = cpu_ref.connect_limbs(all_peaks, paf_avg, "body25", H, thre2)
    candidate, subset = cpu_ref.assemble(all_peaks, conns, special_k, "body25")
    return candidate, subset, all_peaks, conns


def counts(res):
    """(peaks, connections, persons) of an oracle_body result."""
    _, subset, all_peaks, conns = res
    return sum(len(p) for p in all_peaks), sum(len(c) for c in conns), len(subset)


def cap_rule(subset, max_people):
    """The max_people rule: a row stays when fewer than max_people rows come before it in the
    order (larger subset[:, -2] first, the lower row first on a tie); survivors in row order."""
    subset = np.asarray(subset)
    if not max_people or len(subset) <= max_people:
        return subset
    score = subset[:, -2]
    keep = []
    for r in range(len(subset)):
        before = sum(1 for j in range(len(subset)) if score[j] > score[r] or (score[j] == score[r] and j < r))
        if before < max_people:
            keep.append(r)
    return subset[keep]
