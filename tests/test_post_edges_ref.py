"""The inputs and case tables of tests/test_gpu_post_edges.py, on the CPU: the oracle shows the
properties each row claims (peaks on the borders, a peak in the resize's scalar-tail column,
border-to-border connections, exactly tied hand components), the host plan
(isl_debug_*_post_plan) says every case reaches the branch its row names and the tables cover
every branch, and the host's tile sizing keeps every resize tile inside the kernels' LDS window
over the whole range of frame and crop sizes."""
import os

import numpy as np
import pytest

import _post_edges as pe
from islpose import runtime as rt
from islpose.body import KINDS, scale_geometry
from islpose.hand import HAND_SCALES

needs_lib = pytest.mark.skipif(not os.path.exists(rt.LIB_PATH), reason="libislpose.so not built")
ENVS = ("ISLPOSE_FUSED_BLUR", "ISLPOSE_BLUR_LIST", "ISLPOSE_BLUR_BANDS", "ISLPOSE_RESIZE_SKIP", "ISLPOSE_RESIZE_V4",
        "ISLPOSE_BLUR_EXACT")


@pytest.fixture
def default_env(monkeypatch):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)


def test_tail_parts_are_computed():
    """body25 (26 channels): part 24 at odd widths only; COCO (19): by W % 4."""
    assert pe.tail_parts(656, "body25") == [] and pe.tail_parts(657, "body25") == [24]
    assert [pe.tail_parts(W, "coco") for W in (132, 133, 134, 135)] == [[], [16, 17], [17], []]
    assert pe.tail_limb(657, "body25") == (18, 24) and pe.tail_limb(656, "body25") == (18, 24)
    assert pe.tail_limb(133, "coco") == (14, 16) and pe.tail_limb(134, "coco") == (16, 17)


@pytest.mark.parametrize("key", sorted(pe.BODY_CASES))
def test_body_case_properties(key):
    kind, H, W, scales, _, want = pe.BODY_CASES[key]
    got = pe.body_properties(key)
    print("%s: %s" % (key, got))
    assert (got["L"], got["T"], got["R"], got["B"], got["right_b"], got["b2b"]) == want
    assert got["persons"] == 2
    # the right-side peak is a scalar-tail element wherever the width has tail parts
    if pe.tail_parts(W, kind):
        assert got["tail"] == got["right_b"]
    noise = pe.body_oracle(key, 1) if key not in pe.SLOW else None
    if noise is not None:
        assert len(noise[0]) > 0 and len(noise[1]) >= 1


def test_every_body_property_in_three_cases():
    rows = list(pe.BODY_CASES.values())
    for i, name in enumerate(("L", "T", "R", "B", "right_b", "b2b")):
        assert sum(r[5][i] >= 1 for r in rows) >= 3, name
    tail = [k for k, r in pe.BODY_CASES.items() if pe.tail_parts(r[2], r[0]) and r[5][4] >= 1]
    assert len(tail) >= 3 and any(k.startswith("c") for k in tail), tail


@pytest.mark.parametrize("hw", [(s, s) for s in pe.HAND_SQUARE] + [pe.HAND_RECT])
def test_hand_field_properties(hw):
    h, w = hw
    pk, sc, found = pe.hand_oracle(h, w)
    on = [p for p in range(21) if found[p] and (pk[p, 0] in (0, w - 1) or pk[p, 1] in (0, h - 1))]
    print("%dx%d: %d parts found, on a border: %s" % (h, w, sum(found), on))
    assert sum(found) >= 20 and all(sc[p] > 0.05 for p in range(21) if found[p])
    if h == w:
        assert pk[20, 0] == w - 1 and pk[5, 1] == h - 1 and pk[9, 0] == 0 and pk[13, 1] == 0
        assert tuple(pk[17]) == (w - 1, h - 1) and all(found[p] for p in pe.HAND_BORDER)
    else:
        assert len(on) >= 4


@pytest.mark.parametrize("key", sorted(pe.LATTICES))
def test_lattice_components_tie_exactly(key):
    side, scales, start, step, count, amp = pe.LATTICES[key]
    peaks, sums, boost = pe.lattice_oracle(key)
    assert len(sums) == count * count == len(boost)
    assert len({np.float64(s).tobytes() for s in sums}) == 1            # bitwise equal: np.argmax takes label 1
    first = start * 8 + 3
    last = (start + step * (count - 1)) * 8 + 3
    for p in range(21):
        assert list(peaks[p]) == ([last, last] if p == pe.BOOST_PART else [first, first]), p
    assert int(np.argmax(boost)) != 0 and sorted(boost)[-1] > sorted(boost)[-2]


@needs_lib
def test_body_plans_reach_the_named_branches(default_env):
    plans = {k: pe.body_plan(k) for k in pe.BODY_CASES}
    for k, (kind, H, W, scales, branch, _) in pe.BODY_CASES.items():
        p = plans[k]
        assert p["blur"] == branch, (k, p)
        assert p["multi"] == (len(scales) > 1) and all(p["scale_two_stage"])
    assert {p["blur"] for p in plans.values()} == set(rt.BLUR_BRANCHES)
    # the resize forms by case: no band maxima below 64-row stage-2 tiles, hence the dense grid
    for k in ("b120x160", "b97x131", "b64x48", "b185x329", "b240x320", "b369x657s1", "c97x133", "c150x134"):
        f = plans[k]["final"][0]
        assert f["launched"] and f["ty"] % 16 and (f["v4"], f["bm"], f["cols"]) == (0, 0, 128), (k, f)
        assert not plans[k]["blur_bandmax"] and not plans[k]["skip2"]
    p = plans["b369x657"]                       # odd width: band maxima without V4, no skipped tiles
    assert p["final"][0] == dict(launched=1, ty=64, cols=128, v4=0, bm=1, identity=0)
    assert p["stage1"][0] == dict(launched=1, ty=64, cols=128, v4=1, bm=0, identity=0) and not p["skip2"]
    p = plans["b336x132"]                       # both stages in the band-maxima V4 form
    assert p["skip2"] and p["stage1"][0]["bm"] and p["stage1"][0]["v4"] and p["final"][0]["bm"] and p["final"][0]["v4"]
    p = plans["b1001x999"]
    assert (p["fused"], p["fuse2"], p["wide"]) == (1, 1, 0) and not p["final"][0]["launched"]
    every = [r for p in plans.values() for r in p["stage1"] + p["final"] if r["launched"]]
    for field in ("v4", "bm"):
        assert {r[field] for r in every} == {0, 1}, field
    assert {p["skip2"] for p in plans.values()} == {0, 1} and any(p["fuse2"] for p in plans.values())
    assert not any(r["identity"] for r in every) and {r["cols"] for r in every} == {128}   # 256 never pads less
    acc = sorted(p["acc_ty"] for p in plans.values() if p["multi"])
    assert acc[0] < 16 and acc[-1] == 16, acc
    print({k: (p["blur"], p["acc_ty"], [r["ty"] for r in p["final"]]) for k, p in plans.items()})


@needs_lib
def test_hand_plans_cover_the_tile_heights_and_both_component_paths():
    acc = {s: rt.hand_post_plan(s, s, pe.hand_geoms(s, s))["acc_ty"] for s in pe.HAND_SQUARE}
    print(acc)
    assert {1, 2, 3} <= set(acc.values()) and max(acc.values()) >= 4
    assert acc[20] == 1 and acc[185] >= 4
    lds = {}
    for k, (side, scales, _, _, count, _) in pe.LATTICES.items():
        p = rt.hand_post_plan(side, side, pe.hand_geoms(side, side, scales))
        assert p["two_stage"] == [0] and p["acc_ty"] == 16
        lds.setdefault(p["cc_lds"], set()).add(count * count)
    # candidates: <= 4 the fast finish, <= 64 the sorted list, more the all-roots loop.  More than
    # 64 exact ties do not fit an LDS plane (<= 36 864 px) with blobs that do not interact
    assert lds == {0: {4, 16, 81}, 1: {4, 16}}
    for s in pe.HAND_SQUARE + (45,):
        assert rt.hand_post_plan(s, s, pe.hand_geoms(s, s))["cc_lds"] == 1
    p = rt.hand_post_plan(*pe.HAND_RECT, pe.hand_geoms(*pe.HAND_RECT))
    assert p["cc_lds"] == 1 and not any(r["v4"] for r in p["stage1"])           # odd valid widths


def _rows_fit(plan_rs, oh, src_h, scale=None):
    return pe.max_window(oh, src_h, plan_rs["ty"], scale) <= pe.RS_MAXR


@needs_lib
def test_host_sizing_keeps_every_tile_in_the_window(default_env):
    """The resize kernels trap when a tile needs more than 40 source rows; the host sizes the rows
    per tile so that none does.  Every frame height 16..2200 at the default and the pyramid scales
    and every square hand crop 20..736: the window of every tile of every launched resize, from
    the row-index rule restated in numpy, at the plan's rows per tile."""
    for H in range(16, 2201):
        W = (H * 16 + 8) // 9
        for scales in ((0.5,), (0.5, 1.0, 1.5, 2.0)):
            geoms = [g[1:] for g in scale_geometry(H, W, scales)]
            p = rt.body_post_plan(KINDS["body25"], 1, H, W, geoms)
            for si, (nh, nw, vh, vw) in enumerate(geoms):
                if p["stage1"][si]["launched"]:
                    assert _rows_fit(p["stage1"][si], vh, nh // 8, 1.0 / 8.0), (H, scales, si)
                src = vh if p["scale_two_stage"][si] else nh // 8
                sc = None if p["scale_two_stage"][si] else 1.0 / 8.0
                if p["final"][si]["launched"]:
                    assert _rows_fit(p["final"][si], H, src, sc), (H, scales, si)
                if p["multi"]:
                    assert 1 <= p["acc_ty"] <= 16 and pe.max_window(H, src, p["acc_ty"], sc) <= pe.RS_MAXR, (H, si)
    for s in range(20, 737):
        geoms = pe.hand_geoms(s, s, HAND_SCALES)
        p = rt.hand_post_plan(s, s, geoms)
        assert 1 <= p["acc_ty"] <= 16
        for si, (nh, nw, vh, vw) in enumerate(geoms):
            if p["two_stage"][si]:
                assert _rows_fit(p["stage1"][si], vh, nh // 8, 1.0 / 8.0), (s, si)
                assert pe.max_window(s, vh, p["acc_ty"]) <= pe.RS_MAXR, (s, si)
            else:
                assert pe.max_window(s, nh // 8, p["acc_ty"], 1.0 / 8.0) <= pe.RS_MAXR, (s, si)
