"""isl_debug_body_post_plan / isl_debug_hand_post_plan, CPU side: declared, exported, ABI version
unchanged, bad arguments rejected, and the plan of well-known geometries and of the A/B
environment switches (host code only: no device is touched)."""
import ctypes
import os
import re

import pytest

from islpose import runtime as rt
from islpose.body import scale_geometry
from islpose.hand import HAND_SCALES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(rt.LIB_PATH), reason="libislpose.so not built")


def _geoms(H, W, scales):
    return [g[1:] for g in scale_geometry(H, W, scales)]


def test_symbols_declared_and_exported():
    text = open(os.path.join(REPO, "include", "islpose.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(isl_\w+)\s*\(", text, re.M))
    new = {"isl_debug_body_post_plan", "isl_debug_hand_post_plan"}
    assert new <= declared and new <= set(rt.EXPORTS)
    assert re.search(r"#define\s+ISL_ABI_VERSION\s+1\b", text)          # additions only
    assert re.search(r"#define\s+ISL_PLAN_SCALES\s+%d\b" % rt.PLAN_SCALES, text)
    for i, name in enumerate(rt.BLUR_BRANCHES):
        assert re.search(r"ISL_BLUR_%s\s*=\s*%d\b" % (name, i), text)
    # the ctypes mirrors: 18 scalars + 8 flags + 2 x 8 resize plans of 6 ints + 2 switches + 4 reserved
    # (the two took reserved slots: the size stands); 2 x 8 + 8 x 6 + 4 + 4
    assert ctypes.sizeof(rt.IslResizePlan) == 24
    assert ctypes.sizeof(rt.IslBodyPostPlan) == 4 * (18 + 8 + 6) + 2 * 8 * 24
    assert ctypes.sizeof(rt.IslHandPostPlan) == 4 * (16 + 4 + 4) + 8 * 24


@needs_lib
def test_bad_arguments():
    L = rt.lib()
    g = (rt.IslScaleGeom * 9)(*[rt.IslScaleGeom(184, 328, 184, 328)] * 9)
    bp, hp = rt.IslBodyPostPlan(), rt.IslHandPostPlan()
    ok = (rt.ISL_BODY25, 1, 368, 656, 1)
    assert L.isl_debug_body_post_plan(*ok, g, ctypes.byref(bp)) == rt.ISL_OK
    for args in ((rt.ISL_HAND, 1, 368, 656, 1), (7, 1, 368, 656, 1), (rt.ISL_BODY25, 0, 368, 656, 1),
                 (rt.ISL_BODY25, 1, 0, 656, 1), (rt.ISL_BODY25, 1, 368, -1, 1), (rt.ISL_BODY25, 1, 368, 656, 0),
                 (rt.ISL_BODY25, 1, 368, 656, 9)):
        assert L.isl_debug_body_post_plan(*args, g, ctypes.byref(bp)) == rt.ISL_E_ARG, args
    assert L.isl_debug_body_post_plan(*ok, None, ctypes.byref(bp)) == rt.ISL_E_ARG
    assert L.isl_debug_body_post_plan(*ok, g, None) == rt.ISL_E_ARG
    assert b"isl_debug_body_post_plan" in L.isl_last_error()
    assert L.isl_debug_hand_post_plan(184, 184, 1, g, ctypes.byref(hp)) == rt.ISL_OK
    for args in ((0, 184, 1), (184, 0, 1), (184, 184, 0), (184, 184, 9)):
        assert L.isl_debug_hand_post_plan(*args, g, ctypes.byref(hp)) == rt.ISL_E_ARG, args
    assert L.isl_debug_hand_post_plan(184, 184, 1, None, ctypes.byref(hp)) == rt.ISL_E_ARG
    assert L.isl_debug_hand_post_plan(184, 184, 1, g, None) == rt.ISL_E_ARG
    for bad in ((0, 328, 184, 328), (184, 7, 184, 328), (184, 328, 0, 328), (184, 328, 184, 0)):
        gb = (rt.IslScaleGeom * 1)(rt.IslScaleGeom(*bad))
        assert L.isl_debug_body_post_plan(*ok, gb, ctypes.byref(bp)) == rt.ISL_E_ARG, bad
        assert L.isl_debug_hand_post_plan(184, 184, 1, gb, ctypes.byref(hp)) == rt.ISL_E_ARG, bad


@needs_lib
def test_body_plans_of_the_known_geometries(monkeypatch):
    for env in ("ISLPOSE_FUSED_BLUR", "ISLPOSE_BLUR_LIST", "ISLPOSE_BLUR_BANDS", "ISLPOSE_RESIZE_SKIP",
                "ISLPOSE_RESIZE_V4", "ISLPOSE_BLUR_EXACT", "ISLPOSE_LIMB_SPLIT", "ISLPOSE_LIMB_Z"):
        monkeypatch.delenv(env, raising=False)
    plan = lambda H, W, scales, n=1, kind=rt.ISL_BODY25: rt.body_post_plan(kind, n, H, W, _geoms(H, W, scales))  # noqa: E731
    # the net input is the frame: one x8 resize inside the blur
    p = plan(184, 328, (0.5,))
    assert (p["multi"], p["two_stage"], p["fused"], p["fuse2"], p["skip2"], p["blur"]) == (0, 0, 1, 0, 0, "FUSED_LIVE")
    assert not p["stage1"][0]["launched"] and not p["final"][0]["launched"]
    assert (p["env_fused_blur"], p["env_blur_list"], p["env_blur_bands"], p["env_resize_skip"], p["env_resize_v4"],
            p["env_blur_exact"], p["env_fused_wide"]) == (1, 1, 1, 1, 1, 0, 0)
    # Mode R at 368 x 656: both stages in the band-maxima V4 form, stage-2 tiles skipped, live list
    p = plan(368, 656, (0.5,))
    assert (p["two_stage"], p["fused"], p["skip2"], p["blur"], p["stage2_ty"]) == (1, 0, 1, "BAND_LIVE", 64)
    want = dict(launched=1, ty=64, cols=128, v4=1, bm=1, identity=0)
    assert p["stage1"][0] == want and p["final"][0] == want
    # 1080p: the stage-2 window fits the blur's LDS window
    p = plan(1080, 1920, (0.5,))
    assert (p["two_stage"], p["fused"], p["fuse2"], p["wide"], p["blur"]) == (1, 1, 1, 0, "FUSED_LIVE")
    assert p["stage1"][0]["launched"] and not p["final"][0]["launched"]
    # QVGA: 46-row stage-2 tiles, no band maxima, the dense grid
    p = plan(240, 320, (0.5,))
    assert (p["skip2"], p["blur"], p["blur_bandmax"]) == (0, "DENSE", 0)
    assert p["final"][0] == dict(launched=1, ty=46, cols=128, v4=0, bm=0, identity=0)
    # two scales: the fp64 average; no separate final resize
    p = plan(240, 328, (0.5, 1.0))
    assert (p["multi"], p["two_stage"], p["fused"], p["blur"], p["acc_ty"]) == (1, 0, 0, "MULTI_F64", 16)
    assert p["scale_two_stage"] == [1, 1] and not any(r["launched"] for r in p["final"])
    # limb scoring: 1024 / (n * limbs) blocks per limb, one kernel from 128 limb slots on
    assert plan(368, 656, (0.5,), n=1)["limb_z"] == 32 and plan(368, 656, (0.5,), n=2)["limb_z"] == 21
    assert plan(368, 656, (0.5,), n=6)["limb_z"] == 1
    assert plan(368, 656, (0.5,), n=1, kind=rt.ISL_COCO)["limb_z"] == 32
    # the switches
    monkeypatch.setenv("ISLPOSE_FUSED_BLUR", "0")
    p = plan(184, 328, (0.5,))
    assert (p["fused"], p["env_fused_blur"], p["blur"]) == (0, 0, "BAND_LIVE") and p["final"][0]["bm"]
    p = plan(1080, 1920, (0.5,))
    assert (p["fuse2"], p["fused"], p["skip2"], p["blur"]) == (1, 0, 0, "BAND_LIVE")     # stage 1 is 327 wide: no V4
    assert p["final"][0] == dict(launched=1, ty=64, cols=128, v4=1, bm=1, identity=0)
    monkeypatch.delenv("ISLPOSE_FUSED_BLUR")
    monkeypatch.setenv("ISLPOSE_RESIZE_V4", "0")
    p = plan(368, 656, (0.5,))
    assert (p["env_resize_v4"], p["skip2"], p["blur"]) == (0, 0, "BAND_LIVE")
    assert p["final"][0] == dict(launched=1, ty=64, cols=128, v4=0, bm=1, identity=0)
    monkeypatch.delenv("ISLPOSE_RESIZE_V4")
    monkeypatch.setenv("ISLPOSE_RESIZE_SKIP", "0")
    p = plan(368, 656, (0.5,))
    assert (p["env_resize_skip"], p["skip2"]) == (0, 0) and p["final"][0]["v4"] and not p["stage1"][0]["bm"]
    monkeypatch.delenv("ISLPOSE_RESIZE_SKIP")
    monkeypatch.setenv("ISLPOSE_BLUR_LIST", "0")
    p = plan(368, 656, (0.5,))
    assert (p["env_blur_list"], p["skip2"], p["blur"], p["blur_bandmax"]) == (0, 0, "DENSE", 1)
    monkeypatch.delenv("ISLPOSE_BLUR_LIST")
    monkeypatch.setenv("ISLPOSE_BLUR_BANDS", "0")
    p = plan(368, 656, (0.5,))
    assert (p["env_blur_bands"], p["skip2"], p["blur"], p["blur_bandmax"], p["final"][0]["bm"]) == (0, 0, "DENSE", 0, 0)
    monkeypatch.delenv("ISLPOSE_BLUR_BANDS")
    for v in ("1", "2"):
        monkeypatch.setenv("ISLPOSE_BLUR_EXACT", v)
        assert plan(368, 656, (0.5,))["env_blur_exact"] == int(v)
    monkeypatch.delenv("ISLPOSE_BLUR_EXACT")
    monkeypatch.setenv("ISLPOSE_LIMB_SPLIT", "0")
    assert plan(368, 656, (0.5,))["limb_z"] == 1
    monkeypatch.delenv("ISLPOSE_LIMB_SPLIT")
    monkeypatch.setenv("ISLPOSE_LIMB_Z", "10")
    assert plan(368, 656, (0.5,))["limb_z"] == 10


@needs_lib
def test_hand_plans_of_the_known_geometries():
    plan = lambda h, w, scales=HAND_SCALES: rt.hand_post_plan(h, w, _geoms(h, w, scales))  # noqa: E731
    p = plan(184, 184)
    assert p["two_stage"] == [0, 1, 1, 1] and p["identity"] == [0, 0, 0, 0] and (p["acc_ty"], p["cc_lds"]) == (9, 1)
    assert not p["stage1"][0]["launched"]
    assert p["stage1"][1] == dict(launched=1, ty=64, cols=128, v4=1, bm=0, identity=0)
    p = plan(256, 256)
    assert (p["acc_ty"], p["cc_lds"], p["cc_rows"], p["cc_chunks"]) == (13, 0, 16, 16)
    assert plan(192, 192)["cc_lds"] == 1 and plan(192, 193)["cc_lds"] == 0          # 36 864 px is the LDS limit
    assert plan(368, 368, (1.0,)) == dict(two_stage=[0], identity=[0], stage1=[dict.fromkeys(p["stage1"][0], 0)],
                                          acc_ty=16, cc_lds=0, cc_rows=11, cc_chunks=34)
    # the 2.0 scale's 736 rows onto a small crop: 36.8 source rows per output row at 20 px
    assert [plan(s, s)["acc_ty"] for s in (20, 21, 22, 23, 42, 43, 64, 736)] == [1, 1, 2, 2, 2, 3, 4, 16]
