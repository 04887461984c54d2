"""The run-time post-processing options (thre1, thre2, hand_thre, max_people), CPU side: the
validation at every constructor, the CPU path against the oracle at non-default values, the
person-cap helper against the rule stated in numpy, and ISLSignPos.state_key()."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _post_opts as po
from islpose import cpu
from islpose import runtime as rt
from islpose import synth
from oracle import cpu_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
# (constructor keywords by role) -> rejected values
BAD = [("thre1", 0), ("thre1", -1), ("thre1", NAN), ("hand_thre", 0), ("thre2", INF), ("max_people", -1)]


def _torch_weights(kind):
    return {k: torch.from_numpy(v) for k, v in synth.synth_weights(kind).items()}


def test_symbols_declared_and_exported():
    text = open(os.path.join(REPO, "include", "islpose.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(isl_\w+)\s*\(", text, re.M))
    new = {"isl_post_opts_default", "isl_body_post_opts", "isl_hand_post_opts", "isl_hand_post_crops_opts"}
    assert new <= declared and new <= set(rt.EXPORTS)
    assert re.search(r"#define\s+ISL_ABI_VERSION\s+1\b", text)          # additions only
    if os.path.exists(rt.LIB_PATH):
        o = rt.IslPostOpts(1.0, 1.0, 1.0, 5, (1, 2, 3))
        assert rt.lib().isl_post_opts_default(ctypes.byref(o)) == rt.ISL_OK
        assert (o.thre1, o.thre2, o.hand_thre, o.max_people, list(o.reserved)) == (0.1, 0.05, 0.05, 0, [0, 0, 0])
        assert rt.lib().isl_post_opts_default(None) == rt.ISL_E_ARG


def test_check_post_opts():
    assert rt.check_post_opts() == {"thre1": 0.1, "thre2": 0.05, "hand_thre": 0.05, "max_people": 0}
    assert rt.check_post_opts(None, None, None, None) == rt.check_post_opts()
    assert rt.check_post_opts(0.1, 0.05, 0.05, 0) == rt.check_post_opts()
    got = rt.check_post_opts(thre1=0.3, thre2=-0.2, hand_thre=0.01, max_people=2)
    assert got == {"thre1": 0.3, "thre2": -0.2, "hand_thre": 0.01, "max_people": 2}
    for name, v in BAD + [("thre1", INF), ("hand_thre", -1), ("hand_thre", NAN), ("thre2", NAN), ("max_people", 1.5),
                          ("thre1", 1e-40), ("hand_thre", 1e31)]:
        with pytest.raises(ValueError):
            rt.check_post_opts(**{name: v})


def test_c_entry_points_reject_bad_options():
    """ISL_E_ARG for an isl_post_opts outside the accepted ranges, before any device work."""
    if not os.path.exists(rt.LIB_PATH):
        pytest.skip("libislpose.so not built")
    L, vp = rt.lib(), ctypes.c_void_p
    body, hand = rt.Net(rt.ISL_BODY25), rt.Net(rt.ISL_HAND)      # isl_net_create does not touch the device
    g = (rt.IslScaleGeom * 1)(rt.IslScaleGeom(184, 184, 184, 184))
    hp = (vp * 1)(vp(16))
    caps = rt.IslCaps(16, 64, 16, 8)
    ws = (ctypes.c_int32 * 1)(100)
    for name, v in BAD:
        o = rt.post_opts_struct(rt.check_post_opts())
        setattr(o, name, v)
        if name != "hand_thre":
            assert L.isl_body_post_opts(body.h, 1, 184, 184, 1, g, hp, hp, ctypes.byref(caps), vp(16), None,
                                        ctypes.byref(o)) == rt.ISL_E_ARG, (name, v)
        assert L.isl_hand_post_opts(hand.h, 1, 184, 184, 1, g, hp, vp(16), None, ctypes.byref(o)) == rt.ISL_E_ARG
        assert L.isl_hand_post_crops_opts(hand.h, 1, ws, 1, g, hp, vp(16), None, ctypes.byref(o)) == rt.ISL_E_ARG


def test_constructors_validate():
    """ValueError at construction, GPU or not (before the feature: TypeError, no such keyword);
    None and the reference's constants are accepted."""
    from islpose.body import BodyEstimator
    from islpose.hand import HandEstimator
    from src.ISL_Model_parameter import ISLSignPos, ISLSignPosTranslator
    from src.body import Body
    from src.hand import Hand
    wb, wh = _torch_weights(0), _torch_weights(2)
    body, hand = Body(wb, "body25"), Hand(wh)
    for name, v in BAD:
        with pytest.raises(ValueError):
            ISLSignPos(body.model, hand.model, **{name: v})
        with pytest.raises(ValueError):
            ISLSignPosTranslator(body.model, hand.model, None, **{name: v})
        if name == "hand_thre":
            with pytest.raises(ValueError):
                Hand(wh, thre=v)
            with pytest.raises(ValueError):
                HandEstimator(thre=v)
        else:
            with pytest.raises(ValueError):
                Body(wb, "body25", **{name: v})
            with pytest.raises(ValueError):
                BodyEstimator(**{name: v})
    with pytest.raises(TypeError):          # keyword only
        ISLSignPos(body.model, hand.model, 0.2)
    b = Body(wb, "body25", thre1=0.1, thre2=0.05, max_people=0)
    assert (b.thre1, b.thre2, b.max_people) == (0.1, 0.05, 0)
    assert Body(wb, "body25", thre1=None, thre2=None, max_people=None).max_people is None
    assert Hand(wh, thre=0.05).thre == 0.05 and Hand(wh, thre=None).thre is None
    isl = ISLSignPos(body.model, hand.model, thre1=None, thre2=None, hand_thre=None, max_people=None)
    assert isl.post_opts == rt.check_post_opts()
    assert ISLSignPos(body.model, hand.model, max_people=1, hand_thre=0.2).post_opts["max_people"] == 1
    if os.path.exists(rt.LIB_PATH):         # the estimators on nets that exist (no device touched)
        be = BodyEstimator(net=rt.Net(rt.ISL_BODY25), thre1=0.25, max_people=1)
        assert be.post_opts == dict(rt.check_post_opts(), thre1=0.25, max_people=1)
        assert BodyEstimator(net=rt.Net(rt.ISL_BODY25)).post_opts == rt.check_post_opts()
        assert HandEstimator(net=rt.Net(rt.ISL_HAND), thre=0.2).post_opts["hand_thre"] == 0.2


def test_cpu_path_follows_thresholds_like_the_oracle():
    """islpose.cpu on the ramped designed maps (net output of a 184 x 328 frame at multiplier 1.0)
    == the oracle's find_peaks / connect_limbs / assemble at the same (thre1, thre2), exactly.
    First the oracle's own counts: strictly fewer peaks at every larger thre1, fewer connections
    and persons at the larger thre2 -- an implementation that ignores an option cannot pass."""
    peaks = [po.counts(po.oracle_body("fused", t1, 0.05))[0] for t1 in po.THRE1]
    print("oracle peaks at thre1 %s: %s" % (po.THRE1, peaks))
    assert all(a > b > 0 for a, b in zip(peaks, peaks[1:])), peaks
    lo, hi = (po.counts(po.oracle_body("fused", 0.1, t2)) for t2 in po.THRE2)
    print("oracle (peaks, connections, persons) at thre2 %s: %s %s" % (po.THRE2, lo, hi))
    assert lo[1] > hi[1] > 0 and lo[2] > hi[2] > 0, (lo, hi)
    paf, heat = po.ramped_maps()
    frame = np.zeros((184, 328, 3), np.uint8)
    for t1 in po.THRE1:
        for t2 in po.THRE2:
            cand, subset = cpu.body_call(frame, lambda im: (paf[None], heat[None]), "body25", (0.5,), thre1=t1, thre2=t2)
            rc, rs, _, _ = po.oracle_body("fused", t1, t2)
            assert np.array_equal(cand, rc) and np.array_equal(subset, rs), (t1, t2)
    # the defaults are the reference's constants
    cand, subset = cpu.body_call(frame, lambda im: (paf[None], heat[None]), "body25", (0.5,))
    rc, rs, _, _ = po.oracle_body("fused", 0.1, 0.05)
    assert np.array_equal(cand, rc) and np.array_equal(subset, rs)
    # the cap on the CPU seam: candidate unchanged, subset by the rule
    cand, subset = cpu.body_call(frame, lambda im: (paf[None], heat[None]), "body25", (0.5,), max_people=1)
    assert np.array_equal(cand, rc) and np.array_equal(subset, po.cap_rule(rs, 1)) and len(subset) == 1 < len(rs)


def test_cpu_hand_threshold_like_the_oracle():
    """cpu.hand_call(thre=) == cpu_ref.hand_post(heatmap_avg, thre) on designed hand maps with
    some planes scaled down: at least one part is [0, 0] at 0.2 and found at 0.02."""
    maps = synth.designed_hand_maps(23, 23, seed=7).copy()
    maps[::3] *= 0.15
    crop = np.zeros((184, 184, 3), np.uint8)
    heat_avg = cpu_ref.hand_maps(crop, lambda im: maps[None], (0.5,))
    ref = {t: cpu_ref.hand_post(heat_avg.copy(), t) for t in (0.02, 0.05, 0.2)}
    gone = [(ref[0.2][p] == 0).all() and (ref[0.02][p] != 0).any() for p in range(21)]
    assert any(gone), (ref[0.02], ref[0.2])
    for t in (0.02, 0.05, 0.2):
        got = cpu.hand_call(crop, lambda im: maps[None], scale_search=(0.5,), thre=t)
        assert np.array_equal(got, ref[t]), t
    assert np.array_equal(cpu.hand_call(crop, lambda im: maps[None], scale_search=(0.5,)), ref[0.05])


def test_cap_helper_against_the_rule():
    rng = np.random.RandomState(3)
    subset = -np.ones((7, 27))
    subset[:, -2] = [5.0, 9.0, 9.0, 2.0, 9.0, 7.0, 5.0]         # ties at 9 (rows 1, 2, 4) and 5 (0, 6)
    subset[:, -1] = 4
    subset[:, :5] = rng.randint(0, 50, (7, 5))
    for k in range(0, 10):
        got = cpu.cap_people(subset, k)
        assert np.array_equal(got, po.cap_rule(subset, k)), k
        assert len(got) == (7 if k == 0 else min(k, 7))
    assert np.array_equal(cpu.cap_people(subset, 2), subset[[1, 2]])          # the lower rows of the tie
    assert np.array_equal(cpu.cap_people(subset, 4), subset[[1, 2, 4, 5]])    # original order
    assert np.array_equal(cpu.cap_people(subset, 5), subset[[0, 1, 2, 4, 5]])
    assert cpu.cap_people(subset, 8) is subset and cpu.cap_people(subset, None) is subset
    empty = -np.ones((0, 27))
    for k in (None, 0, 1, 3):
        assert cpu.cap_people(empty, k).shape == (0, 27)
        assert po.cap_rule(empty, k).shape == (0, 27)


def test_state_key_follows_each_option():
    """ISLSignPos.state_key() differs between instances that differ in one option only, so the
    translator's cached feature rows are dropped when an option changes (no device needed)."""
    from src.ISL_Model_parameter import ISLSignPos
    from src.body import Body
    from src.hand import Hand
    body, hand = Body(_torch_weights(0), "body25"), Hand(_torch_weights(2))
    k0 = ISLSignPos(body.model, hand.model).state_key()
    assert ISLSignPos(body.model, hand.model).state_key() == k0
    assert ISLSignPos(body.model, hand.model, thre1=0.1, thre2=0.05, hand_thre=0.05, max_people=0).state_key() == k0
    keys = {k0}
    for kw in (dict(thre1=0.2), dict(thre2=0.4), dict(hand_thre=0.02), dict(max_people=1), dict(max_people=2)):
        keys.add(ISLSignPos(body.model, hand.model, **kw).state_key())
    assert len(keys) == 6
