"""The run-time post-processing options on the HIP path: the defaults are the old bits through
the old and the new entry points; thre1 / thre2 / hand_thre against the oracle called with the
same values, bit for bit, on every post path; the person cap against the rule stated in numpy;
the options at the frame seam (ISLSignPos) and through the capacity re-run."""
import ctypes

import numpy as np
import pytest
import torch

import _post_opts as po
import _tame
from islpose import runtime as rt
from islpose import synth
from islpose.body import BodyEstimator, scale_geometry
from islpose.hand import HAND_SCALES, HandEstimator
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

# post path -> (H, W, geometry): the net input is the frame (one x8 resize, fused with the blur),
# or a 368 x 656 frame at multiplier 0.5 (two resizes, materialised planes); 23 x 41 maps both
PATHS = {"fused": (184, 328, (184, 328, 184, 328)), "unfused": (368, 656, (184, 328, 184, 328))}


@pytest.fixture(scope="module")
def net25():
    n = rt.Net(rt.ISL_BODY25)
    n.load_weights(synth.synth_weights(0))
    return n


@pytest.fixture(scope="module")
def nethand():
    n = rt.Net(rt.ISL_HAND)
    n.load_weights(synth.synth_weights(2))
    return n


def _cuda_maps(seeds):
    ms = [po.ramped_maps(s) for s in seeds]
    return ([torch.from_numpy(np.stack([m[0] for m in ms])).cuda()],
            [torch.from_numpy(np.stack([m[1] for m in ms])).cuda()])


def _assert_frame(got, ref, what):
    cand, subset, _, conns = ref
    assert np.array_equal(got.candidate, cand), what
    assert np.array_equal(got.subset, subset), what
    for a, b in zip(got.connection_all, conns):
        assert np.array_equal(np.asarray(a).reshape(-1, 5), np.asarray(b).reshape(-1, 5)), what


def test_geometry_of_the_two_paths():
    assert [g[1:] for g in scale_geometry(184, 328, (0.5,))] == [PATHS["fused"][2]]
    assert [g[1:] for g in scale_geometry(368, 656, (0.5,))] == [PATHS["unfused"][2]]


@pytest.mark.parametrize("path", sorted(PATHS))
def test_body_defaults_are_the_old_bits(net25, path):
    """isl_body_post, isl_body_post_opts(NULL) and isl_body_post_opts(explicit defaults): the
    same record bytes (records zeroed first: the slots past the counts are never written)."""
    H, W, geom = PATHS[path]
    est = BodyEstimator(net=net25)
    pafs, heats = _cuda_maps((100, 101))
    L, n = rt.lib(), 2
    c = rt.IslCaps(**est.caps)
    lay = rt.body_layout(est.kind, c)
    g = (rt.IslScaleGeom * 1)(rt.IslScaleGeom(*geom))
    pp = (ctypes.c_void_p * 1)(rt.ptr(pafs[0]).value)
    hp = (ctypes.c_void_p * 1)(rt.ptr(heats[0]).value)
    dflt = rt.IslPostOpts()
    rt.check(L.isl_post_opts_default(ctypes.byref(dflt)))
    recs = []
    for fn, extra in ((L.isl_body_post, ()), (L.isl_body_post_opts, (None,)),
                      (L.isl_body_post_opts, (ctypes.byref(dflt),)),
                      (L.isl_body_post_opts, (ctypes.byref(est._po),))):
        res = torch.zeros(n * lay.record_bytes, dtype=torch.uint8, device="cuda")
        rt.check(fn(net25.h, n, H, W, 1, g, pp, hp, ctypes.byref(c), rt.ptr(res), rt.stream_handle(), *extra))
        recs.append(res.cpu().numpy())
    for r in recs[1:]:
        assert np.array_equal(recs[0], r)
    frames = est.decode(recs[0], lay, est.caps, n)
    for i, seed in enumerate((100, 101)):
        _assert_frame(frames[i], po.oracle_body(path, 0.1, 0.05, seed), (path, seed))


def test_hand_defaults_are_the_old_bits(nethand):
    L = rt.lib()
    heat = torch.from_numpy(synth.designed_hand_maps(23, 23, seed=7)[None]).cuda()
    g = (rt.IslScaleGeom * 1)(rt.IslScaleGeom(184, 184, 184, 184))
    hp = (ctypes.c_void_p * 1)(rt.ptr(heat).value)
    ws = (ctypes.c_int32 * 1)(184)
    dflt = rt.IslPostOpts()
    rt.check(L.isl_post_opts_default(ctypes.byref(dflt)))
    outs = []
    for extra in ((), (None,), (ctypes.byref(dflt),)):
        for crops in (False, True):
            out = torch.zeros((1, 21, 2), dtype=torch.int64, device="cuda")
            if crops:
                fn = L.isl_hand_post_crops_opts if extra else L.isl_hand_post_crops
                rt.check(fn(nethand.h, 1, ws, 1, g, hp, rt.ptr(out), rt.stream_handle(), *extra))
            else:
                fn = L.isl_hand_post_opts if extra else L.isl_hand_post
                rt.check(fn(nethand.h, 1, 184, 184, 1, g, hp, rt.ptr(out), rt.stream_handle(), *extra))
            outs.append(out.cpu().numpy())
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)
    heat_avg = cpu_ref.hand_maps(np.zeros((184, 184, 3), np.uint8), lambda im: heat.cpu().numpy(), (0.5,))
    assert np.array_equal(outs[0][0], cpu_ref.hand_post(heat_avg, 0.05))


@pytest.mark.parametrize("path", sorted(PATHS))
def test_body_thresholds_vs_oracle(net25, path):
    """candidate, subset and connection_all at every (thre1, thre2) of the grid == the oracle's
    find_peaks(thre1) / connect_limbs(thre2) / assemble, whose counts differ at every value."""
    H, W, geom = PATHS[path]
    peaks = [po.counts(po.oracle_body(path, t1, 0.05))[0] for t1 in po.THRE1]
    assert all(a > b > 0 for a, b in zip(peaks, peaks[1:])), peaks
    lo, hi = (po.counts(po.oracle_body(path, 0.1, t2)) for t2 in po.THRE2)
    assert lo[1] > hi[1] > 0 and lo[2] > hi[2] > 0, (lo, hi)
    pafs, heats = _cuda_maps((100, 101))
    for t1 in po.THRE1:
        for t2 in po.THRE2:
            est = BodyEstimator(net=net25, thre1=t1, thre2=t2)
            got = est.post_maps(H, W, [geom], pafs, heats)
            for i, seed in enumerate((100, 101)):
                _assert_frame(got[i], po.oracle_body(path, t1, t2, seed), (path, t1, t2, seed))


@pytest.mark.parametrize("env", ["ISLPOSE_LIMB_LDS", "ISLPOSE_ASM_REG", "ISLPOSE_LIMB_SPLIT"])
def test_alternate_limb_and_assembly_forms_take_the_options(net25, monkeypatch, env):
    """The per-thread pair loop, the table merge and the one-block-per-limb scoring at a
    non-default (thre1, thre2) on the ramped maps (small pair sets; the large ones:
    test_large_pair_sets_take_thre2)."""
    monkeypatch.setenv(env, "0")
    H, W, geom = PATHS["unfused"]
    pafs, heats = _cuda_maps((100,))
    got = BodyEstimator(net=net25, thre1=0.2, thre2=0.4).post_maps(H, W, [geom], pafs, heats)
    _assert_frame(got[0], po.oracle_body("unfused", 0.2, 0.4), env)


@pytest.fixture(scope="module")
def crowd():
    """16 designed persons, amplitudes ramped along x, on a 184 x 1792 frame (23 x 224 maps):
    limbs with 256 candidate pairs; the oracle at (0.1, 0.05) and at (0.2, 0.4)."""
    H, W = 184, 1792
    paf, heat = synth.designed_pose_maps(23, 224, 16, seed=520)
    ramp = np.linspace(0.3, 1.0, 224, dtype=np.float32)
    paf, heat = np.ascontiguousarray(paf * ramp), np.ascontiguousarray(heat * ramp)
    heat_avg, paf_avg = cpu_ref.body_maps(np.zeros((H, W, 3), np.uint8), lambda im: (paf[None], heat[None]),
                                          "body25", (0.5,))
    ref = {}
    for t1, t2 in ((0.1, 0.05), (0.2, 0.4)):
        all_peaks = cpu_ref.find_peaks(heat_avg, 26, t1)
        conns, special_k = cpu_ref.connect_limbs(all_peaks, paf_avg, "body25", H, t2)
        cand, subset = cpu_ref.assemble(all_peaks, conns, special_k, "body25")
        ref[(t1, t2)] = (cand, subset, all_peaks, conns)
    return {"H": H, "W": W, "geom": [g[1:] for g in scale_geometry(H, W, (0.5,))], "ref": ref,
            "paf": torch.from_numpy(paf[None]).cuda(), "heat": torch.from_numpy(heat[None]).cuda()}


@pytest.mark.parametrize("lds,split", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")])
def test_large_pair_sets_take_thre2(net25, crowd, monkeypatch, lds, split):
    a, b = crowd["ref"][(0.1, 0.05)], crowd["ref"][(0.2, 0.4)]
    assert max(len(p) for p in b[2]) ** 2 > 204           # still the large-pair path at thre1 = 0.2
    assert po.counts(a)[0] > po.counts(b)[0] and po.counts(a)[1] > po.counts(b)[1], (po.counts(a), po.counts(b))
    monkeypatch.setenv("ISLPOSE_LIMB_LDS", lds)
    monkeypatch.setenv("ISLPOSE_LIMB_SPLIT", split)
    got = BodyEstimator(net=net25, thre1=0.2, thre2=0.4).post_maps(crowd["H"], crowd["W"], crowd["geom"],
                                                                  [crowd["paf"]], [crowd["heat"]])
    _assert_frame(got[0], b, (lds, split))


def _hand_case(side):
    """4-scale designed hand maps of a side x side crop, every third plane scaled by 0.15."""
    geoms = [g[1:] for g in scale_geometry(side, side, HAND_SCALES)]
    maps = []
    for (nh, nw, vh, vw) in geoms:
        m = synth.designed_hand_maps(nh // 8, nw // 8, seed=side, n_blobs=2).copy()
        m[::3] *= 0.15
        maps.append(m)
    it = iter(maps)
    heat_avg = cpu_ref.hand_maps(np.zeros((side, side, 3), np.uint8), lambda im: next(it)[None])
    return geoms, maps, heat_avg


@pytest.mark.parametrize("side", [184, 256])
def test_hand_threshold_vs_oracle(nethand, side):
    """hand_thre on the single-workgroup path (184^2 px) and the large-plane chain (256^2 px)
    == cpu_ref.hand_post(heatmap_avg, thre); some part is [0, 0] at 0.2 and found at 0.02."""
    geoms, maps, heat_avg = _hand_case(side)
    ref = {t: cpu_ref.hand_post(heat_avg.copy(), t) for t in (0.02, 0.05, 0.2)}
    gone = [(ref[0.2][p] == 0).all() and (ref[0.02][p] != 0).any() for p in range(21)]
    assert any(gone), (ref[0.02], ref[0.2])
    heats = [torch.from_numpy(m[None]).cuda() for m in maps]
    for t in (0.02, 0.05, 0.2):
        est = HandEstimator(net=nethand, thre=t)
        assert np.array_equal(est.post_maps(side, side, geoms, heats)[0], ref[t]), t
        assert np.array_equal(est.post_crops([(0, 0, 0, side)], heats)[0], ref[t]), t


@pytest.mark.parametrize("case,seed", [("fused", 100), ("unfused", 100), ("large", 105)])
def test_person_cap_vs_rule(net25, monkeypatch, case, seed):
    """subset == the oracle's subset filtered by the rule, candidate unchanged, for max_people 1,
    2 and above the person count; the register merge and the table merge (ISLPOSE_ASM_REG=0)."""
    cand, subset, _, _ = po.oracle_body(case, 0.1, 0.05, seed)
    if case == "large":
        H, W, geom = 368, 656, (368, 656, 368, 656)
        paf, heat = synth.designed_pose_maps(46, 82, 6, seed=seed)
        assert np.argmax(subset[:, -2]) != 0 or np.argsort(-subset[:, -2])[1] != 1    # not a prefix of the rows
    else:
        H, W, geom = PATHS[case]
        paf, heat = po.ramped_maps(seed)
    pafs, heats = [torch.from_numpy(paf[None]).cuda()], [torch.from_numpy(heat[None]).cuda()]
    assert len(subset) >= 3
    for reg in ("1", "0"):
        monkeypatch.setenv("ISLPOSE_ASM_REG", reg)
        for k in (1, 2, len(subset), len(subset) + 3, 0, None):
            got = BodyEstimator(net=net25, max_people=k).post_maps(H, W, [geom], pafs, heats)[0]
            want = po.cap_rule(subset, k)
            assert len(want) == (min(k, len(subset)) if k else len(subset))
            assert np.array_equal(got.candidate, cand), (case, reg, k)
            assert np.array_equal(got.subset, want), (case, reg, k)


def test_person_cap_in_global_table(net25):
    """max_rows above the LDS table (assemble_kernel<false>): the same cap."""
    cand, subset, _, _ = po.oracle_body("large", 0.1, 0.05, 105)
    paf, heat = synth.designed_pose_maps(46, 82, 6, seed=105)
    est = BodyEstimator(net=net25, max_people=2, caps=dict(max_rows=512))
    got = est.post_maps(368, 656, [(368, 656, 368, 656)], [torch.from_numpy(paf[None]).cuda()],
                        [torch.from_numpy(heat[None]).cuda()])[0]
    assert np.array_equal(got.candidate, cand) and np.array_equal(got.subset, po.cap_rule(subset, 2))


def test_capacity_rerun_keeps_the_options(net25):
    """caps of one peak per part force the post's capacity re-run; at thre1 = 0.3, thre2 = 0.4 and
    max_people = 1 the re-run's result is the oracle's for those values."""
    H, W, geom = PATHS["fused"]
    pafs, heats = _cuda_maps((100,))
    est = BodyEstimator(net=net25, thre1=0.3, thre2=0.4, max_people=1, caps=dict(max_peaks=1))
    host, lay, caps = est.post(1, H, W, [geom], pafs, heats)
    assert caps["max_peaks"] > 1                      # it did re-run
    got = est.decode(host, lay, caps, 1)[0]
    cand, subset, all_peaks, conns = po.oracle_body("fused", 0.3, 0.4)
    assert len(subset) > 1 and po.counts(po.oracle_body("fused", 0.1, 0.05)) != po.counts((cand, subset, all_peaks, conns))
    _assert_frame(got, (cand, po.cap_rule(subset, 1), all_peaks, conns), "capacity re-run")


def test_frame_seam_with_options():
    """ISLSignPos(max_people=1, thre1=0.2) on two tamed 368 x 656 frames, graph replay as
    ISLSignPos turns it on: call == call_batch == BodyEstimator + util.handDetect + HandEstimator
    with the same options; at most two hand crops per frame reach the hand estimator, and the
    person kept is the uncapped run's best-scoring row."""
    from src import util
    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPos
    frames = synth.synth_frames(2, 368, 656, seed=41)
    # (gain 0.1: peaks of ~0.2-0.4 on these frames, so thre1 = 0.2 leaves persons to cap)
    wb = _tame.tame_body(synth.synth_weights(0), frames[0], scale=0.5, gain=0.1)
    tw = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    body, hand = Body(tw(wb), "body25"), Hand(tw(synth.synth_weights(2)))
    isl = ISLSignPos(body.model, hand.model, max_people=1, thre1=0.2)
    best, hest = isl._estimators()
    seen = []
    crops = hest.estimate_crops

    def counting(t, boxes):
        seen.append(list(boxes))
        return crops(t, boxes)
    hest.estimate_crops = counting
    batch = isl.call_batch(frames)
    assert len(seen) == 1
    for i in range(2):
        assert sum(1 for b in seen[0] if b[0] == i) <= 2
    dev = torch.cuda.current_device()
    bnet, hnet = body.model.native(dev), hand.model.native(dev)
    b_opt = BodyEstimator(model_type="body25", device=dev, scale_search=(0.5,), net=bnet, thre1=0.2, max_people=1)
    b_all = BodyEstimator(model_type="body25", device=dev, scale_search=(0.5,), net=bnet, thre1=0.2)
    h_opt = HandEstimator(device=dev, net=hnet)
    n_hands = 0
    for i in range(2):
        cand, subset, hands = isl.call(frames[i])
        c2, s2, h2 = batch[i]
        assert np.array_equal(cand, c2) and np.array_equal(subset, s2) and len(hands) == len(h2)
        c3, s3 = b_opt.estimate(frames[i])
        assert np.array_equal(cand, c3) and np.array_equal(subset, s3)
        ca, sa = b_all.estimate(frames[i])
        assert np.array_equal(cand, ca) and len(sa) > 1 and np.array_equal(subset, po.cap_rule(sa, 1))
        boxes = util.handDetect(cand, subset, frames[i])
        assert len(boxes) == len(hands) <= 2
        for (x, y, w, _), pk, pb in zip(boxes, hands, h2):
            ref = h_opt.estimate(np.ascontiguousarray(frames[i, y:y + w, x:x + w]))
            ref[:, 0] = np.where(ref[:, 0] == 0, ref[:, 0], ref[:, 0] + x)
            ref[:, 1] = np.where(ref[:, 1] == 0, ref[:, 1], ref[:, 1] + y)
            assert np.array_equal(pk, ref) and np.array_equal(pk, pb)
        n_hands += len(hands)
    assert n_hands >= 1, "the tamed weights should leave the kept person a hand crop"
