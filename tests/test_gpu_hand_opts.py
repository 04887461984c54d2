"""The hand-path options on the GPU: the mirrored pre-processing bit for bit against the oracle
on the physically mirrored crop, the post's mirrored store and scores against the oracle on
designed maps (every exit of hand_cc_kernel), nets and post together, the defaults unchanged,
and ISLSignPos.hands_for on designed body results."""
import ctypes

import numpy as np
import pytest
import torch

import _hand_opts as ho
from oracle import cpu_ref
from islpose import runtime as rt
from islpose import synth
from islpose.hand import HandEstimator, HAND_SCALES

pytestmark = pytest.mark.gpu

BOXES5 = [(0, 20, 30, 96), (1, 0, 0, 40), (2, 104, 64, 96), (0, 150, 100, 50), (1, 33, 71, 77)]
FLIP5 = [1, 0, 1, 1, 0]


@pytest.fixture(scope="module")
def hest():
    return HandEstimator(synth.synth_weights(2))


def _crop(frames, box):
    f, x, y, w = box
    return np.ascontiguousarray(frames[f, y:y + w, x:x + w])


def _mirror(crop):
    return np.ascontiguousarray(crop[:, ::-1])


# ---- 1. pre-processing ------------------------------------------------------------------

def test_flip_preprocess_bit_exact(hest):
    """isl_net_preprocess_crops_flip: a flagged crop's slot == the oracle's net_input on the
    contiguous crop[:, ::-1], an unflagged one's on the crop, bit for bit: every pyramid scale
    (the cubic path, its float body and fixed-point tail) and scale_times_box == the crop size
    (the identity path)."""
    frames = synth.synth_frames(2, 120, 160, seed=17)
    t = torch.from_numpy(frames).cuda()
    boxes = [(0, 10, 5, 60), (1, 100, 60, 60), (0, 0, 0, 37), (1, 123, 83, 37)]
    for size, flags in ((60, [1, 0]), (37, [0, 1]), (60, [1, 1])):
        same = [b for b in boxes if b[3] == size]
        for stb in [s * 368 for s in HAND_SCALES] + ([60] if size == 60 else []):
            nh, nw = hest.net.preprocess_crops(t, [(f, x, y, w, w) for f, x, y, w in same], stb, flip=flags)
            got = hest.net.debug_input(len(same), nh, nw).cpu().numpy()
            for i, b in enumerate(same):
                crop = _crop(frames, b)
                ref, _, _ = cpu_ref.net_input(_mirror(crop) if flags[i] else crop, stb / size)
                assert ref.shape[2:] == (nh, nw)
                assert np.array_equal(got[i:i + 1], ref), (size, stb, i)
                if flags[i]:      # and the mirror is not a no-op on these pixels
                    assert not np.array_equal(got[i:i + 1], cpu_ref.net_input(crop, stb / size)[0])


# ---- 2. post on designed maps -----------------------------------------------------------

CASES = [(64, 64, 2, "blobs"), (57, 57, 2, "blobs"), (200, 200, 2, "blobs"), (260, 240, 2, "dense"),
         (184, 184, 1, "tie"), (368, 368, 1, "tie")]


@pytest.mark.parametrize("h,w,n,kind", CASES)
def test_post_scores_and_flip_vs_oracle(hest, h, w, n, kind):
    """post_maps(return_scores=True) == the oracle's peaks and its masked map at the peak, as
    fp64 bytes; with flip the detected x is w - 1 - x, the corner part goes to x = w - 1 and the
    empty part stays [0, 0] with score 0.0.  64^2 / 57^2 / 184^2: the LDS kernel; 200^2,
    260 x 240 (dense) and 368^2: the cc_* chain and its fast finish; the 'tie' inputs hold six
    components with the same sum in one part (more than the fast finish takes)."""
    per = ho.designed(h, w, n, kind)
    heats = [torch.from_numpy(p).cuda() for p in per]
    geoms = ho.geoms_of(h, w)
    ref = [ho.oracle(h, w, n, kind, i) for i in range(n)]
    for i, (pk, sc, found) in enumerate(ref):        # the designed preconditions, on the oracle alone
        print("oracle %dx%d %s crop %d: part 5 score %r, min detected %r" % (h, w, kind, i, sc[5], min(sc[list(found)])))
        assert not found[3] and list(pk[3]) == [0, 0] and sc[3] == 0.0
        assert found[5] and list(pk[5]) == [0, 0] and sc[5] > 0
    peaks, scores = hest.post_maps(h, w, geoms, heats, return_scores=True)
    assert peaks.dtype == np.int64 and peaks.shape == (n, 21, 2)
    assert scores.dtype == np.float64 and scores.shape == (n, 21)
    assert np.array_equal(hest.post_maps(h, w, geoms, heats), peaks)
    for flags in ([False] * n, [True] * n, [True, False][:n], [False, True][:n]):
        pf, sf = hest.post_maps(h, w, geoms, heats, flip=flags, return_scores=True)
        assert np.array_equal(hest.post_maps(h, w, geoms, heats, flip=flags), pf)
        for i, (pk, sc, found) in enumerate(ref):
            want = ho.mirrored(pk, found, w) if flags[i] else pk
            assert np.array_equal(pf[i], want), (flags, i)
            assert sf[i].tobytes() == sc.tobytes(), (flags, i)
            assert list(pf[i][3]) == [0, 0] and sf[i][3] == 0.0
            assert list(pf[i][5]) == [w - 1 if flags[i] else 0, 0]
    assert np.array_equal(scores, np.stack([r[1] for r in ref]))


def test_post_crops_mixed_widths_vs_oracle(hest):
    """isl_hand_post_crops_ex: crops of different widths in one call (the LDS kernel and the
    cc_* chain side by side on the post lanes), a flag per crop."""
    sizes = [(64, "blobs"), (200, "blobs"), (57, "blobs"), (184, "tie"), (64, "blobs")]
    idx = [0, 0, 1, 0, 1]
    nn = {64: 2, 200: 2, 57: 2, 184: 1}
    heats = [torch.from_numpy(np.stack([ho.designed(w, w, nn[w], k)[si][i] for (w, k), i in zip(sizes, idx)])).cuda()
             for si in range(len(HAND_SCALES))]
    boxes = [(0, 0, 0, w) for w, _ in sizes]
    ref = [ho.oracle(w, w, nn[w], k, i) for (w, k), i in zip(sizes, idx)]
    for flags in (None, [1, 0, 1, 1, 0], [0, 1, 0, 0, 1]):
        pk, sc = hest.post_crops(boxes, heats, flags, True)
        assert np.array_equal(hest.post_crops(boxes, heats, flags), pk)
        for i, (rp, rs, found) in enumerate(ref):
            w = sizes[i][0]
            want = ho.mirrored(rp, found, w) if flags and flags[i] else rp
            assert np.array_equal(pk[i], want), (flags, i)
            assert sc[i].tobytes() == rs.tobytes(), (flags, i)


# ---- 3. nets and post together ----------------------------------------------------------

def _case3(est, per_crop=True):
    frames = synth.synth_frames(3, 160, 200, seed=23)
    got, sc = est.estimate_crops(frames, BOXES5, flip=FLIP5, return_scores=True)
    assert got.shape == (5, 21, 2) and got.dtype == np.int64 and sc.shape == (5, 21) and sc.dtype == np.float64
    if per_crop:
        ref = [est.estimate(_mirror(_crop(frames, b)) if fl else _crop(frames, b), return_scores=True)
               for b, fl in zip(BOXES5, FLIP5)]
    else:       # the same batch on frames that hold the flagged crops physically mirrored (the boxes are disjoint)
        fm = frames.copy()
        for (f, x, y, w), fl in zip(BOXES5, FLIP5):
            if fl:
                fm[f, y:y + w, x:x + w] = _mirror(_crop(frames, (f, x, y, w)))
        ref = list(zip(*est.estimate_crops(fm, BOXES5, return_scores=True)))
    n_mirrored = 0
    for b, fl, pk, s, (rp, rs) in zip(BOXES5, FLIP5, got, sc, ref):
        assert s.tobytes() == rs.tobytes(), b
        want = ho.mirrored(rp, rs, b[3]) if fl else rp
        assert np.array_equal(pk, want), b
        n_mirrored += int(fl and not np.array_equal(want, rp))
        if per_crop:    # estimate()'s own flip: the same again from the unmirrored crop
            ep, es = est.estimate(_crop(frames, b), flip=bool(fl), return_scores=True)
            assert np.array_equal(ep, pk) and es.tobytes() == s.tobytes()
    assert n_mirrored == sum(FLIP5)
    t = torch.from_numpy(frames).cuda()
    lp, ls = est.finish_crops(est.launch_crops(t, BOXES5, flip=FLIP5, return_scores=True))
    assert np.array_equal(lp, got) and ls.tobytes() == sc.tobytes()
    assert np.array_equal(est.finish_crops(est.launch_crops(t, BOXES5, flip=FLIP5)), got)
    e = est.estimate_crops(frames, [], flip=[], return_scores=True)
    assert e[0].shape == (0, 21, 2) and e[1].shape == (0, 21)
    with pytest.raises(ValueError):
        est.estimate_crops(frames, BOXES5, flip=[1, 0])


def test_estimate_crops_flip_matches_mirrored_crops(hest):
    """estimate_crops(flip=, return_scores=True) per crop == estimate() on the physically
    mirrored contiguous crop with the detected x mirrored back, the scores bit for bit; the same
    through launch_crops / finish_crops and estimate(flip=)."""
    _case3(hest)


def test_fp16_modes_flip_matches_mirrored_crops():
    """Within precision 'fp16' with fp16 activation storage: the batch with flags == the same
    estimator's batch on frames holding those crops physically mirrored, bit for bit -- the
    mirror and the store are independent of the conv arithmetic."""
    _case3(HandEstimator(synth.synth_weights(2), precision="fp16", act_storage="fp16"), per_crop=False)


# ---- 4. defaults ------------------------------------------------------------------------

def test_null_arguments_are_the_old_entry_points(hest):
    L = rt.lib()
    frames = synth.synth_frames(2, 120, 160, seed=17)
    t = torch.from_numpy(frames).cuda()
    crops = [(0, 10, 5, 60, 60), (1, 100, 60, 60, 60)]
    arr = (rt.IslCrop * 2)(*[rt.IslCrop(*c) for c in crops])
    nh, nw = ctypes.c_int32(), ctypes.c_int32()
    ins = []
    for flip_entry in (False, True):
        if flip_entry:
            rc = L.isl_net_preprocess_crops_flip(hest.net.h, rt.ptr(t), 2, 120, 160, arr, None, 2, 368.0,
                                                 ctypes.byref(nh), ctypes.byref(nw), rt.stream_handle())
        else:
            rc = L.isl_net_preprocess_crops(hest.net.h, rt.ptr(t), 2, 120, 160, arr, 2, 368.0, ctypes.byref(nh),
                                            ctypes.byref(nw), rt.stream_handle())
        rt.check(rc)
        ins.append(hest.net.debug_input(2, nh.value, nw.value).cpu().numpy())
    assert ins[0].tobytes() == ins[1].tobytes()
    zero = (ctypes.c_uint8 * 2)(0, 0)       # all-zero flags: the same again
    rt.check(L.isl_net_preprocess_crops_flip(hest.net.h, rt.ptr(t), 2, 120, 160, arr, zero, 2, 368.0,
                                             ctypes.byref(nh), ctypes.byref(nw), rt.stream_handle()))
    assert hest.net.debug_input(2, nh.value, nw.value).cpu().numpy().tobytes() == ins[0].tobytes()

    sizes = [(64, 0), (200, 0), (57, 1)]
    heats = [torch.from_numpy(np.stack([ho.designed(w, w, 2, "blobs")[si][i] for w, i in sizes])).cuda()
             for si in range(4)]
    n, ns = len(sizes), 4
    ws = (ctypes.c_int32 * n)(*[w for w, _ in sizes])
    g = (rt.IslScaleGeom * (n * ns))()
    for i, (w, _) in enumerate(sizes):
        for si, gg in enumerate(ho.geoms_of(w, w)):
            g[i * ns + si] = rt.IslScaleGeom(*gg)
    hp = (ctypes.c_void_p * ns)(*[rt.ptr(hh).value for hh in heats])
    outs = []
    for ex in (False, True):
        out = torch.full((n, 21, 2), -7, dtype=torch.int64, device="cuda")
        if ex:
            rc = L.isl_hand_post_crops_ex(hest.net.h, n, ws, ns, g, hp, rt.ptr(out), rt.stream_handle(), None, None, None)
        else:
            rc = L.isl_hand_post_crops_opts(hest.net.h, n, ws, ns, g, hp, rt.ptr(out), rt.stream_handle(), None)
        rt.check(rc)
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    assert np.array_equal(outs[0], np.stack([ho.oracle(w, w, 2, "blobs", i)[0] for w, i in sizes]))
    # the equal-size entry point likewise
    per = ho.designed(64, 64, 2, "blobs")
    h64 = [torch.from_numpy(p).cuda() for p in per]
    g1 = (rt.IslScaleGeom * ns)(*[rt.IslScaleGeom(*gg) for gg in ho.geoms_of(64, 64)])
    hp1 = (ctypes.c_void_p * ns)(*[rt.ptr(hh).value for hh in h64])
    outs = []
    for ex in (False, True):
        out = torch.full((2, 21, 2), -7, dtype=torch.int64, device="cuda")
        if ex:
            rc = L.isl_hand_post_ex(hest.net.h, 2, 64, 64, ns, g1, hp1, rt.ptr(out), rt.stream_handle(), None, None, None)
        else:
            rc = L.isl_hand_post_opts(hest.net.h, 2, 64, 64, ns, g1, hp1, rt.ptr(out), rt.stream_handle(), None)
        rt.check(rc)
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()


def _models():
    from src.body import Body
    from src.hand import Hand
    tw = lambda k: {n: torch.from_numpy(v) for n, v in synth.synth_weights(k).items()}  # noqa: E731
    return Body(tw(0), "body25"), Hand(tw(2))


def _same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb) == 3
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and len(ra[2]) == len(rb[2])
        for x, y in zip(ra[2], rb[2]):
            assert np.array_equal(x, y)


def test_isl_sign_pos_defaults_unchanged():
    from src.ISL_Model_parameter import ISLSignPos
    body, hand = _models()
    frames = synth.synth_frames(2, 200, 300, seed=31)
    a = ISLSignPos(body.model, hand.model).call_batch(frames)
    b = ISLSignPos(body.model, hand.model, hand_scales=(0.5, 1.0, 1.5, 2.0), flip_left=False).call_batch(frames)
    _same_results(a, b)


# ---- 5. hands_for on designed body results ---------------------------------------------

def _one_person():
    """One person with both arms on a 200 x 300 frame: shoulder, elbow, wrist of the right
    (joints 2-4) and the left (5-7) arm."""
    pts = {2: (95, 50), 3: (90, 80), 4: (90, 112), 5: (200, 40), 6: (210, 80), 7: (210, 112)}
    cand = np.array([[x, y, 0.9, k] for k, (x, y) in enumerate(pts.values())], np.float64)
    sub = -np.ones((1, 27))
    for k, j in enumerate(pts):
        sub[0, j] = k
    sub[0, -2], sub[0, -1] = 5.4, 6
    return cand, sub


def test_hands_for_designed_body_results(hest):
    from src import util
    from src.ISL_Model_parameter import ISLSignPos
    body, hand = _models()
    frames = synth.synth_frames(2, 200, 300, seed=33)
    t = torch.from_numpy(frames).cuda()
    cand, sub = _one_person()
    none = (np.zeros((0, 4)), -np.ones((0, 27)))
    boxes = util.hand_boxes(cand, sub, frames[1])
    assert [(b[3], b[4]) for b in boxes] == [(True, 0), (False, 0)]                    # left first, then right
    assert all(40 <= b[2] <= 60 and b[0] + b[2] <= 300 and b[1] + b[2] <= 200 for b in boxes), boxes
    isl = ISLSignPos(body.model, hand.model, flip_left=True, hand_info=True, hand_scales=(1.0, 1.5))
    res = isl.hands_for(t, [none, (cand, sub)])
    assert len(res) == 2 and all(len(r) == 4 for r in res)
    assert res[0][2] == [] and res[0][3] == []
    c, s, hands, info = res[1]
    assert c is cand and s is sub and len(hands) == len(info) == 2
    est = HandEstimator(net=hest.net, scale_search=(1.0, 1.5))
    for (x, y, w, is_left, row), pk, inf in zip(boxes, hands, info):
        crop = _crop(frames, (1, x, y, w))
        rp, rs = est.estimate(_mirror(crop) if is_left else crop, return_scores=True)
        want = ho.mirrored(rp, rs, w) if is_left else rp.copy()
        want[:, 0] = np.where(want[:, 0] == 0, want[:, 0], want[:, 0] + x)          # _assemble's offsets
        want[:, 1] = np.where(want[:, 1] == 0, want[:, 1], want[:, 1] + y)
        assert np.array_equal(pk, want), (x, y, w, is_left)
        assert inf["person"] == row == 0 and inf["is_left"] is is_left and inf["box"] == (x, y, w)
        assert inf["scores"].dtype == np.float64 and inf["scores"].tobytes() == rs.tobytes()
    # without hand_info: the reference's 3-tuple with the same peaks; call_batches' deferred form too
    isl3 = ISLSignPos(body.model, hand.model, flip_left=True, hand_scales=(1.0, 1.5))
    r3 = isl3.hands_for(t, [none, (cand, sub)])
    _same_results(r3, [r[:3] for r in res])
    _same_results(isl3.hands_for(t, [none, (cand, sub)], defer=True)(), r3)
    # flip_left changes the left hand only
    r0 = ISLSignPos(body.model, hand.model, hand_scales=(1.0, 1.5)).hands_for(t, [none, (cand, sub)])
    assert np.array_equal(r0[1][2][1], hands[1]) and not np.array_equal(r0[1][2][0], hands[0])
    keys = set()
    for sc in (None, (1.0, 1.5)):
        for fl in (False, True):
            for hi in (False, True):
                keys.add(ISLSignPos(body.model, hand.model, hand_scales=sc, flip_left=fl, hand_info=hi).state_key())
    assert len(keys) == 8
