"""The post kernels at small and odd sizes, on the frame border, at exact ties and at the
capacity limits, bit for bit against the oracle (tests/_post_edges.py builds the inputs and
caches the oracle's results; tests/test_post_edges_ref.py proves on the CPU that the inputs have
the properties claimed and that each case reaches the branch its row names).

Body: frames shorter than 332 px at scale 0.5 (stage-2 tiles of fewer than 64 rows: no band
maxima, the dense blur grid), odd widths (the scalar tail of OpenCV's vertical pass in column
W - 1, the plain resize forms), the fused two-stage window, two and four scales, COCO; peaks on
all four borders and connections between them.  Hand: crops from 20 px (36.8 source rows per
output row, accumulate tiles of 1-3 rows), a mixed batch, lattices of 4 / 16 / 81 exactly tied
components on both component paths.  Capacity: each of the four caps alone at 1, a batch where
one frame overflows and one is empty, and the bytes around the records and the hand outputs."""
import ctypes

import numpy as np
import pytest
import torch

import _post_edges as pe
from islpose import runtime as rt
from islpose import synth
from islpose.body import KINDS, BodyEstimator
from islpose.hand import HandEstimator

pytestmark = pytest.mark.gpu

ENVS = ("ISLPOSE_FUSED_BLUR", "ISLPOSE_BLUR_LIST", "ISLPOSE_BLUR_BANDS", "ISLPOSE_RESIZE_SKIP", "ISLPOSE_RESIZE_V4",
        "ISLPOSE_BLUR_EXACT")
GUARD = 4096


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name, kind in (("body25", rt.ISL_BODY25), ("coco", rt.ISL_COCO), ("hand", rt.ISL_HAND)):
        out[name] = rt.Net(kind)
        out[name].load_weights(synth.synth_weights(kind))
    return out


@pytest.fixture
def default_env(monkeypatch):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)


def _cuda_batch(key):
    """Per scale the [2, C, h8, w8] paf and heat tensors: frame 0 the edge maps, frame 1 the noise."""
    f0, f1 = pe.body_maps(key, 0), pe.body_maps(key, 1)
    pafs = [torch.from_numpy(np.stack([a[0], b[0]])).cuda() for a, b in zip(f0, f1)]
    heats = [torch.from_numpy(np.stack([a[1], b[1]])).cuda() for a, b in zip(f0, f1)]
    return pafs, heats


def _assert_oracle(got, ref, what):
    cand, subset, _, conns = ref
    assert np.array_equal(got.candidate, cand), what
    assert np.array_equal(got.subset, subset), what
    assert len(got.connection_all) == len(conns), what
    for a, b in zip(got.connection_all, conns):
        assert np.array_equal(np.asarray(a).reshape(-1, 5), np.asarray(b).reshape(-1, 5)), what


def _assert_same(a, b, what):
    assert np.array_equal(a.candidate, b.candidate) and np.array_equal(a.subset, b.subset), what
    for x, y in zip(a.connection_all, b.connection_all):
        assert np.array_equal(np.asarray(x).reshape(-1, 5), np.asarray(y).reshape(-1, 5)), what


@pytest.mark.parametrize("key", sorted(pe.BODY_CASES))
def test_body_edges_vs_oracle(nets, default_env, monkeypatch, key):
    """post_maps == cpu_ref.body_maps + body_post in candidate, subset and every connection_all
    row, on the edge maps (frame 0) and on one person with threshold noise (frame 1); the
    default run == the fp64 blur passes alone (ISLPOSE_BLUR_EXACT=1), == the materialised planes
    where the plan is fused (ISLPOSE_FUSED_BLUR=0), == the one-column vertical pass where a
    resize of the plan has the V4 form (ISLPOSE_RESIZE_V4=0)."""
    kind, H, W, scales, branch, _ = pe.BODY_CASES[key]
    plan = pe.body_plan(key, n=2)
    assert plan["blur"] == branch, plan
    est = BodyEstimator(net=nets[kind], model_type=kind)
    geoms = pe.body_geoms(key)
    pafs, heats = _cuda_batch(key)
    got = est.post_maps(H, W, geoms, pafs, heats)
    _assert_oracle(got[0], pe.body_oracle(key, 0), (key, "edge frame"))
    assert len(got[0].subset) == 2
    _assert_oracle(got[1], pe.body_oracle(key, 1), (key, "noise frame"))
    assert len(got[1].candidate) > 0
    runs = [("ISLPOSE_BLUR_EXACT", "1")]
    if plan["fused"]:
        runs.append(("ISLPOSE_FUSED_BLUR", "0"))
    if any(r["v4"] for r in plan["stage1"] + plan["final"]):
        runs.append(("ISLPOSE_RESIZE_V4", "0"))
    for env, v in runs:
        monkeypatch.setenv(env, v)
        alt = pe.body_plan(key, n=2)
        assert alt != plan, env                        # the switch does change what runs
        ref = est.post_maps(H, W, geoms, pafs, heats)
        monkeypatch.delenv(env)
        for f in (0, 1):
            _assert_same(got[f], ref[f], (key, env, f))


def _hand_heats(sides):
    """Per scale [n, 22, h8, w8]: the field maps of square crops `sides` (one net size per scale)."""
    per = [pe.hand_field(s, s) for s in sides]
    return [torch.from_numpy(np.stack([p[si] for p in per])).cuda() for si in range(len(per[0]))]


@pytest.mark.parametrize("hw", [(s, s) for s in pe.HAND_SQUARE] + [pe.HAND_RECT])
def test_hand_small_crops_vs_oracle(nets, default_env, hw):
    """post_maps(return_scores=True) at crops from 20 px: the peaks and the scores of the oracle,
    the parts on the crop's border and in its corners among them."""
    h, w = hw
    est = HandEstimator(net=nets["hand"])
    heats = [torch.tensor(m[None]).cuda() for m in pe.hand_field(h, w)]
    peaks, scores = est.post_maps(h, w, pe.hand_geoms(h, w), heats, return_scores=True)
    rp, rs, _ = pe.hand_oracle(h, w)
    assert np.array_equal(peaks[0], rp), (peaks[0], rp)
    assert scores[0].tobytes() == rs.tobytes(), (scores[0], rs)


def test_hand_mixed_batch_vs_oracle(nets, default_env):
    """Crops of 20, 37, 63, 185 and 21 px in one post_crops call: each equals its own oracle."""
    est = HandEstimator(net=nets["hand"])
    heats = _hand_heats(pe.HAND_BATCH)
    peaks, scores = est.post_crops([(0, 0, 0, s) for s in pe.HAND_BATCH], heats, return_scores=True)
    for i, s in enumerate(pe.HAND_BATCH):
        rp, rs, _ = pe.hand_oracle(s, s)
        assert np.array_equal(peaks[i], rp), s
        assert scores[i].tobytes() == rs.tobytes(), s


@pytest.mark.parametrize("key", sorted(pe.LATTICES))
def test_hand_tied_components_vs_oracle(nets, default_env, key):
    """4, 16 and 81 components whose sums are bitwise equal: the first label wins (hand.py:68-69)
    on the fast finish, the sorted candidate list and the all-roots loop of the large-plane
    chain, and on the single-workgroup path; the boosted part takes its outright winner."""
    side, scales, _, _, _, _ = pe.LATTICES[key]
    est = HandEstimator(net=nets["hand"], scale_search=scales)
    heat = torch.tensor(pe.lattice_maps(key)[None]).cuda()
    geoms = pe.hand_geoms(side, side, scales)
    ref = pe.lattice_oracle(key)[0]                       # cpu_ref.hand_post of cpu_ref.hand_maps
    assert np.array_equal(est.post_maps(side, side, geoms, [heat])[0], ref)
    assert np.array_equal(est.post_crops([(0, 0, 0, side)], [heat])[0], ref)


def _guarded(nbytes):
    """A device buffer of nbytes between two guards of 0xA5; the payload zeroed."""
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + nbytes] = 0
    return buf


def _guards_intact(buf, nbytes):
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[GUARD + nbytes:] == 0xA5).all())


CAP_NAMES = ("max_peaks", "max_pairs", "max_conns", "max_rows")


@pytest.mark.parametrize("key", ["b97x131", "b336x132", "b201x121m2", "c150x134"])
def test_capacity_overflow_stays_inside_the_records(nets, default_env, key):
    """isl_body_post_opts on [edge-map frame, all-zero frame] with the records between two 4 KiB
    guards: at the default caps both frames are ISL_OK; with each cap alone at 1 the edge frame
    is ISL_E_CAPACITY, the empty frame ISL_OK with no peaks and no rows, and no byte of either
    guard changes.  Then the estimator's re-run from each starved cap equals the oracle."""
    kind, H, W, scales, _, _ = pe.BODY_CASES[key]
    net = nets[kind]
    est = BodyEstimator(net=net, model_type=kind)
    geoms = pe.body_geoms(key)
    f0 = pe.body_maps(key, 0)
    pafs = [torch.from_numpy(np.stack([a[0], np.zeros_like(a[0])])).cuda() for a in f0]
    heats = [torch.from_numpy(np.stack([a[1], np.zeros_like(a[1])])).cuda() for a in f0]
    ns, n, L = len(geoms), 2, rt.lib()
    g = (rt.IslScaleGeom * ns)(*[rt.IslScaleGeom(*gg) for gg in geoms])
    pp = (ctypes.c_void_p * ns)(*[rt.ptr(p).value for p in pafs])
    hp = (ctypes.c_void_p * ns)(*[rt.ptr(h).value for h in heats])
    nparts = est.njoint - 1
    ref = pe.body_oracle(key, 0)
    for starve in (None,) + CAP_NAMES:
        caps = dict(est.caps, **({starve: 1} if starve else {}))
        c = rt.IslCaps(**caps)
        lay = rt.body_layout(KINDS[kind], c)
        nbytes = n * lay.record_bytes
        buf = _guarded(nbytes)
        rt.check(L.isl_body_post_opts(net.h, n, H, W, ns, g, pp, hp, ctypes.byref(c),
                                      ctypes.c_void_p(rt.ptr(buf).value + GUARD), rt.stream_handle(), None))
        torch.cuda.synchronize()
        assert _guards_intact(buf, nbytes), starve
        host = buf.cpu().numpy()[GUARD:GUARD + nbytes]
        status = [int(host[f * lay.record_bytes + lay.status:][:4].view(np.int32)[0]) for f in range(n)]
        assert status == [rt.ISL_E_CAPACITY if starve else rt.ISL_OK, rt.ISL_OK], (starve, status)
        rec1 = host[lay.record_bytes:]
        assert not rec1[lay.n_peaks:lay.n_peaks + 128].view(np.int32)[:nparts].any(), starve
        assert int(rec1[lay.n_rows:lay.n_rows + 4].view(np.int32)[0]) == 0, starve
        if not starve:
            frames = est.decode(host, lay, caps, n)
            _assert_oracle(frames[0], ref, (key, "default caps"))
            assert len(frames[1].candidate) == 0 and len(frames[1].subset) == 0
    for starve in CAP_NAMES:
        grown = BodyEstimator(net=net, model_type=kind, caps={starve: 1})
        host, lay, caps = grown.post(n, H, W, geoms, pafs, heats)
        assert caps[starve] > 1, starve                   # it did re-run
        frames = grown.decode(host, lay, caps, n)
        _assert_oracle(frames[0], ref, (key, starve, "re-run"))
        assert len(frames[1].candidate) == 0 and len(frames[1].subset) == 0


@pytest.mark.parametrize("side", [20, 185])
def test_hand_outputs_stay_inside_their_arrays(nets, default_env, side):
    """isl_hand_post_ex with the peaks and the scores arrays between guards: the oracle's values
    inside, no byte changed outside."""
    est = HandEstimator(net=nets["hand"])
    heats = [torch.tensor(m[None]).cuda() for m in pe.hand_field(side, side)]
    geoms = pe.hand_geoms(side, side)
    ns = len(geoms)
    g = (rt.IslScaleGeom * ns)(*[rt.IslScaleGeom(*gg) for gg in geoms])
    hp = (ctypes.c_void_p * ns)(*[rt.ptr(t).value for t in heats])
    pk, sc = _guarded(21 * 2 * 8), _guarded(21 * 8)
    rt.check(rt.lib().isl_hand_post_ex(nets["hand"].h, 1, side, side, ns, g, hp,
                                       ctypes.c_void_p(rt.ptr(pk).value + GUARD), rt.stream_handle(), None, None,
                                       ctypes.c_void_p(rt.ptr(sc).value + GUARD)))
    torch.cuda.synchronize()
    assert _guards_intact(pk, 21 * 2 * 8) and _guards_intact(sc, 21 * 8)
    rp, rs, _ = pe.hand_oracle(side, side)
    assert np.array_equal(pk.cpu().numpy()[GUARD:GUARD + 336].view(np.int64).reshape(21, 2), rp)
    assert sc.cpu().numpy()[GUARD:GUARD + 168].view(np.float64).tobytes() == rs.tobytes()
