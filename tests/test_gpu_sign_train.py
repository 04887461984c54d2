"""isl_sign_grad (csrc/sign_train.hip) and islpose.train.SignTrainer on the GPU against the float64
statement of tests/_sign_train_ref.py.

Gradient bar, per parameter array: max|g_gpu - g_64| <= M * max|g_64| with M = 4 * max(E, 2e-7),
E = the same statement run in fp32 on the CPU against fp64 (relative to max|g_64| of the array),
and M never above 1e-5; l_b is held the same way against max|l_64|.  The factor 4 is the project's
3 * E practice plus room for the device's expf / tanhf differing from the host's by an ulp.  The
mean and variance slots must be exactly 0.
"""
import ctypes

import numpy as np
import pytest

import _sign_ref as dense
import _sign_train_ref as ref

pytestmark = pytest.mark.gpu

PAD = 1024                          # guard band, floats
CANARY = 0x7FC0BEEF                 # a quiet NaN with a payload
M_FLOOR, M_CAP = 2e-7, 1e-5

#          T   F    C     B    what it reaches
SHAPES = [(1, 12, 7, 2),        # a single step
          (5, 10, 3, 4),        # F no multiple of 4; leading, interior, trailing masked steps; an all-masked window
          (20, 156, 167, 6),    # the workload's own shape
          (32, 256, 1024, 3),   # every limit at once: the LDS budget
          (20, 156, 2, 1),      # batch 1, two classes
          (3, 8, 3, 300),       # workgroups that own two windows: the accumulation and the 256-slice reduce
          (9, 12, 7, 4)]        # DENSE: the classifier tests' weights and windows (tests/_sign_ref.py)
DENSE = (9, 12, 7, 4)           # no constant bias block, b3 != 0, signed features, a -0.0 frame, two step ranges
DROPOUT_CASES = [(0.2, 0.2, (5, 12, 7, 4)), (0.5, 0.5, (5, 12, 7, 4)),
                 (0.2, 0.2, (20, 156, 167, 3)), (0.5, 0.5, (20, 156, 167, 3))]

_cache = {}


def _case(T, F, C, B):
    """Weights, windows, labels of a shape (made once)."""
    key = ("case", T, F, C, B)
    if key not in _cache:
        w = ref.trained_like_weights(F, C, seed=T + 1)
        x = ref.windows_like(B, T, F, seed=T + C, masked=0.2)
        if (T, F, C, B) == DENSE:
            w, x = dense.dense_weights(F, C, seed=T + 1), dense.windows(B, T, F, seed=T + C)
        if (T, F) == (5, 10):
            x[:, :, 0] = np.maximum(x[:, :, 0], 1)      # every step unmasked, then:
            x[0, 0] = 0                                 # a leading,
            x[1, 2] = 0                                 # an interior,
            x[2, 4] = 0                                 # a trailing masked step,
            x[3] = 0                                    # and a window with nothing in it
        labels = np.random.RandomState(B).randint(0, C, B).astype(np.int32)
        _cache[key] = (w, x, labels)
    return _cache[key]


def _reference(key, w, x, labels, sw=None, masks=None):
    """(l_64, g_64, M_l, [M per array]) of the statement, made once per key and left unchanged."""
    import torch
    if key not in _cache:
        l64, g64 = ref.loss_and_grads(w, x, labels, sw, masks)
        l32, g32 = ref.loss_and_grads(w, x, labels, sw, masks, dtype=torch.float32)
        def m_of(a32, a64):
            top = np.abs(a64).max()
            e = np.abs(a32 - a64).max() / top if top > 0 else 0.0
            return min(4 * max(e, M_FLOOR), M_CAP)
        _cache[key] = (l64, g64, m_of(l32, l64), [m_of(a, b) for a, b in zip(g32, g64)])
    return _cache[key]


def _split(flat, F, C):
    from islpose import translate
    out, o = [], 0
    for s in translate.keras_weight_shapes(F, C):
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s))
        o += n
    assert o == flat.size
    return out


class _Grad:
    """isl_sign_grad through ctypes with d_loss, d_grad and the workspace inside one canary-filled
    buffer; the guard bands are checked after every call."""

    def __init__(self, w, F, C):
        import torch
        from islpose import runtime as rt
        self.rt, self.torch, self.F, self.C = rt, torch, F, C
        self.params = torch.from_numpy(np.concatenate([np.asarray(a, np.float32).ravel() for a in w])).cuda()
        self.P = self.params.numel()

    def __call__(self, x, labels, sw=None, ids=None, opts=None, expect=0, batch=None, T=None, F=None, C=None,
                 null=()):
        torch, rt = self.torch, self.rt
        x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        B = x.shape[0] if batch is None else batch
        lab = torch.from_numpy(np.asarray(labels, np.int32)).cuda()
        swt = None if sw is None else torch.from_numpy(np.asarray(sw, np.float32)).cuda()
        idt = None if ids is None else torch.from_numpy(np.asarray(ids, np.uint64).view(np.int64)).cuda()
        n = ctypes.c_int64()
        rt.check(rt.lib().isl_sign_grad_workspace(self.F, self.C, max(B, 0), ctypes.byref(n)))
        nb, ws = x.shape[0], n.value // 4
        assert ws == min(max(B, 0), 256) * self.P
        sizes = [nb, self.P, ws]
        buf = torch.full((sum(sizes) + 4 * PAD,), CANARY, dtype=torch.int32, device="cuda")
        fl = buf.view(torch.float32)
        offs = [PAD, 2 * PAD + nb, 3 * PAD + nb + self.P]
        loss, grad, work = (fl[o:o + s] for o, s in zip(offs, sizes))
        ptr = lambda name, t: None if (t is None or name in null) else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        rc = rt.lib().isl_sign_grad(ptr("params", self.params), self.F if F is None else F,
                                    x.shape[1] if T is None else T, self.C if C is None else C, ptr("x", x),
                                    ptr("labels", lab), ptr("weights", swt), ptr("ids", idt), B,
                                    None if opts is None else ctypes.byref(opts), ptr("loss", loss), ptr("grad", grad),
                                    ptr("work", work), None)
        torch.cuda.synchronize()
        assert rc == expect, (rc, rt.lib().isl_last_error())
        ib = buf.cpu().numpy()
        guard = np.ones(ib.size, bool)
        for o, s in zip(offs, sizes):
            guard[o:o + s] = False
        assert (ib[guard] == CANARY).all(), "a guard band was written"
        if rc != 0:
            assert (ib == CANARY).all(), "a refused call wrote to its outputs"
            return None
        out_l, out_g = ib[offs[0]:offs[0] + nb], ib[offs[1]:offs[1] + self.P]
        assert (out_g != CANARY).all() and (B == 0 or (out_l != CANARY).all()), "an output element was not written"
        return out_l.view(np.float32).copy(), out_g.view(np.float32).copy()


def _opts(p_drop, p_rec, seed=0, step=0):
    from islpose import runtime as rt
    return rt.IslSignTrainOpts(p_drop, p_rec, seed, step)


def _hold(got_l, got_g, F, C, l64, g64, ml, mg):
    report = []
    top = np.abs(l64).max()
    err = np.abs(got_l - l64).max()
    report.append("loss: err %.3g of max %.3g, bar %.3g" % (err, top, ml * top))
    bad = [] if err <= ml * top else ["loss"]
    for k, (a, b, m) in enumerate(zip(_split(got_g, F, C), g64, mg)):
        top = np.abs(b).max()
        err = np.abs(a - b).max()
        report.append("array %2d: rel err %.3g, M %.3g" % (k, err / top if top else err, m))
        if k in ref.STAT_SLOTS:
            if a.any():
                bad.append("array %d: a mean / variance slot is not 0" % k)
        elif err > m * top:
            bad.append("array %d" % k)
    print("\n".join(report))
    assert not bad, bad


@pytest.mark.parametrize("T,F,C,B", SHAPES)
def test_gradients_match_statement(T, F, C, B):
    w, x, labels = _case(T, F, C, B)
    l64, g64, ml, mg = _reference(("plain", T, F, C, B), w, x, labels)
    got_l, got_g = _Grad(w, F, C)(x, labels)
    _hold(got_l, got_g, F, C, l64, g64, ml, mg)


@pytest.mark.parametrize("p_drop,p_rec,shape", DROPOUT_CASES)
def test_dropout_matches_statement(p_drop, p_rec, shape):
    """The statement gets its factors from the numpy hash; sample weights and ids are given."""
    T, F, C, B = shape
    w, x, labels = _case(T, F, C, B)
    rng = np.random.RandomState(5)
    sw = rng.uniform(0.5, 2, B)
    ids = rng.randint(0, 2 ** 62, B).astype(np.uint64) * np.uint64(3)       # beyond 2^63 too
    seed, step = 0xDEADBEEFCAFE, 41
    masks = [ref.dropout_factors(T, p_drop, p_rec, seed, step, int(i)) for i in ids]
    l64, g64, ml, mg = _reference(("drop", p_drop, p_rec) + shape, w, x, labels, sw.astype(np.float32), masks)
    got_l, got_g = _Grad(w, F, C)(x, labels, sw, ids, _opts(p_drop, p_rec, seed, step))
    _hold(got_l, got_g, F, C, l64, g64, ml, mg)


def test_zero_rates_give_the_bits_of_no_options():
    T, F, C, B = 5, 12, 7, 4
    w, x, labels = _case(T, F, C, B)
    run = _Grad(w, F, C)
    a = run(x, labels)
    b = run(x, labels, opts=_opts(0.0, 0.0, 9, 4))
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    c = run(x, labels, opts=_opts(0.2, 0.2, 9, 4))
    assert not np.array_equal(a[0], c[0])                # and the rates do something


def test_invariances():
    """Bit-equal: the same call twice; l_b of a window alone, in a batch of 5 and at another place
    with the same sample id (dropout on); a weight-0 window and an out-of-range label."""
    import torch
    from islpose.train import SignTrainer
    T, F, C = 20, 156, 167
    w, x, labels = _case(T, F, C, 6)
    tr = SignTrainer(w, F, C, p_drop=0.2, p_rec=0.2, seed=3)
    ids = np.array([11, 12, 13, 14, 15], np.uint64)
    l1, g1 = tr.loss_and_grad(x[:5], labels[:5], ids=ids)
    l2, g2 = tr.loss_and_grad(x[:5], labels[:5], ids=ids)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    alone, _ = tr.loss_and_grad(x[2:3], labels[2:3], ids=ids[2:3])
    assert torch.equal(alone[0], l1[2])
    order = [4, 3, 0, 1, 2]
    moved, _ = tr.loss_and_grad(x[order], labels[order], ids=ids[order])
    assert torch.equal(moved[4], l1[2]) and torch.equal(moved[0], l1[4])
    other, _ = tr.loss_and_grad(x[2:3], labels[2:3], ids=np.array([99], np.uint64))
    assert not torch.equal(other[0], l1[2])              # another id draws other masks
    # an ignored window: weight 0 == label outside [0, C), at the same B
    sw = np.array([1, 1, 0, 1, 1], np.float32)
    _, g_w0 = tr.loss_and_grad(x[:5], labels[:5], weights=sw, ids=ids)
    for bad in (-1, C, 2 ** 31 - 1):
        lab = torch.from_numpy(labels[:5].copy())
        lab[2] = bad
        l_ig, g_ig = tr.loss_and_grad(x[:5], lab, ids=ids)
        assert torch.equal(g_ig, g_w0)
        assert float(l_ig[2]) == 0.0 and torch.equal(l_ig[[0, 1, 3, 4]], l1[[0, 1, 3, 4]])
    assert not torch.equal(g_w0, g1)


def _loss_against_inference(w, x, F, C):
    """|exp(-l_b) - p[label]| / p[label] per window, train=False, and l_b."""
    from islpose.train import SignTrainer
    B = len(x)
    labels = np.random.RandomState(2).randint(0, C, B)
    tr = SignTrainer(w, F, C)
    loss, _ = tr.loss_and_grad(x, labels, train=False)
    loss = loss.cpu().numpy().astype(np.float64)
    p = tr.classifier()(x).cpu().numpy().astype(np.float64)[np.arange(B), labels]
    return np.abs(np.exp(-loss) - p) / p, loss


def test_loss_agrees_with_inference():
    """exp(-l_b) with train=False against isl_sign_classify's p[label], to 1e-6 relative."""
    T, F, C, B = 20, 156, 167, 37
    w = ref.trained_like_weights(F, C)
    x = ref.windows_like(B, T, F)
    x[5] = 0
    rel, _ = _loss_against_inference(w, x, F, C)
    print("max rel %.3g" % rel.max())
    assert rel.max() <= 1e-6


def test_loss_agrees_with_inference_on_dense_weights():
    """The same on the classifier tests' dense weights and signed windows (b3 != 0, l_b up to 14)."""
    T, F, C, B = 20, 156, 167, 37
    rel, loss = _loss_against_inference(dense.dense_weights(F, C, seed=3), dense.windows(B, T, F, seed=0), F, C)
    print("max rel %.3g at l_b %.3g; l_b up to %.3g" % (rel.max(), loss[rel.argmax()], loss.max()))
    assert rel.max() <= 1e-6


def test_refused_calls_leave_the_outputs_intact():
    """Every ISL_E_ARG case returns before any device work: d_loss, d_grad and the workspace keep
    their canaries (checked in _Grad); batch 0 writes a zero gradient."""
    from islpose import runtime as rt
    T, F, C, B = 5, 12, 7, 4
    w, x, labels = _case(T, F, C, B)
    run = _Grad(w, F, C)
    E = rt.ISL_E_ARG
    for name in ("params", "x", "labels", "loss", "grad", "work"):
        run(x, labels, expect=E, null=(name,))
    for kw in (dict(T=0), dict(T=33), dict(F=0), dict(F=257), dict(C=0), dict(C=1025), dict(batch=-1)):
        run(x, labels, expect=E, **kw)
    for p_drop, p_rec in ((0.95, 0.2), (0.2, -0.1), (float("nan"), 0.2), (0.2, float("inf"))):
        run(x, labels, expect=E, opts=_opts(p_drop, p_rec))
    o = _opts(0.2, 0.2)
    o.reserved[1] = 1
    run(x, labels, expect=E, opts=o)
    n = ctypes.c_int64(-1)
    assert rt.lib().isl_sign_grad_workspace(F, C, -1, ctypes.byref(n)) == E
    assert rt.lib().isl_sign_grad_workspace(300, C, 4, ctypes.byref(n)) == E and n.value == -1
    d = rt.IslSignTrainOpts()
    rt.check(rt.lib().isl_sign_train_opts_default(ctypes.byref(d)))
    assert (round(d.p_drop, 6), round(d.p_rec, 6), d.seed, d.step, list(d.reserved)) == (0.2, 0.2, 0, 0, [0] * 4)
    assert rt.lib().isl_sign_train_opts_default(None) == E
    loss, grad = run(x[:0], labels[:0])
    assert loss.size == 0 and not grad.view(np.int32).any()


def test_it_learns():
    """SignTrainer.fit on the seeded toy set of _sign_train_ref.toy_set (4 classes, 8 windows each,
    T 8, F 12, a 20 % masked-frame share, prototypes TOY_SEP * 100 px apart per entry under
    TOY_NOISE * 100 px of noise), dropout 0.2 / 0.2, Adam at TOY_LR, full-batch steps: within
    TOY_STEPS steps the training loss falls to a quarter of the first step's and every held-out draw
    (another seed) is classified right.  The untrained weights get the held-out draws wrong.
    Chosen on the CPU: the float64 statement with the same optimizer and masks meets both conditions
    by TOY_STEPS / 2: its loss with dropout goes 1.331 (step 0), 0.657 (5), 0.204 (10: under a
    quarter of the first), 0.080 (15), 0.020 (20); its held-out accuracy is 0.625 untrained and 1.0
    from step 5 on.  At prototypes as far apart as the noise (0.3 / 0.3) it stays at 31 of 32."""
    from islpose.train import SignTrainer
    x, y = ref.toy_set(8, seed=1, sep=TOY_SEP, noise=TOY_NOISE)
    xh, yh = ref.toy_set(8, seed=2, sep=TOY_SEP, noise=TOY_NOISE)
    tr = SignTrainer(None, 12, 4, p_drop=0.2, p_rec=0.2, seed=0, lr=TOY_LR)
    tr.calibrate_bn0(x)
    assert tr.evaluate(xh, yh)[1] < 1.0
    hist = tr.fit(x, y, TOY_STEPS, batch=32, val=(xh, yh))
    print([(h["epoch"], round(h["loss"], 4), h["val_acc"]) for h in hist])
    assert tr.step_count == TOY_STEPS
    assert hist[-1]["loss"] <= 0.25 * hist[0]["loss"]
    assert hist[-1]["val_acc"] == 1.0


TOY_SEP, TOY_NOISE, TOY_LR, TOY_STEPS = 0.45, 0.3, 3e-3, 20


def test_save_round_trip(tmp_path):
    """save -> SignClassifier(path) gives the trainer's classifier() probabilities bit for bit."""
    import torch
    from islpose.train import SignTrainer
    from islpose.translate import SignClassifier
    T, F, C, B = 20, 156, 167, 6
    w, x, labels = _case(T, F, C, B)
    tr = SignTrainer(w, F, C, seed=1)
    tr.step(x, labels)
    tr.step(x, labels)
    assert tr.step_count == 2
    assert not np.array_equal(tr.weights()[4], w[4])           # the steps moved the weights
    for k in ref.STAT_SLOTS:
        np.testing.assert_array_equal(tr.weights()[k], w[k])   # and left the statistics alone
    path = str(tmp_path / "w.npz")
    tr.save(path)
    back = SignClassifier(path, F, C)
    assert torch.equal(back(x), tr.classifier()(x))
    assert [a.shape for a in tr.weights()] == [np.shape(a) for a in w] and len(tr.weights()) == 28
