"""An independent statement of the sign classifier at inference (csrc/sign.hip, DESIGN.md section
4.2n), written from the keras layer semantics in numpy, with a dtype switch and local mutations.
It shares no code with oracle/sign_classifier.py; tests/test_sign_ref.py holds the two together.

    Masking(0) -> BN0 -> BiLSTM1(sequences) -> BiLSTM2 -> elu -> Dense d1 -> BN1 -> elu
    -> Dense d2 -> BN2 -> elu -> Dense d3 + b3 -> softmax            (dropouts: identity)

Masking: a step is present when any feature != 0 (so a negative feature counts and -0.0 does not).
A masked step carries (h, c); the return_sequences layer emits zeros there; the backward direction
walks the window in reverse and stores its output at the time index; the mask reaches layer 2.
LSTM cell, gate order i, f, c, o: z = x K + h R + b; c' = sig(f) c + sig(i) tanh(z_c);
h' = sig(o) tanh(c').  BN: (x - mean) / sqrt(var + 1e-3) * gamma + beta.

With dtype=np.float32 every intermediate is float32 (numpy keeps float32 under python scalars);
that run against the float64 one is the measure E of what fp32 arithmetic costs, and the bar of the
GPU test is M = min(4 * max(E, 2e-7), 1e-4), relative per element (`bar`).

`MUTATIONS` names locally wrong statements.  Each is what a plausible kernel slip would compute;
tests/test_sign_ref.py proves that every one breaks M by >= 10 x on every case it applies to, and
that `EQUIVALENT` (a masked step of layer 1 emitting the carried h) changes no bit: layer 2 never
reads a masked row.
"""
import numpy as np

UNITS = 32
M_FACTOR, M_FLOOR, M_CAP = 4.0, 2e-7, 1e-4
P_MIN = 1e-30                       # every reference probability of every case is above this
EQUIVALENT = "masked_emits_h"

# name -> what goes wrong
MUTATIONS = {
    "bn_eps": "batch normalisation with eps 1e-5 instead of 1e-3",
    "k1_entry": "K1_fwd[F-1, 5] = 0",
    "r2_entry": "R2_bwd[31, 127] = 0",
    "b1_step8": "layer-1 bias missing at step min(8, T-1), the first step of the second step range",
    "b1_roll_in_gate": "layer-1 forward bias rolled by one row inside each gate block",
    "b2_roll": "layer-2 backward bias rolled by one row (across the gate blocks)",
    "swap_if": "i and f swapped in layer 2 backward",
    "bwd_at_walk": "layer-1 backward sequence stored at the walk index, not flipped back",
    "mask_resets": "a masked step resets (h, c)",
    "l2_no_mask": "layer 2 ignores the mask",
    "mask_gt": "mask from x > 0",
    "mask_skips_last": "mask ignoring the last feature",
    "b3_last": "b3 missing on the last class",
    "b3_256": "class 256 takes class 0's b3",
    "softmax_no_max": "softmax without subtracting the max",
    "c_carried": "c not reset between the layers",
    "last_step_h": "the last step's h (zeros when masked) in place of the last carried h",
    EQUIVALENT: "a masked step of the return_sequences layer emits the carried h (unobservable)",
}


def applies(mutation, T, F, C, designed=True):
    """Whether `mutation` can change the result of a `windows` batch of this shape at all."""
    if C == 1 or mutation == EQUIVALENT:
        return False                          # one class: the row is 1 whatever the logit
    if mutation == "softmax_no_max":
        return False                          # shows only where expf overflows: the shifted case, in float32
    if mutation == "b3_256":
        return C > 256
    if mutation == "b1_step8":
        return T > 8
    if mutation in ("r2_entry", "bwd_at_walk"):
        return T >= 2                         # the first step's h is 0; one step has one index
    if mutation in ("mask_resets", "l2_no_mask", "mask_gt", "mask_skips_last", "last_step_h"):
        return designed                       # they need the designed rows of `windows`
    return True


# ------------------------------------------------------------------ the model
def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def _elu(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))


def _bn(v, p, eps):
    gamma, beta, mean, var = p
    return (v - mean) / np.sqrt(var + eps) * gamma + beta


def _lstm(x, mask, K, R, b, reverse, dt, c0=None, swap_if=False, at_walk=False, resets=False,
          emits_h=False, no_bias_at=None):
    """x [T, Fin] -> (sequence [T, U], last carried h, h of the last walk step, last c)."""
    T = x.shape[0]
    h = np.zeros(UNITS, dt)
    c = np.zeros(UNITS, dt) if c0 is None else c0
    seq = np.zeros((T, UNITS), dt)
    last = np.zeros(UNITS, dt)
    for s in range(T):
        t = T - 1 - s if reverse else s
        if not mask[t]:
            if resets:
                h, c = np.zeros(UNITS, dt), np.zeros(UNITS, dt)
            if emits_h:
                seq[s if at_walk else t] = h
            last = np.zeros(UNITS, dt)
            continue
        z = x[t] @ K + h @ R
        if t != no_bias_at:
            z = z + b
        i, f, g, o = (z[k * UNITS:(k + 1) * UNITS] for k in range(4))
        if swap_if:
            i, f = f, i
        c = _sigmoid(f) * c + _sigmoid(i) * np.tanh(g)
        h = _sigmoid(o) * np.tanh(c)
        seq[s if at_walk else t] = h
        last = h
    return seq, h, last, c


def classify(weights, window, dtype=np.float64, mutation=None, d3_order=None):
    """weights: the 28 keras get_weights() arrays; window [T, F] -> (probabilities [C], logits [C]),
    both of `dtype`.  mutation: a key of MUTATIONS or None.  d3_order: None for v @ d3 + b3;
    "bias_first" / "bias_last" sum the 32 products of a logit one by one in `dtype`, from b3 or
    from 0 with b3 added at the end (the kernel's order before and after section 4.2n's finding)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    dt = np.dtype(dtype).type
    m = mutation
    w = [np.array(a, dtype=dt) for a in weights]
    x = np.asarray(window, dtype=dt)
    T, F = x.shape
    C = w[27].shape[0]
    eps = dt(1e-5 if m == "bn_eps" else 1e-3)

    if m == "mask_gt":
        mask = np.any(x > 0, axis=1)
    elif m == "mask_skips_last":
        mask = np.any(x[:, :F - 1] != 0, axis=1)
    else:
        mask = np.any(x != 0, axis=1)
    if m == "k1_entry":
        w[4][F - 1, 5] = 0
    if m == "r2_entry":
        w[14][31, 127] = 0
    if m == "b1_roll_in_gate":
        w[6] = np.roll(w[6].reshape(4, UNITS), 1, axis=1).ravel()
    if m == "b2_roll":
        w[15] = np.roll(w[15], 1)
    if m == "b3_last":
        w[27][C - 1] = 0
    if m == "b3_256" and C > 256:
        w[27][256] = w[27][0]

    x = _bn(x, w[0:4], eps)
    off = min(8, T - 1) if m == "b1_step8" else None
    f1, _, _, cf = _lstm(x, mask, w[4], w[5], w[6], False, dt, resets=m == "mask_resets",
                         emits_h=m == EQUIVALENT, no_bias_at=off)
    b1, _, _, cb = _lstm(x, mask, w[7], w[8], w[9], True, dt, resets=m == "mask_resets",
                         emits_h=m == EQUIVALENT, no_bias_at=off, at_walk=m == "bwd_at_walk")
    y = np.concatenate([f1, b1], axis=1)
    mask2 = np.ones(T, bool) if m == "l2_no_mask" else mask
    carried = m == "c_carried"
    _, hf, lf, _ = _lstm(y, mask2, w[10], w[11], w[12], False, dt, c0=cf if carried else None,
                         resets=m == "mask_resets")
    _, hb, lb, _ = _lstm(y, mask2, w[13], w[14], w[15], True, dt, c0=cb if carried else None,
                         resets=m == "mask_resets", swap_if=m == "swap_if")
    v = np.concatenate([lf, lb] if m == "last_step_h" else [hf, hb])
    v = _elu(v)
    v = _elu(_bn(v @ w[16], w[17:21], eps))
    v = _elu(_bn(v @ w[21], w[22:26], eps))
    if d3_order is None:
        logits = v @ w[26] + w[27]
    else:
        logits = w[27].copy() if d3_order == "bias_first" else np.zeros(C, dt)
        for i in range(v.shape[0]):
            logits = logits + v[i] * w[26][i]
        if d3_order == "bias_last":
            logits = logits + w[27]
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(logits if m == "softmax_no_max" else logits - logits.max())
        p = e / e.sum()
    assert p.dtype == dt and logits.dtype == dt
    return p, logits


def classify_batch(weights, windows, dtype=np.float64, mutation=None, d3_order=None):
    """-> (probabilities [B, C], logits [B, C])."""
    out = [classify(weights, wnd, dtype, mutation, d3_order) for wnd in windows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def bar(p32, p64):
    """(E, M): E = max |p32 - p64| / p64 of the float32 statement; M = min(4 max(E, 2e-7), 1e-4).
    4 and 2e-7 are those of tests/test_gpu_sign_train.py (the project's 3 E practice plus room for
    the device's expf / tanhf); 1e-4 is the relative term of the bar this one replaces."""
    e = float(np.max(np.abs(p32.astype(np.float64) - p64) / p64))
    return e, min(M_FACTOR * max(e, M_FLOOR), M_CAP)


# ------------------------------------------------------------------ the tests' data
def dense_weights(F, C, seed, spread=1.0):
    """Weights whose 28 arrays are all non-degenerate: keras' default initialisers, then BN0 with
    the statistics of signed pixel-scale features, every LSTM bias moved per row, the head BNs of
    the older tests' recipe, and a final layer with a bias and logits that spread."""
    from islpose import translate
    w = translate.keras_default_weights(F, C, seed)
    rng = np.random.RandomState(seed + 101)
    f32 = lambda a: np.asarray(a, np.float32)                                   # noqa: E731
    w[0] = f32(rng.uniform(0.5, 1.5, F))
    w[1] = f32(rng.uniform(-0.2, 0.2, F))
    w[2] = f32(rng.uniform(-100, 300, F))
    w[3] = f32(rng.uniform(50, 200, F)) ** 2
    for k in (6, 9, 12, 15):
        w[k] = f32(w[k] + rng.uniform(-0.5, 0.5, 4 * UNITS))
    for base in (17, 22):
        w[base:base + 4] = [f32(rng.uniform(0.5, 1.5, 32)), f32(rng.uniform(-.2, .2, 32)),
                            f32(rng.uniform(-.3, .3, 32)), f32(rng.uniform(0.5, 2, 32))]
    w[26] = f32(w[26] * (8 * spread))
    w[27] = f32(rng.uniform(-2, 2, C) * spread)
    assert all(a.dtype == np.float32 for a in w) and len(w) == 28
    return w


def shifted_pair(w, by=100.0):
    """(base, shifted): `shifted` has b3 + `by` on every class.  b3 of both is first put on the
    2^-16 grid, so that the sum is exact in float32 and the two softmaxes are the same numbers."""
    base = [a.copy() for a in w]
    base[27] = (np.round(base[27].astype(np.float64) * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)
    sh = [a.copy() for a in base]
    sh[27] = (base[27].astype(np.float64) + by).astype(np.float32)
    assert np.array_equal(sh[27].astype(np.float64) - by, base[27].astype(np.float64))
    return base, sh


def designed(B, T):
    return T >= 5 and B >= 4


def windows(B, T, F, seed):
    """[B, T, F] float32: features uniform(-200, 600) (augmented keypoints leave the frame), 30 %
    of the non-body features zeroed, 25 % of the frames empty.  When T >= 5 and B >= 4, windows 0-2
    keep every other frame and get: window 0 a leading masked step and, at step 2, a frame whose
    only nonzero is a negative last feature (present); window 1 an interior masked step and, at
    step 1, a frame of -0.0 (masked); window 2 a trailing masked step; window 3 is all masked."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-200, 600, (B, T, F)).astype(np.float32)
    lo = min(30, F // 2)
    x[:, :, lo:] = np.where(rng.rand(B, T, F - lo) < 0.3, 0, x[:, :, lo:])
    empty = rng.rand(B, T) < 0.25
    if designed(B, T):
        empty[:3] = False
        x[:3, :, 0] = np.where(x[:3, :, 0] == 0, np.float32(-3.5), x[:3, :, 0])   # F 1: nothing zeroed away
    x[empty] = 0
    if designed(B, T):
        x[0, 0] = 0
        x[0, 2] = 0
        x[0, 2, F - 1] = -37.5
        x[1, T // 2] = 0
        x[1, 1] = -0.0
        x[2, T - 1] = 0
        x[3] = 0
        assert np.signbit(x[1, 1]).all() and not x[1, 1].any()
    return x


# ------------------------------------------------------------------ the cases
# (name, T, F, C, B, spread, shift).  tests/test_sign_ref.py holds every one to P_MIN and to the
# fairness of M on the CPU; tests/test_gpu_sign_classify.py runs the kernel on every one.
WIDE_SPREAD = 4.0                   # logit range <= 60 (asserted); 6 gave 81 and p down to 2.4e-33
STEP_T = (1, 7, 8, 9, 16, 17, 24, 25, 31, 32)
PATH_F = (1, 3, 4, 5, 8, 155, 156, 255, 256)
LANE_C = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
CASES = ([("steps-T%d" % T, T, 12, 7, 5, 1.0, 0.0) for T in STEP_T]
         + [("paths-F%d" % F, 9, F, 7, 5, 1.0, 0.0) for F in PATH_F]
         + [("lanes-C%d" % C, 5, 8, C, 5, 1.0, 0.0) for C in LANE_C]
         + [("workload", 20, 156, 167, 6, 1.0, 0.0), ("limits", 32, 256, 1024, 5, 1.0, 0.0),
            ("odd", 7, 10, 3, 6, 1.0, 0.0), ("c257", 9, 5, 257, 6, 1.0, 0.0),
            ("wide", 20, 156, 167, 6, WIDE_SPREAD, 0.0), ("shifted", 9, 12, 65, 6, 1.0, 100.0)])
CASE_IDS = [c[0] for c in CASES]
# where every mutation is held to its factor (the statement's cost is per mutation and window)
SHARP = ("workload", "odd", "limits", "c257", "wide")

_cache = {}


def case(name):
    """dict(name, T, F, C, B, w, x, p64, z64, p32, E, M [, base_w, base_p64]) of a case, made once
    and left unchanged."""
    if name not in _cache:
        _, T, F, C, B, spread, shift = CASES[CASE_IDS.index(name)]
        seed = 1000 * T + 7 * F + C
        w = dense_weights(F, C, seed, spread)
        extra = {}
        if shift:
            base, w = shifted_pair(w, shift)
            extra = {"base_w": base, "base_p64": classify_batch(base, windows(B, T, F, seed + 1))[0]}
        x = windows(B, T, F, seed + 1)
        p64, z64 = classify_batch(w, x)
        p32, _ = classify_batch(w, x, np.float32)
        E, M = bar(p32, p64)
        _cache[name] = dict(name=name, T=T, F=F, C=C, B=B, w=w, x=x, p64=p64, z64=z64, p32=p32, E=E, M=M, **extra)
    return _cache[name]
