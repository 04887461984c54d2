"""An independent statement of the sign classifier's training step, for
the tests of csrc/sign_train.hip: torch on the CPU, float64 by default, one window and one step at
a time, gradients from torch.autograd.  The dropout factors are inputs; `dropout_factors` makes
them with a numpy statement of the counter-based hash.

    Masking(0) -> BN0 -> BiLSTM1(sequences) -> Dropout_A -> BiLSTM2 -> elu -> Dense d1 -> BN1
    -> Dropout_B -> elu -> Dense d2 -> BN2 -> elu -> Dropout_C -> Dense d3 + b3 -> softmax

The batch normalisations use their stored statistics; `loss_and_grads` returns zeros for the six
mean / variance arrays (frozen), unless zero_stats=False (the finite-difference test reads them).
"""
import numpy as np
import torch

UNITS = 32
STAT_SLOTS = (2, 3, 19, 20, 24, 25)     # moving mean / variance in keras get_weights() order
BN_EPS = 1e-3


# ------------------------------------------------------------------ the hash
def sm(z):
    """splitmix64 finaliser on a numpy uint64 array (wrapping arithmetic)."""
    z = np.atleast_1d(np.asarray(z, np.uint64)) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw(seed, step, sample_id, site, index):
    """k of the definition for every entry of `index`, uint64."""
    k = sm(np.uint64(seed) ^ np.uint64(step))
    k = sm(k ^ np.uint64(sample_id))
    return sm(k ^ (np.uint64(site) << np.uint64(32) | np.atleast_1d(np.asarray(index, np.uint64))))


def threshold(rate):
    """round(rate * 2^24) of the fp32 rate (the product is exact; halves round up)."""
    return int(np.floor(np.float64(np.float32(rate)) * 2.0 ** 24 + 0.5))


def keep(rate, seed, step, sample_id, site, index):
    return (draw(seed, step, sample_id, site, index) >> np.uint64(40)) >= np.uint64(threshold(rate))


def factors(rate, seed, step, sample_id, site, n):
    """The n multipliers of a site: fp32 1 / (1 - rate) where kept, 0 where dropped; rate 0: ones."""
    if threshold(rate) == 0:
        return np.ones(n)
    scale = np.float64(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))
    return np.where(keep(rate, seed, step, sample_id, site, np.arange(n)), scale, 0.0)


def dropout_factors(T, p_drop, p_rec, seed, step, sample_id):
    """A [T, 64], B [32], C [32], R [4, 32] (layer-1 forward, backward, layer-2 forward, backward)."""
    return {"A": factors(p_drop, seed, step, sample_id, 0, T * 2 * UNITS).reshape(T, 2 * UNITS),
            "B": factors(p_drop, seed, step, sample_id, 1, UNITS),
            "C": factors(p_drop, seed, step, sample_id, 2, UNITS),
            "R": np.stack([factors(p_rec, seed, step, sample_id, 3 + k, UNITS) for k in range(4)])}


def no_dropout(T):
    return {"A": np.ones((T, 2 * UNITS)), "B": np.ones(UNITS), "C": np.ones(UNITS), "R": np.ones((4, UNITS))}


# ------------------------------------------------------------------ the model
def _elu(v):
    return torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0)))


def _bn(v, p):
    gamma, beta, mean, var = p
    return (v - mean) / torch.sqrt(var + BN_EPS) * gamma + beta


def _lstm(x, mask, K, R, b, reverse, rm):
    """x [T, Fin] -> (sequence [T, U] with zeros at masked steps, last carried h); rm multiplies
    h_{t-1} before the recurrent product (one recurrent-dropout mask held over the steps)."""
    T = x.shape[0]
    h = torch.zeros(UNITS, dtype=x.dtype)
    c = torch.zeros(UNITS, dtype=x.dtype)
    rows = [torch.zeros(UNITS, dtype=x.dtype)] * T
    for s in range(T):
        t = T - 1 - s if reverse else s
        if not mask[t]:
            continue                                   # a masked step carries (h, c) and emits zeros
        z = x[t] @ K + (h * rm) @ R + b
        i, f, g, o = (z[k * UNITS:(k + 1) * UNITS] for k in range(4))
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        rows[t] = h
    return torch.stack(rows), h


def logits(w, window, m):
    """w: the 28 tensors; window [T, F] tensor; m: dropout factors as tensors -> logits [C]."""
    mask = (window != 0).any(dim=1)
    x = _bn(window, w[0:4])
    f1, _ = _lstm(x, mask, w[4], w[5], w[6], False, m["R"][0])
    b1, _ = _lstm(x, mask, w[7], w[8], w[9], True, m["R"][1])
    y = torch.cat([f1, b1], dim=1) * m["A"]
    _, hf = _lstm(y, mask, w[10], w[11], w[12], False, m["R"][2])
    _, hb = _lstm(y, mask, w[13], w[14], w[15], True, m["R"][3])
    v = _elu(torch.cat([hf, hb]))
    v = _elu(_bn(v @ w[16], w[17:21]) * m["B"])
    v = _elu(_bn(v @ w[21], w[22:26])) * m["C"]
    return v @ w[26] + w[27]


def loss_and_grads(weights, windows, labels, sample_weights=None, masks=None, dtype=torch.float64,
                   zero_stats=True):
    """l_b [B] and dL/dtheta (28 arrays) of L = (1 / B) sum_b w_b l_b, numpy float64.  A label
    outside [0, C) ignores its window.  masks: one dropout_factors dict per window, None for none."""
    w = [torch.tensor(np.asarray(a, np.float64)).to(dtype).requires_grad_(True) for a in weights]
    B, T = len(windows), np.shape(windows)[1]
    C = w[27].shape[0]
    total = torch.zeros((), dtype=dtype)
    losses = []
    for b in range(B):
        m = {k: torch.tensor(v).to(dtype) for k, v in (masks[b] if masks is not None else no_dropout(T)).items()}
        z = logits(w, torch.tensor(np.asarray(windows[b], np.float64)).to(dtype), m)
        if 0 <= int(labels[b]) < C:
            l = torch.logsumexp(z, 0) - z[int(labels[b])]
            sw = 1.0 if sample_weights is None else float(sample_weights[b])
            total = total + sw * l
            losses.append(float(l.detach()))
        else:
            losses.append(0.0)
    total = total / B
    if total.requires_grad:
        total.backward()
    grads = [np.zeros(tuple(p.shape)) if p.grad is None else p.grad.double().numpy() for p in w]
    if zero_stats:
        for k in STAT_SLOTS:
            grads[k] = np.zeros_like(grads[k])
    return np.array(losses), grads


def batch_loss(weights, windows, labels, sample_weights=None, masks=None):
    """L alone, float64 (finite differences)."""
    w = [torch.tensor(np.asarray(a, np.float64)) for a in weights]
    T = np.shape(windows)[1]
    total = 0.0
    for b in range(len(windows)):
        m = {k: torch.tensor(v) for k, v in (masks[b] if masks is not None else no_dropout(T)).items()}
        z = logits(w, torch.tensor(np.asarray(windows[b], np.float64)), m)
        if 0 <= int(labels[b]) < w[27].shape[0]:
            sw = 1.0 if sample_weights is None else float(sample_weights[b])
            total += sw * float(torch.logsumexp(z, 0) - z[int(labels[b])])
    return total / len(windows)


# ------------------------------------------------------------------ the tests' data
def trained_like_weights(F=156, K=167, seed=3):
    """tests/test_translate.py's _trained_like_weights recipe: keras default initialisers plus BN
    statistics of pixel-scale features, so the LSTMs see unit-scale inputs."""
    from islpose import translate
    w = translate.keras_default_weights(F, K, seed)
    rng = np.random.RandomState(seed + 1)
    w[0] = rng.uniform(0.5, 1.5, F).astype(np.float32)
    w[1] = rng.uniform(-0.2, 0.2, F).astype(np.float32)
    w[2] = rng.uniform(0, 300, F).astype(np.float32)
    w[3] = rng.uniform(50, 200, F).astype(np.float32) ** 2
    for base in (17, 22):
        w[base:base + 4] = [rng.uniform(0.5, 1.5, 32).astype(np.float32), rng.uniform(-.2, .2, 32).astype(np.float32),
                            rng.uniform(-.3, .3, 32).astype(np.float32), rng.uniform(0.5, 2, 32).astype(np.float32)]
    return w


def windows_like(B, T=20, F=156, seed=0, masked=0.25):
    """tests/test_translate.py's _windows recipe: pixel-scale features, missing joints, empty frames."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 600, (B, T, F)).astype(np.float32)
    lo = min(30, F // 2)
    x[:, :, lo:] = np.where(rng.rand(B, T, F - lo) < 0.3, 0, x[:, :, lo:])
    x[rng.rand(B, T) < masked] = 0
    return x


def toy_set(n_per_class, seed, classes=4, T=8, F=12, sep=0.35, noise=1.0, masked=0.2, proto_seed=11):
    """The seeded toy set of the learning test: class prototypes [T, F] around 300 px, `sep` * 100 px
    apart per entry, plus noise of `noise` * 100 px; a `masked` share of the frames is empty.
    Returns (windows [n, T, F] fp32, labels [n] int32)."""
    proto = 300.0 + 100.0 * sep * np.random.RandomState(proto_seed).standard_normal((classes, T, F))
    rng = np.random.RandomState(seed)
    y = np.repeat(np.arange(classes), n_per_class).astype(np.int32)
    x = proto[y] + 100.0 * noise * rng.standard_normal((len(y), T, F))
    x[rng.rand(len(y), T) < masked] = 0
    return x.astype(np.float32), y
