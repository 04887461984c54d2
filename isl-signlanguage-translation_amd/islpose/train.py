"""Training of the sign classifier on one GPU (csrc/sign_train.hip, ``isl_sign_grad``).

``SignTrainer`` holds the parameters of ``SignClassifier``'s model as one flat fp32 tensor on the
device (keras ``get_weights()`` order).  The forward pass with the training-time Dropouts, the
sparse categorical cross-entropy and the backward pass through time are one HIP call; PyTorch
supplies the optimizer and the tensors.  DESIGN.md section 4.2k holds the definition.  Two
deliberate deviations from ``keras.Model.fit``: the batch normalisations use their stored moving
statistics (BN0's are set from the data by ``calibrate_bn0``), and recurrent dropout draws one mask
per direction and window.  ``step`` / ``fit`` / ``fit_clips`` take ``augment=``, a
``sign_augment.WindowAugment`` that redraws every batch in keypoint space by one more launch
(DESIGN.md section 4.2m).

Without libislpose.so or a GPU this raises like the rest of the product layer: no CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .runtime import IslSignTrainOpts, check, lib, ptr, stream_handle
from .translate import N_CLASSES, N_FEATURES, SignClassifier, keras_weight_shapes

MAX_WINDOW, MAX_FEATURES, MAX_CLASSES = 32, 256, 1024     # the limits of isl_sign_classify
MAX_RATE = 0.9


def check_rate(name, rate):
    """A dropout rate as a float; ValueError unless it is a number in [0, 0.9]."""
    try:
        r = float(rate)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number in [0, %g], got %r" % (name, MAX_RATE, rate))
    if not (0.0 <= r <= MAX_RATE) or np.float32(r) > np.float32(MAX_RATE):
        raise ValueError("%s must be in [0, %g], got %r" % (name, MAX_RATE, rate))
    return r


def check_sizes(n_features, n_classes):
    if not 1 <= int(n_features) <= MAX_FEATURES or not 1 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError("n_features must be in [1, %d] and n_classes in [1, %d], got %r and %r"
                         % (MAX_FEATURES, MAX_CLASSES, n_features, n_classes))


def check_windows_shape(shape, n_features):
    if len(shape) != 3 or shape[2] != n_features or not 1 <= shape[1] <= MAX_WINDOW:
        raise ValueError("windows must be [B, T <= %d, %d], got %s" % (MAX_WINDOW, n_features, tuple(shape)))


def check_labels(labels, batch, n_classes):
    """Labels given as numpy (or a sequence): an integer dtype, shape [batch], every label in
    [0, n_classes) or negative (a negative label ignores its window).  Returns int32."""
    lab = np.asarray(labels)
    if lab.dtype.kind not in "iu":
        raise ValueError("labels must have an integer dtype, got %s" % lab.dtype)
    if lab.shape != (batch,):
        raise ValueError("labels must be [%d], got %s" % (batch, lab.shape))
    if lab.size and int(lab.max()) >= n_classes:
        raise ValueError("label %d is outside [0, %d)" % (int(lab.max()), n_classes))
    if lab.size and int(lab.min()) < -2 ** 31:
        raise ValueError("label %d does not fit int32" % int(lab.min()))
    return lab.astype(np.int32)


def bn0_statistics(windows):
    """Mean and variance per feature over the unmasked rows (not all zero) of [N, T, F] windows,
    float64 numpy; with no unmasked row: mean 0 and variance 1."""
    x = np.asarray(windows, np.float64)
    rows = x.reshape(-1, x.shape[-1])
    rows = rows[np.any(rows != 0, axis=1)]
    if not len(rows):
        return np.zeros(x.shape[-1]), np.ones(x.shape[-1])
    return rows.mean(axis=0), rows.var(axis=0)


class SignTrainer:
    """Trains the reference's translation model (demo_isl_translate.py:72-100) on one GPU.

    weights: None (keras' default initialisers from `seed`), the 28 keras-ordered arrays, or the
    path of an ``np.savez(path, *model.get_weights())`` file.  optimizer: None for
    ``torch.optim.Adam([params], lr, eps=1e-7)`` (keras' defaults), or a callable that takes the
    list ``[params]`` and returns any torch optimizer over that one tensor, e.g.
    ``lambda p: torch.optim.SGD(p, lr=0.1, momentum=0.9)`` (the tensor exists only once the trainer
    does; ``trainer.optimizer`` may also be replaced later)."""

    def __init__(self, weights=None, n_features: int = N_FEATURES, n_classes: int = N_CLASSES, p_drop: float = 0.2,
                 p_rec: float = 0.2, seed: int = 0, lr: float = 1e-3, optimizer=None, device=None):
        self.p_drop, self.p_rec = check_rate("p_drop", p_drop), check_rate("p_rec", p_rec)
        check_sizes(n_features, n_classes)
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
        import torch
        self.seed, self.step_count = int(seed), 0
        # the classifier checks the weights and owns the flat device vector; the trainer shares it
        self._clf = SignClassifier(weights, n_features, n_classes, device, int(seed) % 2 ** 32)
        self.device, self.n_features, self.n_classes = self._clf.device, n_features, n_classes
        self.params = self._clf.params
        self.shapes = keras_weight_shapes(n_features, n_classes)
        self.optimizer = (torch.optim.Adam([self.params], lr=lr, eps=1e-7) if optimizer is None
                          else optimizer([self.params]))
        self._ws = None

    # ------------------------------------------------------------------ one step
    def _device_inputs(self, windows, labels, weights, ids):
        import torch
        x = windows if isinstance(windows, torch.Tensor) else torch.from_numpy(np.asarray(windows, np.float32))
        check_windows_shape(tuple(x.shape), self.n_features)
        B = x.shape[0]
        x = x.to(self.device, torch.float32).contiguous()
        if isinstance(labels, torch.Tensor):
            if labels.dtype.is_floating_point or tuple(labels.shape) != (B,):
                raise ValueError("labels must be an integer tensor [%d], got %s %s" % (B, labels.dtype, tuple(labels.shape)))
            lab = labels.to(self.device, torch.int32).contiguous()
        else:
            lab = torch.from_numpy(check_labels(labels, B, self.n_classes)).to(self.device)
        w = i = None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.asarray(weights, np.float32))
            if tuple(w.shape) != (B,):
                raise ValueError("weights must be [%d], got %s" % (B, tuple(w.shape)))
            w = w.to(self.device, torch.float32).contiguous()
        if ids is not None:
            if isinstance(ids, torch.Tensor):
                i = ids.to(self.device, torch.int64).contiguous()       # the same 64 bits
            else:
                i = torch.from_numpy(np.asarray(ids).astype(np.uint64).view(np.int64)).to(self.device)
            if tuple(i.shape) != (B,):
                raise ValueError("ids must be [%d], got %s" % (B, tuple(i.shape)))
        return x, lab, w, i

    def _workspace(self, batch):
        import torch
        n = ctypes.c_int64()
        check(lib().isl_sign_grad_workspace(self.n_features, self.n_classes, batch, ctypes.byref(n)),
              "isl_sign_grad_workspace")
        if self._ws is None or self._ws.numel() * 4 < n.value:
            self._ws = torch.empty(max(1, n.value // 4), dtype=torch.float32, device=self.device)
        return self._ws

    def loss_and_grad(self, windows, labels, weights=None, ids=None, train=True):
        """(l_b [B], dL/dtheta [P]) of one batch, torch float32 on the device: one isl_sign_grad on
        the current stream, no host synchronisation.  train=False: no dropout."""
        import torch
        x, lab, w, i = self._device_inputs(windows, labels, weights, ids)
        B = x.shape[0]
        loss = torch.empty(B, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(self.params)
        opts = None
        if train:
            opts = IslSignTrainOpts(self.p_drop, self.p_rec, self.seed, self.step_count)
        with torch.cuda.device(self.device):
            ws = self._workspace(B)
            check(lib().isl_sign_grad(ptr(self.params), self.n_features, x.shape[1], self.n_classes, ptr(x), ptr(lab),
                                      ptr(w), ptr(i), B, None if opts is None else ctypes.byref(opts), ptr(loss),
                                      ptr(grad), ptr(ws), stream_handle()), "isl_sign_grad")
        return loss, grad

    def _augmented(self, augment, rows, idx, window, nrows, row0, base=0):
        """The batch `idx` (numpy dataset indices, the dropout's ids) as windows built by `augment`
        from the resident rows [n_rows, F]: items of this trainer's seed and step_count."""
        items = augment.items(idx, self.step_count, nrows, row0, base, seed=self.seed)
        return augment.apply(rows, items, window, self.step_count, seed=self.seed)

    def step(self, windows, labels, weights=None, ids=None, augment=None):
        """One optimizer step on a batch; returns l_b [B] (with this step's dropout masks).
        augment: a sign_augment.WindowAugment; the batch is then its view of `windows` (window b is
        the source of item b, drawn with the dropout's ids, this trainer's seed and step_count)."""
        if augment is not None:
            import torch
            x = windows if isinstance(windows, torch.Tensor) else torch.from_numpy(np.asarray(windows, np.float32))
            check_windows_shape(tuple(x.shape), self.n_features)
            x = x.to(self.device, torch.float32).contiguous()
            B, T, F = x.shape
            if ids is None:
                idx = np.arange(B, dtype=np.uint64)
            else:
                idx = np.asarray(ids.cpu() if hasattr(ids, "cpu") else ids).astype(np.uint64)
            if idx.shape != (B,):
                raise ValueError("ids must be [%d], got %s" % (B, idx.shape))
            windows = self._augmented(augment, x.view(B * T, F), idx, T, T, np.arange(B, dtype=np.int64) * T)
        loss, grad = self.loss_and_grad(windows, labels, weights, ids, train=True)
        self.params.grad = grad
        self.optimizer.step()
        self.step_count += 1
        return loss

    # ------------------------------------------------------------------ a run
    def calibrate_bn0(self, windows):
        """Set the first batch normalisation's moving mean and variance from the unmasked rows."""
        import torch
        x = windows.detach().cpu().numpy() if isinstance(windows, torch.Tensor) else np.asarray(windows)
        check_windows_shape(x.shape, self.n_features)
        mean, var = bn0_statistics(x)
        F = self.n_features
        stats = torch.from_numpy(np.concatenate([mean, var]).astype(np.float32)).to(self.device)
        with torch.no_grad():
            self.params[2 * F:4 * F] = stats

    def evaluate(self, windows, labels, batch=256):
        """(mean loss, accuracy) through isl_sign_classify, as Python floats."""
        x = np.asarray(windows, np.float32)
        lab = check_labels(labels, len(x), self.n_classes)
        clf = self.classifier()
        nll, hit, n = 0.0, 0, 0
        for s in range(0, len(x), batch):
            p = clf(x[s:s + batch]).cpu().numpy().astype(np.float64)
            y = lab[s:s + batch]
            keep = y >= 0
            nll += float(-np.log(np.maximum(p[keep, y[keep]], 1e-45)).sum())
            hit += int((p[keep].argmax(1) == y[keep]).sum())
            n += int(keep.sum())
        return (nll / n, hit / n) if n else (0.0, 0.0)

    def fit(self, windows, labels, epochs, batch=256, val=None, shuffle_seed=0, augment=None):
        """`epochs` passes over [N, T, F] windows in batches of `batch`, reshuffled per epoch from
        shuffle_seed; the dropout ids are the dataset indices.  val: (windows, labels) or None
        (never augmented).  augment: a sign_augment.WindowAugment; every batch is then built by its
        one launch from the resident windows (window i is the source of item i: row0 = i * T,
        nrows = T), redrawn every step.  Returns one dict per epoch: epoch, loss (mean l_b over the
        epoch's steps), and with val val_loss and val_acc."""
        x = np.asarray(windows, np.float32)
        check_windows_shape(x.shape, self.n_features)
        lab = check_labels(labels, len(x), self.n_classes)
        import torch
        xd = torch.from_numpy(x).to(self.device)
        if augment is None:
            def batch_of(order, idx):
                return xd[idx]
        else:
            T = x.shape[1]
            rows = xd.view(len(x) * T, x.shape[2])

            def batch_of(order, idx):
                return self._augmented(augment, rows, order, T, T, order.astype(np.int64) * T)
        return self._run(batch_of, len(x), lab, epochs, batch, val, shuffle_seed)

    def fit_clips(self, clips, labels, epochs, batch=256, val=None, shuffle_seed=0, augment=None, window=20,
                  stride=5):
        """`fit` on clips instead of pre-cut windows: clips is a sequence of [n_k, F] row arrays,
        labels one label per clip.  The rows are resident once, as one store; there is one item per
        (clip, static position), enumerated as tools/train_sign.py's cut_windows cuts them (a window
        every `stride` rows while a full one fits, one window for a shorter clip), and every batch
        is built from the store by one isl_sign_augment launch.  A temporal shift or a speed change
        therefore reads the clip's real neighbouring frames.  augment None: identity items, which
        give the bits of `fit` on the cut windows."""
        from . import sign_augment as sa
        T = sa.check_window(window)
        if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
            raise ValueError("stride must be an integer >= 1, got %r" % (stride,))
        cl = [np.asarray(c, np.float32) for c in clips]
        for c in cl:
            if c.ndim != 2 or c.shape[1] != self.n_features:
                raise ValueError("a clip must be [n, %d] rows, got %s" % (self.n_features, c.shape))
        clip_lab = check_labels(labels, len(cl), self.n_classes)
        if augment is None:
            augment = sa.WindowAugment(layout=sa.identity_layout(self.n_features))
        lengths = np.array([len(c) for c in cl], np.int64)
        which, base = sa.clip_items(lengths, T, int(stride))
        first = np.concatenate([[0], np.cumsum(lengths)])[:-1] if len(cl) else np.zeros(0, np.int64)
        row0, nrows = first[which], lengths[which]
        import torch
        store = np.concatenate(cl) if len(which) else np.zeros((1, self.n_features), np.float32)
        rows = torch.from_numpy(np.ascontiguousarray(store)).to(self.device)

        def batch_of(order, idx):
            return self._augmented(augment, rows, order, T, nrows[order], row0[order], base[order])
        return self._run(batch_of, len(which), clip_lab[which], epochs, batch, val, shuffle_seed)

    def _run(self, batch_of, n, lab, epochs, batch, val, shuffle_seed):
        """The loop of fit and fit_clips over n samples: batch_of(order, idx) gives the windows of
        the dataset indices `order` (numpy; `idx` the same on the device)."""
        if int(epochs) < 0 or int(batch) < 1:
            raise ValueError("epochs must be >= 0 and batch >= 1")
        import torch
        ld = torch.from_numpy(lab).to(self.device)
        rng = np.random.RandomState(shuffle_seed)
        history = []
        for ep in range(int(epochs)):
            order = rng.permutation(n)
            total = torch.zeros((), dtype=torch.float64, device=self.device)
            for s in range(0, len(order), int(batch)):
                part = order[s:s + int(batch)]
                idx = torch.from_numpy(part).to(self.device)
                total += self.step(batch_of(part, idx), ld[idx], ids=idx).sum(dtype=torch.float64)
            row = {"epoch": ep, "loss": float(total) / max(1, n)}
            if val is not None:
                row["val_loss"], row["val_acc"] = self.evaluate(val[0], val[1], int(batch))
            history.append(row)
        return history

    # ------------------------------------------------------------------ the weights
    def weights(self):
        """The 28 keras-ordered arrays (numpy fp32), as ``model.get_weights()`` would give them."""
        flat = self.params.detach().cpu().numpy()
        out, o = [], 0
        for s in self.shapes:
            n = int(np.prod(s))
            out.append(flat[o:o + n].reshape(s).copy())
            o += n
        return out

    def save(self, path):
        """``np.savez(path, *weights())``: the format SignClassifier(path) loads."""
        np.savez(path, *self.weights())

    def classifier(self) -> SignClassifier:
        """A SignClassifier that shares the trainer's device vector: it sees every later step."""
        return self._clf
