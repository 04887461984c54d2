"""isl_sign_classify (csrc/sign.hip, sc_project / sc_recur<false> of csrc/sign_common.h) on the GPU
against the float64 statement of tests/_sign_ref.py, on dense weights and signed inputs.

Bar, on every element: |p_gpu - p64| <= M * p64 with M = min(4 * max(E, 2e-7), 1e-4), E the float32
statement's relative error against float64 on the same case (tests/test_sign_ref.py proves on the
CPU that the float32 statement passes it, that every mutation of the statement fails it by >= 10 x
and that every reference probability is >= 1e-30, so no element is left out).  Every row sums to 1
within (C + 2) * 2^-23 (a float32 sum of C terms and one division), and the argmax is the
reference's wherever the reference's top two are more than 2 M apart.

d_probs lies inside a canary-filled buffer with guard bands; the parameter vector and the windows
each lie between bands of a NaN poison, so a read outside sign_layout's extent or B * T * F shows
in the result.

Measured on one MI355X: the kernel sits at 0.20 ... 0.59 M on 34 cases and
at 0.90 M on (7, 10, 3), whose E is the maximum of only 18 elements.  Before sc_logit added b3 last
the shifted case was at 1.38 M and (7, 10, 3) at 1.19 M.
"""
import ctypes

import numpy as np
import pytest

import _sign_ref as sr

pytestmark = pytest.mark.gpu

PAD = 1024                          # guard band, floats
CANARY = 0x7FC0BEEF                 # a quiet NaN with a payload: the output's filling
POISON = 0x7FC0DEAD                 # another payload: around the inputs


class _Classify:
    """isl_sign_classify through ctypes.  offset: floats by which the parameter vector and the
    windows are moved off their 4 KiB-aligned places (1: not 16-byte aligned)."""

    def __init__(self, w, F, C, offset=0):
        import torch
        from islpose import runtime as rt
        self.rt, self.torch, self.F, self.C, self.offset = rt, torch, F, C, offset
        flat = np.concatenate([np.asarray(a, np.float32).ravel() for a in w])
        n = ctypes.c_int64()
        rt.check(rt.lib().isl_sign_param_count(F, C, ctypes.byref(n)))
        assert n.value == flat.size
        self.pbuf, self.params = self._between_poison(flat)

    def _between_poison(self, a):
        torch = self.torch
        a = np.ascontiguousarray(a, np.float32).ravel()
        buf = torch.full((a.size + self.offset + 2 * PAD,), POISON, dtype=torch.int32, device="cuda")
        view = buf.view(torch.float32)[PAD + self.offset:PAD + self.offset + a.size]
        view.copy_(torch.from_numpy(a))
        return buf, view

    def __call__(self, x, expect=0, batch=None, T=None, F=None, C=None, null=(), stream=None):
        torch, rt = self.torch, self.rt
        x = np.ascontiguousarray(x, np.float32)
        nb = x.shape[0]
        B = nb if batch is None else batch
        xbuf, xt = self._between_poison(x)
        n_out = nb * self.C
        obuf = torch.full((n_out + 2 * PAD,), CANARY, dtype=torch.int32, device="cuda")
        out = obuf.view(torch.float32)[PAD:PAD + n_out]
        ptr = lambda name, t: None if name in null else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        handle = None
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            handle = ctypes.c_void_p(stream.cuda_stream)
        rc = rt.lib().isl_sign_classify(ptr("params", self.params), self.F if F is None else F,
                                        x.shape[1] if T is None else T, self.C if C is None else C,
                                        ptr("x", xt), B, ptr("out", out), handle)
        torch.cuda.synchronize()
        assert rc == expect, (rc, rt.lib().isl_last_error())
        ib = obuf.cpu().numpy()
        assert (ib[:PAD] == CANARY).all() and (ib[PAD + n_out:] == CANARY).all(), "a guard band was written"
        if rc != 0 or B == 0:
            assert (ib == CANARY).all(), "a call that must write nothing wrote to d_probs"
            return None
        got = ib[PAD:PAD + n_out]
        assert (got != CANARY).all(), "an output element was not written"
        return got.view(np.float32).reshape(nb, self.C).copy()


_runs = {}


def _run(name):
    """The kernel's probabilities of a case (one launch per case, shared by the tests)."""
    if name not in _runs:
        c = sr.case(name)
        _runs[name] = _Classify(c["w"], c["F"], c["C"])(c["x"])
    return _runs[name]


@pytest.mark.parametrize("name", sr.CASE_IDS)
def test_matches_statement(name):
    """Step ranges (T around every multiple of SC_TQT = 8), projection paths (F % 4 == 0 and not,
    F = 1, the widest), softmax lanes (C around 64 and 256, one class), the workload's shape, every
    limit at once, wide logits and logits beyond log(FLT_MAX)."""
    c = sr.case(name)
    got = _run(name)
    p64, M, C = c["p64"], c["M"], c["C"]
    assert got.shape == p64.shape and got.dtype == np.float32
    g = got.astype(np.float64)
    rel = np.abs(g - p64) / p64
    sums = np.abs(g.sum(axis=1) - 1).max()
    print("%s (T %d, F %d, C %d): kernel at %.3f of M (rel err %.3g, E %.3g, M %.3g); |sum - 1| %.3g of %.3g" % (
        name, c["T"], c["F"], C, np.nanmax(rel) / M, np.nanmax(rel), c["E"], M, sums, (C + 2) * 2.0 ** -23))
    assert np.isfinite(got).all()
    assert p64.min() >= sr.P_MIN                                   # no element is left out
    assert (np.abs(g - p64) <= M * p64).all(), "worst %.3g x M at %s" % (
        rel.max() / M, np.unravel_index(rel.argmax(), rel.shape))
    assert sums <= (C + 2) * 2.0 ** -23
    if C == 1:
        assert (got == 1.0).all()
    else:
        top = np.sort(p64, axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * M * top[:, -1]
        assert (got.argmax(1) == p64.argmax(1))[clear].all()


@pytest.mark.parametrize("name", ["workload", "c257"])
def test_batch_invariance_bit_for_bit(name):
    """Windows 0, 2 and B - 1 alone; the parameter vector and the windows one float off their
    aligned places; a non-default stream: the batch's bits every time."""
    import torch
    c = sr.case(name)
    run = _Classify(c["w"], c["F"], c["C"])
    bits = _run(name).view(np.int32)
    for b in (0, 2, c["B"] - 1):
        assert np.array_equal(run(c["x"][b:b + 1]).view(np.int32)[0], bits[b]), b
    moved = _Classify(c["w"], c["F"], c["C"], offset=1)
    assert moved.params.data_ptr() % 16 == 4
    assert np.array_equal(moved(c["x"]).view(np.int32), bits)
    assert np.array_equal(run(c["x"], stream=torch.cuda.Stream()).view(np.int32), bits)


def test_refused_calls_write_nothing():
    """Every ISL_E_ARG case returns before any device work: d_probs keeps its canaries (checked in
    _Classify); batch 0 is ISL_OK, with null pointers too, and writes nothing."""
    from islpose import runtime as rt
    c = sr.case("steps-T9")
    run = _Classify(c["w"], c["F"], c["C"])
    E = rt.ISL_E_ARG
    for name in ("params", "x", "out"):
        run(c["x"], expect=E, null=(name,))
    for kw in (dict(T=0), dict(T=33), dict(F=0), dict(F=257), dict(C=0), dict(C=1025), dict(batch=-1)):
        run(c["x"], expect=E, **kw)
    assert b"isl_sign_classify" in rt.lib().isl_last_error()
    run(c["x"], batch=0)
    run(c["x"], batch=0, null=("params", "x", "out"))
    run(c["x"][:0])
    n = ctypes.c_int64(-1)
    for F, C in ((0, 7), (257, 7), (12, 0), (12, 1025)):
        assert rt.lib().isl_sign_param_count(F, C, ctypes.byref(n)) == E and n.value == -1
    assert rt.lib().isl_sign_param_count(12, 7, None) == E
