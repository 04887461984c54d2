"""isl_sign_augment (csrc/sign_augment.hip) and its plumbing through islpose.train.SignTrainer on
the GPU, against the scalar statement of tests/_sign_augment.py: bit equality, no tolerance.

Every launch here writes into a buffer with GUARD canary floats on both sides of the output, and
reads a store that sits between NaN poison rows: the canaries must survive and no NaN may show up.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import _sign_augment as ref
import _sign_train_ref as train_ref

pytestmark = pytest.mark.gpu

GUARD = 64                          # guard band, floats
CANARY = 0x7FC0BEEF                 # a quiet NaN with a payload
POISON_ROWS = 3


def _records(items):
    from islpose import sign_augment as sa
    return np.array([ref.record(it) for it in items], sa.ITEM_DTYPE)


class _Store:
    """The rows of a case on the device between NaN poison rows, and guarded output buffers."""

    def __init__(self, rows):
        import torch
        n, F = rows.shape
        big = np.full((n + 2 * POISON_ROWS, F), np.nan, np.float32)
        big[POISON_ROWS:POISON_ROWS + n] = rows
        self.big = torch.from_numpy(big).cuda()
        self.rows = self.big[POISON_ROWS:POISON_ROWS + n]
        assert self.rows.is_contiguous()

    def output(self, n, T):
        import torch
        F = self.rows.shape[1]
        buf = torch.full((2 * GUARD + n * T * F,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)
        return buf, buf[GUARD:GUARD + n * T * F].view(n, T, F)

    @staticmethod
    def check(buf, out):
        """The output as numpy, after checking the canaries and that no poison reached it."""
        whole = buf.view(__import__("torch").int32).cpu().numpy()
        assert np.all(whole[:GUARD] == CANARY) and np.all(whole[-GUARD:] == CANARY), "a guard band was written"
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), "a poison row (or an unwritten element) is in the output"
        return got


def _apply(store, aug, items, T, step):
    buf, out = store.output(len(items), T)
    res = aug.apply(store.rows, items, T, step, out=out)
    assert res is out
    return _Store.check(buf, out)


_stores = {}


def _case(name):
    if name not in _stores:
        case = ref.CASES[name]()
        _stores[name] = (case, _Store(case["rows"]), _records(case["items"]))
    return _stores[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_bit_equal_to_the_statement(name):
    """A: T 1, F 12, one item over a one-row source.  B: T 32 and F 256, both ABI limits.  C: 257
    items over seven ragged clips, every speed, starts from -25 to len + 5, drop 0 / 0.3 / 0.9 and
    jitter 0 / 2.5."""
    from islpose import sign_augment as sa
    case, store, items = _case(name)
    for drop, jitter in case["opts"]:
        aug = sa.WindowAugment(drop=drop, jitter=jitter, layout=case["layout"], seed=case["seed"])
        got = _apply(store, aug, items, case["T"], case["step"])
        want = ref.expected(name, drop, jitter)
        diff = _bits(got) != _bits(want)
        print(name, drop, jitter, "elements", got.size, "differing", int(diff.sum()), "nonzero", int((want != 0).sum()))
        assert not diff.any(), (name, drop, jitter, np.argwhere(diff)[:5].tolist())


def test_identity_items_return_the_source_bits():
    from islpose import sign_augment as sa
    case, store, _ = _case("C")
    T = case["T"]
    aug = sa.WindowAugment(layout=case["layout"], seed=1)
    lengths = np.array(ref.C_LENGTHS)
    first = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    which, base = sa.clip_items(lengths, T, 5)
    items = aug.items(np.arange(len(which), dtype=np.uint64), 7, lengths[which], first[which], base)
    got = _apply(store, aug, items, T, 7)
    rows = case["rows"]
    for k in range(len(which)):
        src = rows[first[which[k]] + base[k]:first[which[k]] + min(base[k] + T, lengths[which[k]])]
        assert np.array_equal(_bits(got[k, :len(src)]), _bits(src)), k
        assert not got[k, len(src):].any()


def test_batch_and_order_invariance():
    """Case C's items reversed, and in batches of 1, 2 and 257: every item keeps its bits."""
    from islpose import sign_augment as sa
    case, store, items = _case("C")
    drop, jitter = 0.3, 2.5
    aug = sa.WindowAugment(drop=drop, jitter=jitter, layout=case["layout"], seed=case["seed"])
    want = ref.windows(case["rows"], case["layout"], case["items"][:40], case["T"], case["seed"], case["step"], drop, jitter)
    whole = _apply(store, aug, items, case["T"], case["step"])
    assert np.array_equal(_bits(whole[:40]), _bits(want))         # the statement, on a part; the rest by invariance
    rev = _apply(store, aug, items[::-1].copy(), case["T"], case["step"])
    assert np.array_equal(_bits(rev[::-1]), _bits(whole))
    for size in (1, 2):
        for s in range(0, len(items), size):
            part = _apply(store, aug, items[s:s + size], case["T"], case["step"])
            assert np.array_equal(_bits(part), _bits(whole[s:s + size])), (size, s)


def test_bad_items_give_zero_windows():
    """Items the host entry cannot see -- nrows 0, q 7, row0 -1, row0 + nrows = n_rows + 1 -- are
    defined behaviour: all-zero windows, nothing outside the output written, their neighbours right."""
    import torch
    from islpose import runtime as rt
    from islpose import sign_augment as sa
    case, store, items = _case("C")
    T, n_rows = case["T"], case["rows"].shape[0]
    aug = sa.WindowAugment(layout=case["layout"])
    good = aug.items(np.array([4, 5], np.uint64), 0, 40, 66)       # the clip of 40 rows
    its = np.concatenate([good[:1]] + [good[:1].copy() for _ in range(6)] + [good[1:]])
    its["nrows"][1] = 0
    its["q"][2] = 7
    its["q"][3] = 33
    its["row0"][4] = -1
    its["row0"][5], its["nrows"][5] = n_rows - 39, 40              # one row past the end
    its["row0"][6], its["nrows"][6] = 2 ** 62, 2 ** 31 - 1
    for k in range(1, 7):
        with pytest.raises(ValueError):
            sa.check_items(its[k:k + 1], n_rows)                   # Python refuses each before upload
    buf, out = store.output(len(its), T)
    items_t = torch.from_numpy(its.view(np.uint8).reshape(-1).copy()).cuda()
    rt.sign_augment(store.rows, case["layout"], items_t, len(its), T, rt.IslSignAugOpts(0, 0, 0, 0), out)
    got = _Store.check(buf, out)
    assert not got[1:7].any()
    src = case["rows"][66:66 + T]
    assert np.array_equal(_bits(got[0]), _bits(src)) and np.array_equal(_bits(got[7]), _bits(src))


def test_refused_calls_leave_the_output_untouched():
    from islpose import runtime as rt
    case, store, items = _case("A")
    import torch
    L = rt.lib()
    T, F = case["T"], case["rows"].shape[1]
    buf, out = store.output(1, T)
    items_t = torch.from_numpy(items.view(np.uint8).reshape(-1).copy()).cuda()
    vp = ctypes.c_void_p

    def call(rows=store.rows.data_ptr(), n_rows=1, F=F, layout=case["layout"] + (0,), items=items_t.data_ptr(), n=1,
             T=T, opts=None, dst=out.data_ptr()):
        lay = rt.IslSignAugLayout(*layout)
        o = rt.IslSignAugOpts() if opts is None else opts
        return L.isl_sign_augment(vp(rows), n_rows, F, ctypes.byref(lay), vp(items), n, T, ctypes.byref(o), vp(dst),
                                  rt.stream_handle())
    E = rt.ISL_E_ARG
    bad_reserved = rt.IslSignAugOpts()
    bad_reserved.reserved[0] = 7
    rcs = [call(rows=None), call(items=None), call(n=-1), call(n=65536), call(n_rows=-1), call(T=0), call(T=33),
           call(F=11), call(layout=(3, 1, 2, 1)), call(layout=(-3, 3, 2, 0)),
           call(opts=rt.IslSignAugOpts(0.95, 0, 0, 0)), call(opts=rt.IslSignAugOpts(float("nan"), 0, 0, 0)),
           call(opts=rt.IslSignAugOpts(0, -1, 0, 0)), call(opts=rt.IslSignAugOpts(0, float("inf"), 0, 0)),
           call(opts=bad_reserved)]
    assert rcs == [E] * len(rcs)
    assert call(n=0) == rt.ISL_OK
    torch.cuda.synchronize()
    assert np.all(buf.view(torch.int32).cpu().numpy() == CANARY)   # the whole buffer, output included
    # Python's own refusals: an output that overlaps the store, a store of another layout
    from islpose import sign_augment as sa
    aug = sa.WindowAugment(layout=case["layout"])
    flat = torch.zeros(4 * F, device="cuda")
    with pytest.raises(ValueError):
        aug.apply(flat[:2 * F].view(2, F), aug.items(np.zeros(1, np.uint64), 0, 1, 0), 2, 0, out=flat[F:3 * F].view(1, 2, F))
    with pytest.raises(ValueError):
        sa.WindowAugment().apply(store.rows, items, T, 0)
    with pytest.raises(ValueError):
        aug.apply(store.rows.cpu(), items, T, 0)


# ------------------------------------------------------------------ the trainer
TOY_LAYOUT = (3, 1, 2)              # T 8, F 12 of _sign_train_ref.toy_set
TOY = dict(sep=0.45, noise=0.3)


def _trainer(seed=0):
    from islpose.train import SignTrainer
    return SignTrainer(None, 12, 4, p_drop=0.2, p_rec=0.2, seed=seed, lr=3e-3)


def test_fit_with_an_identity_augment_is_fit():
    """fit(..., augment=WindowAugment(layout)) with all-zero magnitudes ends with bit-identical
    parameters to fit without the argument, and so does step."""
    from islpose.sign_augment import WindowAugment
    x, y = train_ref.toy_set(8, seed=1, **TOY)
    ends, hists = [], []
    for augment in (None, WindowAugment(layout=TOY_LAYOUT)):
        tr = _trainer(seed=3)
        tr.calibrate_bn0(x)
        hists.append(tr.fit(x, y, 3, batch=12, shuffle_seed=4, augment=augment))
        tr.step(x[:5], y[:5], ids=np.arange(5) + 100, augment=augment)
        assert tr.step_count == 10
        ends.append(tr.params.detach().cpu().numpy().copy())
    assert [h["loss"] for h in hists[0]] == [h["loss"] for h in hists[1]]
    assert np.array_equal(ends[0].view(np.uint32), ends[1].view(np.uint32))


def test_fit_clips_without_augment_is_fit_on_cut_windows():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import train_sign
    T, stride = 8, 3
    x, y = train_ref.toy_set(6, seed=1, **TOY)                     # 24 windows of 8 rows -> clips of ragged lengths
    pool = x.reshape(-1, 12)
    lengths = [3, 8, 9, 14, 20, 1, 11, 30]
    clips, labels, o = [], [], 0
    for k, n in enumerate(lengths):
        clips.append(pool[o:o + n])
        labels.append(k % 4)
        o += n
    cut = [train_sign.cut_windows(c, T, stride) for c in clips]
    wins = np.concatenate(cut)
    wlab = np.concatenate([np.full(len(c), l, np.int32) for c, l in zip(cut, labels)])
    assert len(wins) > len(clips)
    ends = []
    for clipwise in (False, True):
        tr = _trainer(seed=5)
        tr.calibrate_bn0(wins)
        if clipwise:
            h = tr.fit_clips(clips, labels, 2, batch=7, shuffle_seed=2, window=T, stride=stride)
        else:
            h = tr.fit(wins, wlab, 2, batch=7, shuffle_seed=2)
        ends.append((tr.params.detach().cpu().numpy().copy(), [r["loss"] for r in h], tr.step_count))
    assert ends[0][2] == ends[1][2] and ends[0][1] == ends[1][1]
    assert np.array_equal(ends[0][0].view(np.uint32), ends[1][0].view(np.uint32))


def test_it_still_learns():
    """The toy set fitted with a real augment (rotation 10 degrees, scale 0.1, tshift 1, drop 0.1; the
    frame is the toy coordinates' extent, 600 x 600 about their centre 300): the last epoch's mean
    loss is below the first's.  The curve itself is a measurement."""
    from islpose.sign_augment import WindowAugment
    x, y = train_ref.toy_set(8, seed=1, **TOY)
    aug = WindowAugment(rotation=10, scale=0.1, tshift=1, drop=0.1, frame=(601, 601), layout=TOY_LAYOUT)
    tr = _trainer()
    tr.calibrate_bn0(x)
    hist = tr.fit(x, y, 20, batch=32, augment=aug)
    print([round(h["loss"], 4) for h in hist])
    assert tr.step_count == 20
    assert hist[-1]["loss"] < hist[0]["loss"]
