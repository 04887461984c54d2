"""The window augmentation without a GPU: the host derivation of the items
and the numpy form of islpose/sign_augment.py against the scalar statement of tests/_sign_augment.py,
bit for bit (no tolerance anywhere); the validation errors; the host-side refusals of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import _sign_augment as ref
from islpose import runtime as rt
from islpose import sign_augment as sa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sign_aug_items.txt")
REAL = dict(rotation=20.0, scale=0.15, shift=0.05, speed=0.3, tshift=4)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _records(items):
    return np.array([ref.record(it) for it in items], sa.ITEM_DTYPE)


def _augment(case, drop=0.0, jitter=0.0):
    return sa.WindowAugment(drop=drop, jitter=jitter, layout=case["layout"], seed=case["seed"])


# ------------------------------------------------------------------ the hash
def test_hash_continuity():
    """Section 4.2k's known answer, from the scalar statement and from the product's numpy sm."""
    assert ref.draw(ref.key(7, 3, 5), 0, 11) == 0x2D56212C221D27FC
    assert ref.sm(0) == 0xE220A8397B1DCDAF
    kw = sa.window_key(7, 3, np.array([5], np.uint64))
    assert int(sa.site_draw(kw, 0, np.array([11], np.uint64))[0]) == 0x2D56212C221D27FC
    big = np.array([0, 1, 2 ** 63, 2 ** 64 - 1], np.uint64)
    assert [int(v) for v in sa.sm(big)] == [ref.sm(int(v)) for v in big]


# ------------------------------------------------------------------ the host derivation
def test_items_match_statement():
    """items() equals the scalar statement field for field (m by its bits): 64 ids at two steps,
    per-item nrows, row0 and base."""
    aug = sa.WindowAugment(seed=9, **REAL)
    cfg = dict(REAL, frame=aug.frame)
    ids = np.array([(k * 0x9E3779B1 + 17) % 2 ** 64 if k % 3 else 2 ** 64 - 1 - k for k in range(64)], np.uint64)
    nrows = 1 + np.arange(64) % 50
    row0 = np.arange(64) * 7
    base = np.arange(64) % 11 - 3
    seen_q, seen_start = set(), set()
    for step in (0, 12345):
        got = aug.items(ids, step, nrows, row0, base)
        assert got.dtype == sa.ITEM_DTYPE and got.shape == (64,)
        want = _records([ref.item(cfg, 9, step, int(ids[k]), nrows[k], row0[k], base[k]) for k in range(64)])
        for f in ("row0", "nrows", "start", "q", "reserved", "id"):
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(got["m"].view(np.uint64), want["m"].view(np.uint64))
        seen_q |= set(got["q"].tolist())
        seen_start |= set((got["start"] - base).tolist())
    assert min(seen_q) < 16 < max(seen_q) and min(seen_start) < 0 < max(seen_start)
    # the trainer's seed overrides the augment's
    assert np.array_equal(aug.items(ids, 3, 20, 0, seed=4)["m"], sa.WindowAugment(seed=4, **REAL).items(ids, 3, 20, 0)["m"])


def _golden_lines():
    with open(GOLDEN) as f:
        return [ln.split() for ln in f if ln.strip() and not ln.startswith("#")]


def test_items_match_the_recorded_fixture():
    """tests/golden/sign_aug_items.txt: seed step id nrows row0 base -> start q m0..m5 (hex floats),
    for the REAL magnitudes at 1920 x 1080; both the product and the statement reproduce it."""
    lines = _golden_lines()
    assert len(lines) >= 6
    cfg = dict(REAL, frame=(1920, 1080))
    for f in lines:
        seed, step, sid, nrows, row0, base, start, q = (int(v) for v in f[:8])
        m = [float.fromhex(v) for v in f[8:14]]
        got = sa.WindowAugment(seed=seed, **REAL).items(np.array([sid], np.uint64), step, nrows, row0, base)[0]
        assert (int(got["start"]), int(got["q"]), int(got["row0"]), int(got["nrows"]), int(got["id"])) == \
            (start, q, row0, nrows, sid)
        assert [float(v).hex() for v in got["m"]] == [v.hex() for v in m]
        want = ref.item(cfg, seed, step, sid, nrows, row0, base)
        assert (want["start"], want["q"]) == (start, q) and [v.hex() for v in want["m"]] == [v.hex() for v in m]


def test_zero_magnitudes_give_the_identity_item():
    aug = sa.WindowAugment(seed=3)
    it = aug.items(np.arange(40, dtype=np.uint64) * 977, 6, 20, np.arange(40) * 20, base=np.arange(40) - 5)
    assert np.array_equal(it["m"].view(np.uint64),
                          np.tile(np.array([1, 0, 0, 0, 1, 0], np.float64).view(np.uint64), (40, 1)))
    assert np.all(it["q"] == 16) and np.array_equal(it["start"], np.arange(40) - 5) and np.all(it["reserved"] == 0)
    one = ref.item(dict(rotation=0, scale=0, shift=0, speed=0, tshift=0, frame=(1920, 1080)), 3, 6, 977, 20, 20, -4)
    assert [v.hex() for v in one["m"]] == [v.hex() for v in (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)] and one["q"] == 16 and one["start"] == -4


def test_source_rows_of_the_definition():
    """The frame formula: q 16 is the identity; the two sequences DESIGN writes out for T 20."""
    assert sa.source_rows(20, [16], [0])[0].tolist() == list(range(20))
    r13 = sa.source_rows(20, [13], [0])[0].tolist()
    assert r13[:4] == [2, 3, 3, 4] and r13[-1] == 17
    r20 = sa.source_rows(20, [20], [0])[0].tolist()
    assert r20[:5] == [-2, -1, 0, 1, 3] and r20[-1] == 21
    assert sa.source_rows(1, [8, 32], [0, 4]).tolist() == [[0], [4]]


# ------------------------------------------------------------------ apply_numpy against the statement
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_apply_numpy_matches_statement(name):
    case = ref.CASES[name]()
    items = _records(case["items"])
    for drop, jitter in case["opts"]:
        got = _augment(case, drop, jitter).apply_numpy(case["rows"], items, case["T"], case["step"])
        want = ref.expected(name, drop, jitter)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(want)), (name, drop, jitter)


def test_case_c_reaches_what_it_targets():
    """Case C's statement output has live, out-of-range and dropped frames, moved pairs and absent
    pairs: the bit comparisons are not comparing zeros."""
    case = ref.CASES["C"]()
    full = ref.expected("C", 0.0, 2.5)
    part = ref.expected("C", 0.3, 0.0)
    live_full, live_part = full.any(axis=2), part.any(axis=2)
    assert 0.2 < live_full.mean() < 0.9                      # both in-range and out-of-range frames
    assert live_part.sum() < live_full.sum() and not np.any(live_part & ~live_full)
    assert {it["q"] for it in case["items"]} == set(ref.C_SPEEDS)
    starts = [it["start"] for it in case["items"]]
    assert min(starts) == -25 and max(it["start"] - it["nrows"] for it in case["items"]) == 5
    assert not np.isnan(full).any()


def test_apply_numpy_properties():
    layout, T = (15, 2, 21), 20
    rows = ref.make_rows(90, layout, 31)
    aug0 = sa.WindowAugment(layout=layout)
    ident = aug0.items(np.arange(4, dtype=np.uint64), 0, [20, 20, 30, 7], [0, 20, 40, 70], base=[0, 0, 5, 0])
    out = aug0.apply_numpy(rows, ident, T, 0)
    # identity items return the source bits; rows past a short clip's end are zero
    assert np.array_equal(_bits(out[0]), _bits(rows[0:20])) and np.array_equal(_bits(out[2]), _bits(rows[45:65]))
    assert np.array_equal(_bits(out[3, :7]), _bits(rows[70:77])) and not out[3, 7:].any()

    aug = sa.WindowAugment(drop=0.4, jitter=3.0, layout=layout, seed=2, **REAL)
    items = aug.items(np.arange(12, dtype=np.uint64), 5, 30, np.arange(12) % 3 * 30, base=np.arange(12))
    items["q"], items["start"] = 16, np.arange(12)            # frame t of item k reads source row k + t
    out = aug.apply_numpy(rows, items, T, 5)
    xi, yi, li = sa.layout_index(layout)
    r = sa.source_rows(T, items["q"], items["start"])
    live = out.any(axis=2)
    in_range = (r >= 0) & (r < 30)
    src = rows[np.where(in_range, items["row0"][:, None] + r, 0)]
    src_live = in_range & src.any(axis=2)
    assert not np.any(live & ~src_live)                        # out of range, or an empty source row: zero
    dropped = src_live & ~live
    assert 0.2 < dropped.sum() / src_live.sum() < 0.6          # drop 0.4 zeroes whole frames
    absent = (src[..., xi] == 0) & (src[..., yi] == 0)
    assert absent[live].any()
    assert not out[..., xi][live][absent[live]].any() and not out[..., yi][live][absent[live]].any()
    present = ~absent & live[..., None]
    assert np.all((out[..., xi][present] != 0) | (out[..., yi][present] != 0))
    assert not np.array_equal(out[..., xi][present], src[..., xi][present])     # the pairs did move
    assert np.array_equal(_bits(out[..., li][live]), _bits(src[..., li][live]))  # labels untouched


def test_a_present_pair_mapped_to_zero_stays_present():
    """A designed pair whose image is exactly (0, 0) is stored as (2^-10, 0), by the product and by
    the statement; its neighbour maps to (0, 5) and is stored as it is."""
    layout = (2, 0, 0)
    rows = np.array([[4.0, 4.0, 2.5, 7.5]], np.float32)         # pairs (4, 2.5) and (4, 7.5)
    aug = sa.WindowAugment(layout=layout)
    items = aug.items(np.zeros(1, np.uint64), 0, 1, 0)
    items["m"] = [[1.0, 0.0, -4.0, 0.0, 1.0, -2.5]]
    out = aug.apply_numpy(rows, items, 1, 0)
    assert out[0, 0].tolist() == [2.0 ** -10, 0.0, 0.0, 5.0]
    assert np.array_equal(_bits(out), _bits(ref.windows(rows, layout, items, 1, 0, 0, 0.0, 0.0)))


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("kw", [
    dict(rotation=-1), dict(rotation=181), dict(rotation=float("nan")), dict(rotation="3"),
    dict(scale=-0.1), dict(scale=0.6), dict(shift=-0.1), dict(shift=0.51), dict(speed=-0.1), dict(speed=0.6),
    dict(tshift=-1), dict(tshift=33), dict(tshift=1.5), dict(drop=-0.1), dict(drop=0.95), dict(drop=float("nan")),
    dict(jitter=-1), dict(jitter=float("inf")), dict(jitter=1e39), dict(frame=(1920,)), dict(frame=(1920, float("inf"))),
    dict(layout=(15, 2)), dict(layout=(-1, 2, 21)), dict(layout=(15, 2, 21.0)), dict(layout=(0, 0, 0)),
    dict(layout=(100, 2, 21)), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        sa.WindowAugment(**kw)


def test_constructor_accepts_the_range_ends():
    a = sa.WindowAugment(rotation=180, scale=0.5, shift=0.5, speed=0.5, tshift=32, drop=0.9, jitter=0, seed=2 ** 64 - 1)
    assert (a.rotation, a.tshift, a.drop, a.n_features) == (180.0, 32, 0.9, 156)


def test_apply_numpy_rejects():
    layout = (3, 1, 2)
    aug = sa.WindowAugment(layout=layout)
    rows = ref.make_rows(10, layout, 1)
    ok = aug.items(np.arange(2, dtype=np.uint64), 0, 5, [0, 5])
    assert aug.apply_numpy(rows, ok, 4, 0).shape == (2, 4, 12)
    with pytest.raises(ValueError):                            # a layout / F mismatch
        aug.apply_numpy(ref.make_rows(10, (15, 2, 21), 1), ok, 4, 0)
    with pytest.raises(ValueError):
        aug.apply_numpy(rows.astype(np.float64), ok, 4, 0)
    for window in (0, 33, 2.0):
        with pytest.raises(ValueError):
            aug.apply_numpy(rows, ok, window, 0)
    for field, value in (("nrows", 0), ("q", 7), ("q", 33), ("row0", -1), ("row0", 6), ("nrows", 6), ("reserved", 1)):
        bad = ok.copy()
        bad[field][1] = value                                  # items that leave the store, or malformed
        with pytest.raises(ValueError):
            aug.apply_numpy(rows, bad, 4, 0)
    bad = ok.copy()
    bad["m"][0, 2] = np.nan
    with pytest.raises(ValueError):
        aug.apply_numpy(rows, bad, 4, 0)
    with pytest.raises(ValueError):
        aug.apply_numpy(rows, np.zeros(2, [("row0", "<i8")]), 4, 0)
    with pytest.raises(ValueError):
        aug.apply_numpy(rows, ok, 4, -1)
    # overlapping output
    buf = np.zeros(2 * 4 * 12 + 10 * 12, np.float32)
    store = buf[:120].reshape(10, 12)
    store[...] = rows
    with pytest.raises(ValueError):
        aug.apply_numpy(store, ok, 4, 0, out=buf[24:120].reshape(2, 4, 12))
    out = aug.apply_numpy(store, ok, 4, 0, out=buf[120:].reshape(2, 4, 12))
    assert np.array_equal(out, aug.apply_numpy(rows, ok, 4, 0))
    with pytest.raises(ValueError):
        sa.check_no_overlap(1000, 480, 1476, 96)
    sa.check_no_overlap(1000, 480, 1480, 96)
    sa.check_no_overlap(1480, 96, 1000, 480)
    with pytest.raises(ValueError):
        aug.items(np.arange(2, dtype=np.uint64), 0, 0, 0)
    with pytest.raises(ValueError):
        aug.items(np.arange(2, dtype=np.float64), 0, 5, 0)
    with pytest.raises(ValueError):
        aug.items(np.arange(2, dtype=np.uint64), 0, 5, -1)


def test_parse():
    a = sa.WindowAugment.parse("rot:15,scale:0.1,shift:0.05,speed:0.2,tshift:3,drop:0.1,jitter:2", seed=4)
    assert (a.rotation, a.scale, a.shift, a.speed, a.tshift, a.drop, a.jitter, a.seed) == (15.0, 0.1, 0.05, 0.2, 3, 0.1, 2.0, 4)
    assert sa.WindowAugment.parse("") is None and sa.WindowAugment.parse(None) is None
    assert sa.WindowAugment.parse(" drop:0.5 ", layout=(3, 1, 2)).n_features == 12
    for spec in ("rot", "rot:", "rot:x", "mirror:1", "rot:15:2", "rot:15,,scale:0.1", "rot:200", "tshift:1.5",
                 "rot:5,rot:6", "drop:0.95", "rotation:30"):
        with pytest.raises(ValueError):
            sa.WindowAugment.parse(spec)


def test_clip_items_enumerate_as_cut_windows():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import train_sign
    lengths = [0, 1, 19, 20, 21, 24, 25, 40]
    which, base = sa.clip_items(lengths, 20, 5)
    for k, n in enumerate(lengths):
        rows = np.arange(n * 3, dtype=np.float32).reshape(n, 3) + 1
        cut = train_sign.cut_windows(rows, 20, 5)
        mine = base[which == k]
        assert len(cut) == len(mine)
        for w, b in zip(cut, mine):
            assert np.array_equal(w[:min(20, n - b)], rows[b:b + 20])
    assert sa.identity_layout(156) == (78, 0, 0) and sa.identity_layout(13) == (5, 1, 1)
    assert sa.check_layout(sa.identity_layout(3), 3) == (0, 1, 1)


def test_tool_keeps_the_rows_per_clip(tmp_path):
    """tools/train_sign.py build_dataset(keep_rows=True): the training clips' rows, whose cut windows
    are the training windows in order; without the flag the result has no such entry."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import train_sign
    from islpose import pipeline
    r = np.random.RandomState(0)
    for expr, fname, n in (("hello", "v1.npy", 23), ("hello", "v2.npy", 4), ("thanks", "v3.npy", 30)):
        for i in range(n):
            p = pipeline.json_path(str(tmp_path), "words", expr, fname, i, "original")
            os.makedirs(os.path.dirname(p), exist_ok=True)
            cand = np.concatenate([r.uniform(0, 600, (25, 2)), r.uniform(0.2, 1, (25, 1)), np.arange(25)[:, None]], 1)
            subset = np.concatenate([np.arange(25.0), [20.0, 25.0]])[None]
            with open(p, "w") as f:
                f.write(pipeline.frame_json(cand, subset, [r.randint(0, 600, (21, 2))]))
    assert "train_rows" not in train_sign.build_dataset(str(tmp_path), val_share=0)
    data = train_sign.build_dataset(str(tmp_path), val_share=0, keep_rows=True)
    clips, labels = data["train_rows"]
    assert [len(c) for c in clips] == [23, 4, 30] and labels.tolist() == [0, 0, 1] and clips[0].dtype == np.float32
    cut = [train_sign.cut_windows(c, 20, 5) for c in clips]
    assert np.array_equal(np.concatenate(cut), data["train"][0])
    assert np.array_equal(np.concatenate([np.full(len(c), l) for c, l in zip(cut, labels)]), data["train"][1])
    which, base = sa.clip_items([len(c) for c in clips], 20, 5)
    assert which.tolist() == [0, 1, 2, 2, 2] and base.tolist() == [0, 0, 0, 5, 10]


# ------------------------------------------------------------------ the C ABI, host-only calls
def _lib():
    if not os.path.exists(rt.LIB_PATH):
        pytest.skip("libislpose.so not built")
    return rt.lib()


def test_abi_struct_sizes_and_symbols():
    L = _lib()
    assert hasattr(L, "isl_sign_augment") and hasattr(L, "isl_sign_aug_opts_default")
    assert (ctypes.sizeof(rt.IslSignAugItem), ctypes.sizeof(rt.IslSignAugLayout), ctypes.sizeof(rt.IslSignAugOpts)) == (80, 16, 40)
    assert sa.ITEM_DTYPE.itemsize == 80
    for name in sa.ITEM_DTYPE.names:
        assert sa.ITEM_DTYPE.fields[name][1] == getattr(rt.IslSignAugItem, name).offset, name
    d = rt.IslSignAugOpts(0.5, 0.5, 1, 1)
    rt.check(L.isl_sign_aug_opts_default(ctypes.byref(d)))
    assert (d.drop, d.jitter, d.seed, d.step, list(d.reserved)) == (0.0, 0.0, 0, 0, [0] * 4)
    assert L.isl_sign_aug_opts_default(None) == rt.ISL_E_ARG


def test_abi_refusals_before_any_device_work():
    """Every ISL_E_ARG case returns before the device is touched (there is none here): the pointers
    are never dereferenced on the host either, except layout and opts, which are real."""
    L = _lib()
    vp = ctypes.c_void_p
    fake = vp(4096)

    def call(rows=fake, n_rows=10, F=12, layout=(3, 1, 2, 0), items=fake, n=1, T=4, opts=None, out=fake,
             no_layout=False, no_opts=False):
        lay = rt.IslSignAugLayout(*layout)
        o = rt.IslSignAugOpts() if opts is None else opts
        return L.isl_sign_augment(rows, n_rows, F, None if no_layout else ctypes.byref(lay), items, n, T,
                                  None if no_opts else ctypes.byref(o), out, None)
    E = rt.ISL_E_ARG
    assert call(n=0) == rt.ISL_OK and call(n=0, rows=None, out=None, items=None) == rt.ISL_OK
    assert call(n=-1) == E and call(n=65536) == E
    assert call(rows=None) == E and call(items=None) == E and call(out=None) == E
    assert call(no_layout=True) == E and call(no_opts=True) == E
    assert call(n_rows=-1) == E
    assert call(T=0) == E and call(T=33) == E
    assert call(F=0, layout=(0, 0, 0, 0)) == E and call(F=258, layout=(129, 0, 0, 0)) == E
    assert call(layout=(3, 1, 3, 0)) == E and call(layout=(6, 0, 0, 1)) == E
    assert call(layout=(-3, 1, 6, 0)) == E and call(layout=(9, -1, 2, 0)) == E and call(layout=(9, 1, -2, 0)) == E
    for drop, jitter in ((-0.1, 0), (0.95, 0), (float("nan"), 0), (0, -1.0), (0, float("inf")), (0, float("nan"))):
        assert call(opts=rt.IslSignAugOpts(drop, jitter, 0, 0)) == E, (drop, jitter)
    o = rt.IslSignAugOpts()
    o.reserved[3] = 1
    assert call(opts=o) == E
    assert b"isl_sign_augment" in L.isl_last_error()
