"""The training step's float64 statement (tests/_sign_train_ref.py) checked on the CPU: its forward
against the inference oracle, its gradients against central differences with dropout on, the hash's
known answers; the training tool's tree -> windows -> labels -> split; the Python layer's refusals.
No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import _sign_train_ref as ref
from oracle import sign_classifier as oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 12, 7, 4), (20, 156, 167, 2)]       # (T, F, C, B)


def _tool():
    spec = importlib.util.spec_from_file_location("train_sign", os.path.join(REPO, "tools", "train_sign.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("T,F,C,B", SHAPES + [(32, 256, 64, 2)])
def test_statement_forward_matches_inference_oracle(T, F, C, B):
    import torch
    w = ref.trained_like_weights(F, C, seed=T)
    x = ref.windows_like(B, T, F, seed=T)
    x[0, 0] = 0
    wt = [torch.tensor(np.asarray(a, np.float64)) for a in w]
    m = {k: torch.tensor(v) for k, v in ref.no_dropout(T).items()}
    for b in range(B):
        p = torch.softmax(ref.logits(wt, torch.tensor(x[b].astype(np.float64)), m), 0).numpy()
        np.testing.assert_allclose(p, oracle.classify(w, x[b]), rtol=1e-12, atol=1e-15)
    labels = np.arange(B) % C
    loss, _ = ref.loss_and_grads(w, x, labels)
    exp = [-np.log(oracle.classify(w, x[b])[labels[b]]) for b in range(B)]
    np.testing.assert_allclose(loss, exp, rtol=1e-10, atol=1e-12)


def test_statement_gradients_match_central_differences():
    """Four elements of each of the 28 arrays, dropout factors on (0.2, 0.2), sample weights and an
    ignored window in the batch: |g - fd| <= 1e-5 * max|g| of the array (the differences' own
    truncation and rounding at a step of 1e-5 * max(1, |theta|))."""
    T, F, C, B = 5, 12, 7, 4
    w = [a.astype(np.float64) for a in ref.trained_like_weights(F, C, seed=2)]
    x = ref.windows_like(B, T, F, seed=4)
    labels = np.array([1, 6, -1, 3])
    sw = np.array([1.0, 0.5, 2.0, 1.5])
    masks = [ref.dropout_factors(T, 0.2, 0.2, 7, 3, b) for b in range(B)]
    loss, g = ref.loss_and_grads(w, x, labels, sw, masks, zero_stats=False)
    assert loss[2] == 0 and (loss[[0, 1, 3]] > 0).all()
    _, gz = ref.loss_and_grads(w, x, labels, sw, masks)
    rng = np.random.RandomState(0)
    for k in range(28):
        if k in ref.STAT_SLOTS:
            assert not gz[k].any()
        else:
            np.testing.assert_array_equal(gz[k], g[k])
        scale = np.abs(g[k]).max()
        assert scale > 0
        for flat in rng.choice(w[k].size, 4, replace=False):
            idx = np.unravel_index(flat, w[k].shape)
            h = 1e-5 * max(1.0, abs(w[k][idx]))
            keep = w[k][idx]
            w[k][idx] = keep + h
            up = ref.batch_loss(w, x, labels, sw, masks)
            w[k][idx] = keep - h
            dn = ref.batch_loss(w, x, labels, sw, masks)
            w[k][idx] = keep
            assert abs((up - dn) / (2 * h) - g[k][idx]) <= 1e-5 * scale, (k, idx)


def test_hash_known_answers():
    assert int(ref.sm(0)[0]) == 0xE220A8397B1DCDAF
    k = int(ref.draw(7, 3, 5, 0, 11)[0])
    assert k == 0x2D56212C221D27FC
    assert ref.threshold(0.2) == 3355443 and (k >> 40) < ref.threshold(0.2)
    assert not ref.keep(0.2, 7, 3, 5, 0, 11)[0]
    # 256 000 draws at rate 0.2: the keep share within four standard deviations of 0.8
    share = np.mean([ref.keep(0.2, 7, 3, sid, 0, np.arange(1000)).mean() for sid in range(256)])
    assert abs(share - 0.8) < 4 * np.sqrt(0.16 / 256000), share
    f = ref.factors(0.2, 7, 3, 5, 0, 64)
    assert set(np.unique(f)) <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.2)))}
    assert (ref.factors(0.0, 7, 3, 5, 0, 64) == 1).all()
    # a window's masks depend on (seed, step, id) only
    a, b = ref.dropout_factors(5, 0.5, 0.5, 1, 2, 9), ref.dropout_factors(5, 0.5, 0.5, 1, 2, 9)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["A"], ref.dropout_factors(5, 0.5, 0.5, 1, 3, 9)["A"])


def test_tool_tree_to_windows_labels_split(tmp_path):
    from islpose import pipeline, translate
    tool = _tool()

    def frame(seed):
        r = np.random.RandomState(seed)
        cand = np.concatenate([r.uniform(0, 600, (25, 2)), r.uniform(0.2, 1, (25, 1)), np.arange(25)[:, None]], 1)
        subset = np.concatenate([np.arange(25.0), [20.0, 25.0]])[None]
        subset[0, 7] = -1
        hands = [r.randint(0, 600, (21, 2)), r.randint(0, 600, (21, 2))][:seed % 3]
        return cand, subset, hands

    plan = {("words", "hello"): [("v1.npy", 23), ("v2.npy", 7)], ("words", "thanks"): [("v3.npy", 30), ("v4.npy", 20)]}
    made = {}
    for (typ, expr), vids in plan.items():
        for fname, n in vids:
            for transform in ("original", "Rotate"):
                for i in range(n):
                    p = pipeline.json_path(str(tmp_path), typ, expr, fname, i, transform)
                    os.makedirs(os.path.dirname(p), exist_ok=True)
                    c, s, h = frame((sum(map(ord, fname)) * 31 + i) % 1000 + (transform == "Rotate"))
                    made[p] = (c, s, h)
                    with open(p, "w") as f:
                        f.write(pipeline.frame_json(c, s, h))
    clips = tool.scan_tree(str(tmp_path))
    assert len(clips) == 8 and all(len(c["frames"]) == dict(sum(plan.values(), []))[c["stem"] + ".npy"] for c in clips)
    c0 = [c for c in clips if c["stem"] == "v1" and c["transform"] == "Rotate"][0]
    assert [os.path.basename(p) for p in c0["frames"][9:12]] == ["v1.npy-9.json", "v1.npy-10.json", "v1.npy-11.json"]
    # a row is the translator's frame_features of what was written
    from src import util
    cand, subset, hands = made[c0["frames"][10]]
    circles, _ = util.get_bodypose(cand, subset, "body25")
    _, peaks = util.get_handpose(hands)
    np.testing.assert_array_equal(tool.frame_row(open(c0["frames"][10]).read()),
                                  translate.populate_features(circles, peaks).astype(np.float64))

    data = tool.build_dataset(str(tmp_path), stride=5, val_share=0.25, seed=1)
    assert data["names"] == ["hello", "thanks"]
    # windows: 23 frames -> starts 0 (one full window fits at stride 5 only at 0); 7 -> one padded;
    # 30 -> starts 0, 5, 10; 20 -> one
    per_video = {"v1": 1, "v2": 1, "v3": 3, "v4": 1}
    (xt, yt), (xv, yv) = data["train"], data["val"]
    assert xt.dtype == np.float32 and yt.dtype == np.int32 and xt.shape[1:] == (20, 156)
    val_videos = tool.split_stems(clips, 0.25, 1)
    assert len(val_videos) == 1
    (vt, ve, vs), = val_videos
    assert len(xv) == 2 * per_video[vs] and len(xt) == 2 * (sum(per_video.values()) - per_video[vs])
    assert (yv == data["names"].index(ve)).all()
    # the padded clip: 7 real rows, 13 masked ones
    short = tool.cut_windows(np.ones((7, 156)), 20, 5)
    assert short.shape == (1, 20, 156) and short[0, :7].all() and not short[0, 7:].any()
    assert tool.cut_windows(np.ones((30, 4)), 20, 5).shape == (3, 20, 4)
    assert tool.cut_windows(np.ones((0, 4)), 20, 5).shape == (0, 20, 4)
    # an explicit class list orders the labels; a missing expression is refused
    cf = tmp_path / "classes.txt"
    cf.write_text("thanks\nhello\n")
    assert tool.build_dataset(str(tmp_path), str(cf), val_share=0)["names"] == ["thanks", "hello"]
    cf.write_text("hello\n")
    with pytest.raises(ValueError):
        tool.build_dataset(str(tmp_path), str(cf))


def test_python_layer_refusals():
    from islpose import train
    import islpose
    assert islpose.SignTrainer is train.SignTrainer
    for bad in (-0.1, 0.95, float("nan"), "x"):
        with pytest.raises(ValueError):
            train.SignTrainer(p_drop=bad)
        with pytest.raises(ValueError):
            train.SignTrainer(p_rec=bad)
    with pytest.raises(ValueError):
        train.SignTrainer(n_features=257)
    with pytest.raises(ValueError):
        train.SignTrainer(n_classes=0)
    with pytest.raises(ValueError):
        train.SignTrainer(seed=-1)
    with pytest.raises(ValueError):
        train.check_labels(np.array([0.0, 1.0]), 2, 5)           # dtype
    with pytest.raises(ValueError):
        train.check_labels(np.array([0, 5]), 2, 5)               # range
    with pytest.raises(ValueError):
        train.check_labels(np.array([0, 1, 2]), 2, 5)            # shape
    assert train.check_labels([3, -1], 2, 5).dtype == np.int32   # a negative label ignores its window
    for shape in ((2, 20), (2, 33, 156), (2, 0, 156), (2, 20, 155)):
        with pytest.raises(ValueError):
            train.check_windows_shape(shape, 156)
    x = np.zeros((2, 3, 4))
    x[0, 1] = [1, 2, 3, 4]
    x[1, 2] = [3, 2, 1, 0]
    mean, var = train.bn0_statistics(x)                          # the two unmasked rows only
    np.testing.assert_array_equal(mean, [2, 2, 2, 2])
    np.testing.assert_array_equal(var, [1, 0, 1, 4])
