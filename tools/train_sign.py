"""Train the sign classifier on the extractor's output tree, on one GPU.

  python tools/extract_features.py --csv sample.csv --dataset-base data/ --out features/ --augment ...
  python tools/train_sign.py --features features/ --out model/w.npz --epochs 40

Reads <features>/transforms/<type>/<expression>/<stem>-<Transform>/<file>-<idx>.json (the layout of
islpose.pipeline.json_path), turns every frame into the translator's 156-d row
(ISLSignPosTranslator.frame_features), orders the rows of each (video, transform) by frame index and
cuts windows of 20 frames every --stride frames; a video shorter than a window is right-padded with
zero rows, which the model masks.  Labels are the lines of --classes FILE or the sorted expression
folder names; classes.json is written beside the weights.  Train and validation are split by video
stem, so a video's augmented variants never straddle the split.  Then: BN0 statistics from the
training windows, SignTrainer.fit, one JSON line per epoch, and <out> as
np.savez(path, *weights), which SignClassifier(path) loads.

--augment SPEC redraws every training window at every step in keypoint space (islpose.sign_augment,
DESIGN.md section 4.2m), e.g. --augment rot:15,scale:0.1,shift:0.05,speed:0.2,tshift:3,drop:0.1,jitter:2;
--frame W,H is the size of the videos' frames.  With --clips the rows stay whole per clip
(SignTrainer.fit_clips), so a temporal shift or a speed change reads the clip's real neighbouring
frames instead of the zero padding of a pre-cut window.  Validation is never augmented.

The parsing and windowing functions import without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isl-signlanguage-translation_amd"))

WINDOW, N_FEATURES = 20, 156
_FRAME = re.compile(r"^(?P<file>.+)-(?P<idx>\d+)\.json$")


def frame_row(text: str) -> np.ndarray:
    """One per-frame JSON text -> the 156-d row of ISLSignPosTranslator.frame_features."""
    from islpose.translate import populate_features
    from src import util
    d = json.loads(text)
    candidate = np.asarray(d["candidate"], np.float64).reshape(-1, 4)
    subset = np.asarray(d["subset"], np.float64)
    subset = subset.reshape(-1, subset.shape[-1] if subset.ndim == 2 else 27)
    hands = [np.asarray(p) for p in d["all_hand_peaks"]]
    circles, _ = util.get_bodypose(candidate, subset, "body25")
    _, peaks = util.get_handpose(hands)
    return np.asarray(populate_features(circles, peaks), np.float64)


def scan_tree(base: str):
    """Every (video, transform) of the tree: a list of dicts with type, expression, stem, transform
    and `frames`, the JSON paths ordered by frame index."""
    root = os.path.join(base, "transforms")
    clips = []
    for label_type in sorted(os.listdir(root)):
        for expression in sorted(os.listdir(os.path.join(root, label_type))):
            edir = os.path.join(root, label_type, expression)
            for clip in sorted(os.listdir(edir)):
                stem, _, transform = clip.rpartition("-")
                frames = []
                for name in os.listdir(os.path.join(edir, clip)):
                    m = _FRAME.match(name)
                    if m:
                        frames.append((int(m.group("idx")), os.path.join(edir, clip, name)))
                if stem and frames:
                    clips.append({"type": label_type, "expression": expression, "stem": stem, "transform": transform,
                                  "frames": [p for _, p in sorted(frames)]})
    return clips


def cut_windows(rows: np.ndarray, window: int = WINDOW, stride: int = 5) -> np.ndarray:
    """[n, F] rows of one clip -> [k, window, F]: a window every `stride` rows while a full one
    fits; a clip shorter than a window gives one window, right-padded with zero rows."""
    rows = np.asarray(rows)
    n, F = rows.shape
    if n == 0:
        return np.zeros((0, window, F), rows.dtype)
    if n < window:
        out = np.zeros((1, window, F), rows.dtype)
        out[0, :n] = rows
        return out
    return np.stack([rows[s:s + window] for s in range(0, n - window + 1, stride)])


def class_names(clips, classes_file=None):
    if classes_file:
        with open(classes_file) as f:
            names = [ln.strip() for ln in f if ln.strip()]
    else:
        names = sorted({c["expression"] for c in clips})
    if len(set(names)) != len(names):
        raise ValueError("duplicate class names")
    return names


def split_stems(clips, val_share: float, seed: int):
    """The validation stems: a seeded val_share of the distinct (type, expression, stem) videos,
    at least one when val_share > 0 and there are two or more videos."""
    videos = sorted({(c["type"], c["expression"], c["stem"]) for c in clips})
    n_val = int(round(val_share * len(videos)))
    if val_share > 0 and len(videos) > 1:
        n_val = min(max(n_val, 1), len(videos) - 1)
    order = np.random.RandomState(seed).permutation(len(videos))
    return {videos[i] for i in order[:n_val]}


def build_dataset(base: str, classes_file=None, stride: int = 5, val_share: float = 0.2, seed: int = 0,
                  window: int = WINDOW, keep_rows: bool = False):
    """The tree -> dict(names, train=(windows, labels), val=(windows, labels), clips): fp32 windows
    [n, window, 156], int32 labels.  A clip whose expression is not in the class list is an error.
    keep_rows: also train_rows = (the fp32 [n_k, 156] rows of every training clip, one label per
    clip), in the order the training windows were cut from them."""
    clips = scan_tree(base)
    names = class_names(clips, classes_file)
    index = {n: i for i, n in enumerate(names)}
    val_videos = split_stems(clips, val_share, seed)
    parts = {"train": ([], []), "val": ([], [])}
    train_rows = ([], [])
    for c in clips:
        if c["expression"] not in index:
            raise ValueError("expression %r is not in the class list" % c["expression"])
        rows = []
        for p in c["frames"]:
            with open(p) as f:
                rows.append(frame_row(f.read()))
        rows = np.array(rows).reshape(len(rows), N_FEATURES)
        w = cut_windows(rows, window, stride).astype(np.float32)
        in_val = (c["type"], c["expression"], c["stem"]) in val_videos
        part = parts["val" if in_val else "train"]
        if keep_rows and not in_val:
            train_rows[0].append(rows.astype(np.float32))
            train_rows[1].append(index[c["expression"]])
        part[0].append(w)
        part[1].append(np.full(len(w), index[c["expression"]], np.int32))
    out = {"names": names, "clips": clips}
    for k, (ws, ls) in parts.items():
        out[k] = (np.concatenate(ws) if ws else np.zeros((0, window, N_FEATURES), np.float32),
                  np.concatenate(ls) if ls else np.zeros(0, np.int32))
    if keep_rows:
        out["train_rows"] = (train_rows[0], np.array(train_rows[1], np.int32))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--features", required=True, help="the extractor's --out directory")
    ap.add_argument("--out", required=True, help="weights file (.npz)")
    ap.add_argument("--classes", help="file with one expression per line (default: the sorted folder names)")
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--val-share", type=float, default=0.2)
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--p-drop", type=float, default=0.2)
    ap.add_argument("--p-rec", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", help="start from these weights (.npz) instead of keras' initialisers")
    ap.add_argument("--augment", default=None,
                    help="keypoint-space augmentation of every training window at every step, e.g. "
                         "rot:15,scale:0.1,shift:0.05,speed:0.2,tshift:3,drop:0.1,jitter:2 "
                         "(islpose.sign_augment.WindowAugment.parse); default: none")
    ap.add_argument("--frame", default="1920,1080", help="--augment: W,H of the videos' frames")
    ap.add_argument("--clips", action="store_true",
                    help="keep the rows per clip and cut the windows on the GPU (SignTrainer.fit_clips)")
    a = ap.parse_args()

    from islpose.sign_augment import WindowAugment
    augment = WindowAugment.parse(a.augment, frame=tuple(float(v) for v in a.frame.split(",")))
    data = build_dataset(a.features, a.classes, a.stride, a.val_share, a.seed, keep_rows=a.clips)
    from islpose.train import SignTrainer
    tr = SignTrainer(a.weights, N_FEATURES, len(data["names"]), a.p_drop, a.p_rec, a.seed, a.lr)
    tr.calibrate_bn0(data["train"][0])
    val = data["val"] if len(data["val"][0]) else None
    for ep in range(a.epochs):
        if a.clips:
            row = tr.fit_clips(data["train_rows"][0], data["train_rows"][1], 1, a.batch, val, shuffle_seed=a.seed + ep,
                               augment=augment, window=WINDOW, stride=a.stride)[0]
        else:
            row = tr.fit(data["train"][0], data["train"][1], 1, a.batch, val, shuffle_seed=a.seed + ep,
                         augment=augment)[0]
        row["epoch"] = ep
        print(json.dumps(row), flush=True)
    out = a.out if a.out.endswith(".npz") else a.out + ".npz"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    tr.save(out)
    with open(os.path.join(os.path.dirname(os.path.abspath(out)), "classes.json"), "w") as f:
        json.dump(data["names"], f)
    print(json.dumps({"weights": out, "classes": len(data["names"]), "train_windows": int(len(data["train"][0])),
                      "val_windows": int(len(data["val"][0]))}))


if __name__ == "__main__":
    main()
