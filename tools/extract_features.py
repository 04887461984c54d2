"""Config 5 driver: dataset CSV of videos -> per-frame keypoint JSON + feature CSVs,
one process per GPU (the MI355X form of the reference's extract_features_mp.py).

  # 1 GPU
  python tools/extract_features.py --csv sample.csv --dataset-base data/ --out features/
  # 8 GPUs of one node (videos sharded across ranks, no collective on the data path)
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
      tools/extract_features.py --csv sample.csv --dataset-base data/ --out features/

Videos are .npy uint8 [T,H,W,3] RGB arrays (pims / torchvision.io are absent from
this image); --synthetic T,H,W makes seeded frames for a throughput run.
Weights: --body-weights / --hand-weights flat caffe-named dicts (torch.load,
weights_only=True), or synthetic weights when omitted.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isl-signlanguage-translation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv", help="dataset CSV with Filepath,type,expression columns")
    ap.add_argument("--dataset-base", default=".")
    ap.add_argument("--out", required=True)
    ap.add_argument("--body-weights")
    ap.add_argument("--hand-weights")
    ap.add_argument("--batch", type=int, default=64, help="frames of one video per GPU call (Mode R nets fill the GPU from ~64)")
    ap.add_argument("--synthetic", help="T,H,W: synthetic videos instead of .npy files")
    ap.add_argument("--videos", type=int, default=4, help="number of synthetic videos (without --csv)")
    ap.add_argument("--no-resume", action="store_true")
    ap.add_argument("--no-json", action="store_true", help="skip per-frame JSON files (throughput runs)")
    ap.add_argument("--no-export", action="store_true",
                    help="leave out the get_bodypose/get_handpose columns (the reference raises on >2 hands there)")
    ap.add_argument("--precision", choices=["fp32", "fp16"], default=None,
                    help="precision of the body and hand nets' convolutions (Body / Hand precision=): fp16 = one "
                         "fp16 product per multiply-add instead of three, faster, ~2e-3 of the maps' maximum in "
                         "error; default: the library's (fp32 unless ISLPOSE_PRECISION=fp16)")
    ap.add_argument("--thre1", type=float, default=None, help="body peak threshold (body.py:43; default 0.1)")
    ap.add_argument("--thre2", type=float, default=None, help="PAF sample threshold (body.py:44; default 0.05)")
    ap.add_argument("--hand-thre", type=float, default=None, help="hand map threshold (hand.py:62; default 0.05)")
    ap.add_argument("--max-people", type=int, default=None,
                    help="keep the N best-scoring persons of a frame (1: the signer only, at most two hand "
                         "crops per frame); default: no cap")
    ap.add_argument("--hand-scales", default=None,
                    help="the hand pyramid as comma-separated scales of 368 px, e.g. 0.5,1.0 (hand.py:25; default "
                         "0.5,1.0,1.5,2.0; fewer or smaller scales are faster)")
    ap.add_argument("--flip-left", action="store_true",
                    help="mirror left-hand crops before the hand net and the keypoints back (OpenPose's extractor; "
                         "not in the reference)")
    ap.add_argument("--hand-info", action="store_true",
                    help="add a hand_info key to every frame's JSON: per hand its person, is_left, box and the 21 "
                         "keypoint scores (0.0: not found)")
    ap.add_argument("--augment", default=None,
                    help="also extract augmented variants of every frame, as the reference's "
                         "extract_featuressingle.py does: comma-separated rotation:DEGREES (RandomRotation) and "
                         "solarize:THRESHOLD[:P] (RandomSolarize), e.g. rotation:30,solarize:192; each goes to "
                         "<stem>-<TransformClassName>/ with its name in the row's transform column")
    ap.add_argument("--write-jpg", action="store_true",
                    help="also write the reference's stick-model picture of every frame (extract_features_mp.py:"
                         "85-91) as <stem>-<idx>.jpg beside its JSON; needs Pillow")
    ap.add_argument("--jpg-workers", type=int, default=4, help="JPEG encoder threads of --write-jpg")
    ap.add_argument("--jpg-quality", type=int, default=75, help="JPEG quality of --write-jpg (Pillow's default 75)")
    ap.add_argument("--augment-seed", type=int, default=0,
                    help="seed of the --augment draws (per frame: seed, video name, frame index, position)")
    a = ap.parse_args()
    hand_scales = tuple(float(v) for v in a.hand_scales.split(",")) if a.hand_scales else None

    import torch
    from islpose import augment, pipeline, synth
    from islpose.parallel import dist_env

    transforms = augment.parse_spec(a.augment, seed=a.augment_seed)
    rank, local, world = dist_env()
    group = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")          # host-side gather of per-frame results only
    torch.cuda.set_device(local)

    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPos

    def weights(path, kind):
        if path:
            return path
        return {k: torch.from_numpy(v) for k, v in synth.synth_weights(kind).items()}

    body = Body(weights(a.body_weights, 0), "body25", precision=a.precision)
    hand = Hand(weights(a.hand_weights, 2), precision=a.precision)
    model = ISLSignPos(body.model, hand.model, thre1=a.thre1, thre2=a.thre2, hand_thre=a.hand_thre,
                       max_people=a.max_people, hand_scales=hand_scales, flip_left=a.flip_left,
                       hand_info=a.hand_info)

    if a.synthetic:
        T, H, W = (int(v) for v in a.synthetic.split(","))
        decode = pipeline.synthetic_decoder(T, H, W)
    else:
        decode = pipeline.npy_decoder(a.dataset_base)
    rows = pipeline.read_dataset_csv(a.csv) if a.csv else \
        [{"Filepath": "synthetic/v%03d.npy" % i, "type": "synthetic", "expression": "e%d" % (i % 4)}
         for i in range(a.videos)]

    t0 = time.time()
    merged, stats = pipeline.run(rows, decode, model, a.out, rank, world, batch=a.batch,
                                 resume=not a.no_resume, write_json=not a.no_json, group=group,
                                 export=not a.no_export, transforms=transforms,
                                 **({"write_jpg": True, "jpg_workers": a.jpg_workers, "jpg_quality": a.jpg_quality}
                                    if a.write_jpg else {}))
    # (with --augment the extractor's count is units: frames times 1 + the number of transforms)
    stats["units_per_frame"] = 1 + len(transforms or ())
    stats["frames_per_s"] = stats["frames"] / stats["units_per_frame"] / max(time.time() - t0, 1e-9)
    print(json.dumps(stats))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
