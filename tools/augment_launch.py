"""The augment launch alone (isl_augment, csrc/augment.hip), for a rocprofv3 --kernel-trace
--stats run: `--frames` 1080x1920 frames resident, one original plus a RandomRotation(30) and
a RandomSolarize(192) variant of each in one launch, `--reps` launches.  Prints the byte floor
(2*H*W*3 per item) and the wall time per launch between events as one JSON line; the kernel's
own duration comes from the profiler."""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isl-signlanguage-translation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--mode", choices=["mixed", "copy", "rotate", "solarize"], default="mixed",
                    help="mixed: original + rotation + solarize per frame; else every item of one kind")
    a = ap.parse_args()
    import torch
    from islpose import augment
    H, W = a.height, a.width
    g = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randint(0, 256, (a.frames, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    ts = [augment.RandomRotation(30), augment.RandomSolarize(192, 1.0)]
    kinds = {"mixed": (None, 0, 1), "copy": (None,) * 3, "rotate": (0,) * 3, "solarize": (1,) * 3}[a.mode]
    items = []
    for i in range(a.frames):
        for k in kinds:
            items.append(augment.item(i, None if k is None else augment.params_for(ts[k], "clip", i, k)))
    out = augment.apply(src, items, swap_rb=True)         # warm-up: the table ring, the allocator
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        out = augment.apply(src, items, swap_rb=True)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    floor = 2 * H * W * 3 * len(items)
    print(json.dumps({"mode": a.mode, "items": len(items), "H": H, "W": W, "floor_bytes": floor,
                      "ms_per_launch_events": round(ms, 4), "floor_GBps_events": round(floor / ms / 1e6, 1),
                      "checksum": int(out[::17, ::97, ::89].sum().item())}))


if __name__ == "__main__":
    main()
