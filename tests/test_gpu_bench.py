"""bench.py on the GPU: one plain run with --dump-outputs on a small batch.

The result line carries the headline fields and none of the --full sub-measurements;
the dumped arrays are what the product API computes for the same seeded inputs
(BodyEstimator.post_maps on the designed maps, run_scales on the frames), bit for bit:
the same kernels on the same data.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from islpose import synth
from islpose.body import BodyEstimator, scale_geometry

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, STEPS = 2, 368, 656, 2


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--batch", str(B), "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(str(out / f)) for f in sorted(os.listdir(str(out)))}


def test_plain_line_has_headline_only(run):
    line, _ = run
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["value"] > 0
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    assert line["dtype"].startswith("fp32") and line["roofline"]["frac"] > 0
    assert line["full"] is False
    assert line["mode_r"] is None and line["e2e"] is None and line["cpu_baseline"] is None and "frame" not in line


def test_dump_is_what_the_api_computes(run):
    _, d = run
    assert sorted(d) == ["candidate", "net_heat", "net_paf", "subset"]
    assert d["candidate"].dtype == np.float64 and d["subset"].dtype == np.float64
    assert d["net_paf"].dtype == np.float32 and d["net_heat"].dtype == np.float32
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    (m, nh, nw, vh, vw), = scale_geometry(H, W, (1.0,))
    assert d["net_paf"].shape == (B, 52, nh // 8, nw // 8) and d["net_heat"].shape == (B, 26, nh // 8, nw // 8)
    est = BodyEstimator(synth.synth_weights(0), "body25", scale_search=(1.0,))
    # the records: the post on the designed maps of frames 0..B-1
    maps = [synth.designed_pose_maps(nh // 8, nw // 8, 3, seed=i) for i in range(B)]
    paf = torch.from_numpy(np.stack([p for p, _ in maps])).cuda()
    heat = torch.from_numpy(np.stack([h for _, h in maps])).cuda()
    res = est.post_maps(H, W, [(nh, nw, vh, vw)], [paf], [heat], details=False)
    for f, (cand, subset) in enumerate(res):
        assert len(subset) == 3
        assert np.array_equal(d["candidate"][d["candidate"][:, 0] == f][:, 1:], cand)
        assert np.array_equal(d["subset"][d["subset"][:, 0] == f][:, 1:], subset)
    # the network maps: the same frames through the same kernels
    frames = torch.from_numpy(synth.synth_frames(B, H, W, seed=1000)).cuda()
    _, pafs, heats = est.run_scales(frames, keep_maps=True)
    torch.cuda.synchronize()
    assert np.array_equal(d["net_paf"], pafs[0].cpu().numpy())
    assert np.array_equal(d["net_heat"], heats[0].cpu().numpy())
