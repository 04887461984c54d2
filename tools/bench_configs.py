"""Throughput of the other BASELINE.json configs on one GPU (bench.py measures configs[1]).

  C3  body_25 + handpose, batch 16 frames, 1 person and 2 hand crops per frame
      (crop widths 120-200 px, Hand.__call__'s 4-scale pyramid 184/368/552/736):
      body net (Mode R, scale 0.5 like the ISL scripts) + body post on designed
      1-person maps + one batched hand pass over the 32 crops per step.
  C4  body_25 4-scale pyramid (scale_search 0.5/1/1.5/2 -> nets 184x328 ... 736x1312),
      batch 16 frames per GPU (128 over 8 GPUs, sharded), post on designed maps.

  C5  the video -> JSON pipeline (islpose.pipeline) on 1080x1920 RGB frames, body
      (Mode R) + batched hand crops + per-frame JSON files, sequential vs overlapped.
  FRAME  the unchanged scripts' per-frame path: ISLSignPos.call on one 1080x1920 frame at a
      time (extract_features_mp.py:125-130, model(frame[:, :, ::-1])), with the C5 tamed body
      weights (hand crops up to ~1000 px); wall time per call, split into the body part
      (bodypos + handDetect on the same frames) and the hand part (the rest).
  C6  translator head: the HIP sign classifier (csrc/sign.hip) on [B, 20, 156]
      windows -- latency of one window (the demo's per-frame call) and throughput
      of a batch of 4096 windows; plus translate_stream over a 64-frame clip
      (body + hands once per frame, 45 windows classified in one launch).

  TRAIN  (--config train only) SignTrainer.step (csrc/sign_train.hip) at the workload's own shape:
      batch 256, T 20, F 156, C 167, dropout 0.2 / 0.2, Adam; HIP events, 10 warm-up calls and 30
      timed.  Interleaved with it, the same step written as batched torch ops on the GPU (the
      definition of DESIGN.md 4.2k vectorised over the batch, autograd, torch's own dropout
      draws), and the forward-only isl_sign_classify at 256 windows.  Appends the result to
      profiles/signtrain/train.jsonl.

Prints one JSON line per config: frames/s, ms per step and the conv TFLOP/s of the
step (direct-conv FLOP count, HIP events around the whole step).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isl-signlanguage-translation_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def conv_gflop(kind, h, w):
    from islpose import netspec
    g, H, W = 0.0, h, w
    for c in netspec.convs_for(kind):
        g += 2.0 * c.cout * c.cin * c.k * c.k * H * W / 1e9
        if c.name in ("conv1_2", "conv2_2", "conv3_4"):
            H, W = H // 2, W // 2
    return g


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def c3(args):
    from islpose import synth
    from islpose.body import BodyEstimator, scale_geometry
    from islpose.hand import HandEstimator, HAND_SCALES
    B, H, W = args.batch, 368, 656
    body = BodyEstimator(synth.synth_weights(0), "body25", scale_search=(0.5,), max_people=args.max_people)
    scales = args.hand_scales or HAND_SCALES
    hand = HandEstimator(synth.synth_weights(2), scale_search=scales)
    frames = torch.from_numpy(synth.synth_frames(B, H, W, seed=5)).cuda()
    (m, nh, nw, vh, vw), = scale_geometry(H, W, (0.5,))
    maps = [synth.designed_pose_maps(nh // 8, nw // 8, 1, seed=i) for i in range(B)]
    paf = torch.from_numpy(np.stack([a for a, _ in maps])).cuda()
    heat = torch.from_numpy(np.stack([b for _, b in maps])).cuda()
    rng = np.random.RandomState(0)
    boxes = []
    for f in range(B):
        for _ in range(2):
            w = int(rng.randint(120, 201))
            boxes.append((f, int(rng.randint(0, W - w)), int(rng.randint(0, H - w)), w))
    flip = [k % 2 == 0 for k in range(len(boxes))] if args.flip_left else None   # the first crop of a frame: left

    # designed hand maps for the post (random weights give dense maps: one giant component
    # per plane, unlike real footage); the hand nets still run in full on every crop
    hgeo = [((round(s * 368) + 7) // 8, (round(s * 368) + 7) // 8) for s in scales]
    hmaps = [torch.from_numpy(np.stack([synth.designed_hand_maps(int(hh), int(ww), seed=31 * i + k)
                                        for i in range(len(boxes))])).cuda()
             for k, (hh, ww) in enumerate(hgeo)]

    def step():
        body.net.preprocess(frames, m)
        body.net.run()
        body.post_maps(H, W, [(nh, nw, vh, vw)], [paf], [heat], details=False)
        heats = hand.run_crops(frames, boxes, flip)
        hand.post_crops(boxes, hmaps if args.designed_hands else heats, flip)

    sec = timed(step, args.steps, args.warmup)
    gf = B * conv_gflop(0, nh, nw) + len(boxes) * sum(conv_gflop(2, 8 * hh, 8 * ww) for hh, ww in hgeo)
    return {"config": "C3 body_25 + hand (2 crops/frame, 4 scales)", "batch": B, "crops": len(boxes),
            "hand_crops_per_frame": round(len(boxes) / B, 2), "max_people": args.max_people,
            "frames_per_s": round(B / sec, 2), "ms_per_step": round(sec * 1e3, 2),
            "conv_gflop_per_step": round(gf, 1), "conv_tflops_fp32_equiv_wall": round(gf / sec / 1e3, 1),
            "hand_scales": list(scales), "flip_left": bool(args.flip_left),
            "hand_post_on": "designed maps" if args.designed_hands else "raw net output (random weights: dense maps)"}


def c4(args):
    from islpose import synth
    from islpose.body import BodyEstimator, scale_geometry
    B, H, W = args.batch, 368, 656
    scales = (0.5, 1.0, 1.5, 2.0)
    body = BodyEstimator(synth.synth_weights(0), "body25", scale_search=scales)
    frames = torch.from_numpy(synth.synth_frames(B, H, W, seed=6)).cuda()
    geo = scale_geometry(H, W, scales)
    pafs, heats = [], []
    for i, g in enumerate(geo):
        mp = [synth.designed_pose_maps(g[1] // 8, g[2] // 8, 3, seed=10 * i + k) for k in range(B)]
        pafs.append(torch.from_numpy(np.stack([a for a, _ in mp])).cuda())
        heats.append(torch.from_numpy(np.stack([b for _, b in mp])).cuda())
    geoms = [g[1:] for g in geo]

    def step():
        for (m, nh, nw, vh, vw) in geo:
            body.net.preprocess(frames, m)
            body.net.run()
        body.post_maps(H, W, geoms, pafs, heats, details=False)

    sec = timed(step, args.steps, args.warmup)
    gf = B * sum(conv_gflop(0, g[1], g[2]) for g in geo)
    return {"config": "C4 body_25 4-scale pyramid", "batch_per_gpu": B, "nets": [[g[1], g[2]] for g in geo],
            "frames_per_s": round(B / sec, 2), "ms_per_step": round(sec * 1e3, 2),
            "conv_gflop_per_step": round(gf, 1), "conv_tflops_fp32_equiv_wall": round(gf / sec / 1e3, 1)}


def c5(args):
    """configs[4]: the extract_features_mp.py:122-132 pipeline on 1080x1920 RGB frames
    (Mode R body net 184x327 -> 184x328, batched hand crops, per-frame JSON files),
    sequential vs overlapped (prefetch + async H2D + GPU flip + writer thread).  --augment
    adds the reference's augmented variants (extract_featuressingle.py:49-52,116-120): the
    unit of work is then (frame, original-or-transform), each a full model pass, and the
    *_frames_per_s figures are reported beside *_units_per_s."""
    import shutil
    import tempfile
    from islpose import augment, pipeline, synth
    from islpose.body import BodyEstimator
    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPos
    transforms = augment.parse_spec(args.augment, seed=args.augment_seed)
    jpg = {"write_jpg": True, "jpg_workers": args.jpg_workers} if args.write_jpg else {}
    per_frame = 1 + len(transforms or ())
    T, H, W = args.c5_frames, 1080, 1920
    B = args.c5_batch
    rgb = synth.synth_frames(T, H, W, seed=57)
    # heat layer tamed on the GPU net's own output for frame 0 (a few persons per frame)
    wb = synth.synth_weights(0)
    cal = BodyEstimator(wb, "body25", scale_search=(0.5,))
    _, _, heats = cal.run_scales(torch.from_numpy(np.ascontiguousarray(rgb[:1, ..., ::-1])).cuda(), keep_maps=True)
    wb = synth.tame_heat_layer(wb, heats[0].cpu().numpy(), "body25", gain=0.05)
    del cal
    tw = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    isl = ISLSignPos(Body(tw(wb), "body25").model, Hand(tw(synth.synth_weights(2))).model,
                     max_people=args.max_people, hand_scales=args.hand_scales, flip_left=args.flip_left)
    clips = {"v%d.mp4" % k: rgb for k in range(args.c5_videos)}
    rows = [{"Filepath": f, "type": "Greetings", "expression": "hello"} for f in clips]
    res = {"config": "C5 video -> per-frame JSON, 1080x1920 RGB frames", "frames": T * len(rows),
           "videos": len(rows), "batch": B, "export": False, "max_people": args.max_people,
           "hand_scales": list(isl.hand_opts["hand_scales"]), "flip_left": bool(args.flip_left),
           "augment": args.augment or None, "units_per_frame": per_frame,
           "write_jpg": bool(args.write_jpg), "jpg_workers": args.jpg_workers if args.write_jpg else None,
           "decode": "frames already decoded in host memory (pims/ffmpeg absent); the pipeline reads them as "
                     "slices of the [T,H,W,3] array"}
    for ov in ((True,) if args.c5_overlap_only else (False, True)):
        out = tempfile.mkdtemp(prefix="c5_")
        try:
            # warm-up (arenas, hand scales) on the first video, then the timed pass over all
            pipeline.extract_dataset(rows[:1], clips.__getitem__, isl, out, batch=B, export=False, overlap=ov,
                                     transforms=transforms, **jpg)
            shutil.rmtree(out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            feats, ex = pipeline.extract_dataset(rows, clips.__getitem__, isl, out, batch=B,
                                                 export=False, overlap=ov, transforms=transforms, **jpg)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            hands = peaks = 0
            for f in feats:
                hands += len(f["all_hand_peaks"])
                peaks += len(f["candidate"])
        finally:
            shutil.rmtree(out, ignore_errors=True)
        key = "overlap" if ov else "sequential"
        # (the extractor counts units: frames, times 1 + the number of transforms)
        res[key + "_units_per_s"] = round(ex.frames_done / dt, 2)
        res[key + "_frames_per_s"] = round(ex.frames_done / per_frame / dt, 2)
        res[key + "_s"] = round(dt, 3)
        if args.write_jpg:
            res[key + "_jpg_stage_s"] = {k: round(v, 3) for k, v in ex.jpg_seconds.items()}
        res["hand_crops_per_frame"] = round(hands / max(len(feats), 1), 2)     # (per unit with --augment)
        res["body_peaks_per_frame"] = round(peaks / max(len(feats), 1), 2)
    return res


def frame(args):
    """ISLSignPos.call per frame, 1080x1920 RGB frames flipped to BGR as a view (the script's
    frame[:, :, ::-1]); every call returns to the host (numpy results), as in the script."""
    from islpose import runtime as rt, synth
    from islpose.body import BodyEstimator
    from src import util
    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPos
    T, H, W = args.frame_count, 1080, 1920
    rgb = synth.synth_frames(T, H, W, seed=57)
    wb = synth.synth_weights(0)
    cal = BodyEstimator(wb, "body25", scale_search=(0.5,))
    _, _, heats = cal.run_scales(torch.from_numpy(np.ascontiguousarray(rgb[:1, ..., ::-1])).cuda(), keep_maps=True)
    wb = synth.tame_heat_layer(wb, heats[0].cpu().numpy(), "body25", gain=0.05)
    del cal
    tw = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    isl = ISLSignPos(Body(tw(wb), "body25").model, Hand(tw(synth.synth_weights(2))).model,
                     max_people=args.max_people, hand_scales=args.hand_scales, flip_left=args.flip_left)
    body = isl._estimators()[0]
    for i in range(min(5, T)):          # warm-up: arenas of the body and of the hand crop sizes
        isl.call(rgb[i][:, :, ::-1])
    torch.cuda.synchronize()
    crops, widths, persons = 0, [], 0
    # the T frames REPEAT times over (a pass is ~0.35 s: one pass read +-4 % run to run)
    R = max(1, getattr(args, "frame_repeat", 1))
    t0 = time.perf_counter()
    for _ in range(R):
        for i in range(T):
            _, sub, hands = isl.call(rgb[i][:, :, ::-1])
            crops += len(hands)
            persons += len(sub)
    dt = (time.perf_counter() - t0) / R
    crops /= R
    t0 = time.perf_counter()
    for i in range(T):
        f = rgb[i][:, :, ::-1]
        (c, sb), = body.estimate(isl._upload(f))
        widths += [w for _, _, w, _ in util.handDetect(c, sb, f)]
    db = time.perf_counter() - t0
    # conv launches per frame: the body net (one run) and the hand net (one run per scale of the
    # frame's crop batch), from the op variants of their last runs; a split-K layer adds its reduce
    hand = isl._estimators()[1]

    def launches(net):
        codes = [v for _, v in net.op_variants()]
        return sum(1 for v in codes if v not in (-1, -2)) + sum(1 for v in codes if rt.decode_variant(v).get("split"))
    body_launches = launches(body.net)
    # the hand net's conv launches over its four scales for one crop of a frame with hands (each
    # scale run once more, after the timed passes, to read its op variants)
    hand_launches = 0
    if widths:
        from islpose.hand import BOXSIZE
        f = rgb[0][:, :, ::-1]
        x = isl._upload(f)
        w0 = widths[0]
        crop = [(0, 0, 0, w0, w0)]
        for s in hand.scale_search:
            gh, gw = hand.net.preprocess_crops(x, crop, s * BOXSIZE)
            hand.net.run(torch.empty((1, 22, gh // 8, gw // 8), device=x.device))
            torch.cuda.synchronize()
            hand_launches += launches(hand.net)
    return {"config": "FRAME ISLSignPos.call per 1080x1920 frame (extract_features_mp.py:130 pattern)",
            "body_conv_launches_per_frame": body_launches,
            "hand_conv_launches_per_crop_4_scales": hand_launches,
            "frames": T, "passes": R, "frames_per_s": round(T / dt, 2), "ms_per_frame": round(dt / T * 1e3, 3),
            "body_ms_per_frame": round(db / T * 1e3, 3), "hand_ms_per_frame": round((dt - db) / T * 1e3, 3),
            "hand_crops_per_frame": round(crops / T, 2), "persons_per_frame": round(persons / R / T, 2),
            "max_people": args.max_people,
            "hand_scales": list(isl.hand_opts["hand_scales"]), "flip_left": bool(args.flip_left),
            "crop_width_px": [int(min(widths)), int(max(widths))] if widths else [],
            "basis": "wall time of T sequential calls (host frame -> pinned H2D -> GPU flip -> body net + post -> "
                     "handDetect -> hand crops batched per scale -> peaks on the host); body = upload + estimate + "
                     "handDetect on the same frames, hand = the rest"}


def hands2(args):
    """ISLSignPos.hands_for per 1080x1920 frame on a designed one-person body result whose two
    arms give one left and one right hand box of about 300 px: the signer workload's hand path
    alone (boxes -> hand nets per scale -> posts -> assembled results on the host)."""
    from islpose import synth
    from src import util
    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPos
    T, H, W = args.frame_count, 1080, 1920
    tw = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    isl = ISLSignPos(Body(tw(synth.synth_weights(0)), "body25").model, Hand(tw(synth.synth_weights(2))).model,
                     hand_scales=args.hand_scales, flip_left=args.flip_left)
    ests = isl._estimators()
    # shoulder, elbow, wrist of the right (joints 2-4) and left (5-7) arm: forearms of 200 px
    # -> boxes of 1.5 * 200 = 300 px
    pts = {2: (800, 300), 3: (700, 500), 4: (700, 700), 5: (1100, 300), 6: (1200, 500), 7: (1200, 700)}
    cand = np.array([[x, y, 0.9, k] for k, (x, y) in enumerate(pts.values())], np.float64)
    sub = -np.ones((1, 27))
    for k, j in enumerate(pts):
        sub[0, j] = k
    sub[0, -2], sub[0, -1] = 6 * 0.9, 6
    frames = [torch.from_numpy(f[None]).cuda() for f in synth.synth_frames(T, H, W, seed=57)]
    boxes = util.hand_boxes(cand, sub, frames[0][0])
    crops = 0
    for t in frames[:min(3, T)]:
        isl.hands_for(t, [(cand, sub)], ests)
    torch.cuda.synchronize()
    R = max(1, args.frame_repeat)
    t0 = time.perf_counter()
    for _ in range(R):
        for t in frames:
            crops += len(isl.hands_for(t, [(cand, sub)], ests)[0][2])
    dt = (time.perf_counter() - t0) / R
    return {"config": "HANDS2 ISLSignPos.hands_for per 1080x1920 frame, one designed person, two hand boxes",
            "frames": T, "passes": R, "frames_per_s": round(T / dt, 2), "ms_per_frame": round(dt / T * 1e3, 3),
            "hand_crops_per_frame": round(crops / R / T, 2),
            "boxes": [[int(b[0]), int(b[1]), int(b[2]), bool(b[3])] for b in boxes],
            "hand_scales": list(isl.hand_opts["hand_scales"]), "flip_left": bool(args.flip_left)}


def render(args):
    """isl_draw on 64 resident 1080x1920 frames, each with HANDS2's designed arms (plus neck, nose
    and mid-hip) and two designed hands (their 21 peaks spread over the two hand boxes): ms per batch in place, out of
    place and on the blank canvas (HIP events around `steps` launches with a prebuilt table, so
    the figure is the upload of the table plus the kernel), out-of-place bytes per second against
    the 2*H*W*3 floor beside isl_augment's plain copy of the same frames on the same box, the wall
    time of islpose.render.apply (which also builds the records), and apply_numpy per frame."""
    from islpose import augment, render as rd, runtime as rt, synth
    from src import util
    B, H, W = 64, 1080, 1920
    pts = {2: (800, 300), 3: (700, 500), 4: (700, 700), 5: (1100, 300), 6: (1200, 500), 7: (1200, 700),
           1: (950, 280), 0: (950, 180), 8: (950, 640)}
    cand = np.array([[x, y, 0.9, k] for k, (x, y) in enumerate(pts.values())], np.float64)
    sub = -np.ones((1, 27))
    for k, j in enumerate(pts):
        sub[0, j] = k
    sub[0, -2], sub[0, -1] = len(pts) * 0.9, len(pts)
    frames = torch.from_numpy(synth.synth_frames(B, H, W, seed=57)).cuda()
    hands = []
    for x, y, w, _left, _row in util.hand_boxes(cand, sub, frames[0]):
        rng = np.random.RandomState(x)
        hands.append(np.stack([x + rng.randint(10, w - 10, 21), y + rng.randint(10, w - 10, 21)], axis=1).astype(np.int64))
    one = rd.body_primitives(cand, sub, "body25") + rd.hand_primitives(hands)
    lists = [one] * B
    flat = [rt.IslDrawPrim(q.kind, q.p, q.c, q.s, q.r2, q.color, q.blend, 0) for lst in lists for q in lst]
    arr = (rt.IslDrawPrim * len(flat))(*flat)
    first = [len(one) * f for f in range(B + 1)]
    work, dst = frames.clone(), torch.empty_like(frames)
    reps = max(args.steps, 1) * 10

    def events(step):
        for _ in range(max(args.warmup, 10)):      # (past the eight table slots' first-use allocations)
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_in = events(lambda: rt.draw(work, work, arr, first))
    ms_out = events(lambda: rt.draw(frames, dst, arr, first))
    ms_blank = events(lambda: rt.draw(None, dst, arr, first))
    copies = [rt.IslAugItem(1.0, 0.0, i, 0, 256, 0) for i in range(B)]
    ms_copy = events(lambda: rt.augment(frames, copies, out=dst))
    wall = timed(lambda: rd.apply(frames, lists, out=dst), args.steps, args.warmup)
    host = frames[:1].cpu().numpy()
    t0 = time.perf_counter()
    ref = rd.apply_numpy(host, lists[:1])
    t_np = time.perf_counter() - t0
    same = bool(np.array_equal(rd.apply(frames[:1].contiguous(), lists[:1]).cpu().numpy(), ref))
    floor = 2.0 * H * W * 3 * B
    tiles = ((W + 127) // 128) * ((H + 15) // 16)
    return {"config": "RENDER isl_draw on 64 resident 1080x1920 frames, one designed person and two hands each",
            "frames": B, "prims_per_frame": len(one), "launches_timed": reps,
            "in_place_ms": round(ms_in, 4), "out_of_place_ms": round(ms_out, 4), "blank_ms": round(ms_blank, 4),
            "floor_bytes": floor, "out_of_place_tb_per_s": round(floor / ms_out / 1e9, 3),
            "augment_copy_ms": round(ms_copy, 4), "augment_copy_tb_per_s": round(floor / ms_copy / 1e9, 3),
            "apply_wall_ms": round(wall * 1e3, 3), "apply_numpy_ms_per_frame": round(t_np * 1e3, 2),
            "gpu_equals_apply_numpy": same, "tiles_per_frame": tiles,
            "basis": "HIP events around the timed launches on one stream, each launch with its table upload"}


def c6(args):
    from islpose import synth, translate
    from src.body import Body
    from src.hand import Hand
    from src.ISL_Model_parameter import ISLSignPosTranslator
    clf = translate.SignClassifier()
    rng = np.random.RandomState(0)
    res = {"config": "C6 translator head (sign classifier + translate_stream)"}
    for B in (1, 4096):
        x = torch.from_numpy(rng.uniform(0, 600, (B, 20, 156)).astype(np.float32)).cuda()
        out = torch.empty(B, clf.n_classes, device="cuda")
        sec = timed(lambda: clf(x), args.steps * 10, args.warmup)
        res["windows_%d_us" % B] = round(sec * 1e6, 1)
        res["windows_%d_per_s" % B] = round(B / sec, 1)
        del out
    print(json.dumps(res), flush=True)
    wts = lambda k: {n: torch.from_numpy(v) for n, v in synth.synth_weights(k).items()}  # noqa: E731
    t = ISLSignPosTranslator(Body(wts(0), "body25").model, Hand(wts(2)).model, clf)
    full = t.call_batch
    n_hands = []

    def two_hands(f):      # random weights detect many people; keep <= 2 hands per frame for the export
        r = full(f)
        n_hands.append(sum(len(h) for _, _, h in r))
        return [(c, s, h[:2]) for c, s, h in r]
    t.call_batch = two_hands
    frames = synth.synth_frames(64, 368, 656, seed=4)
    sec = timed(lambda: t.translate_stream(frames), args.steps, args.warmup)
    res.update({"stream_frames": 64, "stream_windows": 45, "stream_ms": round(sec * 1e3, 1),
                "stream_frames_per_s": round(64 / sec, 1),
                "stream_hand_crops_per_clip": int(sum(n_hands) / (args.steps + args.warmup)),
                "stream_note": "synthetic weights: hand crops per clip is set by the random body net"})
    return res


def torch_train_step(params, opt, x, y, p_drop, p_rec):
    """The training step of DESIGN.md 4.2k as batched torch ops (frozen BN statistics, masks,
    one recurrent-dropout mask per direction and window), autograd and `opt`; returns l_b."""
    B, T, _ = x.shape
    U = 32
    w = params

    def drop(shape, p):
        return (torch.rand(shape, device=x.device) >= p).float() / (1.0 - p) if p > 0 else None

    def bn(v, p):
        return (v - p[2]) / torch.sqrt(p[3] + 1e-3) * p[0] + p[1]

    mask = (x != 0).any(dim=2)

    def lstm(inp, K, R, b, reverse, seq):
        zx = inp @ K + b
        h = torch.zeros(B, U, device=x.device)
        c = torch.zeros(B, U, device=x.device)
        rm = drop((B, U), p_rec)
        rows = [None] * T
        for s in range(T):
            t = T - 1 - s if reverse else s
            z = zx[:, t] + (h if rm is None else h * rm) @ R
            i, f, g, o = z.split(U, dim=1)
            c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h2 = torch.sigmoid(o) * torch.tanh(c2)
            mk = mask[:, t:t + 1]
            c, h = torch.where(mk, c2, c), torch.where(mk, h2, h)
            if seq:
                rows[t] = torch.where(mk, h2, torch.zeros_like(h2))
        return (torch.stack(rows, 1) if seq else None), h

    def dropped(v, p):
        m = drop(v.shape, p)
        return v if m is None else v * m

    xn = bn(x, w[0:4])
    f1, _ = lstm(xn, w[4], w[5], w[6], False, True)
    b1, _ = lstm(xn, w[7], w[8], w[9], True, True)
    yseq = dropped(torch.cat([f1, b1], 2), p_drop)
    _, hf = lstm(yseq, w[10], w[11], w[12], False, False)
    _, hb = lstm(yseq, w[13], w[14], w[15], True, False)
    v = torch.nn.functional.elu(torch.cat([hf, hb], 1))
    v = torch.nn.functional.elu(dropped(bn(v @ w[16], w[17:21]), p_drop))
    v = dropped(torch.nn.functional.elu(bn(v @ w[21], w[22:26])), p_drop)
    loss = torch.nn.functional.cross_entropy(v @ w[26] + w[27], y, reduction="none")
    opt.zero_grad(set_to_none=True)
    loss.mean().backward()
    opt.step()
    return loss.detach()


def train(args):
    from islpose import translate
    from islpose.train import SignTrainer
    B, T, F, C = 256, 20, 156, 167
    rng = np.random.RandomState(0)
    xh = rng.uniform(0, 600, (B, T, F)).astype(np.float32)
    xh[rng.rand(B, T) < 0.2] = 0
    x = torch.from_numpy(xh).cuda()
    y = torch.from_numpy(rng.randint(0, C, B).astype(np.int64)).cuda()
    y32 = y.to(torch.int32)
    tr = SignTrainer(None, F, C, p_drop=0.2, p_rec=0.2)
    tr.calibrate_bn0(xh)
    stat = (2, 3, 19, 20, 24, 25)
    tw = [torch.from_numpy(a).cuda().requires_grad_(k not in stat) for k, a in enumerate(tr.weights())]
    topt = torch.optim.Adam([p for p in tw if p.requires_grad], lr=1e-3, eps=1e-7)
    clf = tr.classifier()
    runs = {"hip_step": lambda: tr.step(x, y32), "torch_step": lambda: torch_train_step(tw, topt, x, y, 0.2, 0.2),
            "classify": lambda: clf(x)}
    if args.augment:                                  # --augment SPEC: the step with its batch built by isl_sign_augment
        from islpose.sign_augment import WindowAugment
        aug = WindowAugment.parse(args.augment, seed=args.augment_seed)
        rows, ids = x.view(B * T, F), np.arange(B, dtype=np.uint64)
        row0 = np.arange(B, dtype=np.int64) * T
        runs["hip_step_aug"] = lambda: tr.step(x, y32, augment=aug)
        runs["augment_only"] = lambda: aug.apply(rows, aug.items(ids, tr.step_count, T, row0), T, tr.step_count)
    warm, steps, rounds = 10, 30, 3
    for fn in runs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):                       # interleaved: one block of timed calls each, in turn
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps // rounds):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / (steps // rounds))
    res = {"config": "TRAIN SignTrainer.step, batch 256, T 20, F 156, C 167, dropout 0.2 / 0.2, Adam",
           "basis": "HIP events around blocks of %d calls, %d blocks each, interleaved; %d warm-up calls"
                    % (steps // rounds, rounds, warm)}
    for k, v in ms.items():
        res[k + "_us"] = [round(t * 1e3, 1) for t in v]
        res[k + "_windows_per_s"] = round(B / (float(np.median(v)) * 1e-3), 1)
    res["torch_over_hip"] = round(float(np.median(ms["torch_step"]) / np.median(ms["hip_step"])), 2)
    if args.augment:
        res["augment"] = args.augment
    out = os.path.join(REPO, "profiles", "signaug" if args.augment else "signtrain")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "train.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["c3", "c4", "c5", "c6", "frame", "hands2", "render", "train", "all"], default="all")
    ap.add_argument("--frame-count", type=int, default=64, help="FRAME: sequential per-frame calls timed")
    ap.add_argument("--frame-repeat", type=int, default=4, help="FRAME: timed passes over the frames")
    ap.add_argument("--batch", type=int, default=16, help="C3 / C4 frames per step")
    ap.add_argument("--c5-batch", type=int, default=32, help="C5 frames per pipeline batch")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--c5-frames", type=int, default=96, help="C5: frames per (synthetic 1080p) video")
    ap.add_argument("--c5-videos", type=int, default=3)
    ap.add_argument("--c5-overlap-only", action="store_true")
    ap.add_argument("--raw-hand-maps", dest="designed_hands", action="store_false",
                    help="C3: run the hand post on the raw net maps instead of designed maps")
    ap.add_argument("--precision", choices=["fp32", "fp16"], default=None,
                    help="precision of the x3 convs of every net (rt.Net.set_precision): fp32 = three fp16 "
                         "products per multiply-add (fp32-accurate, the default), fp16 = one (faster, ~2e-3 "
                         "of the maps' maximum in error); default: the library's (env ISLPOSE_PRECISION)")
    ap.add_argument("--act-storage", choices=["fp32", "fp16"], default=None,
                    help="storage of the activations between the fp16-precision convs of every net "
                         "(rt.Net.set_act_storage): fp16 halves the activation buffers at the same bits; "
                         "default: the library's (env ISLPOSE_ACT_STORAGE)")
    ap.add_argument("--max-people", type=int, default=None,
                    help="FRAME / C3 / C5: keep the N best-scoring persons of a frame (ISLSignPos / BodyEstimator "
                         "max_people; 1: the signer only, at most two hand crops per frame); default: no cap")
    ap.add_argument("--hand-scales", default=None,
                    help="FRAME / C3 / C5 / HANDS2: the hand pyramid as comma-separated scales of 368 px "
                         "(default 0.5,1.0,1.5,2.0)")
    ap.add_argument("--flip-left", action="store_true",
                    help="FRAME / C3 / C5 / HANDS2: mirror left-hand crops before the hand net (C3: every first "
                         "crop of a frame)")
    ap.add_argument("--augment", default=None,
                    help="C5: augmented variants per frame, e.g. rotation:30,solarize:192 (RandomRotation / "
                         "RandomSolarize, islpose.augment.parse_spec); TRAIN: also time the step with its batch "
                         "augmented in keypoint space, e.g. rot:15,scale:0.1,tshift:3,drop:0.1 "
                         "(islpose.sign_augment.WindowAugment.parse); default: none")
    ap.add_argument("--augment-seed", type=int, default=0, help="C5: seed of the --augment draws")
    ap.add_argument("--write-jpg", action="store_true",
                    help="C5: also write every frame's stick-model JPEG (KeypointExtractor write_jpg)")
    ap.add_argument("--jpg-workers", type=int, default=4, help="C5: JPEG encoder threads of --write-jpg")
    a = ap.parse_args()
    a.hand_scales = tuple(float(v) for v in a.hand_scales.split(",")) if a.hand_scales else None
    if a.precision:
        os.environ["ISLPOSE_PRECISION"] = a.precision   # read by every net at its creation
    if a.act_storage:
        os.environ["ISLPOSE_ACT_STORAGE"] = a.act_storage
    if a.config == "train":                          # writes its profile; not part of "all"
        print(json.dumps(train(a)), flush=True)
        return
    for name, fn in (("c3", c3), ("c4", c4), ("c5", c5), ("c6", c6), ("frame", frame),
                     ("hands2", hands2), ("render", render)):
        if a.config in (name, "all"):
            res = fn(a)
            res["precision"] = os.environ.get("ISLPOSE_PRECISION", "fp32")
            res["act_storage"] = os.environ.get("ISLPOSE_ACT_STORAGE", "fp32")
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
