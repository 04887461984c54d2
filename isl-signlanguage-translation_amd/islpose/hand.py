"""Batched hand keypoints on the HIP path (frame seam of src/hand.py).

``HandEstimator.estimate(crops)`` runs the 4-scale pyramid of Hand.__call__
(hand.py:25, scales 0.5/1/1.5/2 of 368 px) through the fused pre-processing
kernel and the hand network, then isl_hand_post: cubic resize of every scale
back to the crop, fp64 averaging, fp64 blur, 8-connected components of the
thresholded map, largest-mass component and its first maximum.  Returns int64
[21, 2] (x, y) per crop exactly like the reference (hand.py:74).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import runtime as rt
from .body import BOXSIZE, scale_geometry

HAND_SCALES = rt.HAND_SCALES


CROP_CHUNK = 64     # hand crops per batched pass of estimate_crops


class HandEstimator:
    def __init__(self, weights: dict = None, device: int = 0, scale_search=HAND_SCALES, net: "rt.Net" = None,
                 precision: str = None, *, act_storage: str = None, thre: float = None):
        """precision: 'fp32' or 'fp16' (rt.Net.set_precision) for the net, or None to keep
        the net's own -- fp32 unless ISLPOSE_PRECISION=fp16 was set when it was created.
        act_storage: 'fp32' or 'fp16' (rt.Net.set_act_storage: fp16 activation buffers under
        precision 'fp16', the same results; the small scales keep fp32 buffers), or None to keep
        the net's own.
        thre (rt.check_post_opts' hand_thre): the threshold of the blurred part map (hand.py:62,
        0.05) of every post this estimator runs; None is the reference's constant.
        scale_search (rt.check_hand_opts' hand_scales): the pyramid, None for HAND_SCALES.

        The estimating methods take `flip` (one bool per crop, None for none: a flagged crop
        goes through the net mirrored left to right -- the pre-processing reads crop[:, ::-1] --
        and its detected keypoints come back in the caller's crop, x -> w - 1 - x) and
        `return_scores` (the result is then (peaks int64 [n,21,2], scores float64 [n,21]): the
        scale-averaged map at the returned pixel, 0.0 for a part that was not found, whose peak
        is the reference's [0, 0])."""
        scale_search = rt.check_hand_opts(hand_scales=scale_search)["hand_scales"]
        rt.check_precision(precision)
        rt.check_act_storage(act_storage)
        self.post_opts = rt.check_post_opts(hand_thre=thre)
        self._po = rt.post_opts_struct(self.post_opts)
        self.device = device
        self.scale_search = tuple(scale_search)
        if net is None:
            net = rt.Net(rt.ISL_HAND, device)
            net.load_weights(weights)
        assert net.kind == rt.ISL_HAND
        if precision is not None:
            net.set_precision(precision)
        if act_storage is not None:
            net.set_act_storage(act_storage)
        self.net = net

    def run_scales(self, crops, flip=None):
        import torch
        n, h, w, _ = crops.shape
        fl = flip if rt.flip_array(flip, n) is not None else None
        boxes = [(i, 0, 0, w, h) for i in range(n)] if fl is not None else None
        cur = torch.cuda.current_stream(crops.device)
        # the scales side by side on the lanes of rt.lane_plan, as run_crops
        sg = scale_geometry(h, w, self.scale_search)
        streams, order = rt.lane_plan(self, crops.device, [(g[1], g[2]) for g in sg])
        rt.fork_streams(cur, streams)
        heats = [None] * len(sg)
        for i in order:
            st, (m, nh, nw, vh, vw) = streams[i], sg[i]
            with torch.cuda.stream(st):
                if fl is None:
                    gh, gw = self.net.preprocess(crops, m)
                else:       # the same resize (fx = fy = s * 368 / h), the source read mirrored
                    gh, gw = self.net.preprocess_crops(crops, boxes, self.scale_search[i] * BOXSIZE, flip=fl)
                assert (gh, gw) == (nh, nw)
                heat = torch.empty((n, 22, nh // 8, nw // 8), device=crops.device)
                self.net.run(heat)
            crops.record_stream(st)
            heat.record_stream(cur)
            heats[i] = heat
        rt.join_streams(cur, streams)
        geoms = [(nh, nw, vh, vw) for (m, nh, nw, vh, vw) in sg]
        return geoms, heats

    def post_maps(self, h, w, geoms, heats, out=None, flip=None, return_scores=False):
        """isl_hand_post on low-res maps [n,22,h8,w8] per scale -> int64 [n,21,2]; with
        `out` (a cuda tensor) the result is written there and not synchronised (with
        return_scores the float64 [n,21] cuda tensor of the scores is returned, not
        synchronised either)."""
        import torch
        n = heats[0].shape[0]
        ns = len(geoms)
        dst = out if out is not None else torch.empty((n, 21, 2), dtype=torch.int64, device=heats[0].device)
        g = (rt.IslScaleGeom * ns)(*[rt.IslScaleGeom(*gg) for gg in geoms])
        hp = (ctypes.c_void_p * ns)(*[rt.ptr(t).value for t in heats])
        fl = rt.flip_array(flip, n)
        if fl is None and not return_scores:
            rt.check(rt.lib().isl_hand_post_opts(self.net.h, n, h, w, ns, g, hp, rt.ptr(dst), rt.stream_handle(),
                                                ctypes.byref(self._po)), "isl_hand_post_opts")
            return None if out is not None else dst.cpu().numpy()
        sc = torch.empty((n, 21), dtype=torch.float64, device=heats[0].device) if return_scores else None
        rt.check(rt.lib().isl_hand_post_ex(self.net.h, n, h, w, ns, g, hp, rt.ptr(dst), rt.stream_handle(),
                                          ctypes.byref(self._po), fl, rt.ptr(sc)), "isl_hand_post_ex")
        if out is not None:
            return sc
        return (dst.cpu().numpy(), sc.cpu().numpy()) if return_scores else dst.cpu().numpy()

    def estimate_crops(self, frames, boxes, flip=None, return_scores=False):
        """Batched Hand.__call__ over crops of different sizes: frames uint8 [n,H,W,3]
        (numpy or torch), boxes [(frame_index, x, y, w)] (util.handDetect's square boxes,
        oriImg[y:y+w, x:x+w]) -> int64 [len(boxes), 21, 2] in crop coordinates, equal to
        estimate() on each crop.  The 4 scales run as one batch of all crops each (every
        crop resizes to round(s*368) px); the post runs per crop (its resize-back target
        is the crop size)."""
        import torch
        if flip is not None:
            flip = [bool(v) for v in flip]
            rt.flip_array(flip, len(boxes))
        if len(boxes) == 0:
            return _empty(return_scores)
        t = torch.as_tensor(np.ascontiguousarray(frames) if isinstance(frames, np.ndarray) else frames)
        t = t.to("cuda:%d" % self.device).contiguous()
        out = []
        # bounded batches: the 736 px scale costs ~0.4 GB of activations per crop
        for c in range(0, len(boxes), CROP_CHUNK):
            part = boxes[c:c + CROP_CHUNK]
            fp = flip[c:c + CROP_CHUNK] if flip is not None else None
            peaks = self.post_crops(part, self.run_crops(t, part, fp), fp, return_scores)
            if not self.net.range_ok():
                with self.net.algo_scope("direct"):
                    peaks = self.post_crops(part, self.run_crops(t, part, fp), fp, return_scores)
            out.append(peaks)
        return _concat(out, return_scores)

    def run_crops(self, frames_t, boxes, flip=None):
        """The hand net over all crops, one batch per scale -> low-res heat [n,22,h8,w8] per
        scale.  The scales run side by side on the streams of rt.lane_plan (three lanes, the
        largest scales first), forked from the current stream and joined back (every scale
        has its own arena, table and split-K workspace in the net): the small scales' grids
        fill the CUs the large ones leave idle."""
        import torch
        crops = [(f, x, y, w, w) for (f, x, y, w) in boxes]
        cur = torch.cuda.current_stream(frames_t.device)
        # one lane per net size at most (scales that pad to one size share its arena)
        keys = [rt.crop_net_size(crops[0][4], crops[0][3], s * BOXSIZE) for s in self.scale_search]
        streams, order = rt.lane_plan(self, frames_t.device, keys)
        rt.fork_streams(cur, streams)
        heats = [None] * len(keys)
        for i in order:
            st, s = streams[i], self.scale_search[i]
            with torch.cuda.stream(st):
                gh, gw = self.net.preprocess_crops(frames_t, crops, s * BOXSIZE, flip=flip)
                heat = torch.empty((len(crops), 22, gh // 8, gw // 8), device=frames_t.device)
                self.net.run(heat)
            frames_t.record_stream(st)
            heat.record_stream(cur)
            heats[i] = heat
        rt.join_streams(cur, streams)
        return heats

    def launch_crops(self, frames_t, boxes, flip=None, return_scores=False):
        """Enqueue estimate_crops() on the current stream without waiting (nets, posts,
        peaks to pinned host memory, stream-ordered range check); finish_crops(job)
        completes it."""
        import torch
        if flip is not None:
            flip = [bool(v) for v in flip]
            rt.flip_array(flip, len(boxes))
        if not boxes:      # nothing to enqueue (and no flag copy left in flight into a freed buffer)
            return dict(t=frames_t, boxes=boxes, parts=[], flag=None, ev=None, scores=return_scores)
        parts = []
        for c in range(0, len(boxes), CROP_CHUNK):
            part = boxes[c:c + CROP_CHUNK]
            fp = flip[c:c + CROP_CHUNK] if flip is not None else None
            heats = self.run_crops(frames_t, part, fp)
            out, sc = self._post_crops_dev(part, heats, fp, return_scores)
            host = torch.empty(out.shape, dtype=torch.int64, pin_memory=True)
            host.copy_(out, non_blocking=True)
            hsc = None
            if return_scores:
                hsc = torch.empty(sc.shape, dtype=torch.float64, pin_memory=True)
                hsc.copy_(sc, non_blocking=True)
            parts.append((part, heats, (out, sc), (host, hsc), fp))
        flag = rt.flag_slot(self)
        self.net.check_async(flag)
        ev = torch.cuda.Event()
        ev.record()
        return dict(t=frames_t, boxes=boxes, parts=parts, flag=flag, ev=ev, scores=return_scores)

    def finish_crops(self, job):
        rs = job["scores"]
        if not job["boxes"]:
            return _empty(rs)
        job["ev"].synchronize()
        if int(job["flag"][0]) != 0:     # split-fp16 range left: the whole call again on fp32
            with self.net.algo_scope("direct"):
                return _concat([self.post_crops(part, self.run_crops(job["t"], part, fp), fp, rs)
                                for part, _, _, _, fp in job["parts"]], rs)
        return _concat([(host.numpy(), hsc.numpy()) if rs else host.numpy()
                        for _, _, _, (host, hsc), _ in job["parts"]], rs)

    def post_crops(self, boxes, heats, flip=None, return_scores=False):
        """isl_hand_post per crop (its resize-back target is the crop size) -> int64 [n,21,2]
        (with return_scores: and float64 [n,21])."""
        out, sc = self._post_crops_dev(boxes, heats, flip, return_scores)
        return (out.cpu().numpy(), sc.cpu().numpy()) if return_scores else out.cpu().numpy()

    def _post_crops_dev(self, boxes, heats, flip=None, return_scores=False):
        """-> (peaks, scores or None) on the device, not synchronised."""
        import torch
        n, ns = len(boxes), len(heats)
        out = torch.empty((n, 21, 2), dtype=torch.int64, device=heats[0].device)
        # one call: the crops' kernel chains run side by side on the net's post streams
        ws = (ctypes.c_int32 * n)(*[b[3] for b in boxes])
        g = (rt.IslScaleGeom * (n * ns))()
        for i, b in enumerate(boxes):
            geoms = [gg[1:] for gg in scale_geometry(b[3], b[3], self.scale_search)]
            assert all((gg[0], gg[1]) == (hh.shape[2] * 8, hh.shape[3] * 8) for gg, hh in zip(geoms, heats))
            for si, gg in enumerate(geoms):
                g[i * ns + si] = rt.IslScaleGeom(*gg)
        assert all(hh.is_contiguous() for hh in heats)
        hp = (ctypes.c_void_p * ns)(*[rt.ptr(hh).value for hh in heats])
        fl = rt.flip_array(flip, n)
        if fl is None and not return_scores:
            rt.check(rt.lib().isl_hand_post_crops_opts(self.net.h, n, ws, ns, g, hp, rt.ptr(out), rt.stream_handle(),
                                                      ctypes.byref(self._po)), "isl_hand_post_crops_opts")
            return out, None
        sc = torch.empty((n, 21), dtype=torch.float64, device=heats[0].device) if return_scores else None
        rt.check(rt.lib().isl_hand_post_crops_ex(self.net.h, n, ws, ns, g, hp, rt.ptr(out), rt.stream_handle(),
                                                ctypes.byref(self._po), fl, rt.ptr(sc)), "isl_hand_post_crops_ex")
        return out, sc

    def estimate(self, crops, flip=None, return_scores=False):
        """crops: uint8 [n,h,w,3] or one [h,w,3] (numpy or torch) -> int64 [n,21,2] / [21,2];
        flip: one bool per crop (a single bool for one crop); with return_scores also the
        float64 scores [n,21] / [21]."""
        import torch
        single = crops.ndim == 3
        t = torch.as_tensor(np.ascontiguousarray(crops) if isinstance(crops, np.ndarray) else crops)
        if single:
            t = t[None]
        t = t.to("cuda:%d" % self.device).contiguous()
        n, h, w, _ = t.shape
        if flip is not None:
            flip = [bool(flip)] if single and np.ndim(flip) == 0 else [bool(v) for v in flip]
        geoms, heats = self.run_scales(t, flip)
        res = self.post_maps(h, w, geoms, heats, flip=flip, return_scores=return_scores)
        if not self.net.range_ok():
            # split-fp16 range exceeded: recompute the crops on the fp32 kernels
            with self.net.algo_scope("direct"):
                geoms, heats = self.run_scales(t, flip)
                res = self.post_maps(h, w, geoms, heats, flip=flip, return_scores=return_scores)
        if return_scores:
            return (res[0][0], res[1][0]) if single else res
        return res[0] if single else res


def _empty(return_scores):
    peaks = np.zeros((0, 21, 2), np.int64)
    return (peaks, np.zeros((0, 21), np.float64)) if return_scores else peaks


def _concat(parts, return_scores):
    if return_scores:
        return np.concatenate([p for p, _ in parts]), np.concatenate([s for _, s in parts])
    return np.concatenate(parts)
