"""Drop-in for the reference's src/body.py: ``Body(model_path, model_type)``.

Same constructor (body.py:16-37: model_type 'coco' | 'body25', anything else
prints a message and falls back to COCO; weights through util.transfer) and
the same call (body.py:39-235): ``Body(...)(oriImg) -> (candidate, subset)``
with identical dtypes, shapes and values.  The whole call runs on the GPU
(pre-processing, network, resize, blur/NMS, PAF, assembly) -- on a host without a
visible HIP device, on the CPU instead (islpose.cpu, as the reference); ``scale_search``
defaults to the reference's [0.5] and can be changed per instance.
``precision`` (keyword only, not in the reference) selects the arithmetic of the GPU
convolutions: 'fp32', or 'fp16' (one fp16 product per multiply-add, faster, ~2e-3 of the maps'
maximum in error); the default None is the library's own, fp32 unless ISLPOSE_PRECISION=fp16
is set.  An unknown value raises ValueError.  The CPU path is fp32 whatever
is given.
``act_storage`` (keyword only, not in the reference): 'fp32' or 'fp16' for the buffers between the
GPU convolutions of precision 'fp16' (fp16: half the activation memory, the same results); None
keeps the library's own (fp32 unless ISLPOSE_ACT_STORAGE=fp16 is set); an unknown value raises
ValueError; no effect on the CPU path or under precision 'fp32'.
``thre1``, ``thre2``, ``max_people`` (keyword only, not in the reference, on the GPU and the CPU
path alike): the peak threshold (body.py:43, 0.1), the PAF sample threshold (body.py:44, 0.05)
and a cap on the persons returned -- when more than ``max_people`` rows of ``subset`` remain
after the reference's pruning, the ``max_people`` rows with the largest total score
``subset[:, -2]`` stay (ties to the lower row, original order; ``candidate`` is unchanged).
None is the reference's constant, and no cap (as ``max_people=0``).  ``thre1`` not a finite
number in [1e-30, 1e30], ``thre2`` not finite or ``max_people < 0`` raises ValueError.
``estimate_batch(frames)`` processes a batch of frames in one pass.
"""
from __future__ import annotations

import numpy as np
import torch

from islpose import cpu
from islpose import runtime as rt
from islpose.body import BodyEstimator

from . import util
from .model import bodypose_25_model, bodypose_model


class Body(object):
    def __init__(self, model_path, model_type="coco", *, precision=None, act_storage=None, thre1=None, thre2=None,
                 max_people=None):
        rt.check_precision(precision)
        rt.check_act_storage(act_storage)
        rt.check_post_opts(thre1=thre1, thre2=thre2, max_people=max_people)
        self.thre1, self.thre2, self.max_people = thre1, thre2, max_people
        if model_type == "coco":
            self.model, self.njoint, self.npaf = bodypose_model(), 19, 38
        elif model_type == "body25":
            self.model, self.njoint, self.npaf = bodypose_25_model(), 26, 52
        else:
            print("not right model_type, use coco")
            self.model, self.njoint, self.npaf = bodypose_model(), 19, 38
        self.model_type = model_type
        if torch.cuda.is_available():
            self.model = self.model.cuda()
        weights = model_path if isinstance(model_path, dict) else torch.load(model_path, map_location="cpu",
                                                                            weights_only=True)
        self.model.load_state_dict(util.transfer(self.model, weights))
        self.model.eval()
        self.precision = precision
        self.model.set_precision(precision)
        self.act_storage = act_storage
        self.model.set_act_storage(act_storage)
        self.scale_search = [0.5]          # body.py:41
        self._est = None

    def estimator(self) -> BodyEstimator:
        dev = torch.cuda.current_device()
        net = self.model.native(dev)
        kind = "body25" if self.model_type == "body25" else "coco"
        if self._est is None or self._est.net is not net or self._est.scale_search != tuple(self.scale_search):
            self._est = BodyEstimator(model_type=kind, device=dev, scale_search=self.scale_search, net=net,
                                      thre1=self.thre1, thre2=self.thre2, max_people=self.max_people)
        return self._est

    def __call__(self, oriImg):
        img = oriImg.cpu().numpy() if isinstance(oriImg, torch.Tensor) else np.asarray(oriImg)
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if not torch.cuda.is_available():   # GPU-less host: the product's CPU path (body.py:31-32)
            return cpu.body_call(img, self._cpu_net, "body25" if self.model_type == "body25" else "coco",
                                 tuple(self.scale_search), thre1=self.thre1, thre2=self.thre2,
                                 max_people=self.max_people)
        return self.estimator().estimate(img)

    def _cpu_net(self, im):
        with torch.no_grad():
            return tuple(o.numpy() for o in self.model(torch.from_numpy(im)))

    def estimate_batch(self, frames):
        """frames: uint8 [n, H, W, 3] (numpy or torch, BGR) -> [(candidate, subset)] * n."""
        if not torch.cuda.is_available():
            return [self(f) for f in frames]
        return self.estimator().estimate(frames)
