"""Drop-in for the reference's src/hand.py: ``Hand(model_path)(oriImg) -> int64 [21, 2]``.

Same constructor (hand.py:16-22) and call (hand.py:24-74): 4-scale pyramid,
fp64 averaging, blur, connected components, largest-mass component, first
maximum -- all on the GPU (on a host without a visible HIP device, on the CPU: islpose.cpu).  ``estimate_batch(crops)`` takes equal-size crops.
``precision`` (keyword only, not in the reference): 'fp32' or 'fp16' for the GPU convolutions;
the default None is the library's own (fp32 unless ISLPOSE_PRECISION=fp16 is set); an unknown
value raises ValueError; no effect on the CPU path, which is fp32.
``act_storage`` (keyword only, not in the reference): 'fp32' or 'fp16' for the buffers between the
GPU convolutions of precision 'fp16' (the same results at half the activation memory); None keeps
the library's own; an unknown value raises ValueError.
``thre`` (keyword only, not in the reference, on the GPU and the CPU path alike): the threshold
of the blurred part map (hand.py:62, 0.05); None is the reference's constant; a value that is
not a finite number in [1e-30, 1e30] raises ValueError.
``scales`` (keyword only, not in the reference, GPU and CPU path alike): the pyramid of hand.py:25,
None for (0.5, 1.0, 1.5, 2.0); islpose.runtime.check_hand_opts states what is accepted, anything
else raises ValueError.
``__call__(oriImg, *, flip=False, return_scores=False)`` and ``estimate_batch(crops, flip=None,
return_scores=False)`` (not in the reference): ``flip`` runs the image mirrored left to right
through the net -- the network is a one-handedness model, and OpenPose mirrors a left hand's crop
-- and mirrors the detected keypoints back (x -> w - 1 - x); with ``return_scores`` the result is
``(peaks, scores)``, scores float64 [21]: the scale-averaged map at the returned pixel, and 0.0
for a part that was not found, whose peak is the reference's [0, 0].
"""
from __future__ import annotations

import numpy as np
import torch

from islpose import cpu
from islpose import runtime as rt
from islpose.hand import HandEstimator

from . import util
from .model import handpose_model


class Hand(object):
    def __init__(self, model_path, *, precision=None, act_storage=None, thre=None, scales=None):
        rt.check_precision(precision)
        rt.check_act_storage(act_storage)
        rt.check_post_opts(hand_thre=thre)
        self.scales = rt.check_hand_opts(hand_scales=scales)["hand_scales"]
        self.thre = thre
        self.model = handpose_model()
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
        self._est = None

    def estimator(self) -> HandEstimator:
        dev = torch.cuda.current_device()
        net = self.model.native(dev)
        if self._est is None or self._est.net is not net:
            self._est = HandEstimator(device=dev, net=net, thre=self.thre, scale_search=self.scales)
        return self._est

    def __call__(self, oriImg, *, flip=False, return_scores=False):
        img = oriImg.cpu().numpy() if isinstance(oriImg, torch.Tensor) else np.asarray(oriImg)
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if not torch.cuda.is_available():   # GPU-less host: the product's CPU path (hand.py:18-20)
            return cpu.hand_call(img, self._cpu_net, self.scales, thre=self.thre, flip=flip,
                                 return_scores=return_scores)
        return self.estimator().estimate(img, flip=bool(flip), return_scores=return_scores)

    def _cpu_net(self, im):
        with torch.no_grad():
            return self.model(torch.from_numpy(im)).numpy()

    def estimate_batch(self, crops, flip=None, return_scores=False):
        if not torch.cuda.is_available():
            fl = [False] * len(crops) if flip is None else list(flip)
            return [self(c, flip=f, return_scores=return_scores) for c, f in zip(crops, fl)]
        return self.estimator().estimate(crops, flip=flip, return_scores=return_scores)
