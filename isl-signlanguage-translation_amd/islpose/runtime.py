"""ctypes binding of libislpose.so (include/islpose.h).

The HIP library is the only compute path: if it is missing or a call fails,
this module raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

ISL_OK, ISL_E_ARG, ISL_E_PARAM, ISL_E_HIP, ISL_E_CAPACITY, ISL_E_STATE, ISL_E_INDEX = 0, -1, -2, -3, -4, -5, -6
ISL_E_RANGE = -7
ISL_BODY25, ISL_COCO, ISL_HAND = 0, 1, 2
# conv arithmetic (isl_algo): split-fp16 x3 (default), Winograd fp32, direct fp32
ISL_ALGO_X3, ISL_ALGO_WINO, ISL_ALGO_DIRECT = 0, 1, 2
ALGOS = {"x3": ISL_ALGO_X3, "wino": ISL_ALGO_WINO, "direct": ISL_ALGO_DIRECT}
# precision of the x3 convs (isl_precision): fp32-accurate three-term products (default), or one
# fp16 product per multiply-add (opt-in; ~2e-3 of the maps' maximum in error)
ISL_PREC_FP32, ISL_PREC_FP16 = 0, 1
PRECISIONS = {"fp32": ISL_PREC_FP32, "fp16": ISL_PREC_FP16}
# storage of the activations between the fp16-precision convs (isl_act_storage): fp32 (default) or
# fp16 (opt-in; the same bits as fp32 storage, half the activation bytes)
ISL_ACT_FP32, ISL_ACT_FP16 = 0, 1
ACT_STORAGES = {"fp32": ISL_ACT_FP32, "fp16": ISL_ACT_FP16}


def check_precision(name):
    """`name` if it is a key of PRECISIONS (or None: keep the net's own), else ValueError."""
    if name is not None and name not in PRECISIONS:
        raise ValueError("unknown precision %r (expected one of %s)" % (name, ", ".join(PRECISIONS)))
    return name


def check_act_storage(name):
    """`name` if it is a key of ACT_STORAGES (or None: keep the net's own), else ValueError."""
    if name is not None and name not in ACT_STORAGES:
        raise ValueError("unknown activation storage %r (expected one of %s)" % (name, ", ".join(ACT_STORAGES)))
    return name


# post-processing options (isl_post_opts): the reference's constants and "no cap"
POST_DEFAULTS = {"thre1": 0.1, "thre2": 0.05, "hand_thre": 0.05, "max_people": 0}
MAP_THRE_RANGE = (1e-30, 1e30)   # accepted thre1 / hand_thre (include/islpose.h)


def check_post_opts(thre1=None, thre2=None, hand_thre=None, max_people=None):
    """The four post-processing options as a dict of POST_DEFAULTS' keys, a None replaced by the
    reference's constant (max_people: 0, no cap).  ValueError for thre1 or hand_thre that is
    not a finite number in MAP_THRE_RANGE (so not for 0, a negative or nan), thre2 not finite,
    max_people negative or not an integer -- the checks of isl_body_post_opts."""
    out = dict(POST_DEFAULTS)
    for name, v in (("thre1", thre1), ("hand_thre", hand_thre)):
        if v is None:
            continue
        v = float(v)
        if not (np.isfinite(v) and MAP_THRE_RANGE[0] <= v <= MAP_THRE_RANGE[1]):
            raise ValueError("%s must be a finite number in [%g, %g], got %r" % ((name,) + MAP_THRE_RANGE + (v,)))
        out[name] = v
    if thre2 is not None:
        thre2 = float(thre2)
        if not np.isfinite(thre2):
            raise ValueError("thre2 must be finite, got %r" % thre2)
        out["thre2"] = thre2
    if max_people is not None:
        if isinstance(max_people, bool) or int(max_people) != max_people or max_people < 0 or max_people >= 2 ** 31:
            raise ValueError("max_people must be an integer >= 0 (0 or None: no cap), got %r" % (max_people,))
        out["max_people"] = int(max_people)
    return out


HAND_SCALES = (0.5, 1.0, 1.5, 2.0)   # Hand.__call__'s pyramid (hand.py:25)
MAX_HAND_SCALES = 8                  # MAX_SCALES of the post kernels
HAND_BOXSIZE = 368                   # hand.py:26
MIN_HAND_SCALE_PX = 8                # one stride-8 cell of the hand net


def check_hand_opts(hand_scales=None, flip_left=False):
    """The hand-path options as a dict(hand_scales=tuple of floats, flip_left=bool).
    hand_scales: the pyramid of Hand.__call__ (hand.py:25), None for the reference's
    (0.5, 1.0, 1.5, 2.0); 1 to MAX_HAND_SCALES entries, each a finite number > 0 whose
    round(s * 368) is at least 8 px.  flip_left: mirror left-hand crops before the net and the
    keypoints back after it (OpenPose's own hand extractor; not in the reference).  ValueError
    for anything else, with or without a GPU."""
    if hand_scales is None:
        scales = HAND_SCALES
    else:
        try:
            scales = tuple(float(s) for s in hand_scales)
        except TypeError:
            raise ValueError("hand_scales must be a sequence of numbers, got %r" % (hand_scales,))
        if not 1 <= len(scales) <= MAX_HAND_SCALES:
            raise ValueError("hand_scales needs 1 to %d entries, got %d" % (MAX_HAND_SCALES, len(scales)))
        for s in scales:
            if not (np.isfinite(s) and s > 0 and int(np.rint(s * HAND_BOXSIZE)) >= MIN_HAND_SCALE_PX):
                raise ValueError("hand scale %r: expected a finite number > 0 with round(s * %d) >= %d"
                                 % (s, HAND_BOXSIZE, MIN_HAND_SCALE_PX))
    if not isinstance(flip_left, (bool, np.bool_)):
        raise ValueError("flip_left must be a bool, got %r" % (flip_left,))
    return {"hand_scales": scales, "flip_left": bool(flip_left)}


def flip_array(flip, n):
    """A per-crop mirror flag sequence as the uint8 host array the *_flip / *_ex entry points
    take, or None (NULL) when no crop is mirrored.  ValueError if its length is not n."""
    if flip is None:
        return None
    f = [bool(v) for v in flip]
    if len(f) != n:
        raise ValueError("flip needs one flag per crop: %d flags for %d crops" % (len(f), n))
    return (ctypes.c_uint8 * n)(*[int(v) for v in f]) if any(f) else None


LIB_PATH = os.environ.get("ISLPOSE_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "libislpose.so"))

# every symbol include/islpose.h declares
EXPORTS = ["isl_abi_version", "isl_last_error", "isl_net_create", "isl_net_destroy", "isl_net_param_count",
           "isl_net_param_info", "isl_net_set_param", "isl_net_forward", "isl_net_preprocess", "isl_net_run", "isl_net_debug_input",
           "isl_net_set_timing", "isl_net_timing", "isl_body_layout", "isl_body_post", "isl_hand_post",
           "isl_net_set_algo", "isl_net_get_algo", "isl_net_check", "isl_net_preprocess_crops",
           "isl_sign_param_count", "isl_sign_classify", "isl_net_set_split_k", "isl_net_arena_info",
           "isl_debug_np_sum", "isl_hand_post_crops", "isl_net_check_async", "isl_net_range_info",
           "isl_net_op_info", "isl_net_set_graph", "isl_lane_stream_create", "isl_lane_stream_destroy",
           "isl_net_set_precision", "isl_net_get_precision", "isl_net_set_act_storage",
           "isl_net_get_act_storage", "isl_net_act_storage_active", "isl_post_opts_default",
           "isl_body_post_opts", "isl_hand_post_opts", "isl_hand_post_crops_opts",
           "isl_net_preprocess_crops_flip", "isl_hand_post_ex", "isl_hand_post_crops_ex", "isl_augment",
           "isl_draw", "isl_sign_train_opts_default", "isl_sign_grad_workspace", "isl_sign_grad",
           "isl_sign_aug_opts_default", "isl_sign_augment",
           "isl_debug_conv3x3", "isl_debug_conv", "isl_debug_body_post_plan", "isl_debug_hand_post_plan"]


class IslCaps(ctypes.Structure):
    _fields_ = [("max_peaks", ctypes.c_int32), ("max_pairs", ctypes.c_int32),
                ("max_conns", ctypes.c_int32), ("max_rows", ctypes.c_int32)]


class IslLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in
                ("status", "n_peaks", "n_conns", "n_rows", "peaks", "conns", "subset", "record_bytes")]


class IslScaleGeom(ctypes.Structure):
    _fields_ = [("net_h", ctypes.c_int32), ("net_w", ctypes.c_int32),
                ("valid_h", ctypes.c_int32), ("valid_w", ctypes.c_int32)]


class IslCrop(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("frame", "x", "y", "w", "h")]


class IslPostOpts(ctypes.Structure):
    _fields_ = [("thre1", ctypes.c_double), ("thre2", ctypes.c_double), ("hand_thre", ctypes.c_double),
                ("max_people", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class IslAugItem(ctypes.Structure):
    """isl_aug_item: c, s = cos / sin of radians(-angle); src frame index; rotate 0 / 1; solarize
    threshold in [0, 256] (256: off); swap_rb 0 / 1; reserved zero."""
    _fields_ = [("c", ctypes.c_double), ("s", ctypes.c_double), ("src", ctypes.c_int32),
                ("rotate", ctypes.c_int32), ("threshold", ctypes.c_int32), ("swap_rb", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 2)]


class IslDrawPrim(ctypes.Structure):
    """isl_draw_prim: kind 0 stick (p = cx, cy, a, b; c, s), 1 disc (p = cx, cy; r2), 2 segment
    (p = x0, y0, x1, y1; r2); color for channels 0, 1, 2; blend 0 / 1; reserved zero."""
    _fields_ = [("kind", ctypes.c_int32), ("p", ctypes.c_int32 * 4), ("c", ctypes.c_int32), ("s", ctypes.c_int32),
                ("r2", ctypes.c_int32), ("color", ctypes.c_uint8 * 3), ("blend", ctypes.c_uint8),
                ("reserved", ctypes.c_int32)]


class IslSignTrainOpts(ctypes.Structure):
    """isl_sign_train_opts: the rates of the three Dropout layers and of the recurrent dropout, each
    in [0, 0.9] (0: off); seed and step of the counter-based draws; reserved zero."""
    _fields_ = [("p_drop", ctypes.c_float), ("p_rec", ctypes.c_float), ("seed", ctypes.c_uint64),
                ("step", ctypes.c_uint64), ("reserved", ctypes.c_int32 * 4)]


class IslSignAugItem(ctypes.Structure):
    """isl_sign_aug_item (80 bytes): the source rows [row0, row0 + nrows) of the store, the source
    row `start` of output frame 0, the speed q in 1/16, the sample id of the kernel's draws, and the
    affine map m of every present pair."""
    _fields_ = [("row0", ctypes.c_int64), ("nrows", ctypes.c_int32), ("start", ctypes.c_int32),
                ("q", ctypes.c_int32), ("reserved", ctypes.c_int32), ("id", ctypes.c_uint64),
                ("m", ctypes.c_double * 6)]


class IslSignAugLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_body", "n_slots", "n_hand", "reserved")]


class IslSignAugOpts(ctypes.Structure):
    """isl_sign_aug_opts: frame-drop rate in [0, 0.9], jitter amplitude >= 0 (both 0: off); seed and
    step of the counter-based draws; reserved zero."""
    _fields_ = [("drop", ctypes.c_float), ("jitter", ctypes.c_float), ("seed", ctypes.c_uint64),
                ("step", ctypes.c_uint64), ("reserved", ctypes.c_int32 * 4)]


class IslDebugSeg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("phys", "logical", "len")]


class IslDebugConvDesc(ctypes.Structure):
    """isl_debug_conv_desc (include/islpose.h)."""
    _fields_ = ([(n, ctypes.c_int32) for n in
                 ("n", "h", "w", "cin", "cout", "ks", "act", "kernel", "f16", "act16", "allow_split",
                  "in_pad", "out_pad", "in_cs", "in_coff", "out_cs", "out_coff", "nseg")] +
                [("seg", IslDebugSeg * 4), ("hpool", ctypes.c_int32), ("vin", ctypes.c_int32),
                 ("range_error", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7)])


class IslDebugConvResult(ctypes.Structure):
    """isl_debug_conv_result (include/islpose.h)."""
    _fields_ = [("variant", ctypes.c_int32), ("range_flag", ctypes.c_int32),
                ("stray_writes", ctypes.c_int64), ("unwritten", ctypes.c_int64),
                ("stray_stage", ctypes.c_int32), ("stray_frame", ctypes.c_int32),
                ("stray_chunk", ctypes.c_int32), ("stray_y", ctypes.c_int32), ("stray_x", ctypes.c_int32),
                ("stray_lane", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


DEBUG_KERNELS = {"x3": 0, "wino2": 1, "direct": 2, "wino": 3, "rgb": 4}
DEBUG_ACTS = {"none": 0, "relu": 1, "prelu": 2}


class DebugConvResult:
    """What isl_debug_conv returns: y (numpy fp32 [n, cout, h, w]; with hpool the pair-max map
    [n, cout, h, w // 2]), pooled (with hpool: [n, cout, h // 2, w // 2], else None), variant (the
    x3 variant code; decode_variant reads it), range_flag, stray_writes and unwritten (element
    counts), stray (the first stray write as a dict, or None)."""

    def __init__(self, y, pooled, r):
        self.y, self.pooled = y, pooled
        self.variant, self.range_flag = int(r.variant), int(r.range_flag)
        self.stray_writes, self.unwritten = int(r.stray_writes), int(r.unwritten)
        self.stray = None if not self.stray_writes else dict(
            stage="pool" if r.stray_stage else "conv", frame=int(r.stray_frame), chunk=int(r.stray_chunk),
            y=int(r.stray_y), x=int(r.stray_x), lane=int(r.stray_lane))


def debug_conv(x, weight, bias, slope=None, *, act="none", kernel="x3", f16=False, act16=False,
               allow_split=False, in_pad=None, out_pad=1, in_cs=None, in_coff=0, out_cs=None, out_coff=0,
               segs=None, hpool=False, vin=False, range_error=False):
    """One convolution layer on one of the conv kernels, on host arrays (isl_debug_conv; the
    header describes the buffers, the canary and the poison).  x [n, cin, h, w] (with vin the
    pre-pool map [n, cin, 2h, 2w]), weight [cout, cin, ks, ks], bias [cout], slope [cout] for
    act "prelu".  segs: up to four (phys, logical, len) triples, default one segment of all
    channels; in_cs / out_cs default to the smallest buffers that hold the slices; in_pad
    defaults to max(1, ks // 2).  Returns a DebugConvResult."""
    import numpy as np
    x, weight, bias = (np.ascontiguousarray(a, np.float32) for a in (x, weight, bias))
    if x.ndim != 4 or weight.ndim != 4 or weight.shape[2] != weight.shape[3] or weight.shape[1] != x.shape[1]:
        raise ValueError("debug_conv: x [n, cin, h, w] and weight [cout, cin, ks, ks] expected")
    n, cin, h, w = x.shape
    cout, ks = weight.shape[0], weight.shape[2]
    if vin:
        if h % 2 or w % 2:
            raise ValueError("debug_conv: vin takes an even pre-pool map")
        h, w = h // 2, w // 2
    if bias.shape != (cout,):
        raise ValueError("debug_conv: bias [cout] expected")
    if kernel not in DEBUG_KERNELS or act not in DEBUG_ACTS:
        raise ValueError("debug_conv: kernel is one of %s, act one of %s" % (sorted(DEBUG_KERNELS), sorted(DEBUG_ACTS)))
    if act == "prelu":
        if slope is None:
            raise ValueError("debug_conv: act 'prelu' needs slopes")
        slope = np.ascontiguousarray(slope, np.float32)
        if slope.shape != (cout,):
            raise ValueError("debug_conv: slope [cout] expected")
    else:
        slope = None
    segs = [(0, 0, cin)] if segs is None else [tuple(int(v) for v in s) for s in segs]
    if not 1 <= len(segs) <= 4:
        raise ValueError("debug_conv: 1 to 4 segments")
    phys = (max(p + l for p, _, l in segs) + 7) // 8 * 8
    d = IslDebugConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ks = n, h, w, cin, cout, ks
    d.act, d.kernel = DEBUG_ACTS[act], DEBUG_KERNELS[kernel]
    d.f16, d.act16, d.allow_split = int(bool(f16)), int(bool(act16)), int(bool(allow_split))
    d.in_pad = max(1, ks // 2) if in_pad is None else int(in_pad)
    d.out_pad = int(out_pad)
    d.in_coff, d.out_coff = int(in_coff), int(out_coff)
    d.in_cs = d.in_coff + phys if in_cs is None else int(in_cs)
    d.out_cs = d.out_coff + (cout + 7) // 8 * 8 if out_cs is None else int(out_cs)
    d.nseg = len(segs)
    for i, (p, lg, ln) in enumerate(segs):
        d.seg[i] = IslDebugSeg(p, lg, ln)
    d.hpool, d.vin, d.range_error = int(bool(hpool)), int(bool(vin)), int(bool(range_error))
    y = np.empty((n, cout, h, w // 2 if hpool else w), np.float32)
    pooled = np.empty((n, cout, h // 2, w // 2), np.float32) if hpool else None
    r = IslDebugConvResult()
    check(lib().isl_debug_conv(ctypes.byref(d), x.ctypes.data, weight.ctypes.data, bias.ctypes.data,
                               None if slope is None else slope.ctypes.data, y.ctypes.data,
                               None if pooled is None else pooled.ctypes.data, ctypes.byref(r)),
          "isl_debug_conv")
    return DebugConvResult(y, pooled, r)


PLAN_SCALES = 8
BLUR_BRANCHES = ("MULTI_F64", "FUSED_LIVE", "BAND_LIVE", "DENSE")      # enum isl_blur_branch


class IslResizePlan(ctypes.Structure):
    """isl_resize_plan (include/islpose.h): one launch of the separable resize."""
    _fields_ = [(n, ctypes.c_int32) for n in ("launched", "ty", "cols", "v4", "bm", "identity")]


class IslBodyPostPlan(ctypes.Structure):
    """isl_body_post_plan (include/islpose.h)."""
    _fields_ = ([(n, ctypes.c_int32) for n in
                 ("multi", "two_stage", "fused", "fuse2", "wide", "skip2", "blur", "blur_bandmax", "acc_ty",
                  "stage2_ty", "limb_z", "env_fused_blur", "env_fused_wide", "env_blur_list", "env_blur_bands",
                  "env_resize_skip", "env_resize_v4", "env_blur_exact")] +
                [("scale_two_stage", ctypes.c_int32 * PLAN_SCALES), ("stage1", IslResizePlan * PLAN_SCALES),
                 ("final_rs", IslResizePlan * PLAN_SCALES), ("env_limb_lds", ctypes.c_int32),
                 ("env_asm_reg", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)])


class IslHandPostPlan(ctypes.Structure):
    """isl_hand_post_plan (include/islpose.h)."""
    _fields_ = [("two_stage", ctypes.c_int32 * PLAN_SCALES), ("identity", ctypes.c_int32 * PLAN_SCALES),
                ("stage1", IslResizePlan * PLAN_SCALES), ("acc_ty", ctypes.c_int32), ("cc_lds", ctypes.c_int32),
                ("cc_rows", ctypes.c_int32), ("cc_chunks", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


def _resize_dict(r):
    return {n: int(getattr(r, n)) for n, _ in IslResizePlan._fields_}


def _geom_array(geoms):
    return (IslScaleGeom * max(len(geoms), 1))(*[IslScaleGeom(*[int(v) for v in g]) for g in geoms])


def body_post_plan(kind, n, H, W, geoms):
    """isl_debug_body_post_plan as a dict: the host-side choices isl_body_post_opts makes for n
    frames of H x W with the scale geometries `geoms` [(net_h, net_w, valid_h, valid_w)] and the
    environment switches as they stand now.  `blur` is one of BLUR_BRANCHES; stage1 / final are
    per-scale lists of resize dicts (launched, ty, cols, v4, bm, identity).  No device work."""
    p = IslBodyPostPlan()
    check(lib().isl_debug_body_post_plan(int(kind), int(n), int(H), int(W), len(geoms), _geom_array(geoms),
                                         ctypes.byref(p)), "isl_debug_body_post_plan")
    out = {name: int(getattr(p, name)) for name, t in IslBodyPostPlan._fields_ if t is ctypes.c_int32}
    out["blur"] = BLUR_BRANCHES[p.blur]
    out["scale_two_stage"] = [int(p.scale_two_stage[i]) for i in range(len(geoms))]
    out["stage1"] = [_resize_dict(p.stage1[i]) for i in range(len(geoms))]
    out["final"] = [_resize_dict(p.final_rs[i]) for i in range(len(geoms))]
    return out


def hand_post_plan(h, w, geoms):
    """isl_debug_hand_post_plan as a dict: per scale two_stage, identity and the stage-1 resize
    dict; acc_ty (resize_acc_kernel's rows per tile); cc_lds (1: the single-workgroup component
    path, 0: the large-plane chain) with cc_rows / cc_chunks.  No device work."""
    p = IslHandPostPlan()
    check(lib().isl_debug_hand_post_plan(int(h), int(w), len(geoms), _geom_array(geoms), ctypes.byref(p)),
          "isl_debug_hand_post_plan")
    k = len(geoms)
    return {"two_stage": [int(p.two_stage[i]) for i in range(k)], "identity": [int(p.identity[i]) for i in range(k)],
            "stage1": [_resize_dict(p.stage1[i]) for i in range(k)], "acc_ty": int(p.acc_ty),
            "cc_lds": int(p.cc_lds), "cc_rows": int(p.cc_rows), "cc_chunks": int(p.cc_chunks)}


def post_opts_struct(opts: dict) -> IslPostOpts:
    """check_post_opts' dict -> the isl_post_opts the *_opts entry points take."""
    return IslPostOpts(opts["thre1"], opts["thre2"], opts["hand_thre"], opts["max_people"])


class IslError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libislpose.so once; raise loudly if it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libislpose.so not found at %s -- build it with `make` (or __graft_entry__.build())"
                          % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    L.isl_abi_version.restype = i32
    L.isl_last_error.restype = ctypes.c_char_p
    L.isl_net_create.argtypes = [i32, i32, ctypes.POINTER(vp)]
    L.isl_net_destroy.argtypes = [vp]
    L.isl_net_param_count.argtypes = [vp]
    L.isl_net_param_info.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i64)]
    L.isl_net_set_param.argtypes = [vp, ctypes.c_char_p, vp, i64]
    L.isl_net_forward.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.isl_net_preprocess.argtypes = [vp, vp, i32, i32, i32, dbl, ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    L.isl_net_run.argtypes = [vp, vp, vp, vp]
    L.isl_net_debug_input.argtypes = [vp, vp, vp]
    L.isl_net_set_timing.argtypes = [vp, i32]
    L.isl_net_preprocess_crops.argtypes = [vp, vp, i32, i32, i32, ctypes.POINTER(IslCrop), i32, dbl,
                                           ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    L.isl_net_set_algo.argtypes = [vp, i32]
    L.isl_net_get_algo.argtypes = [vp]
    L.isl_net_set_precision.argtypes = [vp, i32]
    L.isl_net_get_precision.argtypes = [vp]
    L.isl_net_set_act_storage.argtypes = [vp, i32]
    L.isl_net_get_act_storage.argtypes = [vp]
    L.isl_net_act_storage_active.argtypes = [vp]
    L.isl_net_check.argtypes = [vp, i32]
    L.isl_net_check_async.argtypes = [vp, vp, vp]
    L.isl_net_range_info.argtypes = [vp, ctypes.POINTER(i64)]
    L.isl_net_op_info.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i32)]
    pi, pd = ctypes.POINTER(i32), ctypes.POINTER(dbl)
    L.isl_net_timing.argtypes = [vp, i32, pi, pi, pd, pi, pd, pd]
    L.isl_body_layout.argtypes = [i32, ctypes.POINTER(IslCaps), ctypes.POINTER(IslLayout)]
    L.isl_body_post.argtypes = [vp, i32, i32, i32, i32, ctypes.POINTER(IslScaleGeom), ctypes.POINTER(vp),
                                ctypes.POINTER(vp), ctypes.POINTER(IslCaps), vp, vp]
    L.isl_hand_post.argtypes = [vp, i32, i32, i32, i32, ctypes.POINTER(IslScaleGeom), ctypes.POINTER(vp), vp, vp]
    L.isl_sign_param_count.argtypes = [i32, i32, ctypes.POINTER(i64)]
    L.isl_net_set_split_k.argtypes = [vp, i32]
    L.isl_net_set_graph.argtypes = [vp, i32]
    L.isl_lane_stream_create.argtypes = [i32, i32, ctypes.POINTER(vp)]
    L.isl_lane_stream_destroy.argtypes = [vp]
    L.isl_net_arena_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.isl_sign_classify.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp]
    L.isl_debug_np_sum.argtypes = [vp, i64, vp, vp]
    L.isl_hand_post_crops.argtypes = [vp, i32, ctypes.POINTER(i32), i32, ctypes.POINTER(IslScaleGeom),
                                      ctypes.POINTER(vp), vp, vp]
    po = ctypes.POINTER(IslPostOpts)
    L.isl_post_opts_default.argtypes = [po]
    L.isl_body_post_opts.argtypes = L.isl_body_post.argtypes + [po]
    L.isl_hand_post_opts.argtypes = L.isl_hand_post.argtypes + [po]
    L.isl_hand_post_crops_opts.argtypes = L.isl_hand_post_crops.argtypes + [po]
    pu8 = ctypes.POINTER(ctypes.c_uint8)
    L.isl_net_preprocess_crops_flip.argtypes = [vp, vp, i32, i32, i32, ctypes.POINTER(IslCrop), pu8, i32, dbl,
                                                ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    L.isl_hand_post_ex.argtypes = L.isl_hand_post_opts.argtypes + [pu8, vp]
    L.isl_hand_post_crops_ex.argtypes = L.isl_hand_post_crops_opts.argtypes + [pu8, vp]
    L.isl_augment.argtypes = [vp, i32, i32, i32, vp, ctypes.POINTER(IslAugItem), i32, vp]
    L.isl_draw.argtypes = [vp, vp, i32, i32, i32, ctypes.POINTER(IslDrawPrim), ctypes.POINTER(i32), vp]
    L.isl_sign_train_opts_default.argtypes = [ctypes.POINTER(IslSignTrainOpts)]
    L.isl_sign_grad_workspace.argtypes = [i32, i32, i32, ctypes.POINTER(i64)]
    L.isl_sign_grad.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, ctypes.POINTER(IslSignTrainOpts), vp, vp,
                                vp, vp]
    L.isl_sign_aug_opts_default.argtypes = [ctypes.POINTER(IslSignAugOpts)]
    L.isl_sign_augment.argtypes = [vp, i64, i32, ctypes.POINTER(IslSignAugLayout), vp, i32, i32,
                                   ctypes.POINTER(IslSignAugOpts), vp, vp]
    L.isl_debug_conv3x3.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp]
    L.isl_debug_conv.argtypes = [ctypes.POINTER(IslDebugConvDesc), vp, vp, vp, vp, vp, vp,
                                 ctypes.POINTER(IslDebugConvResult)]
    L.isl_debug_body_post_plan.argtypes = [i32, i32, i32, i32, i32, ctypes.POINTER(IslScaleGeom),
                                           ctypes.POINTER(IslBodyPostPlan)]
    L.isl_debug_hand_post_plan.argtypes = [i32, i32, i32, ctypes.POINTER(IslScaleGeom),
                                           ctypes.POINTER(IslHandPostPlan)]
    for name in EXPORTS[2:]:
        getattr(L, name).restype = i32
    if L.isl_abi_version() != 1:
        raise ImportError("libislpose ABI mismatch")
    _lib = L
    return L


def debug_conv3x3(x, weight, bias, slope, kernel: str):
    """One 3x3 layer (pad 1, bias, PReLU) of the split-fp16 path on host arrays (isl_debug_conv3x3):
    x [n, cin, h, w], weight [cout, cin, 3, 3], bias and slope [cout]; kernel "x3" (conv_x3) or
    "wino2" (wino_f16).  Returns y [n, cout, h, w] (numpy fp32)."""
    import numpy as np
    x, weight, bias, slope = (np.ascontiguousarray(a, np.float32) for a in (x, weight, bias, slope))
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    if weight.shape != (cout, cin, 3, 3) or bias.shape != (cout,) or slope.shape != (cout,):
        raise ValueError("debug_conv3x3: weight [cout, cin, 3, 3], bias [cout], slope [cout] expected")
    if kernel not in ("x3", "wino2"):
        raise ValueError("debug_conv3x3: kernel is 'x3' or 'wino2'")
    y = np.empty((n, cout, h, w), np.float32)
    check(lib().isl_debug_conv3x3(x.ctypes.data, n, cin, h, w, weight.ctypes.data, bias.ctypes.data,
                                  slope.ctypes.data, cout, 1 if kernel == "wino2" else 0, y.ctypes.data),
          "isl_debug_conv3x3")
    return y


def check(rc: int, what: str = ""):
    if rc == ISL_OK:
        return
    msg = lib().isl_last_error().decode(errors="replace")
    if rc == ISL_E_PARAM:
        raise KeyError(msg)
    if rc == ISL_E_INDEX:
        raise IndexError("list assignment index out of range")
    raise IslError("%s failed (%d): %s" % (what or "libislpose", rc, msg))


def augment(src_u8, items, out=None, stream=None):
    """isl_augment: src_u8 cuda uint8 [n_src, H, W, 3] (contiguous), items a sequence of
    IslAugItem -> cuda uint8 [len(items), H, W, 3], item k's variant of frame items[k].src, in
    one launch on `stream` (None: the current stream of the frames' device).  `out`: the
    destination, which must not overlap the source."""
    import torch
    n, H, W, _ = src_u8.shape
    m = len(items)
    if out is None:
        out = torch.empty((m, H, W, 3), dtype=torch.uint8, device=src_u8.device)
    arr = (IslAugItem * max(m, 1))(*items)
    with torch.cuda.device(src_u8.device):
        s = stream if stream is not None else torch.cuda.current_stream(src_u8.device)
        check(lib().isl_augment(ptr(src_u8), n, H, W, ptr(out), arr, m, ctypes.c_void_p(s.cuda_stream)), "isl_augment")
    return out


def sign_augment(rows_t, layout, items_t, n_items, window, opts, out, stream=None):
    """isl_sign_augment as it is: rows_t cuda fp32 [n_rows, F] (contiguous), layout (n_body, n_slots,
    n_hand), items_t a cuda uint8 tensor holding n_items isl_sign_aug_item records (not validated
    here: islpose.sign_augment.WindowAugment.apply does that), opts an IslSignAugOpts, out cuda fp32
    with n_items * window * F elements; one launch on `stream` (None: the current stream of the
    rows' device).  Returns out."""
    import torch
    lay = IslSignAugLayout(int(layout[0]), int(layout[1]), int(layout[2]), 0)
    with torch.cuda.device(rows_t.device):
        s = stream if stream is not None else torch.cuda.current_stream(rows_t.device)
        check(lib().isl_sign_augment(ptr(rows_t), rows_t.shape[0], rows_t.shape[1], ctypes.byref(lay), ptr(items_t),
                                     n_items, window, ctypes.byref(opts), ptr(out), ctypes.c_void_p(s.cuda_stream)),
              "isl_sign_augment")
    return out


def draw(src_u8, dst_u8, prims, first, stream=None):
    """isl_draw: dst_u8 cuda uint8 [n, H, W, 3] (contiguous) receives src_u8 (the same tensor: in
    place; another of the same shape: a copy; None: an all-zero canvas) with frame f's primitives
    prims[first[f]:first[f + 1]] drawn in list order, in one launch on `stream` (None: the
    current stream of the destination's device).  prims: a ctypes array of IslDrawPrim (or None
    when first[n] == 0); first: n + 1 ints."""
    import torch
    n, H, W, _ = dst_u8.shape
    arr = (ctypes.c_int32 * (n + 1))(*first)
    with torch.cuda.device(dst_u8.device):
        s = stream if stream is not None else torch.cuda.current_stream(dst_u8.device)
        check(lib().isl_draw(None if src_u8 is None else ptr(src_u8), ptr(dst_u8), n, H, W, prims, arr,
                             ctypes.c_void_p(s.cuda_stream)), "isl_draw")
    return dst_u8


def body_layout(kind: int, caps: IslCaps) -> IslLayout:
    lay = IslLayout()
    check(lib().isl_body_layout(kind, ctypes.byref(caps), ctypes.byref(lay)), "isl_body_layout")
    return lay


def stream_handle(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def flag_slot(owner, ring: int = 4):
    """A pinned int32 slot for Net.check_async, from a ring kept on `owner` for its life
    (the copy into it is issued outside torch, so the buffer must never go back to torch's
    pinned cache while a copy may be in flight); at most `ring` launches in flight."""
    import torch
    slots = getattr(owner, "_flag_slots", None)
    if slots is None:
        slots = owner._flag_slots = [torch.zeros(1, dtype=torch.int32, pin_memory=True) for _ in range(ring)]
        owner._flag_next = 0
    f = slots[owner._flag_next % len(slots)]
    owner._flag_next += 1
    f.zero_()
    return f


_LANES = {}   # device index -> [torch.cuda.ExternalStream], lane k of every estimator


def lane_priorities(k):
    """Priority class of each of k lanes (isl_lane_stream_create): lane 0 (the largest scale,
    the critical path) high, lane 1 low, the rest normal -- three classes, three queue pools.
    ISLPOSE_LANE_PRIO=0: every lane normal (A/B)."""
    if os.environ.get("ISLPOSE_LANE_PRIO", "1") == "0":
        return [0] * k
    return [(-1, 1)[j] if j < 2 else 0 for j in range(k)]


def scale_streams(owner, device, k):
    """k non-blocking streams for a pyramid's scales (isl_lane_stream_create with the classes
    of lane_priorities).  One pool per device, shared by every estimator (work on one stream
    stays in order) and never destroyed: torch's allocator may still hold events on a stream
    that a tensor was recorded on.  `owner` is unused (kept for the callers' signature)."""
    import torch
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    prios = lane_priorities(k)
    key = (idx, tuple(prios[:3]))
    pool = _LANES.setdefault(key, [])
    while len(pool) < k:
        h = ctypes.c_void_p()
        check(lib().isl_lane_stream_create(idx, prios[len(pool)], ctypes.byref(h)), "isl_lane_stream_create")
        pool.append(torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx)))
    return pool[:k]


SCALE_LANES = 4   # streams a pyramid's scales share (lane_plan)


def lane_plan(owner, device, keys, lanes=None):
    """Streams for a pyramid's scales (keys: their net sizes) and the order to enqueue them:
    the distinct sizes go largest first onto the least loaded of SCALE_LANES streams (load =
    net area), and the scales are enqueued largest first.  One stream per scale ran the two
    largest hand scales one after the other (a process has 4 hardware queues, the current
    stream holds one, so the fourth scale stream shared one with the third): 6.70 ms for one
    crop's four scales; [736] [552] [368 -> 184] on three lanes: 5.48 ms
    (tools/hand_conc_events.py, profiles/r06/fr6/lanes.txt).  Scales of one size share a
    lane, in their order (they share that size's arena)."""
    lane, order, n = lane_assign(keys, SCALE_LANES if lanes is None else lanes)
    ss = scale_streams(owner, device, n)
    return [ss[j] for j in lane], order


def lane_assign(keys, lanes):
    """lane_plan without the streams: (lane index per key, enqueue order, lanes used)."""
    distinct = list(dict.fromkeys(keys))
    area = {k: k[0] * k[1] for k in distinct}
    n = max(1, min(lanes, len(distinct)))
    load, lane = [0] * n, {}
    for k in sorted(distinct, key=lambda k: -area[k]):
        j = min(range(n), key=lambda i: load[i])
        lane[k] = j
        load[j] += area[k]
    order = sorted(range(len(keys)), key=lambda i: (-area[keys[i]], i))
    return [lane[k] for k in keys], order, n


def fork_streams(cur, streams):
    """Every distinct stream of `streams` waits for the work queued so far on `cur`.  All
    forks come before any join: a stream forked after `cur` joined an earlier one would wait
    for that one's whole chain, and the scales would run one after another."""
    for st in dict.fromkeys(streams):
        st.wait_stream(cur)


def join_streams(cur, streams):
    """`cur` waits for everything queued on `streams` (after fork_streams and the launches)."""
    for st in dict.fromkeys(streams):
        cur.wait_stream(st)


def crop_net_size(crop_h: int, crop_w: int, scale_times_box: float):
    """Padded net size isl_net_preprocess_crops gives a crop (runtime.cpp: fx = fy =
    scale_times_box / h, cvRound, then padRightDownCorner to a multiple of 8)."""
    m = scale_times_box / crop_h
    rh, rw = int(np.rint(crop_h * m)), int(np.rint(crop_w * m))
    return (rh + 7) // 8 * 8, (rw + 7) // 8 * 8


def ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def decode_variant(code: int) -> dict:
    """isl_net_op_info's variant code -> dict(var=VAR bits, bpx, bco, ks, rgb, pool_fused, ...):
    wave_ranges (conv_x3_wr, VAR 8), c12 (conv1_1 -> conv1_2 in one launch, 4), wino2 (the
    split-fp16 Winograd kernel wino_f16, 64), f16 (one-term fp16 products, precision 'fp16', 2),
    act16 (the launch reads or writes fp16 activations, act_storage 'fp16', 1).  Under precision
    'fp16' the c12 launch also carries rgb (conv1_1 runs the 3-channel kernel's one-term K packing
    inside it) and conv1_2 reports -1 (it ran fused with its pool inside conv1_1's launch)."""
    if code == -1:
        return {"pool_fused": True}
    if code == -2:
        return {"fused_into_prev": True}     # the second layer of a fused 1x1 pair (VAR 16)
    if code <= 0:
        return {}
    f67 = bool(code & 16)   # the fused pair records its all-channel tile halved (4-bit field)
    return {"var": code & 0xfffff, "bpx": ((code >> 20) & 31) * 32,
            "bco": ((code >> 25) & 15) * 32 * (2 if f67 else 1), "fused67": f67, "g2": bool(code & 32),
            "ks": 2 * ((code >> 29) & 3) + 1, "rgb": bool(code & (1 << 18)),
            "union": bool(code & 512), "ranged": bool(code & 1024), "split": bool(code & 2048),
            "pairs2": bool(code & 4096), "vin": bool(code & 32768), "sib": bool(code & 65536),
            "fold": bool(code & 8192), "m16": bool(code & 131072), "fold_out": bool(code & (1 << 19)),
            "wave_ranges": bool(code & 8), "c12": bool(code & 4), "wino2": bool(code & 64),
            "f16": bool(code & 2), "act16": bool(code & 1)}


class Net:
    """One network (body25 / coco / hand) on one device, owned by libislpose."""

    def __init__(self, kind: int, device: int = 0):
        self.kind = kind
        self.device = device
        h = ctypes.c_void_p()
        check(lib().isl_net_create(kind, device, ctypes.byref(h)), "isl_net_create")
        self.h = h
        self.loaded = False
        e = os.environ.get("ISLPOSE_X3_SPLITK", "")[:1]
        self.split_k = int(e) if e in ("0", "2") else 1      # isl_net_create's default

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and _lib is not None:
            _lib.isl_net_destroy(h)
            self.h = None

    def param_names(self):
        out = []
        n = lib().isl_net_param_count(self.h)
        for i in range(n):
            name = ctypes.c_char_p()
            numel = ctypes.c_int64()
            check(lib().isl_net_param_info(self.h, i, ctypes.byref(name), ctypes.byref(numel)))
            out.append((name.value.decode(), numel.value))
        return out

    def load_weights(self, weights: dict):
        """weights: flat {caffe_name: array/tensor} (the dict util.transfer reads).
        A missing name raises KeyError like util.transfer (src/util.py:39-43)."""
        for name, numel in self.param_names():
            v = weights[name]
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
            if a.size != numel:
                raise KeyError("%s: expected %d elements, got %d" % (name, numel, a.size))
            check(lib().isl_net_set_param(self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size),
                  "isl_net_set_param")
        self.loaded = True

    def forward(self, x, out0=None, out1=None, stream=None):
        """Module seam: x float32 NCHW cuda tensor -> (paf, heat) or heat."""
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
        x = x.contiguous()
        n, _, h, w = x.shape
        h8, w8 = h // 8, w // 8
        if self.kind == ISL_HAND:
            o0 = out0 if out0 is not None else torch.empty((n, 22, h8, w8), device=x.device)
            o1 = None
        else:
            npaf, nj = (52, 26) if self.kind == ISL_BODY25 else (38, 19)
            o0 = out0 if out0 is not None else torch.empty((n, npaf, h8, w8), device=x.device)
            o1 = out1 if out1 is not None else torch.empty((n, nj, h8, w8), device=x.device)
        check(lib().isl_net_forward(self.h, ptr(x), n, h, w, ptr(o0), ptr(o1), stream_handle(stream)),
              "isl_net_forward")
        if not self.range_ok():
            # an activation left the split-fp16 range: recompute on the fp32 kernels
            with self.algo_scope("direct"):
                check(lib().isl_net_forward(self.h, ptr(x), n, h, w, ptr(o0), ptr(o1), stream_handle(stream)),
                      "isl_net_forward")
        return o0 if o1 is None else (o0, o1)

    # -- conv arithmetic -----------------------------------------------------------
    @property
    def algo(self) -> str:
        a = lib().isl_net_get_algo(self.h)
        return {v: k for k, v in ALGOS.items()}[a]

    def set_algo(self, algo: str):
        """'x3' (split-fp16 on the FP16 matrix cores, fp32-accurate; default), 'wino'
        (Winograd F(2x2,3x3), FP32 MFMA) or 'direct' (implicit GEMM, FP32 MFMA)."""
        check(lib().isl_net_set_algo(self.h, ALGOS[algo]), "isl_net_set_algo")

    # -- precision of the x3 convs ---------------------------------------------------
    @property
    def precision(self) -> str:
        p = lib().isl_net_get_precision(self.h)
        return {v: k for k, v in PRECISIONS.items()}[p]

    def set_precision(self, name: str):
        """'fp32' (three fp16 products per multiply-add, fp32-accurate; default, or the env
        ISLPOSE_PRECISION at creation) or 'fp16' (one product: a third of the matrix work, half
        the operand bytes, ~2e-3 of the maps' maximum in error).  It changes the 'x3' algorithm
        only; the range guard and its fp32 ('direct') recompute are unchanged.  Unknown names
        raise ValueError."""
        check(lib().isl_net_set_precision(self.h, PRECISIONS[check_precision(name)]), "isl_net_set_precision")

    def precision_scope(self, name: str):
        import contextlib

        @contextlib.contextmanager
        def scope():
            prev = self.precision
            self.set_precision(name)
            try:
                yield
            finally:
                self.set_precision(prev)
        return scope()

    # -- storage of the activations between the fp16-precision convs ------------------
    @property
    def act_storage(self) -> str:
        a = lib().isl_net_get_act_storage(self.h)
        return {v: k for k, v in ACT_STORAGES.items()}[a]

    def set_act_storage(self, name: str):
        """'fp32' (default, or the env ISLPOSE_ACT_STORAGE at creation) or 'fp16': under the 'x3'
        algorithm with precision 'fp16' the arena buffers between the convs hold fp16 -- the
        roundings the kernels would have made anyway, so the outputs are the same bits -- at
        half the activation bytes.  Stored without effect otherwise; a run with a conv that has
        no fp16-storage kernel keeps fp32 buffers as a whole (act_storage_active).  Unknown names
        raise ValueError."""
        check(lib().isl_net_set_act_storage(self.h, ACT_STORAGES[check_act_storage(name)]), "isl_net_set_act_storage")

    def act_storage_scope(self, name: str):
        import contextlib

        @contextlib.contextmanager
        def scope():
            prev = self.act_storage
            self.set_act_storage(name)
            try:
                yield
            finally:
                self.set_act_storage(prev)
        return scope()

    @property
    def act_storage_active(self) -> bool:
        """Whether the last run stored its activations as fp16 (isl_net_act_storage_active)."""
        return lib().isl_net_act_storage_active(self.h) == 1

    def set_split_k(self, mode):
        """K-range mode of the x3 convs (isl_net_set_split_k): 1 canonical ranges (default,
        batch-invariant bits), 0 none, 2 latency (also an adaptive, batch-dependent split
        of the other small grids).  True/False map to 2/0."""
        mode = {True: 2, False: 0}.get(mode, mode) if isinstance(mode, bool) else int(mode)
        check(lib().isl_net_set_split_k(self.h, mode), "isl_net_set_split_k")
        self.split_k = mode

    def set_graph(self, on: bool):
        """Replay the conv chain as a HIP graph after its first runs (isl_net_set_graph;
        default off, env ISLPOSE_NET_GRAPH=0|1 overrides): the same kernels and bits, without
        the per-launch host cost that bounds batch-1 frames."""
        check(lib().isl_net_set_graph(self.h, 1 if on else 0), "isl_net_set_graph")

    def algo_scope(self, algo: str):
        import contextlib

        @contextlib.contextmanager
        def scope():
            prev = self.algo
            self.set_algo(algo)
            try:
                yield
            finally:
                self.set_algo(prev)
        return scope()

    def range_ok(self, clear: bool = True) -> bool:
        """Synchronous check of the split-fp16 range flag (isl_net_check; it waits for the
        streams this net's runs were queued on, not the whole device): False if any conv
        output since the last clear reached |x| >= 65504."""
        rc = lib().isl_net_check(self.h, 1 if clear else 0)
        if rc == ISL_E_RANGE:
            return False
        check(rc, "isl_net_check")
        return True

    def check_async(self, flag_host, stream=None):
        """Stream-ordered range check (isl_net_check_async): flag_host, a pinned int32
        tensor of one element, holds the flag (then cleared on the device) once `stream`
        has reached this point."""
        assert flag_host.is_pinned() and flag_host.dtype.itemsize == 4
        check(lib().isl_net_check_async(self.h, ptr(flag_host), stream_handle(stream)), "isl_net_check_async")

    def range_trips(self) -> int:
        """Range-guard trips so far (isl_net_range_info): batches whose split-fp16 range
        check failed and that the caller recomputed on the fp32 kernels.  Synchronising."""
        t = ctypes.c_int64()
        check(lib().isl_net_range_info(self.h, ctypes.byref(t)), "isl_net_range_info")
        return t.value

    def preprocess(self, frames_u8, scale: float, stream=None):
        """frames uint8 [n,H,W,3] cuda -> fills the net input; returns (net_h, net_w)."""
        n, H, W, _ = frames_u8.shape
        nh, nw = ctypes.c_int32(), ctypes.c_int32()
        check(lib().isl_net_preprocess(self.h, ptr(frames_u8), n, H, W, float(scale), ctypes.byref(nh),
                                       ctypes.byref(nw), stream_handle(stream)), "isl_net_preprocess")
        return nh.value, nw.value

    def preprocess_crops(self, frames_u8, crops, scale_times_box: float, stream=None, flip=None):
        """frames uint8 [n,H,W,3] cuda; crops [(frame, x, y, w, h)] -> fills one net-input
        slot per crop (Hand.__call__'s resize of each crop); returns (net_h, net_w).
        flip: one bool per crop, None for none -- a flagged crop's slot is that of the
        contiguous crop[:, ::-1] (isl_net_preprocess_crops_flip)."""
        n, H, W, _ = frames_u8.shape
        arr = (IslCrop * len(crops))(*[IslCrop(*map(int, c)) for c in crops])
        nh, nw = ctypes.c_int32(), ctypes.c_int32()
        fl = flip_array(flip, len(crops))
        if fl is not None:
            check(lib().isl_net_preprocess_crops_flip(self.h, ptr(frames_u8), n, H, W, arr, fl, len(crops),
                                                      float(scale_times_box), ctypes.byref(nh), ctypes.byref(nw),
                                                      stream_handle(stream)), "isl_net_preprocess_crops_flip")
            return nh.value, nw.value
        check(lib().isl_net_preprocess_crops(self.h, ptr(frames_u8), n, H, W, arr, len(crops), float(scale_times_box),
                                             ctypes.byref(nh), ctypes.byref(nw), stream_handle(stream)),
              "isl_net_preprocess_crops")
        return nh.value, nw.value

    def debug_input(self, n, h, w, stream=None):
        import torch
        x = torch.empty((n, 3, h, w), device="cuda:%d" % self.device)
        check(lib().isl_net_debug_input(self.h, ptr(x), stream_handle(stream)), "isl_net_debug_input")
        return x

    def run(self, out0=None, out1=None, stream=None):
        check(lib().isl_net_run(self.h, ptr(out0), ptr(out1), stream_handle(stream)), "isl_net_run")

    def arena_info(self):
        """(bytes, arenas) of the net's activation arenas (isl_net_arena_info)."""
        b, k = ctypes.c_int64(), ctypes.c_int32()
        check(lib().isl_net_arena_info(self.h, ctypes.byref(b), ctypes.byref(k)), "isl_net_arena_info")
        return b.value, k.value

    def op_variants(self):
        """[(op name, variant code)] of the last run (isl_net_op_info): the conv kernel
        variant of every op; decode with decode_variant."""
        L = lib()
        n_ops, n_runs = ctypes.c_int32(), ctypes.c_int32()
        check(L.isl_net_timing(self.h, 0, ctypes.byref(n_ops), ctypes.byref(n_runs), None, None, None, None),
              "isl_net_timing")
        out = []
        for k in range(n_ops.value):
            name, var = ctypes.c_char_p(), ctypes.c_int32()
            check(L.isl_net_op_info(self.h, k, ctypes.byref(name), ctypes.byref(var)), "isl_net_op_info")
            out.append((name.value.decode(), var.value))
        return out

    def set_timing(self, on: bool):
        """Record HIP events around every op of the following runs (isl_net_set_timing)."""
        check(lib().isl_net_set_timing(self.h, 1 if on else 0), "isl_net_set_timing")

    def timing(self):
        """Per-op sums over the recorded runs: dict of numpy arrays ms, kind (0 pool,
        1 direct conv, 2 Winograd conv), flops (algorithmic), mfma_flops; plus n_runs."""
        import numpy as np
        L = lib()
        n_ops, n_runs = ctypes.c_int32(), ctypes.c_int32()
        check(L.isl_net_timing(self.h, 0, ctypes.byref(n_ops), ctypes.byref(n_runs), None, None, None, None),
              "isl_net_timing")
        k = n_ops.value
        ms, fl, mf = np.zeros(k), np.zeros(k), np.zeros(k)
        kind = np.zeros(k, np.int32)
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
        check(L.isl_net_timing(self.h, k, ctypes.byref(n_ops), ctypes.byref(n_runs), dp(ms),
                               kind.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dp(fl), dp(mf)), "isl_net_timing")
        return {"ms": ms, "kind": kind, "flops": fl, "mfma_flops": mf, "n_runs": n_runs.value}
