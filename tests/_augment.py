"""Test helper for the augmented extraction: a numpy restatement of the variant definition
(DESIGN.md section 4.2h), written independently of islpose/augment.py, and a restatement of
torchvision v2's fp32 tensor route for the rotation on torch CPU ops (torchvision itself is
absent, so that parity is unpinned; the route is restated from its source).

variant(frame, angle=None, threshold=256, swap_rb=False): rotation (nearest neighbour, about
the centre, counter-clockwise for positive angles, fill 0, fp64 coordinates in a fixed
operation order), then solarize (v -> 255 - v where v >= threshold; 256: off), with the
channel reversal applied to the source."""
import math

import numpy as np


def source_coords(H, W, angle):
    """fp64 source coordinates (xs, ys), each [H, W], of every output pixel."""
    r = math.radians(-angle)
    c, s = math.cos(r), math.sin(r)
    cx = (W - 1) * 0.5
    cy = (H - 1) * 0.5
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx = np.subtract(ii, cx)
    dy = np.subtract(jj, cy)
    t0 = np.multiply(c, dx)
    t1 = np.multiply(s, dy)
    xs = np.add(np.add(t0, t1), cx)
    u0 = np.multiply(-s, dx)
    u1 = np.multiply(c, dy)
    ys = np.add(np.add(u0, u1), cy)
    return xs, ys


def variant(frame, angle=None, threshold=256, swap_rb=False):
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    H, W, _ = frame.shape
    src = frame[:, :, [2, 1, 0]] if swap_rb else frame
    if angle is None:
        out = src.copy()
    else:
        xs, ys = source_coords(H, W, angle)
        xr, yr = np.rint(xs), np.rint(ys)              # half to even
        ok = (0 <= xr) & (xr <= W - 1) & (0 <= yr) & (yr <= H - 1)
        flat = (np.where(ok, yr, 0).astype(np.int64) * W + np.where(ok, xr, 0).astype(np.int64)).ravel()
        out = np.take(src.reshape(H * W, 3), flat, axis=0).reshape(H, W, 3)
        out[~ok] = 0
    out = np.ascontiguousarray(out, dtype=np.uint8)
    if threshold < 256:
        hit = out >= threshold
        out[hit] = 255 - out[hit]
    return out


def variants(frames, items, swap_rb=False):
    """items: [(src, angle or None, threshold)] -> uint8 [len(items), H, W, 3]."""
    return np.stack([variant(frames[src], angle, thr, swap_rb) for src, angle, thr in items])


def tv_inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix(inverted=True)."""
    rot = math.radians(angle)
    sx = math.radians(shear[0])
    sy = math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def tv_rotate_fp32(frame, angle):
    """torchvision v2 F.rotate of a uint8 tensor image (nearest, expand=False, centre None,
    fill 0): _get_inverse_affine_matrix -> _gen_affine_grid -> grid_sample(mode='nearest',
    padding_mode='zeros', align_corners=False), all fp32 on torch CPU ops."""
    import torch
    H, W, _ = frame.shape
    matrix = tv_inverse_affine_matrix([0.0, 0.0], -angle, [0.0, 0.0], 1.0, [0.0, 0.0])
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, H, W, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + d, W * 0.5 + d - 1, steps=W))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + d, H * 0.5 + d - 1, steps=H).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32)
    grid = base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)
    img = torch.from_numpy(np.ascontiguousarray(frame)).permute(2, 0, 1)[None].to(torch.float32)
    out = torch.nn.functional.grid_sample(img, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    return out.round_()[0].permute(1, 2, 0).to(torch.uint8).numpy()
