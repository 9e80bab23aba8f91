"""numpy restatement of k_remap_u8 (camera_calibration_amd/csrc/kernels_undistort.hip), the arithmetic include/cba_undistort.h
fixes: every operation in float32 and rounded on its own (numpy does not fuse), so every byte is reproduced.

    (sx, sy) = the map entry; NaN or a magnitude above 2^24 in either: fill
    x0 = floorf(sx), wx = sx - x0, x1 = x0 + 1, both clamped into [0, src_w - 1]; y alike
    top = p00 + wx * (p10 - p00), bot = p01 + wx * (p11 - p01), v = top + wy * (bot - top), byte = (uint8_t)(int)(v + 0.5f)
"""
import numpy as np

F32 = np.float32
LIMIT = F32(16777216.0)


def _split(map_xy, src_w, src_h):
    m = np.asarray(map_xy, dtype=np.float32)
    sx, sy = m[..., 0], m[..., 1]
    with np.errstate(invalid="ignore"):
        good = (np.abs(sx) <= LIMIT) & (np.abs(sy) <= LIMIT)
    sx, sy = np.where(good, sx, F32(0)), np.where(good, sy, F32(0))
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = sx - fx, sy - fy
    assert wx.dtype == np.float32 and wy.dtype == np.float32
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    return good, wx, wy, ix, iy


def remap(map_xy, image, fill=0):
    """image (src_h, src_w) or (src_h, src_w, 3) uint8 -> (H, W[, 3]) uint8 through map_xy (H, W, 2)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim in (2, 3)
    src_h, src_w = image.shape[:2]
    good, wx, wy, ix, iy = _split(map_xy, src_w, src_h)
    x0, x1 = np.clip(ix, 0, src_w - 1), np.clip(ix + 1, 0, src_w - 1)
    y0, y1 = np.clip(iy, 0, src_h - 1), np.clip(iy + 1, 0, src_h - 1)
    if image.ndim == 3:
        wx, wy = wx[..., None], wy[..., None]
    p00, p10 = image[y0, x0].astype(np.float32), image[y0, x1].astype(np.float32)
    p01, p11 = image[y1, x0].astype(np.float32), image[y1, x1].astype(np.float32)
    top = p00 + wx * (p10 - p00)
    bot = p01 + wx * (p11 - p01)
    v = top + wy * (bot - top)
    assert v.dtype == np.float32
    out = (v + F32(0.5)).astype(np.int32).astype(np.uint8)
    out[~good] = fill
    return out


def clamped_samples(map_xy, src_w, src_h):
    """How many of the four sampled indices of the valid entries were moved by the border clamp."""
    good, _, _, ix, iy = _split(map_xy, src_w, src_h)
    moved = sum((np.clip(i, 0, n - 1) != i).astype(int) for i, n in ((ix, src_w), (ix + 1, src_w), (iy, src_h), (iy + 1, src_h)))
    return int(moved[good].sum())


def remap_longdouble(map_xy, image):
    """The same bilinear formula in long double, unrounded: (value (H, W[, 3]) before the + 0.5 and the truncation, valid (H, W))."""
    image = np.asarray(image)
    src_h, src_w = image.shape[:2]
    good, _, _, ix, iy = _split(map_xy, src_w, src_h)
    m = np.asarray(map_xy, dtype=np.float32).astype(np.longdouble)
    sx, sy = np.where(good, m[..., 0], 0), np.where(good, m[..., 1], 0)
    wx, wy = sx - np.floor(sx), sy - np.floor(sy)
    x0, x1 = np.clip(ix, 0, src_w - 1), np.clip(ix + 1, 0, src_w - 1)
    y0, y1 = np.clip(iy, 0, src_h - 1), np.clip(iy + 1, 0, src_h - 1)
    if image.ndim == 3:
        wx, wy = wx[..., None], wy[..., None]
    ld = lambda a: a.astype(np.longdouble)
    top = ld(image[y0, x0]) * (1 - wx) + ld(image[y0, x1]) * wx
    bot = ld(image[y1, x0]) * (1 - wx) + ld(image[y1, x1]) * wx
    return top * (1 - wy) + bot * wy, good
