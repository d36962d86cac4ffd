"""ingest_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

numpy restatement of the colour / packed-YUV ingest (erp_ingest*): the grey image that a luma rule makes of a
packed frame, then tests/resize_general_oracle.py's cv::resize(..., INTER_AREA).

Formats (include/vio360.h VIO_PIX_*): GRAY8 (H, W) or (H, W, 1); BGR8 / RGB8 (H, W, 3); BGRA8 / RGBA8 (H, W, 4),
alpha ignored; YUYV / UYVY (H, W, 2), the luma byte of pixel x being byte 2x / 2x + 1 of the row, taken as is
(OpenCV's COLOR_YUV2GRAY_YUY2 / _UYVY).  Luma rules (VIO_LUMA_*), integer arithmetic only:
  CVTCOLOR  (3735 B + 19235 G + 9798 R + 16384) >> 15   OpenCV 4.x cvtColor(BGR2GRAY) for u8
  IMREAD    (1868 B +  9617 G + 4899 R +  8192) >> 14   imread(IMREAD_GRAYSCALE) of a colour PNG
OpenCV is not available to the tests: parity with it is unpinned; pinned here by closed forms
(tests/test_ingest.py).
"""
import numpy as np

import resize_general_oracle as rgo

GRAY8, BGR8, RGB8, BGRA8, RGBA8, YUYV, UYVY = range(7)
CVTCOLOR, IMREAD = 0, 1
BPP = {GRAY8: 1, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4, YUYV: 2, UYVY: 2}


def luma_bgr(b, g, r, rule):
    b, g, r = (np.asarray(c).astype(np.int64) for c in (b, g, r))
    if rule == CVTCOLOR:
        return ((3735 * b + 19235 * g + 9798 * r + 16384) >> 15).astype(np.uint8)
    assert rule == IMREAD
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def luma(img, fmt, rule=CVTCOLOR):
    """packed pixels (..., bpp) u8 -> grey (...) u8"""
    a = np.asarray(img, np.uint8)
    if fmt == GRAY8:
        return a[..., 0].copy() if a.ndim == 3 else a.copy()
    assert a.shape[-1] == BPP[fmt]
    if fmt in (YUYV, UYVY):
        return a[..., 0 if fmt == YUYV else 1].copy()
    if fmt in (BGR8, BGRA8):
        return luma_bgr(a[..., 0], a[..., 1], a[..., 2], rule)
    return luma_bgr(a[..., 2], a[..., 1], a[..., 0], rule)


def ingest(img, fmt, rule, dW, dH):
    return rgo.resize_area_any(luma(img, fmt, rule), dW, dH)


def from_bgr(bgr, fmt, seed=0):
    """a packed frame of format fmt whose colour is the (H, W, 3) BGR array (alpha random; the 4:2:2 formats
    take channel 1 as luma and random chroma)"""
    bgr = np.asarray(bgr, np.uint8)
    rng = np.random.default_rng(seed)
    H, W = bgr.shape[:2]
    if fmt == GRAY8:
        return bgr[..., 1].copy()
    if fmt == BGR8:
        return bgr.copy()
    if fmt == RGB8:
        return bgr[..., ::-1].copy()
    if fmt in (BGRA8, RGBA8):
        alpha = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
        return np.concatenate([bgr if fmt == BGRA8 else bgr[..., ::-1], alpha], axis=2)
    chroma = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return np.stack([bgr[..., 1], chroma] if fmt == YUYV else [chroma, bgr[..., 1]], axis=2)
