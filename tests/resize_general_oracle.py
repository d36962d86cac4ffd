"""resize_general_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

numpy restatement of cv::resize(src, dst, Size(dW, dH), 0, 0, INTER_AREA) of a 1-channel u8 image for
any downscale (OpenCV 4.x modules/imgproc/src/resize.cpp):

* both scale factors integers: the area-fast path, oracle/resize_oracle.py;
* otherwise the general area path.  computeResizeAreaTab builds, per axis and in IEEE double, the taps
  (output index, source index, f32 weight) of every output cell [d·scale, (d+1)·scale): a partial head
  pixel, the whole pixels at weight 1/cell, a partial tail pixel (head / tail only when wider than 1e-3).
  ResizeArea_Invoker<uchar, float> then accumulates in f32, multiply and add rounded separately, taps in
  ascending source order: dst = saturate_cast<uchar>(Σ_y beta · (Σ_x src · alpha)).

OpenCV is not available to the tests: parity with it is unpinned; pinned here by closed forms
(tests/test_resize_general.py).
"""
import importlib.util
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _integer_oracle():
    spec = importlib.util.spec_from_file_location("resize_oracle", os.path.join(ROOT, "oracle", "resize_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def area_tab(ssize, dsize):
    """computeResizeAreaTab for one axis -> (di int32, si int32, alpha float32), taps in OpenCV's order."""
    scale = float(ssize) / float(dsize)
    di, si, al = [], [], []
    for d in range(dsize):
        fsx1 = d * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = math.ceil(fsx1), math.floor(fsx2)
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            di.append(d), si.append(sx1 - 1), al.append(np.float32((sx1 - fsx1) / cell))
        for sx in range(sx1, sx2):
            di.append(d), si.append(sx), al.append(np.float32(1.0 / cell))
        if fsx2 - sx2 > 1e-3:
            di.append(d), si.append(sx2), al.append(np.float32(min(min(fsx2 - sx2, 1.0), cell) / cell))
    return np.array(di, np.int32), np.array(si, np.int32), np.array(al, np.float32)


def _by_position(ssize, dsize):
    """the taps as (dsize, P) arrays indexed by tap position: source index (0 where there is no such tap)
    and weight (0 where there is no such tap: x + 0·s = x exactly, the sums stay non-negative)"""
    di, si, al = area_tab(ssize, dsize)
    start = np.searchsorted(di, np.arange(dsize))
    pos = np.arange(len(di)) - start[di]
    P = int(pos.max()) + 1
    idx = np.zeros((dsize, P), np.int64)
    w = np.zeros((dsize, P), np.float32)
    idx[di, pos] = si
    w[di, pos] = al
    return idx, w


def resize_area_any(src, dW, dH):
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    assert 0 < dW <= W and 0 < dH <= H
    if W % dW == 0 and H % dH == 0:
        return _integer_oracle().resize_area(src, dW, dH)
    ix, wx = _by_position(W, dW)
    iy, wy = _by_position(H, dH)
    s32 = src.astype(np.float32)
    total = np.zeros((dH, dW), np.float32)
    for j in range(iy.shape[1]):
        rows = s32[iy[:, j]]  # (dH, W)
        buf = np.zeros((dH, dW), np.float32)
        for k in range(ix.shape[1]):
            buf = buf + rows[:, ix[:, k]] * wx[None, :, k]
        total = total + wy[:, j, None] * buf
    return np.clip(np.rint(total), 0, 255).astype(np.uint8)
