"""CPU checks of the general (non-integer factor) INTER_AREA resize: closed forms of the numpy oracle
(tests/resize_general_oracle.py), the library's host tap table (erp_resize_area_tab) against the oracle's
— indices equal, weights bit-equal — and the C-ABI additions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resize_general_oracle as rgo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["erp_resize_area_any", "erp_resize_area_any_device", "erp_resize_area_tab",
               "erp_frontend_track_resized"]


def test_oracle_three_pixels_to_two():
    # cells [0, 1.5) and [1.5, 3): (30 + 60/2) / 1.5 = 40, (60/2 + 90) / 1.5 = 80; y is the identity axis
    row = np.array([[30, 60, 90]], np.uint8)
    np.testing.assert_array_equal(rgo.resize_area_any(row, 2, 1), [[40, 80]])


@pytest.mark.parametrize("W,H,dW,dH", [(7, 5, 3, 2), (100, 37, 30, 11), (64, 48, 64, 20), (33, 17, 32, 16)])
def test_oracle_constant_images(W, H, dW, dH):
    for v in (200, 255, 0):  # 255 / 0: saturation
        out = rgo.resize_area_any(np.full((H, W), v, np.uint8), dW, dH)
        assert out.shape == (dH, dW) and out.dtype == np.uint8
        assert (out == v).all(), (v, np.unique(out))


def test_oracle_sliver_tail_is_dropped():
    """1001 -> 1000: the first cell [0, 1.001) ends 0.001 into pixel 1, which is not > 1e-3, so output 0 has
    the single tap (0, 1/1.001) — OpenCV's quirk, kept."""
    di, si, al = rgo.area_tab(1001, 1000)
    m = di == 0
    assert m.sum() == 1 and si[m][0] == 0
    assert al[m][0] == np.float32(1 / 1.001)
    assert (di == 1).sum() == 2  # the next cell has its head and tail


def test_oracle_integer_factors_delegate():
    img = np.random.default_rng(0).integers(0, 256, (40, 100), dtype=np.uint8)
    np.testing.assert_array_equal(rgo.resize_area_any(img, 20, 8), rgo._integer_oracle().resize_area(img, 20, 8))


TAB_PAIRS = [(4096, 960), (5376, 960), (2048, 480), (960, 640), (1001, 1000), (7, 3), (37, 11), (48, 20), (17, 16),
             (64, 64)]


@pytest.mark.parametrize("ssize,dsize", TAB_PAIRS)
def test_library_tab_equals_oracle(vio, ssize, dsize):
    di, si, al = vio.Context.resize_area_tab(ssize, dsize)
    odi, osi, oal = rgo.area_tab(ssize, dsize)
    np.testing.assert_array_equal(di, odi)
    np.testing.assert_array_equal(si, osi)
    assert al.dtype == oal.dtype == np.float32
    np.testing.assert_array_equal(al.view(np.uint32), oal.view(np.uint32))
    assert si.min() >= 0 and si.max() < ssize
    assert set(di.tolist()) == set(range(dsize))
    # ascending source index within an output index, output indices ascending
    assert (np.diff(di) >= 0).all() and (np.diff(si)[np.diff(di) == 0] == 1).all()


def test_tab_sizing_and_rejects(vio):
    L = vio.lib()
    n = C.c_int()
    assert L.erp_resize_area_tab(7, 3, None, None, None, 0, C.byref(n)) == 0 and n.value == 9
    di, si, al = np.full(4, -1, np.int32), np.full(4, -1, np.int32), np.zeros(4, np.float32)
    p = [a.ctypes.data_as(C.c_void_p) for a in (di, si, al)]
    assert L.erp_resize_area_tab(7, 3, *p, 2, C.byref(n)) == 0 and n.value == 9  # writes cap taps only
    assert di.tolist() == [0, 0, -1, -1] and si.tolist() == [0, 1, -1, -1]
    assert L.erp_resize_area_tab(3, 7, None, None, None, 0, C.byref(n)) == -38  # enlarging: VIO_ENOSYS
    assert L.erp_resize_area_tab(0, 0, None, None, None, 0, C.byref(n)) == -22
    assert L.erp_resize_area_tab(7, 3, None, None, None, 4, C.byref(n)) == -22


def test_header_and_library_export_the_new_symbols(vio):
    header = open(os.path.join(ROOT, "include", "vio360.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(vio.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in vio.EXPORTS
    assert lib.vio_abi_version() == 4  # additive
