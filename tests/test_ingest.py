"""CPU checks of the colour / packed-YUV ingest: closed forms of the two luma rules in the numpy oracle
(tests/ingest_oracle.py), the library's host luma (erp_luma_u8, the function every kernel uses) against the
oracle over all 2^24 BGR triples, the other formats, erp_pixel_bytes, the host-side rejects and the C-ABI
additions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ingest_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["erp_pixel_bytes", "erp_luma_u8", "erp_ingest", "erp_ingest_device", "erp_ingest_set_route",
               "erp_ingest_check", "erp_tracker_upload_pixels", "erp_frontend_track_pixels"]
RULES = (io.CVTCOLOR, io.IMREAD)
EINVAL, ENOSYS = -22, -38


@pytest.fixture(scope="module")
def all_bgr():
    """every (B, G, R) triple once, (2^24, 3) u8, B the slowest axis"""
    v = np.arange(256, dtype=np.uint8)
    out = np.empty((256, 256, 256, 3), np.uint8)
    out[..., 0] = v[:, None, None]
    out[..., 1] = v[None, :, None]
    out[..., 2] = v[None, None, :]
    return out.reshape(-1, 3)


@pytest.fixture(scope="module")
def all_luma(all_bgr):
    return {rule: io.luma(all_bgr, io.BGR8, rule) for rule in RULES}


def test_oracle_grey_triples_map_to_themselves():
    v = np.arange(256, dtype=np.uint8)
    for rule in RULES:
        np.testing.assert_array_equal(io.luma_bgr(v, v, v, rule), v)


def test_oracle_primaries():
    for rule in RULES:
        assert io.luma_bgr(255, 0, 0, rule) == 29
        assert io.luma_bgr(0, 255, 0, rule) == 150
        assert io.luma_bgr(0, 0, 255, rule) == 76


def test_oracle_rules_differ_by_one_on_43864_triples(all_luma):
    assert io.luma_bgr(0, 15, 106, io.CVTCOLOR) == 41 and io.luma_bgr(0, 15, 106, io.IMREAD) == 40
    d = all_luma[io.CVTCOLOR].astype(np.int16) - all_luma[io.IMREAD].astype(np.int16)
    assert int((d != 0).sum()) == 43864
    assert int(np.abs(d).max()) == 1


@pytest.mark.parametrize("rule", RULES)
def test_library_luma_all_bgr_triples(vio, all_bgr, all_luma, rule):
    np.testing.assert_array_equal(vio.Context.luma_u8(all_bgr, vio.VIO_PIX_BGR8, rule), all_luma[rule])


@pytest.mark.parametrize("fmt", [io.RGB8, io.BGRA8, io.RGBA8])
@pytest.mark.parametrize("rule", RULES)
def test_library_luma_other_colour_formats(vio, fmt, rule):
    """2^16 random triples, random alpha; RGB is BGR with the ends swapped"""
    bgr = np.random.default_rng(fmt).integers(0, 256, (1 << 16, 1, 3), dtype=np.uint8)
    px = io.from_bgr(bgr, fmt, seed=3)
    assert px.shape == (1 << 16, 1, io.BPP[fmt])
    want = io.luma(bgr, io.BGR8, rule)
    np.testing.assert_array_equal(io.luma(px, fmt, rule), want)
    np.testing.assert_array_equal(vio.Context.luma_u8(px, fmt, rule), want)


def test_library_luma_422_and_grey(vio):
    px = np.random.default_rng(5).integers(0, 256, (64, 2), dtype=np.uint8)
    for luma in (0, 1, 77):  # ignored
        np.testing.assert_array_equal(vio.Context.luma_u8(px, vio.VIO_PIX_YUYV, luma), px[:, 0])
        np.testing.assert_array_equal(vio.Context.luma_u8(px, vio.VIO_PIX_UYVY, luma), px[:, 1])
    np.testing.assert_array_equal(io.luma(px, io.YUYV), px[:, 0])
    np.testing.assert_array_equal(io.luma(px, io.UYVY), px[:, 1])
    g = px[:, 0].copy()
    np.testing.assert_array_equal(vio.Context.luma_u8(g, vio.VIO_PIX_GRAY8), g)


def test_pixel_bytes(vio):
    L = vio.lib()
    assert [L.erp_pixel_bytes(f) for f in range(7)] == [1, 3, 3, 4, 4, 2, 2]
    assert [vio.Context.pixel_bytes(f) for f in range(7)] == [io.BPP[f] for f in range(7)]
    assert L.erp_pixel_bytes(7) == EINVAL and L.erp_pixel_bytes(-1) == EINVAL
    with pytest.raises(vio.VioError):
        vio.Context.pixel_bytes(7)


def test_luma_rejects(vio):
    L = vio.lib()
    px, out = np.zeros(16, np.uint8), np.zeros(4, np.uint8)
    p, o = px.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.erp_luma_u8(vio.VIO_PIX_BGR8, 0, p, 4, o) == 0
    assert L.erp_luma_u8(7, 0, p, 4, o) == EINVAL           # unknown format
    assert L.erp_luma_u8(vio.VIO_PIX_BGR8, 2, p, 4, o) == EINVAL   # unknown luma rule
    assert L.erp_luma_u8(vio.VIO_PIX_YUYV, 0, p, 3, o) == EINVAL   # half a 4:2:2 pixel pair
    assert L.erp_luma_u8(vio.VIO_PIX_BGR8, 0, None, 4, o) == EINVAL
    assert L.erp_luma_u8(vio.VIO_PIX_BGR8, 0, p, -1, o) == EINVAL


def test_ingest_argument_check(vio):
    """erp_ingest_check is the check erp_ingest and erp_ingest_device make before anything else"""
    chk = vio.lib().erp_ingest_check
    BGR, YUYV = vio.VIO_PIX_BGR8, vio.VIO_PIX_YUYV
    assert chk(BGR, 0, 40, 24, 120, 10, 6, 10) == 0
    assert chk(BGR, 1, 40, 24, 125, 11, 7, 16) == 0
    assert chk(BGR, 0, 40, 24, 120, 40, 24, 40) == 0        # convert only
    assert chk(7, 0, 40, 24, 120, 10, 6, 10) == EINVAL      # unknown format
    assert chk(-1, 0, 40, 24, 120, 10, 6, 10) == EINVAL
    assert chk(BGR, 2, 40, 24, 120, 10, 6, 10) == EINVAL    # unknown luma rule
    assert chk(YUYV, 2, 40, 24, 80, 10, 6, 10) == 0         # ... which 4:2:2 ignores
    assert chk(vio.VIO_PIX_GRAY8, 2, 40, 24, 40, 10, 6, 10) == 0
    assert chk(YUYV, 0, 41, 24, 82, 10, 6, 10) == EINVAL    # odd W for 4:2:2
    assert chk(vio.VIO_PIX_UYVY, 0, 41, 24, 82, 10, 6, 10) == EINVAL
    assert chk(BGR, 0, 40, 24, 119, 10, 6, 10) == EINVAL    # stride < W * bpp
    assert chk(vio.VIO_PIX_BGRA8, 0, 40, 24, 159, 10, 6, 10) == EINVAL
    assert chk(YUYV, 0, 40, 24, 79, 10, 6, 10) == EINVAL
    assert chk(BGR, 0, 40, 24, 120, 10, 6, 9) == EINVAL     # dst_stride < dW
    assert chk(BGR, 0, 0, 24, 120, 10, 6, 10) == EINVAL
    assert chk(BGR, 0, 40, 24, 120, 41, 6, 41) == ENOSYS    # enlarging
    assert chk(BGR, 0, 40, 24, 120, 10, 25, 10) == ENOSYS


def test_ingest_rejects_without_a_context(vio):
    """a null context is refused before anything else is looked at (the size rejects need a context: GPU tests)"""
    L = vio.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.erp_ingest(None, p, vio.VIO_PIX_BGR8, 0, 4, 4, 12, p, 2, 2, 2) == EINVAL
    assert L.erp_ingest_device(None, p, vio.VIO_PIX_BGR8, 0, 4, 4, 12, 1, p, 2, 2, 2) == EINVAL
    assert L.erp_ingest_set_route(None, 0) == EINVAL
    assert L.erp_tracker_upload_pixels(None, 0, p, vio.VIO_PIX_BGR8, 0, 4, 4, 12) == EINVAL
    assert L.erp_frontend_track_pixels(None, p, vio.VIO_PIX_BGR8, 0, 4, 4, 12, None) == EINVAL


def test_wrapper_rejects_wrong_pixel_axis(vio):
    with pytest.raises(vio.VioError):
        vio.Context.luma_u8(np.zeros((4, 4), np.uint8), vio.VIO_PIX_BGR8)


def test_header_and_library_export_the_new_symbols(vio):
    header = open(os.path.join(ROOT, "include", "vio360.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(vio.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in vio.EXPORTS
    for name, value in [("VIO_PIX_GRAY8", 0), ("VIO_PIX_BGR8", 1), ("VIO_PIX_RGB8", 2), ("VIO_PIX_BGRA8", 3),
                        ("VIO_PIX_RGBA8", 4), ("VIO_PIX_YUYV", 5), ("VIO_PIX_UYVY", 6), ("VIO_LUMA_CVTCOLOR", 0),
                        ("VIO_LUMA_IMREAD", 1)]:
        assert re.search(r"\b" + name + r"\s*=\s*%d\b" % value, header), name
        assert getattr(vio, name) == value
    assert lib.vio_abi_version() == 4  # additive
