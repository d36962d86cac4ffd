"""CPU checks of the lens-to-ERP warp's host side (csrc/warp_host.cpp) against tests/warp_oracle.py: the
quantisation bitwise, the three map generators against their float64 restatement, closed-form properties of the
blend on library-made maps, and the argument checks.  The kernel itself: tests/test_warp_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import ingest_oracle as io
import warp_oracle as wo

MODES = (wo.X_CONSTANT, wo.X_WRAP, wo.Y_REPLICATE)
R_DST = wo.rot_y(0.1234) @ wo.rot_x(0.0567)
DSTS = [(48, 24), (96, 48)]
EINVAL = -22


def coordinates(S, n, seed):
    """n float32 coordinates: uniform in [-3, S + 3], exact integers, ties of the rounding, and the special values"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-3, S + 3, n).astype(np.float32)
    k = n // 4
    s[:k] = rng.integers(-3, S + 4, k)                                     # exact integers
    s[k:2 * k] = rng.integers(-3, S + 4, k) + rng.integers(0, 32, k) / 32 + 1 / 64   # ties: q + 1/2 exactly
    sp = wo.special_coordinates(S)
    s[2 * k:2 * k + sp.size] = sp
    return s


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [37, 1, 5760])
def test_quantize_equals_the_oracle(vio, mode, S):
    s = coordinates(S, 100000, seed=S + mode)
    q, valid = vio.warp_quantize(s, S, mode)
    oq, ov = wo.quantize(s, S, mode)
    np.testing.assert_array_equal(valid.astype(bool), ov)
    np.testing.assert_array_equal(q, oq)
    assert (~ov).sum() >= 3 and (q[~ov] == 0).all()
    if mode == wo.X_WRAP:
        assert q.min() >= 0 and q.max() < 32 * S
    else:
        assert q.min() == -32 and q.max() == 32 * S


def test_quantize_known_values(vio):
    s = [5 + 1 / 64, 5 + 3 / 64, -1, -0.5, 36, 36.5, 37, 1e9, -1e9]
    q, valid = vio.warp_quantize(s, 37, wo.X_CONSTANT)
    assert valid.all() and q.tolist() == [160, 162, -32, -16, 1152, 1168, 1184, 1184, -32]  # half to even; clamped
    q, _ = vio.warp_quantize(s, 37, wo.X_WRAP)
    assert q.tolist() == [160, 162, 1152, 1168, 1152, 1168, 0, int(32e9) % 1184, -int(32e9) % 1184]
    q, valid = vio.warp_quantize([np.nan, np.inf, -np.inf], 37, wo.Y_REPLICATE)
    assert not valid.any() and not q.any()


# ---- generators against the float64 restatement ----

def assert_maps_close(got, want, margin, what):
    """|d| <= 2^-22 max(1, |s|) + 1e-9 px (float32 rounding of the stored map plus libm noise) and identical NaN
    positions, on every pixel at least 1e-9 off a selection boundary; at most 1 % may be that close"""
    keep = margin > 1e-9
    print(f"{what}: smallest margin {margin.min():.3e}, excluded {(~keep).sum()} of {keep.size}")
    assert (~keep).sum() <= 0.01 * keep.size
    for g, w in zip(got, want):
        assert g.dtype == np.float32
        np.testing.assert_array_equal(np.isnan(g)[keep], np.isnan(w)[keep])
        ok = keep & ~np.isnan(w)
        err = np.abs(g.astype(np.float64)[ok] - w[ok])
        assert (err <= 2.0 ** -22 * np.maximum(1.0, np.abs(w[ok])) + 1e-9).all(), (what, err.max())


@pytest.mark.parametrize("dW,dH", DSTS)
def test_map_erp(vio, dW, dH):
    sW, sH = 64, 32
    got = vio.warp_map_erp(sW, sH, dW, dH, R_DST)
    b = wo.dst_bearings(dW, dH, R_DST)
    margin = np.pi - np.abs(np.arctan2(b[..., 0], b[..., 2]))  # the +-pi seam of atan2
    assert_maps_close(got, wo.map_erp(sW, sH, dW, dH, R_DST), margin, "erp")
    assert not np.isnan(got[0]).any()


@pytest.mark.parametrize("theta_max_deg", [95.0, 80.0])
@pytest.mark.parametrize("dW,dH", DSTS)
def test_map_fisheye(vio, dW, dH, theta_max_deg):
    lenses = wo.dual_fisheye(theta_max_deg)
    got = vio.warp_map_fisheye(lenses, dW, dH, R_DST)
    theta, _ = wo.fisheye_angles(lenses, dW, dH, R_DST)
    margin = np.minimum(np.abs(theta[0] - theta[1]),                      # the seam between the lenses
                        np.abs(theta - np.deg2rad(theta_max_deg)).min(axis=0))   # the rim of either field of view
    assert_maps_close(got, wo.map_fisheye(lenses, dW, dH, R_DST), margin, f"fisheye {theta_max_deg}")
    invalid = np.isnan(got[0]).mean()
    if theta_max_deg < 90:
        assert 0.1 < invalid < 0.4, invalid  # the band that neither lens covers
    else:
        assert invalid == 0
        assert (got[0] < 32).any() and (got[0] >= 32).any()  # both lenses are used


@pytest.mark.parametrize("eac", [0, 1])
@pytest.mark.parametrize("dW,dH", DSTS)
def test_map_cubemap(vio, dW, dH, eac):
    faces = wo.cube_faces_3x2(16)
    got = vio.warp_map_cubemap(faces, eac, 48, 32, dW, dH, R_DST)
    z, _ = wo.cube_depths(faces, dW, dH, R_DST)
    zs = np.sort(z, axis=0)
    margin = zs[-1] - zs[-2]  # the edge between two faces
    want = wo.map_cubemap(faces, eac, dW, dH, R_DST)
    assert_maps_close(got, want, margin, f"cubemap eac={eac}")
    assert not np.isnan(got[0]).any()
    cell = (got[0] // 16).astype(int) + 3 * (got[1] // 16).astype(int)
    assert set(np.unique(cell)) == set(range(6))  # every face is used
    assert got[0].min() >= 0 and got[0].max() <= 47 and got[1].min() >= 0 and got[1].max() <= 31


def test_eac_differs_from_the_plain_cubemap(vio):
    faces = wo.cube_faces_3x2(16)
    a = vio.warp_map_cubemap(faces, 0, 48, 32, 48, 24, R_DST)
    b = vio.warp_map_cubemap(faces, 1, 48, 32, 48, 24, R_DST)
    assert np.abs(a[0] - b[0]).max() > 0.5


# ---- properties: the oracle's blend on the library's maps and quantisation ----

def library_quantized_remap(vio, grey, mx, my, bx, by, bv=0):
    """wo.remap_grey, after a check that the library quantises these maps as the oracle does"""
    sH, sW = grey.shape
    for m, S, mode in ((mx, sW, bx), (my, sH, by)):
        q, valid = vio.warp_quantize(m, S, mode)
        oq, ov = wo.quantize(m.reshape(-1), S, mode)
        np.testing.assert_array_equal(q, oq)
        np.testing.assert_array_equal(valid.astype(bool), ov)
    return wo.remap_grey(grey, mx, my, bx, by, bv)


def test_identity_map_reproduces_the_image(vio):
    img = np.random.default_rng(1).integers(0, 256, (24, 48), dtype=np.uint8)
    mx, my = vio.warp_map_erp(48, 24, 48, 24)
    for bx in (wo.X_CONSTANT, wo.X_WRAP):
        for by in (wo.Y_CONSTANT, wo.Y_REPLICATE):
            np.testing.assert_array_equal(library_quantized_remap(vio, img, mx, my, bx, by, 77), img)


@pytest.mark.parametrize("k", [1, 5, 24, 47])
def test_yaw_of_whole_pixels_is_a_roll(vio, k):
    """R_dst = rotY(2 pi k / W): every row but the pole's (row 0, where the longitude is ill-conditioned) is the
    source row rolled by k pixels"""
    W, H = 48, 24
    img = np.random.default_rng(k).integers(0, 256, (H, W), dtype=np.uint8)
    mx, my = vio.warp_map_erp(W, H, W, H, wo.rot_y(2 * np.pi * k / W))
    qx, _ = vio.warp_quantize(mx[1:], W, wo.X_WRAP)
    qy, _ = vio.warp_quantize(my[1:], H, wo.Y_REPLICATE)
    assert not (qx & 31).any() and not (qy & 31).any()  # the map lands on integers
    out = library_quantized_remap(vio, img, mx, my, wo.X_WRAP, wo.Y_REPLICATE)
    np.testing.assert_array_equal(out[1:], np.roll(img, -k, axis=1)[1:])


def test_a_constant_image_stays_constant(vio):
    rng = np.random.default_rng(3)
    maps = [vio.warp_map_erp(37, 23, 48, 24, R_DST),
            (rng.uniform(-50, 90, (11, 19)).astype(np.float32), rng.uniform(-50, 70, (11, 19)).astype(np.float32))]
    for mx, my in maps:
        for v in (0, 1, 128, 255):
            out = library_quantized_remap(vio, np.full((23, 37), v, np.uint8), mx, my, wo.X_WRAP, wo.Y_REPLICATE, 99)
            assert (out == v).all()


def test_oracle_blend_closed_forms():
    """the oracle itself: a half-pixel step is the rounded mean, borders and invalid pixels read border_value"""
    img = np.array([[10, 20], [31, 41]], np.uint8)
    mx = np.array([[0.5, 0.0, 0.5, 1.5, -1.0, np.nan]], np.float32)
    my = np.array([[0.0, 0.5, 0.5, 0.0, 0.0, 0.0]], np.float32)
    out = wo.remap_grey(img, mx, my, wo.X_CONSTANT, wo.Y_CONSTANT, 200)
    assert out.tolist() == [[15, 21, 26, 110, 200, 200]]  # (10+20)/2, (10+31+1)/2, (102+2)/4, (20+200)/2
    out = wo.remap_grey(img, mx, my, wo.X_WRAP, wo.Y_REPLICATE, 200)
    assert out.tolist() == [[15, 21, 26, 15, 20, 200]]  # column 2 is column 0; -1 is column 1
    my2 = np.array([[1.5, -3.0, 7.0, 1.0, 1.0, 1.0]], np.float32)
    out = wo.remap_grey(img, np.zeros((1, 6), np.float32), my2, wo.X_CONSTANT, wo.Y_REPLICATE, 200)
    assert out.tolist() == [[31, 10, 31, 31, 31, 31]]  # rows clamped


# ---- argument errors ----

def host_warp(vio, sW=40, sH=24, dW=10, dH=6, map_stride=None, bx=0, by=0, bv=0, maps=True):
    """erp_warp_create without a context (a host-only object) -> (rc, handle)"""
    stride = dW if map_stride is None else map_stride
    m = np.zeros((max(dH, 1), max(stride, 1)), np.float32)
    h = C.c_void_p()
    p = m.ctypes.data_as(C.c_void_p) if maps else None
    rc = vio.lib().erp_warp_create(None, p, p, dW, dH, stride, sW, sH, bx, by, bv, C.byref(h))
    return rc, h


def test_create_rejects_bad_arguments(vio):
    for kw in (dict(dW=0), dict(dH=-1), dict(sW=0), dict(sH=0), dict(sW=(1 << 25) + 1), dict(map_stride=9),
               dict(bx=2), dict(bx=3), dict(by=1), dict(by=3), dict(bv=-1), dict(bv=256), dict(maps=False)):
        rc, h = host_warp(vio, **kw)
        assert rc == EINVAL and not h.value, kw
    rc = vio.lib().erp_warp_create(None, None, None, 10, 6, 10, 40, 24, 0, 0, 0, None)
    assert rc == EINVAL


def test_check_rejects_bad_arguments(vio):
    L = vio.lib()
    rc, h = host_warp(vio, sW=40, sH=24, dW=10, dH=6)
    assert rc == 0 and h.value
    try:
        for fmt in range(7):
            bpp = io.BPP[fmt]
            for luma in (io.CVTCOLOR, io.IMREAD):
                assert L.erp_warp_check(h, fmt, luma, 40 * bpp, 10) == 0
            assert L.erp_warp_check(h, fmt, 0, 40 * bpp + 7, 31) == 0
            assert L.erp_warp_check(h, fmt, 0, 40 * bpp - 1, 10) == EINVAL   # stride < sW * bpp
            assert L.erp_warp_check(h, fmt, 0, 40 * bpp, 9) == EINVAL        # dst_stride < dW
        assert L.erp_warp_check(h, 7, 0, 400, 10) == EINVAL                  # unknown format
        assert L.erp_warp_check(h, -1, 0, 400, 10) == EINVAL
        assert L.erp_warp_check(h, io.BGR8, 2, 120, 10) == EINVAL            # unknown luma rule
        assert L.erp_warp_check(h, io.GRAY8, 2, 40, 10) == 0                 # ignored, as by erp_ingest
        assert L.erp_warp_check(h, io.YUYV, 2, 80, 10) == 0
        assert L.erp_warp_check(None, io.GRAY8, 0, 40, 10) == EINVAL
        # a host-only object launches nothing
        buf = np.zeros(40 * 24, np.uint8)
        p = buf.ctypes.data_as(C.c_void_p)
        assert L.erp_warp_apply(h, p, io.GRAY8, 0, 40, p, 10) == EINVAL
        assert L.erp_warp_apply_device(h, p, io.GRAY8, 0, 40, 1, p, 10) == EINVAL
        assert L.erp_warp_kernel_ms(h, C.byref(C.c_double())) == EINVAL
    finally:
        L.erp_warp_destroy(h)
    rc, h = host_warp(vio, sW=41)
    assert rc == 0
    try:
        assert L.erp_warp_check(h, io.YUYV, 0, 82, 10) == EINVAL             # odd sW for 4:2:2
        assert L.erp_warp_check(h, io.UYVY, 0, 82, 10) == EINVAL
        assert L.erp_warp_check(h, io.BGR8, 0, 123, 10) == 0
    finally:
        L.erp_warp_destroy(h)


def test_quantize_rejects_bad_arguments(vio):
    L = vio.lib()
    s, q, v = np.zeros(4, np.float32), np.zeros(4, np.int32), np.zeros(4, np.uint8)
    p = [a.ctypes.data_as(C.c_void_p) for a in (s, q, v)]
    assert L.erp_warp_quantize(p[0], 4, 37, wo.X_WRAP, p[1], p[2]) == 0
    assert L.erp_warp_quantize(p[0], 4, 37, 3, p[1], p[2]) == EINVAL      # unknown border mode
    assert L.erp_warp_quantize(p[0], 4, 37, -1, p[1], p[2]) == EINVAL
    assert L.erp_warp_quantize(p[0], 4, 0, wo.X_WRAP, p[1], p[2]) == EINVAL
    assert L.erp_warp_quantize(p[0], -1, 37, wo.X_WRAP, p[1], p[2]) == EINVAL
    assert L.erp_warp_quantize(None, 4, 37, wo.X_WRAP, p[1], p[2]) == EINVAL
    assert L.erp_warp_quantize(None, 0, 37, wo.X_WRAP, None, None) == 0


def test_generators_reject_bad_arguments(vio):
    lenses, faces = wo.dual_fisheye(95.0), wo.cube_faces_3x2(16)
    with pytest.raises(vio.VioError):
        vio.warp_map_fisheye([], 48, 24)                       # n_lenses <= 0
    with pytest.raises(vio.VioError):
        vio.warp_map_fisheye([dict(lenses[0], f=0.0)], 48, 24)
    with pytest.raises(vio.VioError):
        vio.warp_map_fisheye(lenses, 0, 24)
    with pytest.raises(vio.VioError):
        vio.warp_map_cubemap([], 0, 48, 32, 48, 24)
    with pytest.raises(vio.VioError):
        vio.warp_map_cubemap(faces, 0, 47, 32, 48, 24)         # a face outside the source
    with pytest.raises(vio.VioError):
        vio.warp_map_cubemap(faces, 0, 48, 31, 48, 24)
    with pytest.raises(vio.VioError):
        vio.warp_map_cubemap(faces[:5] + [dict(faces[5], x0=-1)], 0, 48, 32, 48, 24)
    with pytest.raises(vio.VioError):
        vio.warp_map_cubemap(faces[:5] + [dict(faces[5], w=0)], 0, 48, 32, 48, 24)
    with pytest.raises(vio.VioError):
        vio.warp_map_erp(0, 24, 48, 24)
    L = vio.lib()
    m = np.zeros((24, 48), np.float32)
    p = m.ctypes.data_as(C.c_void_p)
    assert L.erp_warp_map_erp(48, 24, None, 48, -1, p, p) == EINVAL
    assert L.erp_warp_map_erp(48, 24, None, 48, 24, None, p) == EINVAL
    assert L.erp_warp_map_fisheye(None, 2, None, 48, 24, p, p) == EINVAL
    assert L.erp_warp_map_cubemap(None, 6, 0, 48, 32, None, 48, 24, p, p) == EINVAL


def test_lens_and_face_tables_match_the_header(vio, tmp_path):
    """abi.ErpFisheyeLens / ErpCubeFace are byte-identical to include/vio360.h's structs"""
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vio360.h")
    structs = {"erp_fisheye_lens": ("ErpFisheyeLens", ["R", "cx", "cy", "f", "theta_max"]),
               "erp_cube_face": ("ErpCubeFace", ["R", "x0", "y0", "w", "h"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){"]
    want = []
    for cs, (py, fields) in structs.items():
        cls = getattr(vio.abi, py)
        lines.append(f'printf("%zu\\n", sizeof({cs}));')
        want.append(C.sizeof(cls))
        for f in fields:
            lines.append(f'printf("%zu\\n", offsetof({cs}, {f}));')
            want.append(getattr(cls, f).offset)
    src = tmp_path / "warp_layout.c"
    src.write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "warp_layout"), str(src)])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "warp_layout")]).split()] == want
