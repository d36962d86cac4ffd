"""CPU checks of the region masks: erp_mask_check's argument rules and closed-form pins of tests/mask_oracle.py,
the numpy restatement that the GPU is compared with (tests/test_mask_gpu.py)."""
import numpy as np
import pytest

import mask_oracle as mo
import resize_general_oracle as rgo
import warp_oracle as wo

BORDERS = (mo.X_CLAMP, mo.X_WRAP)


@pytest.mark.parametrize("args,radius,border,code", [
    (dict(sW=53, sH=37, dW=53, dH=37), 0, 0, 0),
    (dict(sW=3840, sH=1920, dW=960, dH=480), 255, 1, 0),
    (dict(sW=101, sH=67, dW=37, dH=23, stride=130, dst_stride=40), 5, 0, 0),
    (dict(sW=53, sH=37, dW=54, dH=37), 0, 0, -38),   # enlarging on x
    (dict(sW=53, sH=37, dW=53, dH=38), 0, 0, -38),   # enlarging on y
    (dict(sW=53, sH=37, dW=53, dH=37), 256, 0, -22),  # r outside [0, 255]
    (dict(sW=53, sH=37, dW=53, dH=37), -1, 0, -22),
    (dict(sW=53, sH=37, dW=53, dH=37), 1, 2, -22),   # unknown border_x
    (dict(sW=53, sH=37, dW=53, dH=37), 1, -1, -22),
    (dict(sW=53, sH=37, dW=53, dH=37, stride=52), 0, 0, -22),      # stride < width
    (dict(sW=53, sH=37, dW=20, dH=20, dst_stride=19), 0, 0, -22),
    (dict(sW=0, sH=37, dW=0, dH=37), 0, 0, -22),
    (dict(sW=53, sH=37, dW=53, dH=0), 0, 0, -22),
    (dict(sW=65536, sH=37, dW=53, dH=37), 0, 0, -22),
    (dict(sW=53, sH=37, dW=54, dH=37), 256, 0, -22),  # a bad argument wins over "not supported"
])
def test_mask_check(vio, args, radius, border, code):
    assert vio.mask_check(params=vio.mask_params(radius, border), **args) == code


def test_mask_check_null_params(vio):
    assert vio.mask_check(53, 37, 53, 37, None) == -22


def test_constants_match_the_oracle(vio):
    assert (vio.VIO_MASK_X_CLAMP, vio.VIO_MASK_X_WRAP) == (mo.X_CLAMP, mo.X_WRAP)


@pytest.mark.parametrize("border", BORDERS)
def test_all_usable_stays_all_usable(border):
    m = np.full((9, 21), 255, np.uint8)
    for r in (0, 1, 5, 8, 9, 20, 21, 40, 255):
        assert (mo.erode(m, r, border) == 255).all(), r


def square(W, H, x, y, r, border):
    out = np.full((H, W), 255, np.uint8)
    ys = [yy for yy in range(y - r, y + r + 1) if 0 <= yy < H]
    xs = range(x - r, x + r + 1)
    xs = [xx % W for xx in xs] if border == mo.X_WRAP else [xx for xx in xs if 0 <= xx < W]
    out[np.ix_(ys, xs)] = 0
    return out


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("x,y", [(0, 3), (36, 0), (18, 11), (36, 22), (0, 22), (5, 0)])
def test_single_pixel_becomes_a_square(border, x, y):
    """(2r+1)^2, clipped at top and bottom, clipped or wrapped in x (x = 0 and x = W - 1 included)"""
    W, H = 37, 23
    m = np.full((H, W), 255, np.uint8)
    m[y, x] = 0
    for r in (0, 1, 2, 5, 18, 19, 36, 40):
        np.testing.assert_array_equal(mo.erode(m, r, border), square(W, H, x, y, r, border), err_msg=str(r))
    if border == mo.X_WRAP and x in (0, W - 1):  # the square really crosses the seam
        e = mo.erode(m, 2, border)
        assert e[y, (x + 2) % W] == 0 and e[y, (x - 2) % W] == 0


@pytest.mark.parametrize("border", BORDERS)
def test_erosions_compose(border):
    rng = np.random.default_rng(3)
    m = np.where(rng.random((19, 45)) < 0.03, 0, 255).astype(np.uint8)
    for r1, r2 in [(1, 1), (2, 3), (0, 4), (7, 9), (30, 20)]:
        np.testing.assert_array_equal(mo.erode(mo.erode(m, r1, border), r2, border), mo.erode(m, r1 + r2, border))


def test_reduce_integer_factors_is_a_block_minimum():
    rng = np.random.default_rng(4)
    m = np.where(rng.random((2 * 11, 3 * 17)) < 0.1, 0, rng.integers(1, 256, (22, 51))).astype(np.uint8)
    want = (m.reshape(11, 2, 17, 3).min(axis=(1, 3)) != 0) * 255
    np.testing.assert_array_equal(mo.reduce(m, 17, 11), want.astype(np.uint8))


def test_reduce_identity():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 3, (9, 97)).astype(np.uint8)
    np.testing.assert_array_equal(mo.reduce(m, 97, 9), (m != 0) * np.uint8(255))


def test_reduce_single_pixel_hits_its_footprints():
    """101 -> 37: a single excluded source pixel excludes exactly the destination pixels whose table footprint
    holds it (one, or two where neighbouring cells share their edge pixel)"""
    S, D = 101, 37
    di, si, _ = rgo.area_tab(S, D)
    shared = 0
    for s in range(S):
        m = np.full((3, S), 255, np.uint8)
        m[1, s] = 0
        got = mo.reduce(m, D, 3)
        hit = np.unique(di[si == s])
        assert 1 <= len(hit) <= 2 and (len(hit) == 1 or hit[1] == hit[0] + 1)
        want = np.full((3, D), 255, np.uint8)
        want[1, hit] = 0
        np.testing.assert_array_equal(got, want)
        shared += len(hit) == 2
        # the same along y
        np.testing.assert_array_equal(mo.reduce(m.T.copy(), 3, D), want.T)
    assert shared > 0


def test_footprints_match_the_library_table(vio):
    """the reduce's footprints come from erp_resize_area_tab: the library's table is the oracle's"""
    for S, D in [(101, 37), (96, 32), (200, 65), (97, 97), (67, 23), (3840, 960)]:
        di, si, _ = vio.Context.resize_area_tab(S, D)
        odi, osi, _ = rgo.area_tab(S, D)
        assert np.array_equal(di, odi) and np.array_equal(si, osi)


def test_warp_usable_null_mask_is_the_border_free_region():
    """a fisheye map with theta_max short of the hemisphere, CONSTANT borders, no source mask: usable = the map
    entry is finite and no tap is outside the source = no border_value and no invalid pixel enters the output"""
    sW, sH, dW, dH = 64, 32, 64, 32
    mx, my = wo.map_fisheye(wo.dual_fisheye(80.0), dW, dH, wo.rot_y(0.1234) @ wo.rot_x(0.0567))
    mx, my = mx.astype(np.float32), my.astype(np.float32)
    got = mo.warp_usable(None, mx, my, sW, sH, wo.X_CONSTANT, wo.Y_CONSTANT) != 0
    qx, vx = wo.quantize(mx, sW, wo.X_CONSTANT)
    qy, vy = wo.quantize(my, sH, wo.Y_CONSTANT)
    ix, iy = qx >> 5, qy >> 5
    want = np.isfinite(mx) & np.isfinite(my) & (ix >= 0) & (ix + 1 < sW) & (iy >= 0) & (iy + 1 < sH)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(vx & vy, np.isfinite(mx) & np.isfinite(my))
    assert (~got).any() and got.any() and (~np.isfinite(mx)).any()
    # the same statement on pixels: two frames that differ only in border_value differ only on unusable pixels
    img = np.random.default_rng(6).integers(0, 256, (sH, sW)).astype(np.uint8)
    a = wo.remap_grey(img, mx, my, wo.X_CONSTANT, wo.Y_CONSTANT, 0)
    b = wo.remap_grey(img, mx, my, wo.X_CONSTANT, wo.Y_CONSTANT, 255)
    assert (a == b)[got].all()


def test_warp_usable_reads_the_mask_at_the_wrapped_and_clamped_taps():
    sW, sH = 8, 6
    mx = np.array([[7.5, 3.0, 3.0]], np.float32)   # taps 7 and 0 under wrap; 3 and 4; 3 and 4
    my = np.array([[2.0, 5.5, -0.5]], np.float32)  # rows 2, 3; 5, 5 (clamped); 0, 0 (clamped)
    for col, row, hit in [(0, 2, 0), (7, 3, 0), (4, 5, 1), (3, 0, 2)]:
        m = np.full((sH, sW), 255, np.uint8)
        m[row, col] = 0
        u = mo.warp_usable(m, mx, my, sW, sH, wo.X_WRAP, wo.Y_REPLICATE)[0] != 0
        assert not u[hit] and u.sum() == 2, (col, row, u)
    full = np.full((sH, sW), 255, np.uint8)
    assert (mo.warp_usable(full, mx, my, sW, sH, wo.X_WRAP, wo.Y_REPLICATE) == 255).all()
    # CONSTANT borders: the seam tap and the rows outside are not usable
    assert (mo.warp_usable(full, mx, my, sW, sH, wo.X_CONSTANT, wo.Y_CONSTANT)[0] == [0, 0, 0]).all()


def test_params_layout(vio, tmp_path):
    import ctypes as C
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vio360.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             'printf("%zu %zu %zu\\n", sizeof(erp_mask_params), offsetof(erp_mask_params, erode_radius), '
             'offsetof(erp_mask_params, border_x));',
             'printf("%d %d\\n", VIO_MASK_X_CLAMP, VIO_MASK_X_WRAP);']
    (tmp_path / "mk.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "mk"), str(tmp_path / "mk.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "mk")]).split()]
    cls = vio.abi.ErpMaskParams
    assert out[:3] == [C.sizeof(cls), cls.erode_radius.offset, cls.border_x.offset]
    assert out[3:] == [vio.VIO_MASK_X_CLAMP, vio.VIO_MASK_X_WRAP]


def test_no_device_fails_loudly(vio):
    """the device entry points need a context, a tracker or a front end: there is no CPU fallback"""
    import ctypes as C
    L, p = vio.lib(), vio.mask_params(1)
    a = np.full((8, 8), 255, np.uint8)
    ptr = a.ctypes.data_as(C.c_void_p)
    assert L.erp_mask_build(None, ptr, 8, 8, 8, 8, 8, C.byref(p), ptr, 8) == -22
    assert L.erp_mask_build_device(None, ptr, 8, 8, 8, 8, 8, C.byref(p), ptr, 8) == -22
    assert L.erp_mask_build_warped(None, ptr, 8, 8, 8, C.byref(p), ptr, 8) == -22
    assert L.erp_mask_kernel_ms(None, None) == -22
    for fn in (L.erp_tracker_set_mask, L.erp_tracker_set_mask_device, L.erp_frontend_set_mask,
               L.erp_frontend_set_mask_device):
        assert fn(None, ptr, 8, 8, 8, C.byref(p)) == -22
    assert L.erp_tracker_set_mask_warped(None, None, ptr, 8, C.byref(p)) == -22
    assert L.erp_frontend_set_mask_warped(None, None, ptr, 8, C.byref(p)) == -22
    assert L.erp_tracker_get_mask(None, ptr, 8) == -22


def test_kernels_have_no_scratch(vio):
    """the kernels of csrc/mask.hip keep everything in registers and LDS (code-object metadata, as tools/kd_info.py
    prints it); only the row erosion uses LDS: its two extended rows"""
    import test_build as tb
    blob = open(vio.lib()._name, "rb").read()
    found = {kd[".name"]: kd for co in tb._gfx950_code_objects(blob) for kd in tb._kernel_descriptors(co)
             if "mask_" in kd[".name"] and "vio360" in kd[".name"] and "disc_mask" not in kd[".name"]}
    names = " ".join(sorted(found))
    for k in ("mask_reduce_kernel", "mask_warp_kernel", "mask_erode_h_kernel", "mask_erode_v_kernel",
              "mask_unpack_kernel", "mask_gather_kernel"):
        assert k in names, (k, names)
    assert len(found) == 7, names  # the reduce is instantiated for bytes and for bits
    for name, kd in found.items():
        assert kd[".private_segment_fixed_size"] == 0, (name, kd[".private_segment_fixed_size"])
        lds = kd[".group_segment_fixed_size"]
        assert lds <= 17 * 1024 if "erode_h" in name else lds == 0, (name, lds)
