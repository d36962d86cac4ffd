"""CPU checks of the contrast equalisation (erp_equalize*, include/vio360.h): the host LUT rule erp_equalize_lut
against tests/equalize_oracle.py (bitwise), the argument check, the struct mirror, and closed forms that keep the
oracle itself honest (OpenCV is not available here: parity with it is unpinned)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import equalize_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vio360.h")
AREAS = (32, 72, 7200, 115200)
CLIPS = (0, 0.01, 2, 3, 40)
EINVAL = -22


def levels(area, first, k):
    """a histogram of `area` pixels over the k levels first .. first + k - 1, as evenly as they go"""
    h = np.zeros(256, np.int64)
    h[first:first + k] = area // k
    h[first:first + area % k] += 1
    assert h.sum() == area and np.count_nonzero(h) == min(k, area)
    return h


def histograms(area):
    """name -> 256 counts that sum to area"""
    rng = np.random.default_rng(area)
    out = {"random": eo.histogram(rng.integers(0, 256, area, dtype=np.uint8)),
           "skewed": eo.histogram(np.clip(rng.normal(90, 9, area), 0, 255).astype(np.uint8)),
           "constant": levels(area, 137, 1),
           "two-valued": levels(area, 20, 1) // 3 + np.roll(levels(area - area // 3, 20, 1), 180),
           "narrow 100..110": levels(area, 100, 11),
           "every level": levels(area, 0, 256)}
    for k in (31, 32, 33):  # with c = 1 the excess is area - k: area 7200 gives resid 1, 0 and 255
        out[f"{k} levels"] = levels(area, 60, k)
    for h in out.values():
        assert h.sum() == area
    return out


def test_clahe_lut_matches_the_oracle(vio):
    resid_seen = set()
    n = 0
    for area in AREAS:
        for name, h in histograms(area).items():
            for clip in CLIPS:
                clipped, info = eo.clahe_clip(h, area, clip)
                assert clipped.sum() == area, (area, name, clip)  # the clip moves counts, it loses none
                if clip > 0:
                    assert clipped.max() <= info["c"] + info["batch"] + 1
                    resid_seen.add(info["resid"])
                want = eo.clahe_lut(h, area, clip)
                assert np.all(np.diff(want.astype(int)) >= 0), (area, name, clip)
                assert want[-1] == 255
                got = vio.equalize_lut(vio.VIO_EQ_CLAHE, h, area, clip)
                np.testing.assert_array_equal(got, want, err_msg=f"area {area} {name} clip {clip}")
                n += 1
    assert {0, 1, 61, 255} <= resid_seen, sorted(resid_seen)
    assert n == len(AREAS) * 9 * len(CLIPS)


def test_the_issue_example_reaches_the_residual_loop():
    """a 12 x 6 tile of values 100..110 at any clip limit <= 3: c = 1, excess = resid = 61"""
    h = eo.histogram(np.arange(72) % 11 + 100)
    for clip in (0.01, 2, 3):
        clipped, info = eo.clahe_clip(h, 72, clip)
        assert (info["c"], info["excess"], info["batch"], info["resid"]) == (1, 61, 0, 61)
        # step = 4: bins 0, 4, ..., 240 take the 61 residual counts
        want = np.zeros(256, np.int64)
        want[100:111] = 1
        want[0:244:4] += 1
        np.testing.assert_array_equal(clipped, want)


def test_hist_lut_matches_the_oracle(vio):
    for area in AREAS:
        for name, h in histograms(area).items():
            want = eo.hist_lut(h, area)
            assert np.all(np.diff(want.astype(int)) >= 0) or name == "constant", (area, name)
            got = vio.equalize_lut(vio.VIO_EQ_HIST, h, area)
            np.testing.assert_array_equal(got, want, err_msg=f"area {area} {name}")
    # the single-bin frame: every pixel keeps its value
    np.testing.assert_array_equal(vio.equalize_lut(vio.VIO_EQ_HIST, levels(7200, 137, 1), 7200), np.full(256, 137))
    # every level equally often (n each): lut[i] = round(i n * (255 / (255 n))) = i
    for n in (1, 7, 450):
        np.testing.assert_array_equal(vio.equalize_lut(vio.VIO_EQ_HIST, np.full(256, n), 256 * n), np.arange(256))


def test_lut_rejects_bad_arguments(vio):
    lib = vio.lib()
    h = np.ones(256, np.uint32)
    lut = np.zeros(256, np.uint8)
    hp, lp = h.ctypes.data_as(C.c_void_p), lut.ctypes.data_as(C.c_void_p)
    assert lib.erp_equalize_lut(vio.VIO_EQ_CLAHE, hp, 256, 3.0, lp) == 0
    assert lib.erp_equalize_lut(vio.VIO_EQ_NONE, hp, 256, 3.0, lp) == EINVAL
    assert lib.erp_equalize_lut(7, hp, 256, 3.0, lp) == EINVAL
    assert lib.erp_equalize_lut(vio.VIO_EQ_CLAHE, None, 256, 3.0, lp) == EINVAL
    assert lib.erp_equalize_lut(vio.VIO_EQ_CLAHE, hp, 256, 3.0, None) == EINVAL
    assert lib.erp_equalize_lut(vio.VIO_EQ_CLAHE, hp, 0, 3.0, lp) == EINVAL
    assert lib.erp_equalize_lut(vio.VIO_EQ_CLAHE, hp, 256, -1.0, lp) == EINVAL
    assert lib.erp_equalize_lut(vio.VIO_EQ_CLAHE, hp, 256, float("nan"), lp) == EINVAL


def test_check(vio):
    P = vio.equalize_params
    ok = [(P(), 960, 480), (P(), 16, 16), (P(tiles_x=4, tiles_y=3), 37, 23), (P(clip_limit=0), 64, 32),
          (P(border_x=vio.VIO_EQ_X_WRAP), 64, 32), (P(vio.VIO_EQ_HIST), 2, 2), (P(vio.VIO_EQ_NONE), 2, 2),
          (P(vio.VIO_EQ_HIST, tiles_x=0, clip_limit=-1), 5, 7),  # HIST reads neither
          (P(tiles_x=1, tiles_y=1), 2, 2), (P(), 32768, 32768)]
    for p, W, H in ok:
        assert vio.equalize_check(p, W, H) == 0, (p.mode, W, H)
    assert vio.equalize_check(P(), 64, 32, 64 + 5, 64 + 9) == 0
    bad = [(P(mode=3), 64, 32), (P(mode=-1), 64, 32),
           (P(tiles_x=0), 64, 32), (P(tiles_y=0), 64, 32), (P(tiles_x=-8), 64, 32),
           (P(tiles_x=33), 64, 32), (P(tiles_y=17), 64, 32), (P(tiles_x=2, tiles_y=1), 3, 2),
           (P(clip_limit=-0.5), 64, 32), (P(clip_limit=float("nan")), 64, 32), (P(clip_limit=float("inf")), 64, 32),
           (P(border_x=vio.VIO_EQ_X_WRAP), 65, 32), (P(border_x=vio.VIO_EQ_X_WRAP), 64, 33), (P(border_x=2), 64, 32),
           (P(vio.VIO_EQ_HIST), 1, 8), (P(vio.VIO_EQ_HIST), 8, 1), (P(vio.VIO_EQ_HIST), 32768, 32769)]
    for p, W, H in bad:
        assert vio.equalize_check(p, W, H) == EINVAL, (p.mode, p.tiles_x, p.tiles_y, p.clip_limit, p.border_x, W, H)
    assert vio.equalize_check(P(), 64, 32, 63, 64) == EINVAL  # stride < W
    assert vio.equalize_check(P(), 64, 32, 64, 63) == EINVAL
    assert vio.lib().erp_equalize_check(None, 64, 32, 64, 64) == EINVAL


def test_params_layout(vio, tmp_path):
    fields = ["mode", "tiles_x", "tiles_y", "border_x", "clip_limit"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("%zu\\n", sizeof(erp_equalize_params));']
    lines += [f'printf("%zu\\n", offsetof(erp_equalize_params, {f}));' for f in fields]
    lines += ['printf("%d %d %d %d %d\\n", VIO_EQ_NONE, VIO_EQ_HIST, VIO_EQ_CLAHE, VIO_EQ_X_CLAMP, VIO_EQ_X_WRAP);']
    (tmp_path / "eq.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "eq"), str(tmp_path / "eq.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "eq")]).split()]
    cls = vio.abi.ErpEqualizeParams
    assert out[0] == C.sizeof(cls)
    assert out[1:6] == [getattr(cls, f).offset for f in fields]
    assert out[6:] == [vio.VIO_EQ_NONE, vio.VIO_EQ_HIST, vio.VIO_EQ_CLAHE, vio.VIO_EQ_X_CLAMP, vio.VIO_EQ_X_WRAP]
    assert out[6:] == [eo.NONE, eo.HIST, eo.CLAHE, eo.X_CLAMP, eo.X_WRAP]


def test_no_device_fails_loudly(vio):
    """the device entry points need a context: there is no CPU fallback"""
    p = vio.equalize_params()
    a = np.zeros((8, 8), np.uint8)
    ptr = a.ctypes.data_as(C.c_void_p)
    assert vio.lib().erp_equalize(None, ptr, 8, 8, 8, C.byref(p), ptr, 8) == EINVAL
    assert vio.lib().erp_equalize_device(None, ptr, 8, 8, 8, 1, C.byref(p), ptr, 8) == EINVAL
    assert vio.lib().erp_tracker_equalize(None, 1, C.byref(p)) == EINVAL
    assert vio.lib().erp_frontend_set_equalize(None, C.byref(p)) == EINVAL


def test_kernels_have_no_scratch(vio):
    """the four kernels of csrc/equalize.hip keep everything in registers and LDS (code-object metadata, as
    tools/kd_info.py prints it), none with more than 20 KB of LDS (eight workgroups per CU)"""
    import test_build as tb
    blob = open(vio.lib()._name, "rb").read()
    found = {kd[".name"]: kd for co in tb._gfx950_code_objects(blob) for kd in tb._kernel_descriptors(co)
             if any(k in kd[".name"] for k in ("eq_hist_kernel", "eq_lut_kernel", "eq_apply_kernel"))}
    assert len(found) == 4, sorted(found)
    for name, kd in found.items():
        assert kd[".private_segment_fixed_size"] == 0, (name, kd[".private_segment_fixed_size"])
        assert kd[".group_segment_fixed_size"] <= 20 * 1024, (name, kd[".group_segment_fixed_size"])


# ---- closed forms of the oracle (no library) ----

def images(W, H):
    rng = np.random.default_rng(W * 1000 + H)
    return {"noise": rng.integers(0, 256, (H, W), dtype=np.uint8),
            "narrow": rng.integers(100, 111, (H, W), dtype=np.uint8),
            "ramp": np.broadcast_to((np.arange(W) * 255 // (W - 1)).astype(np.uint8), (H, W)).copy()}


@pytest.mark.parametrize("W,H", [(2, 2), (37, 23), (64, 32), (333, 7), (960, 480)])
def test_oracle_one_tile_without_clip_is_the_plain_lut(W, H):
    """tiles 1 x 1, clip 0: the four interpolated LUTs are one, the weights sum to 1 exactly, and the result is
    lut[src] with lut = round(cumsum * (255 / area))"""
    for name, img in images(W, H).items():
        cs = np.cumsum(np.bincount(img.reshape(-1), minlength=256))
        lut = np.clip(np.rint(cs.astype(np.float32) * (np.float32(255) / np.float32(W * H))), 0, 255).astype(np.uint8)
        np.testing.assert_array_equal(eo.clahe(img, 1, 1, 0), lut[img], err_msg=name)


def test_oracle_hist_of_every_level_equally_often():
    img = np.random.default_rng(3).permutation(np.repeat(np.arange(256), 12)).astype(np.uint8).reshape(48, 64)
    np.testing.assert_array_equal(eo.equalize_hist(img), img)
    np.testing.assert_array_equal(eo.equalize_hist(np.full((5, 9), 77, np.uint8)), np.full((5, 9), 77))
    # two values: the lower one maps to 0, the upper one to 255
    two = np.where(np.arange(40).reshape(5, 8) % 3 == 0, 60, 200).astype(np.uint8)
    np.testing.assert_array_equal(eo.equalize_hist(two), np.where(two == 60, 0, 255))


@pytest.mark.parametrize("W,H,tx,ty", [(64, 32, 8, 8), (128, 48, 8, 8), (96, 48, 8, 8), (120, 40, 6, 4)])
def test_oracle_wrap_commutes_with_a_roll_by_whole_tiles(W, H, tx, ty):
    """X_WRAP has no horizontal border: rolling the frame by a whole tile rolls the result.  Bitwise where the tile
    width is a power of two: then 1.f / tw and x * (1.f / tw) are exact, so pixel x and pixel x + k tw get the same
    weights.  At other widths the rule's own float32 rounding of x * (1.f / tw) differs between the two pixels by a
    few ulp, i.e. res by less than 255 * 2^-20: the rounded bytes then differ by at most 1, and only where res lies
    that close to a half."""
    img = images(W, H)["noise"]
    tw = W // tx
    ref = eo.clahe(img, tx, ty, 3.0, eo.X_WRAP)
    for k in (1, 3, tx - 1):
        rolled = eo.clahe(np.roll(img, k * tw, axis=1), tx, ty, 3.0, eo.X_WRAP)
        if tw & (tw - 1) == 0:
            np.testing.assert_array_equal(rolled, np.roll(ref, k * tw, axis=1))
        else:
            diff = np.abs(rolled.astype(int) - np.roll(ref, k * tw, axis=1))
            assert diff.max() <= 1 and np.count_nonzero(diff) <= diff.size // 100
    clamp = eo.clahe(img, tx, ty, 3.0, eo.X_CLAMP)
    assert np.any(clamp[:, 0] != ref[:, 0]) and np.any(clamp[:, -1] != ref[:, -1])
    np.testing.assert_array_equal(clamp[:, tw // 2 + 1:W - tw // 2 - 1], ref[:, tw // 2 + 1:W - tw // 2 - 1])


def test_oracle_extension_is_reflect_101():
    img = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    e = eo.extended(img, 3, 2)  # 7 -> 9 columns (2 more), 5 -> 6 rows (1 more)
    assert e.shape == (6, 9)
    np.testing.assert_array_equal(e[:5, :7], img)
    np.testing.assert_array_equal(e[:5, 7], img[:, 5])
    np.testing.assert_array_equal(e[:5, 8], img[:, 4])
    np.testing.assert_array_equal(e[5, :7], img[3])
    # a divisible axis grows by a whole tiles count as soon as the other is not divisible
    assert eo.extended(np.zeros((23, 40), np.uint8), 4, 3).shape == (24, 44)
    assert eo.extended(np.zeros((24, 40), np.uint8), 4, 3).shape == (24, 40)
