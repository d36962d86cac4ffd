"""The walk kernels' division-free lane geometry (CPU): the window descriptor carries LC = 256 // K, the
chunk and group counts and the multiply-shift reciprocals of K and LC (csrc/ba_types.h: ba_win_set_geometry,
walk_div); the kernels form tid // K and t // LC from them.  Checked here against integer division,
exhaustively: every K in 1..16, every thread index, every index of the 9 x LC landmark-sum jobs and of the
9 K / 27 K pose-partial loops.  The host hook (vio_ba_walk_geometry / vio_ba_walk_div) runs the packer's
own code; the device's multiply is the 24-bit one, equal on these arguments (both factors below 2^24)."""
import ctypes as C

import numpy as np
import pytest

BA_THREADS, BA_KMAX = 256, 16


@pytest.fixture(scope="module")
def geo(vio):
    lib = C.CDLL(vio.LIB_PATH)
    lib.vio_ba_walk_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    lib.vio_ba_walk_div.argtypes = [C.c_int, C.c_int]

    def geometry(K, L=0, gs=1):
        out = (C.c_int32 * 5)()
        assert lib.vio_ba_walk_geometry(K, L, gs, out) == 0
        return tuple(out)  # LC, nch, ng, rK, rLC
    return lib, geometry


def test_lane_geometry_every_k_every_thread(geo):
    lib, geometry = geo
    for K in range(1, BA_KMAX + 1):
        LC, _, _, rK, rLC = geometry(K)
        assert LC == BA_THREADS // K
        for tid in range(BA_THREADS):
            jf = lib.vio_ba_walk_div(tid, rK)
            assert (jf, tid - jf * K) == (tid // K, tid % K), (K, tid)
        # the landmark sums' 9 x LC jobs, strided over the workgroup: (entry, slot) = (t // LC, t % LC)
        for t in range(9 * LC):
            i = lib.vio_ba_walk_div(t, rLC)
            assert (i, t - i * LC) == (t // LC, t % LC), (K, t)


def test_pose_partial_loop_indices(geo):
    """the walks write a chunk's 27 K pose partials in three passes of 9 K jobs: job e of pass `part` is
    (keyframe, term) = (e // 9, e % 9), formed with the reciprocal of 9, and goes to slot 27 k + 9 part + i.
    Every index of the 9 K loop splits exactly, and the three passes cover the 27 K slots once each."""
    lib, geometry = geo
    r9 = geometry(9)[3]          # the packer's reciprocal of 9 (as of a window with K = 9): walk_recip(9)
    assert r9 == -(-(1 << 20) // 9)
    for K in range(1, BA_KMAX + 1):
        slots = []
        for part in range(3):
            for e in range(9 * K):
                k = lib.vio_ba_walk_div(e, r9)
                i = e - 9 * k
                assert (k, i) == (e // 9, e % 9), (K, e)
                slots.append(27 * k + 9 * part + i)
        assert sorted(slots) == list(range(27 * K)), K


def test_whole_argument_range_of_every_divisor(geo):
    """beyond the sites' ranges: every t the hook accepts (< 4096), every divisor a window can have"""
    lib, geometry = geo
    t = np.arange(4096, dtype=np.int64)
    for d in range(1, BA_THREADS + 1):
        r = -(-(1 << 20) // d)
        assert np.array_equal((t * r) >> 20, t // d), d
    for K in range(1, BA_KMAX + 1):   # the packer's reciprocals are those
        LC, _, _, rK, rLC = geometry(K)
        assert rK == -(-(1 << 20) // K) and rLC == -(-(1 << 20) // LC)
    assert lib.vio_ba_walk_div(4096, 1 << 20) < 0 and lib.vio_ba_walk_div(-1, 1) < 0  # out of range: refused


def test_chunk_and_group_counts(geo):
    _, geometry = geo
    assert geometry(0)[0] == BA_THREADS and geometry(0)[3] == 1 << 20   # no keyframes: as one
    for K in (1, 2, 3, 7, 10, 16):
        LC = BA_THREADS // K
        for L in (0, 1, LC - 1, LC, LC + 1, 2 * LC - 1, 2 * LC, 500, 5000):
            for gs in (1, 2, 5):
                g = geometry(K, L, gs)
                nch = -(-L // LC)
                assert g[:3] == (LC, nch, -(-nch // gs)), (K, L, gs)
