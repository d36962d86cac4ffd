"""Every instance of the tracker's two table-dispatched kernels, each against the oracle on inputs where a launch of
any other instance gives another answer: lk_kernel [seam wrap][guided][round-trip check] and gftt_select_kernel
[grid in global memory][cell chains][seam wrap].  A table entry wired to the wrong index would otherwise pass wherever
the suite happens not to reach that instance at a size where it matters.

The references are the ones the other tracker tests use: tests/klt_guess_oracle.py and tests/klt_fb_oracle.py for LK,
oracle_lib (flat) and tests/seam_oracle.py (wrapped) for detection.  Everything is bitwise."""
import itertools

import numpy as np
import pytest

import klt_fb_oracle as fbo
import klt_guess_oracle as ko
import oracle_lib
import seam_cases as sc
import seam_oracle as so

gpu = pytest.mark.gpu  # (the two tests of the cases themselves need none)

# ---- lk_kernel: a 96 x 64 pair, max_level 2 (the size check stops at level 1, 48 wide: wide enough for WRAP)
LK_W, LK_H = 96, 64
LK_FLOW = sc.FLOWS[2]


def lk_inputs(vio):
    prev, curr = sc.pair(LK_W, LK_H, LK_FLOW)
    c = sc.corners(LK_W, LK_H)
    pts = np.ascontiguousarray(c[::max(1, -(-len(c) // 40))])  # about 40, evenly spaced, the seam bands included
    klt = vio.default_klt_params()
    klt.max_level = 2
    # guesses: the flow for two points of three, a start 10 px off for the third (it ends elsewhere or is lost)
    guess = pts + np.float32(LK_FLOW)
    guess[::3] += np.float32([9, -5])
    return prev, curr, pts, klt, guess


def lk_reference(prev, curr, pts, klt, guess, mode, fb):
    """-> (next, status, err) or, with the check, (next, status, err, back, fb_state, fb_d2)"""
    if fb:
        return fbo.fb_track(prev, curr, pts, klt, guess, mode, 0.5)
    return ko.klt_track(prev, curr, pts, klt, guess, mode)[:3]


@pytest.fixture(scope="module")
def lk_refs(vio):
    prev, curr, pts, klt, guess = lk_inputs(vio)
    return {(mode, guided, fb): lk_reference(prev, curr, pts, klt, guess if guided else None, mode, fb)
            for mode, guided, fb in itertools.product((ko.CUT, ko.WRAP), (False, True), (False, True))}


def test_lk_cases_tell_the_instances_apart(vio, lk_refs):
    """the references themselves (no GPU work): flipping seam or guided changes next / status, and the check runs its
    backward search, so no other instance's outputs pass for an instance"""
    assert 30 <= len(lk_refs[(ko.CUT, False, False)][0]) <= 45
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for guided, fb in itertools.product((False, True), (False, True)):
        assert not same(lk_refs[(ko.CUT, guided, fb)], lk_refs[(ko.WRAP, guided, fb)]), (guided, fb)
    for mode, fb in itertools.product((ko.CUT, ko.WRAP), (False, True)):
        assert not same(lk_refs[(mode, False, fb)], lk_refs[(mode, True, fb)]), (mode, fb)
    for mode, guided in itertools.product((ko.CUT, ko.WRAP), (False, True)):
        o = lk_refs[(mode, guided, True)]
        assert (o[4] == fbo.PASS).sum() >= 10 and o[3].any(), (mode, guided)
    o = lk_refs[(ko.CUT, False, False)]
    prev, curr, pts, klt, _ = lk_inputs(vio)
    for a, b in zip(o, oracle_lib.klt_track(prev, curr, pts, klt)):  # the restatement is the C oracle here too
        assert np.array_equal(a, b)


@gpu
@pytest.mark.parametrize("fb", (False, True))
@pytest.mark.parametrize("guided", (False, True))
@pytest.mark.parametrize("mode", (ko.CUT, ko.WRAP))
def test_lk_instance_bitwise(vio, gpu_ctx, lk_refs, mode, guided, fb):
    prev, curr, pts, klt, guess = lk_inputs(vio)
    o = lk_refs[(mode, guided, fb)]
    g = gpu_ctx.klt_track(prev, curr, pts, klt, seam=mode, guess=guess if guided else None,
                          fb=vio.default_fb_params(0.5) if fb else None)
    assert len(g) == len(o)
    assert np.array_equal(g[1], o[1]) and np.array_equal(g[0], o[0])
    assert np.array_equal(g[2][o[1] == 1], o[2][o[1] == 1])
    if fb:
        assert np.array_equal(g[4], o[4])
        ran = (o[4] == fbo.PASS) | (o[4] == fbo.TOO_FAR)
        assert np.array_equal(g[3][ran], o[3][ran]) and np.array_equal(g[5][ran], o[5][ran])


# ---- gftt_select_kernel.  With c = round(min_dist) and n = ceil(W / c) * ceil(H / c) cells, the launcher keeps the
# 12 n bytes of the grid in LDS while they fit 136 KB (n <= 11605), and chains the survivors per cell while the 4 n
# bytes of chain heads fit beside it (n <= 8704 in LDS, n <= 34816 with the grid in global memory).
GF_LDS = 136 * 1024
GF_CUT = [(96, 64, 6.0), (384, 240, 3.4), (480, 288, 3.4), (768, 432, 3.4)]
GF_WRAP = [(96, 64, 6.0), (128, 80, 1.4), (160, 96, 1.4), (256, 144, 1.4)]


def select_instance(W, H, min_dist):
    """(grid in global memory, cell chains) as launch_select decides them"""
    c = int(round(min_dist))
    n = -(-W // c) * -(-H // c)
    in_global = 12 * n > GF_LDS
    return in_global, (4 * n if in_global else 16 * n) <= GF_LDS


def test_gftt_cases_reach_every_select_instance():
    for cases in (GF_CUT, GF_WRAP):
        assert [select_instance(*c) for c in cases] == [(False, True), (False, False), (True, True), (True, False)]


@gpu
@pytest.mark.parametrize("W,H,md", GF_CUT)
def test_select_instance_cut_bitwise(vio, gpu_ctx, synth, W, H, md):
    """two equal blobs on flat patches give corners at x = 1 and x = W - 2 of one row: 3 px apart round the cylinder,
    under min_dist, so the flat pass keeps both and a wrapped one could not"""
    img = synth.render_erp(W, H).copy()
    r = H // 2
    img[r - 5:r + 7, :8] = img[r - 5:r + 7, W - 8:] = 60
    img[r:r + 2, 1] = img[r:r + 2, W - 2] = 255
    want = oracle_lib.gftt(img, None, 0, sc.Q, md)
    row = want[want[:, 1] == r + 1]
    assert md > 3 and (row[:, 0] == 1).any() and (row[:, 0] == W - 2).any()
    for seam in (None, vio.VIO_SEAM_CUT):
        got = gpu_ctx.gftt(img, None, 0, sc.Q, md, seam=seam)
        assert np.array_equal(got, want), (len(got), len(want))


@gpu
@pytest.mark.parametrize("W,H,md", GF_WRAP)
def test_select_instance_wrap_bitwise(vio, gpu_ctx, synth, W, H, md):
    """a blob across the seam gives tied candidates at x = W - 1 and x = 0: the reference rejects one of them by the
    wrapped distance alone (a flat pass would keep it)"""
    img = synth.render_erp(W, H).copy()
    r = H // 2
    img[r - 5:r + 7, :6] = img[r - 5:r + 7, W - 6:] = 60
    img[r:r + 2, 0] = img[r:r + 2, W - 1] = 255
    want, _, seam_only = so.gftt_stats(img, None, 0, sc.Q, md)
    assert seam_only >= 1
    got = gpu_ctx.gftt(img, None, 0, sc.Q, md, seam=vio.VIO_SEAM_WRAP)
    assert np.array_equal(got, want), (len(got), len(want))
