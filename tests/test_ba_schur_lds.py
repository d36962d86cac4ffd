"""The phase route's Schur kernel: which shapes take the staged instance (a group's landmark values and rhs
column kept in LDS) and what LDS a launch asks for (CPU).  The staged instance is chosen only where two
workgroups per CU still fit the CU's 160 KB of LDS -- with one, a CU's matrix cores idle through every panel
fill -- and every other shape keeps the unstaged kernel.  The host hook (vio_ba_schur_lds) runs the launcher's
own sizing code; the register and private-segment figures come from the library's code-object metadata."""
import ctypes as C

import pytest

import schur_stage_cases as ssc
import test_build as tb

LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def lds(vio):
    lib = C.CDLL(vio.LIB_PATH)
    lib.vio_ba_schur_lds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]

    def info(K, L, T, gs):
        out = (C.c_int32 * 3)()
        assert lib.vio_ba_schur_lds(K, L, T, gs, out) == 0
        return out[0], out[1], bool(out[2])  # dynamic bytes, static bytes, staged
    return info


def panel_doubles(K, T):
    LC = 256 // K
    kc = (3 * LC + 3) & ~3
    ks = 16 * T if T & 1 else 16 * T + 16
    return kc * ks + kc, kc, LC


def test_config3_groups_are_staged_at_two_workgroups_per_cu(lds):
    for gs in (10, 5, 3):
        dyn, static, staged = lds(10, 500, 4, gs)
        pd, kc, LC = panel_doubles(10, 4)
        assert staged, gs
        assert dyn == 8 * (pd - kc + gs * kc + 9 * gs * LC), (gs, dyn)   # panel | rhs columns | landmark values
        assert 2 * (static + dyn) <= LDS_CU, (gs, static, dyn)
    assert lds(10, 500, 4, 10)[:2] == (72720, 5184)


def test_every_staged_shape_fits_twice_and_no_other_is_staged(lds):
    """over every K, tile count and group size a window can have: staged means T <= 5 and two workgroups'
    static + dynamic LDS within the CU's; an unstaged launch asks for exactly the panel or combine area"""
    for K in range(1, 17):
        pdT = {T: panel_doubles(K, T) for T in range(1, 7)}
        for T in range(1, 7):
            pd, kc, LC = pdT[T]
            comb = T * (T + 1) // 2 * 256 + 16 * T
            for gs in (1, 2, 3, 5, 10, 40):
                for L in (1, LC, LC + 1, 20 * LC):
                    dyn, static, staged = lds(K, L, T, gs)
                    gsc = min(gs, -(-L // LC))
                    if staged:
                        assert T <= 5 and 2 * (static + dyn) <= LDS_CU, (K, T, gs, L, dyn)
                        assert dyn == 8 * max(pd - kc + gsc * kc + 9 * gsc * LC, 2 * comb), (K, T, gs, L, dyn)
                    else:
                        assert dyn == 8 * max(pd, comb), (K, T, gs, L, dyn)
                        need = static + 8 * max(pd - kc + gsc * kc + 9 * gsc * LC, 2 * comb)
                        assert T == 6 or 2 * need > LDS_CU - 2 * 2048, (K, T, gs, L, need)  # (sized in 2 KB units)


def test_gpu_cases_take_the_path_their_name_says(vio, synth, lds):
    cases = ssc.build(vio, synth)
    for gs, idx in ssc.RUNS[:6]:
        for i in idx:
            name, w, _, staged = cases[i]
            K, L = len(w["kf_const"]), len(w["lm_const"])
            assert lds(K, L, ssc.tiles(K), gs)[2] == staged, (name, gs)
    assert {staged for _, _, _, staged in cases} == {True, False}
    # the run that sets the unstaged kernel against the staged one: alone at its group size the small windows are
    # staged, the large one (hence a batch holding it, for the whole tile count) is not
    gs, idx = ssc.RUNS[ssc.UNSTAGED_MIX]
    shapes = {cases[i][0]: (len(cases[i][1]["kf_const"]), len(cases[i][1]["lm_const"])) for i in idx}
    assert {ssc.tiles(K) for K, _ in shapes.values()} == {4}
    assert sorted((n, lds(K, L, 4, gs)[2]) for n, (K, L) in shapes.items()) == \
        [("K10-L26-vi", True), ("K10-L500-vi", False), ("K10-L51-vi", True)]


def test_schur_kernels_registers_and_private_segment(vio):
    """staged and unstaged instances of tile counts 1..5 touch no scratch, and the 4-tile staged instance (the
    256-window workload's) stays within the 226 VGPRs of the unstaged one"""
    blob = open(vio.lib()._name, "rb").read()
    found = {}
    for co in tb._gfx950_code_objects(blob):
        for kd in tb._kernel_descriptors(co):
            if "ph_schur_kernelILi" in kd[".name"]:
                t = int(kd[".name"].split("ph_schur_kernelILi")[1][0])
                st = "Lb1E" in kd[".name"]
                found[t, st] = kd
    assert set(found) == {(t, st) for t in range(1, 6) for st in (False, True)} | {(6, False)}, sorted(found)
    for (t, st), kd in found.items():
        if t <= 5:
            assert kd[".private_segment_fixed_size"] == 0, (t, st, kd[".private_segment_fixed_size"])
    assert found[4, True][".vgpr_count"] <= 226, found[4, True][".vgpr_count"]
    assert found[4, False][".vgpr_count"] <= 226, found[4, False][".vgpr_count"]
