"""Small window-BA problems at the shapes where the phase route's Schur kernel can go wrong once a group's
landmark values and rhs column stay in LDS (tests/test_ba_schur_stage_gpu.py, tests/test_ba_schur_lds.py).
A chunk holds LC = 256 // K landmarks, a group `gs` chunks (VIO_BA_SCHUR_GS); T = ceil(6 (K - 1) / 16) tiles
(the first keyframe is constant).  `staged`: whether a launch of that shape alone takes the staged instance.

    name            K   L   T  gs  staged  what
    K10-L26-vi      10  26  4  1   yes     two groups, the second holds one landmark (a third of the
                                           observations missing, outliers)
    K10-L26-vi      10  26  4  2   yes     one group, its second chunk holds one landmark
    K10-L26-full    10  26  4  1,2 yes     the same shape visual-only, not thinned
    K10-L51-vi      10  51  4  2   yes     groups {0, 1} and {2}; constant landmarks at the first and last slots
                                           of a chunk and of a group (0, 24, 25, 49, 50); a third of the
                                           observations missing; gross-noise outliers
    K3-L86-vi       3   86  1  2   yes     T = 1, a second chunk of one landmark, constant landmarks 0 and 85
    K16-L17-local   16  17  6  2   no      T = 6 has no staged instance
    K4-L65-local    4   65  2  2   no      LC = 64: the 75 KB panel leaves no room for the staging at two
                                           workgroups per CU
    K10-L500-vi     10  500 4  20  no      a group of 20 chunks does not fit (at gs = 2 it would)

The last run pins the staged instance bitwise to the unstaged body: at gs = 20 K10-L51 and K10-L26 alone are
staged (their groups hold 3 and 2 chunks), in one batch with K10-L500 the launch of their tile count is not
(a launch is staged only where every window of the tile count fits), so the test's batch-against-solo
comparison sets the unstaged kernel's results against the staged kernel's.
"""
import walk_shape_cases as wsc

ITERS = 10  # fixed LM iterations, the timed mode


def tiles(K):
    return max(1, (6 * (K - 1) + 15) // 16)


def build(vio, synth):
    """[(name, window, variant, staged)]"""
    mk = synth.make_window
    k10 = mk(K=10, L=26, seed=41, imu=True, outlier_frac=0.05, all_visible=False)
    return [
        ("K10-L26-vi", wsc.thin(k10, 1.0 / 3.0, 4), vio.VIO_BA_VI, True),
        ("K10-L26-full", mk(K=10, L=26, seed=42, all_visible=False), vio.VIO_BA_FULL, True),
        ("K10-L51-vi", wsc.const_landmarks(wsc.thin(mk(K=10, L=51, seed=43, imu=True, outlier_frac=0.06,
                                                       all_visible=False), 1.0 / 3.0, 5), (0, 24, 25, 49, 50)),
         vio.VIO_BA_VI, True),
        ("K3-L86-vi", wsc.const_landmarks(mk(K=3, L=86, seed=44, imu=True, all_visible=False), (0, 85)),
         vio.VIO_BA_VI, True),
        ("K16-L17-local", wsc.thin(mk(K=16, L=17, seed=45, outlier_frac=0.05, all_visible=False), 1.0 / 3.0, 6),
         vio.VIO_BA_LOCAL, False),
        ("K4-L65-local", mk(K=4, L=65, seed=46, all_visible=False), vio.VIO_BA_LOCAL, False),
        ("K10-L500-vi", mk(K=10, L=500, seed=47, imu=True), vio.VIO_BA_VI, False),
    ]


# (group size, indices into build()'s list): the single shapes, then mixed batches of 8, 9 and 16 windows
RUNS = [
    (1, [0, 1]),
    (2, [0, 1]),
    (2, [2]),
    (2, [3]),
    (2, [4]),
    (2, [5]),
    (2, [0, 1, 2, 3, 4, 5, 2, 0]),
    (2, [2, 5, 4, 3, 1, 0, 3, 2, 5]),
    (2, [0, 1, 2, 3, 4, 5, 2, 3, 5, 4, 1, 0, 2, 2, 3, 0]),
    (20, [2, 6, 0]),
]
UNSTAGED_MIX = len(RUNS) - 1  # the run whose batch is unstaged while its small windows alone are staged


def problems(vio, cases):
    return [vio.BaProblem(w, variant=var, max_iterations=ITERS, fixed_iterations=1) for _, w, var, _ in cases]
