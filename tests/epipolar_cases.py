"""TEST INFRASTRUCTURE: the shared cases of tests/test_epipolar.py and tests/test_epipolar_gpu.py."""
import functools
import importlib

import numpy as np

import epipolar_reference as ref

vio = importlib.import_module("360_visual_inertial_odometry_amd")

# the two-view scenes of the CPU checks (seeds for which the f64 reference alone leaves at most 2 % of the points
# inside its 1e-3 band, asserted in test_epipolar.py): name -> make_scene arguments
SCENES = {
    "translation": dict(seed=11, step=0.3, rot_deg=3.0),
    "pure_rotation": dict(seed=12, step=0.0, rot_deg=3.0),
    "mixed": dict(seed=13, step=0.6, rot_deg=10.0),
}


def params(**kw):
    p = vio.default_epi_params(vio.VIO_EPI_ON)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def scene(name):
    return ref.make_scene(**SCENES[name])


@functools.lru_cache(maxsize=None)
def samples(seed, n, iters):
    return vio.ransac_samples(seed, n, iters).reshape(-1, 3) if n >= 3 and iters > 0 else np.zeros((0, 3), np.int32)


def sized(n, W, H, seed):
    """n tracks of the translation geometry on a W x H frame (n = 0 .. 1000: the one-shot size sweep)"""
    s = ref.make_scene(seed=seed, n=max(n, 1), W=W, H=H, step=0.3, rot_deg=3.0, noise_px=0.2 * W / 960.0)
    return dict(s, p0=s["p0"][:n], p1=s["p1"][:n])


@functools.lru_cache(maxsize=None)
def translation_sequence(W, H, frames, step=0.05, yaw_px=0):
    """synth.erp_translation_sequence (a camera moving along its Y axis past near and far columns), kept per size"""
    synth = importlib.import_module("360_visual_inertial_odometry_amd.synth")
    return synth.erp_translation_sequence(W, H, frames, step, yaw_px)
