"""The scenes of tests/test_gpu_secondary_chain.py (device against oracle) and tests/test_secondary_chain_reference.py
(their oracle side, no GPU): the smallest trees and active lists at which the secondary rays' start entries, the
climb that reads its parent one level ahead and the list phase can go wrong.

Every case is rendered at 16 x 16 with its one light and 3 environment samples, step 0.01, t_eps 0. A case is
(arrays, camera, pixels): arrays as records_compare's scene builders return them (mean, cov6, density, albedo,
light positions, light intensities), camera (position, view direction, fov).
"""
import functools

import numpy as np

import pyoracle as O
import records_compare as RC
import tree_reference as T
from helpers import CAM_POS, FOV, main_view_dir

W = 16
ENV_SAMPLES = 3
LIGHT = RC.NESTED_LIGHT
MAIN_CAMERA = (CAM_POS, main_view_dir(), FOV)
# The chain scene: its cluster (257 Gaussians, 3 sigma = 0.047) sits at the origin, the chain runs out along the
# three axes. The camera's rays start on its 2 x 2 sensor plane and meet in its pinhole (camera.h), which is put
# just behind the cluster: they run down the z axis through the chain's Gaussians on it and cross the cluster
# 0.0125 apart. The light lies on the y axis, behind the chain's Gaussians there.
CHAIN_CAMERA = (np.float32([0.0, 0.0, 0.9]), np.float32([0.0, 0.0, -1.0]), np.float32(0.5 * np.pi))
CHAIN_LIGHT = ([0.0, 3.0, 0.0], [1.0, 1.0, 1.0])
CHAIN_PIXELS = [(8, 8), (7, 8), (8, 6), (6, 7), (9, 9), (5, 8)]


def _isotropic(mean, sigma, density, light=LIGHT):
    mean = np.asarray(mean, np.float32).reshape(-1, 3)
    sig = np.broadcast_to(np.asarray(sigma, np.float64), (len(mean),))
    cov = np.stack([sig ** 2, 0 * sig, 0 * sig, sig ** 2, 0 * sig, sig ** 2], 1).astype(np.float32)
    dens = np.full(len(mean), density, np.float32)
    return mean, cov, dens, np.full(len(mean), 0.5, np.float32), np.float32([light[0]]), np.float32([light[1]])


def scattered_gaussians(n, density, seed):
    """n isotropic Gaussians (sigma 0.2 .. 0.35) scattered over a box of half extent 0.7 around (0, 1, 0)."""
    rng = np.random.default_rng(seed)
    mean = np.float32([0.0, 1.0, 0.0]) + rng.uniform(-0.7, 0.7, (n, 3))
    return _isotropic(mean, rng.uniform(0.2, 0.35, n), density)


@functools.lru_cache(maxsize=None)
def chain_levels():
    """Levels of the chain scene's radix tree: the deepest the device builder keeps (kMaxDepth + 1), twice the 14
    entries of the persistent kernel's LDS traversal stack."""
    return T.limits()["max_depth"] + 1


def chain_gaussians(density):
    rows = T.chain_gaussians(T.chain_k_for(chain_levels(), T.limits()["leaf_max"]))
    n = len(rows)
    return (rows[:, 0:3].copy(), rows[:, 3:9].copy(), np.full(n, density, np.float32), np.full(n, 0.5, np.float32),
            np.float32([CHAIN_LIGHT[0]]), np.float32([CHAIN_LIGHT[1]]))


# name: (arrays, camera, pixels). Densities: chosen with the oracle alone so that a quarter of the rays and more have
# a Tr in [0.05, 0.95] (test_secondary_chain_reference.py asserts the shares).
CASES = {
    # a single 4-wide node: the start entry is the root (up = -1, no climb); one member: no second index
    "single-1": lambda: (_isotropic([[0.0, 1.0, 0.0]], 0.35, 0.5), MAIN_CAMERA, RC.NESTED_PIXELS),
    "single-2": lambda: (_isotropic([[-0.2, 1.0, 0.0], [0.25, 1.1, 0.1]], [0.3, 0.35], 0.3), MAIN_CAMERA, RC.NESTED_PIXELS),
    # lists of 1, 2 and 3 members: the index read two ahead stops at the list's end, and the last record's list
    # ends where the active-list buffer's used part ends
    "nested-3": lambda: (RC.nested_gaussians(3, 0.2), MAIN_CAMERA, RC.NESTED_PIXELS),
    # the root with leaf children only / one climb, to the root, whose own parent entry is -1
    "scattered-6": lambda: (scattered_gaussians(6, 0.12, 5), MAIN_CAMERA, RC.NESTED_PIXELS),
    "scattered-24": lambda: (scattered_gaussians(24, 0.04, 6), MAIN_CAMERA, RC.NESTED_PIXELS),
    # climbs over every level of the deepest tree
    "chain": lambda: (chain_gaussians(1.2e-5), CHAIN_CAMERA, CHAIN_PIXELS),
}
# (case, option, value): the same walks from the root (no start entries), and on the device-built tree (another
# parent table)
OPTION_CASES = [("scattered-24", "start_subtree", 0), ("chain", "start_subtree", 0),
                ("scattered-24", "device_bvh", 1), ("chain", "device_bvh", 1)]


def oracle_rows(arrays, camera, pixels):
    """{pixel: the oracle's rows} under the device's tie rule."""
    osc = RC.oracle_scene(arrays)
    with O.stable_ties():
        return {(int(x), int(y)): O.debug_pixel_records(osc, camera[0], camera[1], camera[2], int(x), int(y), W, W, RC.STEP,
                                                        ENV_SAMPLES) for x, y in pixels}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(arrays, camera, pixels, oracle rows) of a case, computed once and shared (read-only)."""
    arrays, camera, pixels = CASES[name]()
    rows = oracle_rows(arrays, camera, pixels)
    for r in rows.values():
        r.setflags(write=False)
    return arrays, camera, pixels, rows


def oracle_report(name):
    """The oracle's rows of a case against themselves: the spread of its rays, and Li + Le from its own Tr."""
    arrays, _, _, rows = reference(name)
    rep = RC.Report()
    for r in rows.values():
        rep.merge(RC.compare_rows(r, r, arrays[4], arrays[5], RC.ENV))
    return rep, rows
