"""Hand-built maps for the smoothing tests (pure numpy) beside those of normalscenes and regionscenes: tests/test_smooth_host.py shows on the
reference that they contain what they claim, tests/test_gpu_smooth.py runs them on the device."""
import numpy as np

import regionscenes as rs
from outlierscenes import rows_of

F = np.float32
PITCH = 0.01                 # the lattices' pitch (regionscenes.PITCH)
R_DRIFT = 2.0 ** -5          # the drift scene's radius
SIGMA_PLANE = 0.003          # the noisy plane's sigma_z
SIGMA_BOX = 0.001            # the noisy box corner's position noise, per axis


def plane_lattice(m=40, sigma=SIGMA_PLANE, seed=21):
    """m x m rows on the lattice of pitch PITCH in the plane z = 1 with Gaussian noise of `sigma` in z, stored normals +z, shuffled.  The true
    plane is z = 1"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    S = rows_of(m * m)
    S[:, 0], S[:, 1] = (i.reshape(-1) * PITCH).astype(F), (j.reshape(-1) * PITCH).astype(F)
    S[:, 2] = (1.0 + rng.normal(0.0, sigma, m * m)).astype(F)
    S[:, 8:11] = (0.0, 0.0, 1.0)
    return np.ascontiguousarray(S[rng.permutation(m * m)], F)


def plane_rms(P):
    """the RMS distance of positions [n, 3] to the true plane of plane_lattice"""
    return float(np.sqrt(np.mean((np.asarray(P, np.float64)[:, 2] - 1.0) ** 2)))


def noisy_box_corner(sigma=SIGMA_BOX, seed=22):
    """(S, marks, near): regionscenes.box_corner with Gaussian noise of `sigma` per axis on every finite position; near = per face the rows that
    lay within 2 PITCH of a crease before the noise (a face's own plane is its coordinate = 0: faces z = 0, x = 0, y = 0 in marks["faces"])"""
    S, marks = rs.box_corner()
    rng = np.random.default_rng(seed)
    clean = S[:, :3].astype(np.float64)
    ok = np.isfinite(clean).all(1)
    S = S.copy()
    S[ok, :3] = (clean[ok] + rng.normal(0.0, sigma, (int(ok.sum()), 3))).astype(F)
    near = []
    for rows, axis in zip(marks["faces"], (2, 0, 1)):
        others = [a for a in range(3) if a != axis]
        near.append(rows[(clean[rows][:, others] < 2 * PITCH).any(1)])
    return np.ascontiguousarray(S, F), marks, tuple(near)


def crease_rms(P, marks, near):
    """the RMS distance to a surfel's own face over the rows of `near`"""
    P = np.asarray(P, np.float64)
    d = np.concatenate([P[rows, axis] for rows, axis in zip(near, (2, 0, 1))])
    return float(np.sqrt(np.mean(d ** 2)))


def drift_scene(n=700, seed=23):
    """a thin random patch (about ten neighbours within R_DRIFT, so that most rows use every neighbour they have, out to the radius) with noise of a
    sixth of the radius across it: rows move far enough for used neighbours to end up past the radius in a later iteration.  Stored normals +z
    but for a tenth of the rows, which have -z (the gate drops them)"""
    rng = np.random.default_rng(seed)
    side = (n * np.pi * R_DRIFT ** 2 / 10.0) ** 0.5
    S = rows_of(n)
    S[:, 0], S[:, 1] = rng.uniform(0.0, side, n).astype(F), rng.uniform(0.0, side, n).astype(F)
    S[:, 2] = (2.0 + rng.normal(0.0, R_DRIFT / 6.0, n)).astype(F)
    S[:, 8:11] = (0.0, 0.0, 1.0)
    S[rng.random(n) < 0.1, 10] = -1.0
    return np.ascontiguousarray(S, F)
