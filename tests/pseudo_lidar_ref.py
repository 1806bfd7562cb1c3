"""The pseudo-LiDAR point rule of ``fusiondepth_amd.detection`` (``fd_points_export``) restated in numpy, written for this project: float64
elementwise operations in the stated order - numpy's ufuncs round each once and never contract -, the boolean selection that gives
row-major order, one cast to float32.  A helper, not a test."""
import numpy as np


def calib_scalars(calib):
    """``(calibration, A, t)`` as ``points_export`` takes it -> the six camera scalars, A [3,3], t [3], all float64."""
    c, A, t = calib
    cam = tuple(np.float64(v) for v in (c.c_u, c.c_v, c.f_u, c.f_v, c.b_x, c.b_y))
    return cam, np.asarray(A, dtype=np.float64), np.asarray(t, dtype=np.float64)


def velo_coordinates(depth, calib):
    """X, Y, Z [H,W] float64 of every pixel of a float32 map, unrounded and unfiltered."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 2
    (c_u, c_v, f_u, f_v, b_x, b_y), A, t = calib_scalars(calib)
    H, W = depth.shape
    z = depth.astype(np.float64)
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):                              # inf and NaN depths are part of the rule
        x = ((u - c_u) * z) / f_u + b_x
        y = ((v - c_v) * z) / f_v + b_y
        X, Y, Z = (((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + t[r] for r in range(3))
    return X, Y, Z


def points(depth, calib, max_high=1.0):
    """The cloud of one map: float32 [M,4] (x, y, z, 1), kept points in row-major pixel order."""
    X, Y, Z = velo_coordinates(depth, calib)
    with np.errstate(all="ignore"):
        keep = (X >= 0) & (Z < np.float64(max_high))
        cloud = np.stack([X, Y, Z, np.ones_like(X)], axis=-1)[keep].astype(np.float32)
    return cloud, keep


def hand_made_case():
    """A 2 x 3 map worked out by hand -> (depth, calib, the cloud at max_high = 1): camera z -> Velodyne x, camera x -> -y, camera y ->
    -z; f = 1, c = (1, 0.5), no offsets.  Kept, in row-major order: (0,0) with Z = 0.5, (1,1) with Z = -1.5, (1,2) with X = Z = 0."""
    import types
    cam = types.SimpleNamespace(c_u=1.0, c_v=0.5, f_u=1.0, f_v=1.0, b_x=0.0, b_y=0.0)
    calib = (cam, np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]), np.zeros(3))
    depth = np.array([[1.0, np.nan, 2.0], [-1.0, 3.0, 0.0]], dtype=np.float32)
    return depth, calib, np.array([[1.0, 1.0, 0.5, 1.0], [3.0, 0.0, -1.5, 1.0], [0.0, 0.0, 0.0, 1.0]], dtype=np.float32)


def clouds(depths, calibs, max_high=1.0):
    """N maps -> (the list of clouds, starts [N+1] int64: the first point of each map, the total last)."""
    out = [points(d, c, max_high)[0] for d, c in zip(depths, calibs)]
    starts = np.zeros(len(out) + 1, dtype=np.int64)
    starts[1:] = np.cumsum([len(o) for o in out])
    return out, starts
