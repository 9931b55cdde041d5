"""The two ends of the pipeline around the matcher: raw calibrated pair -> rectified pair, disparity -> depth.

    cal = StereoCalibration.load("rig.npz")          # K1 D1 K2 D2 R T size (and R1 R2 P1 P2 Q when it has them)
    rect = Rectifier(cal)                            # both sampling maps, built once on the device
    m = StereoMatcher(*rect.out_size, ndisp)
    m.load_raw(left_raw, right_raw, rect)            # upload + one remap launch into the matcher's resident pair
    depth = rect.depth(m.match())                    # metric depth, 0 where there is no disparity

The reference does this on the host with OpenCV (Calibration/mycalibration.cpp:826-839: stereoRectify,
initUndistortRectifyMap(..., CV_16SC2, ...), remap(..., INTER_LINEAR)) and leaves the triangulation to its GUI.
Here the per-frame work is two HIP kernels of libsde.so (include/sde_geom.h: sdg_remap_u8, sdg_reproject) and the
per-calibration map build a third (sdg_rectify_map); `stereo_rectify` is host NumPy, a few 3x3 products.  The
estimation of a calibration (chessboard detection, Zhang's method) is out of scope: a calibration is an input.

Conventions: `R`, `T` take a point from the first (left) camera's frame to the second's, X2 = R @ X1 + T, as
OpenCV's stereoCalibrate returns them; `size` is (height, width) of the raw images, the order of every shape in
this package (OpenCV's imageSize is (width, height)); distortion vectors hold k1 k2 p1 p2 [k3 [k4 k5 k6]].
"""
from __future__ import annotations

import json

import numpy as np

_MATRICES = ("K1", "D1", "K2", "D2", "R", "T")
_OPTIONAL = ("R1", "R2", "P1", "P2", "Q")
_SHAPES = {"K1": (3, 3), "K2": (3, 3), "R": (3, 3), "T": (3,), "R1": (3, 3), "R2": (3, 3), "P1": (3, 4),
           "P2": (3, 4), "Q": (4, 4)}


def rodrigues(om):
    """Rotation vector (axis * angle) -> 3x3 rotation matrix, float64."""
    om = np.asarray(om, np.float64).reshape(3)
    th = float(np.linalg.norm(om))
    if th < 1e-300:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def rotation_vector(R):
    """3x3 rotation matrix -> rotation vector, the inverse of `rodrigues` for angles below pi."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0   # axis * sin(angle)
    s, c = float(np.linalg.norm(w)), (np.trace(R) - 1.0) / 2.0
    if s < 1e-300:
        if c > 0:
            return np.zeros(3)
        raise ValueError("a relative rotation of pi between the two cameras is not a stereo rig")
    return w * (np.arctan2(s, c) / s)


def stereo_rectify(K1, K2, R, T):
    """Bouguet's rectification of a horizontal rig, host float64 -> (R1, R2, P1, P2, Q).

    Each camera is turned by half the relative rotation (r = rodrigues(-om/2), om the rotation vector of R), so
    both look the same way, then both by wR, the smallest rotation that lays the baseline t = r @ T along the x
    axis: about t x (+-e_x), by acos(|t_x| / |t|).  R1 = wR @ r.T and R2 = wR @ r take a point of camera 1 / 2 into
    its rectified frame.  The new intrinsics are shared and build-defined (no valid-region scaling):
    f = (K1[1,1] + K2[1,1]) / 2, (cx, cy) the mean of the two principal points.  With tx = (R2 @ T)[0],
        P1 = [f 0 cx 0; 0 f cy 0; 0 0 1 0],  P2 = P1 with P2[0,3] = f * tx,
        Q  = [1 0 0 -cx; 0 1 0 -cy; 0 0 0 f; 0 0 -1/tx 0],
    so a left pixel (x, y) with disparity d = x_left - x_right has depth Z = -f * tx / d.  A rig whose baseline is
    more vertical than horizontal after the first step raises ValueError."""
    K1, K2, R = (np.asarray(a, np.float64).reshape(3, 3) for a in (K1, K2, R))
    T = np.asarray(T, np.float64).reshape(3)
    r = rodrigues(-0.5 * rotation_vector(R))
    t = r @ T
    if not abs(t[0]) > abs(t[1]):
        raise ValueError("vertical stereo rigs are not supported (the baseline must run along x)")
    uu = np.array([1.0 if t[0] > 0 else -1.0, 0.0, 0.0])
    ww = np.cross(t, uu)
    nw = float(np.linalg.norm(ww))
    wR = np.eye(3)
    if nw > 0.0:
        wR = rodrigues(ww * (np.arccos(min(1.0, abs(t[0]) / float(np.linalg.norm(t)))) / nw))
    R1, R2 = wR @ r.T, wR @ r
    tx = float((R2 @ T)[0])
    f = (K1[1, 1] + K2[1, 1]) / 2.0
    cx, cy = (K1[0, 2] + K2[0, 2]) / 2.0, (K1[1, 2] + K2[1, 2]) / 2.0
    P1 = np.array([[f, 0.0, cx, 0.0], [0.0, f, cy, 0.0], [0.0, 0.0, 1.0, 0.0]])
    P2 = P1.copy()
    P2[0, 3] = f * tx
    Q = np.array([[1.0, 0.0, 0.0, -cx], [0.0, 1.0, 0.0, -cy], [0.0, 0.0, 0.0, f], [0.0, 0.0, -1.0 / tx, 0.0]])
    return R1, R2, P1, P2, Q


def _distortion(D, name):
    D = np.asarray(D, np.float64).reshape(-1)
    if D.size > 8 and np.any(D[8:] != 0.0):
        raise ValueError(f"{name}: thin-prism and tilt terms (coefficients past k6) are not modelled")
    out = np.zeros(8)
    out[:min(D.size, 8)] = D[:8]
    return out


class StereoCalibration:
    """A calibrated pair: intrinsics K1, K2 (3x3), distortion D1, D2 (k1 k2 p1 p2 k3 k4 k5 k6, shorter vectors are
    zero-extended), the pose R (3x3), T (3) of camera 1 in camera 2's frame and the raw image size (H, W).
    rectification: optionally the R1, R2, P1, P2, Q of an earlier rectification, used as given (all five or
    none); otherwise `stereo_rectify` computes them."""

    def __init__(self, K1, D1, K2, D2, R, T, size, **rectification):
        self.K1, self.K2, self.R = (np.array(a, np.float64).reshape(3, 3) for a in (K1, K2, R))
        self.D1, self.D2 = _distortion(D1, "D1"), _distortion(D2, "D2")
        self.T = np.array(T, np.float64).reshape(3)
        self.size = (int(size[0]), int(size[1]))
        for name, K in (("K1", self.K1), ("K2", self.K2)):
            if K[1, 0] != 0.0 or tuple(K[2]) != (0.0, 0.0, 1.0):
                raise ValueError(f"{name} must be [fx s cx; 0 fy cy; 0 0 1]")
        given = {k: v for k, v in rectification.items() if v is not None}
        if set(given) - set(_OPTIONAL):
            raise TypeError(f"unknown arguments {sorted(set(given) - set(_OPTIONAL))}")
        if given and set(given) != set(_OPTIONAL):
            raise ValueError(f"a stored rectification needs all of {_OPTIONAL}, got {sorted(given)}")
        self.rectification = {k: np.array(given[k], np.float64).reshape(_SHAPES[k]) for k in _OPTIONAL} if given else None

    def rectify(self):
        """(R1, R2, P1, P2, Q): the stored rectification, else stereo_rectify's."""
        if self.rectification is not None:
            return tuple(self.rectification[k] for k in _OPTIONAL)
        return stereo_rectify(self.K1, self.K2, self.R, self.T)

    def _items(self):
        d = {k: getattr(self, k) for k in _MATRICES}
        d["size"] = np.array(self.size, np.int64)
        d.update(self.rectification or {})
        return d

    def save(self, path):
        """Write `.npz` (float64 arrays) or `.json` (nested lists; repr-exact float64) with the keys K1 D1 K2 D2 R T
        size, and R1 R2 P1 P2 Q when the calibration carries a rectification."""
        path = str(path)
        if path.endswith(".npz"):
            np.savez(path, **self._items())
        elif path.endswith(".json"):
            with open(path, "w") as fh:
                json.dump({k: v.tolist() for k, v in self._items().items()}, fh, indent=1)
                fh.write("\n")
        else:
            raise ValueError(f"{path}: a calibration file is .npz or .json")

    @classmethod
    def load(cls, path):
        path = str(path)
        if path.endswith(".npz"):
            with np.load(path) as z:
                d = {k: z[k] for k in z.files}
        elif path.endswith(".json"):
            with open(path) as fh:
                d = json.load(fh)
        else:
            raise ValueError(f"{path}: a calibration file is .npz or .json")
        missing = [k for k in _MATRICES + ("size",) if k not in d]
        if missing:
            raise KeyError(f"{path}: missing {missing}")
        return cls(*(d[k] for k in _MATRICES), np.asarray(d["size"]).reshape(-1)[:2],
                   **{k: d[k] for k in _OPTIONAL if k in d})


def camera_cal(K, D, R_rect, P):
    """The 26 float64 sdg_rectify_map takes for one camera: K, the 8 distortion terms, inv(P[:, :3] @ R_rect)."""
    Minv = np.linalg.inv(np.asarray(P, np.float64)[:, :3] @ np.asarray(R_rect, np.float64))
    return np.concatenate([np.asarray(K, np.float64).reshape(9), _distortion(D, "D"), Minv.reshape(9)])


class Rectifier:
    """Device-side rectification and reprojection for one calibration.  The two int32 [H,W,2] sampling maps are
    built once, into `maps` [2,H,W,2]; out_size (H, W) defaults to the raw size.  R1, R2, P1, P2, Q are attributes
    (host float64)."""

    def __init__(self, calibration: StereoCalibration, out_size=None, device=None):
        import torch

        from . import ops
        self.calibration = c = calibration
        self.raw_size = c.size
        self.out_size = c.size if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.R1, self.R2, self.P1, self.P2, self.Q = c.rectify()
        H, W = self.out_size
        self.cal = [camera_cal(c.K1, c.D1, self.R1, self.P1), camera_cal(c.K2, c.D2, self.R2, self.P2)]
        self.maps = torch.empty((2, H, W, 2), dtype=torch.int32, device=self.device)
        for i in range(2):
            ops.rectify_map(self.cal[i], H, W, out=self.maps[i])

    def remap(self, raw2, out=None, valid=None):
        """Raw pair u8 [2,Hs,Ws] on the device -> rectified pair u8 [2,H,W], one launch.  valid (optional u8
        [2,H,W]) gets 1 where the sample lay wholly inside the raw image."""
        from . import ops
        if tuple(raw2.shape) != (2,) + self.raw_size:
            raise ValueError(f"raw pair must be [2,{self.raw_size[0]},{self.raw_size[1]}], got {tuple(raw2.shape)}")
        return ops.remap_u8(raw2, self.maps, out=out, valid=valid)

    def depth(self, disp, min_disp: float = 0.0, out=None):
        """Disparity f32 [H,W] of the rectified left view -> depth along the rectified optical axis, in T's unit;
        0 where the disparity is not finite or not above min_disp."""
        from . import ops
        return ops.reproject(disp, self.Q, min_disp, depth=out, want=("depth",))[0]

    def points(self, disp, min_disp: float = 0.0, out=None):
        """Disparity f32 [H,W] -> XYZ f32 [H,W,3] in the rectified left camera's frame; zeros where invalid."""
        from . import ops
        return ops.reproject(disp, self.Q, min_disp, xyz=out, want=("xyz",))[1]
