"""PFM (portable float map) reader and writer with the behaviour of the reference's training data path.

`load_pfm` is `ImagePatchesGenerator.load_pfm` (data_generator.py:63-102): header `Pf` (one channel) or `PF`
(three), `width height`, a scale whose sign gives the byte order (negative = little-endian), float32 rows stored
bottom-up, returned flipped as `[height][width][channels]` together with |scale|.  `save_pfm` writes what the
patch-preparation scripts write (image_patches_prepare/middlebury_2003.py:8-32) and can also write big-endian.
"""
from __future__ import annotations

import sys

import numpy as np


def load_pfm(fname):
    """-> (float32 [H][W][C] array, top row first, in the file's byte order; scale)."""
    with open(fname, "rb") as fh:
        header = fh.readline().decode().rstrip()
        if header == "PF":
            channels = 3
        elif header == "Pf":
            channels = 1
        else:
            raise ValueError(f"{fname}: not a PFM file")
        dims = fh.readline().decode().split()
        if len(dims) != 2 or not all(d.isdigit() for d in dims):
            raise ValueError(f"{fname}: malformed PFM header")
        width, height = int(dims[0]), int(dims[1])
        scale = float(fh.readline().decode().rstrip())
        endian = "<f" if scale < 0 else ">f"
        data = np.frombuffer(fh.read(), dtype=endian)
    if data.size != width * height * channels:
        raise ValueError(f"{fname}: {data.size} floats for a {width}x{height}x{channels} image")
    return np.flipud(data.reshape(height, width, channels)), abs(scale)


def save_pfm(fname, image, scale: float = 1.0, big_endian=None) -> None:
    """Write a float32 [H][W], [H][W][1] or [H][W][3] image.  big_endian=None keeps the array's byte order."""
    image = np.asarray(image)
    if image.dtype.kind != "f" or image.dtype.itemsize != 4:
        raise TypeError(f"a PFM holds float32 samples, got {image.dtype}")
    if image.ndim == 3 and image.shape[2] == 3:
        color = True
    elif image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1):
        color = False
    else:
        raise ValueError(f"a PFM holds one or three channels, got shape {image.shape}")
    if big_endian is None:
        bo = image.dtype.byteorder
        big_endian = bo == ">" or (bo == "=" and sys.byteorder == "big")
    out = np.flipud(image).astype(">f4" if big_endian else "<f4")
    with open(fname, "wb") as fh:
        fh.write(b"PF\n" if color else b"Pf\n")
        fh.write(b"%d %d\n" % (image.shape[1], image.shape[0]))
        fh.write(b"%f\n" % (scale if big_endian else -scale))
        fh.write(out.tobytes())
