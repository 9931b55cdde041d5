"""Generate the right-view golden vectors (run in the build container only).

The right view is pinned to the reference's own NumPy functions on the mirrored, swapped pair:

    disp_r = flipW( WTA1( compute_cost_volume( flipW(fr), flipW(fl), D ) ) )

``compute_cost_volume`` / ``WTA1`` are extracted from the reference source exactly as make_golden.py does
(its loader is reused; no reference text is copied) and applied to the inputs already stored in
``golden_cpu_path.npz``.  Only the result arrays are written (``golden_right_view.npz``: ``<case>__disp_r``
for every case of the existing fixture).

Usage (in the build container, where the reference exists):

    python tests/golden/make_golden_right.py

The produced fixture is committed; tests never read the reference.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference_cpu_functions  # noqa: E402

SRC = os.path.join(HERE, "golden_cpu_path.npz")
OUT = os.path.join(HERE, "golden_right_view.npz")


def flip(a):
    return np.ascontiguousarray(a[:, ::-1])


def main():
    compute_cost_volume, _, WTA1 = load_reference_cpu_functions()
    out = {}
    with np.load(SRC, allow_pickle=False) as z:
        names = [str(n) for n in z["__cases__"]]
        for name in names:
            fl, fr, d = z[name + "__fl"], z[name + "__fr"], int(z[name + "__ndisp"])
            disp = WTA1(compute_cost_volume(flip(fr), flip(fl), d))
            assert disp.dtype == np.float32
            out[name + "__disp_r"] = flip(disp)
    out["__cases__"] = np.array(names)
    out["__numpy_version__"] = np.array(np.__version__)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(names)} right-view cases", file=sys.stderr)


if __name__ == "__main__":
    main()
