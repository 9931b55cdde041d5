"""Adversarial inputs for the uniqueness check of the fused cost volume + WTA, modelled on cert_cases.near_tie_pair.

margin_pair builds a feature pair in which every built left pixel has a planted winner at dA and a planted
runner-up at dB, |dA - dB| >= 2, whose costs differ by tau + t, t of either sign from cert_cases.T_GRID (0, 2^-8 ..
2^-24): margins on both sides of the threshold, at distances around the certificate's eps.  A share of the pixels
gets a third planted candidate next to the winner that scores between the two, so that the unrestricted runner-up
is the adjacent disparity the definition must ignore.  The left features are left un-normalised (the solution of
the Gram system as it stands): normalising would rescale the planted margin.

integer_pair: features with entries 0..3, so every dot product -- and every margin -- is an exact small integer and
pixels sit at m == tau exactly.

Shared by tests/test_unique_host.py (the builder's own conditions, from the oracle alone) and
tests/test_gpu_unique.py (the kernels on these inputs).
"""
import numpy as np

import cert_cases as cc

TAU = 0.1
H, W = 4, 1000


def margin_pair(rng, H, W, D, tau=TAU, d0=0, C=64, score=1.0, adjacent=0.3):
    """(fl, fr, info).  fr: unit-norm noise.  Every left pixel x >= d0 + 2 gets dA, dB in [d0, min(x, D - 1)] with
    |dA - dB| >= 2 and fl[x] the vector of span{fr[x - dA], fr[x - dB] (, fr[x - dN])} with fl[x] . fr[x - dA] =
    score, fl[x] . fr[x - dB] = score - (tau + t); with probability `adjacent` a third candidate dN = dA +- 1
    scores score - (tau + t) / 2.  The other disparities score |fl[x]| times unit noise (about 0.5 at most for C =
    64), far below both."""
    fr = cc.l2n(rng.standard_normal((H, W, C)).astype(np.float32))
    fl = cc.l2n(rng.standard_normal((H, W, C)).astype(np.float32))
    dA = np.full((H, W), -1, np.int32)
    dB = np.full((H, W), -1, np.int32)
    dN = np.full((H, W), -1, np.int32)
    tt = np.zeros((H, W))
    fr64 = fr.astype(np.float64)
    for y in range(H):
        for x in range(d0 + 2, W):
            hi = min(x, D - 1)
            if hi - d0 < 2:
                continue
            while True:
                da, db = (int(v) for v in rng.choice(hi - d0 + 1, size=2, replace=False) + d0)
                if abs(da - db) >= 2:
                    break
            t = float(cc.T_GRID[int(rng.integers(cc.T_GRID.size))]) * (1.0 if rng.integers(2) else -1.0)
            m = tau + t
            ds, scores = [da, db], [score, score - m]
            if rng.random() < adjacent:
                dn = da + (1 if rng.integers(2) else -1)
                if d0 <= dn <= hi and dn != db:
                    ds.append(dn)
                    scores.append(score - 0.5 * m)
                    dN[y, x] = dn
            V = np.stack([fr64[y, x - d] for d in ds])
            coef = np.linalg.solve(V @ V.T, np.array(scores))
            fl[y, x] = (coef @ V).astype(np.float32)
            dA[y, x], dB[y, x], tt[y, x] = da, db, t
    info = {"dA": dA, "dB": dB, "dN": dN, "t": tt, "built": dA >= 0, "loud": np.zeros((H, W), bool), "scale": 1.0,
            "d0": d0, "D": D, "tau": np.float32(tau)}
    return fl, fr, info


def integer_pair(rng, H, W, C=64):
    """Features with integer entries 0..3: dot products of at most 9 C, exact in float32 in any order."""
    fl = rng.integers(0, 4, (H, W, C)).astype(np.float32)
    fr = rng.integers(0, 4, (H, W, C)).astype(np.float32)
    return fl, fr


# name -> (seed, H, W, D, d0, C)
CASES = {}
for _i, (_D, _d0) in enumerate([(192, 0), (64, 0), (256, 17), (192, 40)]):
    CASES[f"D{_D}-d{_d0}"] = (70 + _i, H, W, _D, _d0, 64)
CASES["narrow-W37"] = (75, H, 37, 64, 0, 64)          # W < D: every pixel's range is cut by the image edge
CASES["wide-D512"] = (76, H, W, 512, 0, 64)           # past one row sweep: the exact form in either mode
CASES["generic-C16"] = (77, H, 200, 48, 0, 16)        # C != 64: the generic form
# the cases whose planted margins must meet the shares below (C = 16 noise scores too high for the planted pair to
# be the top two everywhere; the narrow case builds few pixels per row)
SHARE_CASES = [n for n in CASES if n.startswith("D") or n == "wide-D512"]

MIN_NEAR = 0.20       # built pixels with |m - tau| <= 16 eps
MIN_SIDE = 0.05       # ... of them, on each side of tau
MIN_ADJACENT = 0.10   # built pixels whose unrestricted runner-up is next to the winner
MIN_DECISION = 0.05   # built pixels rejected, and kept


def build_case(name):
    seed, h, w, D, d0, C = CASES[name]
    return margin_pair(np.random.default_rng(seed), h, w, D, d0=d0, C=C)


def loud_case(norm=200.0):
    """D192-d0 with one right pixel per row scaled to `norm` (past the row sweep's fp16 range guard of 127 when
    norm >= 127.5) and one loud left pixel per row; returns (fl, fr, info) with info['loud'] / info['loud_left']."""
    fl, fr, info = build_case("D192-d0")
    rng = np.random.default_rng(90)
    left = np.zeros(info["built"].shape, bool)
    for y in range(fl.shape[0]):
        q = int(rng.integers(100, 800))
        fr[y, q] *= np.float32(norm)
        info["loud"][y, q] = True
        x = int(rng.integers(300, 900))
        fl[y, x] *= np.float32(norm / max(np.sqrt((fl[y, x].astype(np.float64) ** 2).sum()), 1e-12))
        left[y, x] = True
    info["loud_left"] = left
    return fl, fr, info


def nonfinite_case():
    """D192-d0 with a NaN, a +inf and a -inf channel planted in single right and left pixels; info['bad_right'] /
    info['bad_left'] mark them."""
    fl, fr, info = build_case("D192-d0")
    br = np.zeros(info["built"].shape, bool)
    bl = np.zeros(info["built"].shape, bool)
    for y, (q, x, v) in enumerate([(300, 700, np.nan), (450, 650, np.inf), (5, 999, -np.inf), (640, 130, np.nan)]):
        fr[y, q, 7 * y + 1] = v
        fl[y, x, 5 * y + 2] = v
        br[y, q] = True
        bl[y, x] = True
    info["bad_right"], info["bad_left"] = br, bl
    return fl, fr, info


def analyse(cv, fl, fr, info, K, ABS, fused):
    """cert_cases.analyse plus the definition's margin of every pixel (`fused`: unique_literal.fused of the oracle's
    volume) and the plain runner-up's distance from the winner."""
    import unique_literal as ul
    an = cc.analyse(cv, fl, fr, info, K, ABS)
    d0 = info["d0"]
    an["m"] = fused["m"].astype(np.float64)
    an["dist"] = np.abs(an["m"] - float(info["tau"]))
    sec = ul.plain_second(np.moveaxis(cv[d0:], 0, -1)) + d0
    an["adjacent"] = np.abs(sec - fused["argmin"]) == 1
    an["reject"] = fused["reject"].astype(bool)
    return an


def shares(an, info):
    b = info["built"]
    near = an["dist"] <= 16 * an["eps"]
    tau = float(info["tau"])
    return {"near": near[b].mean(), "below": (near & (an["m"] < tau))[b].mean(),
            "above": (near & (an["m"] >= tau))[b].mean(), "adjacent": an["adjacent"][b].mean(),
            "rejected": an["reject"][b].mean(), "kept": (~an["reject"])[b].mean()}


def check_shares(name, sh):
    assert sh["near"] >= MIN_NEAR, (name, sh)
    assert sh["below"] >= MIN_SIDE and sh["above"] >= MIN_SIDE, (name, sh)
    assert sh["adjacent"] >= MIN_ADJACENT, (name, sh)
    assert sh["rejected"] >= MIN_DECISION and sh["kept"] >= MIN_DECISION, (name, sh)
