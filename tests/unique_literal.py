"""The uniqueness check's definition (include/sde_unique.h) restated in NumPy,
and literal volumes with hand-written expected maps that hold the restatement itself to the text.

Shared by tests/test_unique_host.py (CPU) and tests/test_gpu_unique.py (GPU): every expected value of those tests
is this restatement applied to the oracle's volumes.  Everything is float32 and compared by bytes.
"""
import numpy as np

F = np.float32
INF = F(np.inf)
NAN = F(np.nan)


def winner(c, rule="inf"):
    """The winner scan of a pixel's costs c[..., D] (last axis = d): rule 'inf' is best = +inf, `v < best` in
    increasing d (WTA / WTA1; no winner -> -1), rule 'd0' is best = c[0], `best > v` (the SGM WTA kernel: a NaN
    at d = 0 is never replaced, and there is always a winner)."""
    c = np.asarray(c, F)
    D = c.shape[-1]
    best = np.full(c.shape[:-1], INF, F) if rule == "inf" else c[..., 0].copy()
    arg = np.full(c.shape[:-1], -1 if rule == "inf" else 0, np.int32)
    with np.errstate(invalid="ignore"):
        for d in range(0 if rule == "inf" else 1, D):
            v = c[..., d]
            take = v < best
            best = np.where(take, v, best)
            arg = np.where(take, np.int32(d), arg)
    return arg


def unique(c, tau, rule="inf", d0=0):
    """The definition on costs c[..., D] over the scanned range [d0, d0 + D): a dict of
    i (int32 winner, -1 if none), c1, c2, m (float32), reject (uint8) and disp (float32: i, -1 where rejected)."""
    c = np.ascontiguousarray(c, F)
    D = c.shape[-1]
    tau = F(tau)
    i = winner(c, rule)
    has = i >= 0
    c1 = np.take_along_axis(c, np.maximum(i, 0)[..., None], -1)[..., 0]
    c2 = np.full(c.shape[:-1], INF, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            v = c[..., d]
            take = (np.abs(d - i) >= 2) & (v < c2)
            c2 = np.where(take, v, c2)
        m = np.where(c2 == c1, F(0.0), (c2 - c1).astype(F)).astype(F)
        m = np.where(has, m, F(0.0)).astype(F)
        m = np.where(np.isnan(m), np.array([0x7fc00000], np.uint32).view(F)[0], m).astype(F)   # the canonical NaN
        reject = has & (m < tau)
    disp = np.where(reject, F(-1.0), (i + np.where(has, d0, 0)).astype(F)).astype(F)
    return {"i": np.where(has, i + d0, -1).astype(np.int32), "c1": np.where(has, c1, INF).astype(F), "c2": c2, "m": m,
            "reject": reject.astype(np.uint8), "disp": disp}


def plain_second(c):
    """Index of the smallest cost other than the first minimum's (the unrestricted runner-up), -1 if D < 2."""
    c = np.asarray(c, F)
    if c.shape[-1] < 2:
        return np.full(c.shape[:-1], -1, np.int32)
    i = winner(c, "inf")
    masked = np.where(np.arange(c.shape[-1]) == i[..., None], INF, np.nan_to_num(c, nan=np.inf))
    return np.argmin(masked, -1).astype(np.int32)


def right_volume(cv, fill=-0.0):
    """The right view's costs of a left DHW volume cv[d, y, x] = cost(x, d): R[d, y, x'] = cost(x' + d, d), the
    fill where x' + d >= W (sde_cv_wta_right's scan)."""
    D, H, W = cv.shape
    out = np.full((D, H, W), F(fill), F)
    for d in range(min(D, W)):
        out[d, :, :W - d] = cv[d, :, d:]
    return out


def fused(cv, tau, d0=0, side="left"):
    """The fused forms' expected outputs from the oracle's DHW volume cv over [d0, D): unique() of the pixel's costs
    (the right view's through right_volume), min_cost / argmin the winner's."""
    vol = cv if side == "left" else right_volume(cv)
    u = unique(np.moveaxis(vol[d0:], 0, -1), tau, "inf", d0)
    return {"disp": u["disp"], "reject": u["reject"], "argmin": u["i"], "min_cost": u["c1"], "m": u["m"]}


def ulp_below(x):
    return np.nextafter(F(x), F(-np.inf))


# ----------------------------------------------------------------------------
# Literal volumes: (name, costs [npix][D], tau, rule, expected i, expected m, expected reject), written by hand
# from the text of the definition
# ----------------------------------------------------------------------------
_T = F(0.25)
LITERALS = [
    # the runner-up next to the winner is ignored: the second-best 1.01 at d = 3 does not count, 1.5 at d = 0 does
    ("adjacent-ignored", [[1.5, 3.0, 1.0, 1.01, 2.0]], 0.4, "inf", [2], [0.5], [0]),
    ("adjacent-ignored-rejects", [[1.5, 3.0, 1.0, 1.01, 2.0]], 0.75, "inf", [2], [0.5], [1]),
    # both neighbours excluded
    ("both-neighbours", [[9.0, 1.25, 1.0, 1.125, 4.0]], 2.0, "inf", [2], [3.0], [0]),
    # winner at d = 0 and at d = D - 1
    ("winner-first", [[1.0, 1.0625, 3.0, 2.0]], 1.5, "inf", [0], [1.0], [1]),
    ("winner-last", [[2.0, 3.0, 1.0625, 1.0]], 0.5, "inf", [3], [1.0], [0]),
    # D = 1, 2, 3 with the winner in the middle: no disparity two away, m = +inf, never rejected
    ("D1", [[5.0]], 1e30, "inf", [0], [np.inf], [0]),
    ("D2", [[5.0, 4.0]], 1e30, "inf", [1], [np.inf], [0]),
    ("D3-middle", [[5.0, 4.0, 6.0]], 1e30, "inf", [1], [np.inf], [0]),
    ("D3-edge", [[4.0, 5.0, 6.0]], 1.0, "inf", [0], [2.0], [0]),
    # m == tau exactly is kept; one ulp below tau is rejected
    ("m-equals-tau", [[1.0, 9.0, 1.25]], 0.25, "inf", [0], [0.25], [0]),
    ("m-ulp-below-tau", [[0.0, 9.0, ulp_below(_T)]], 0.25, "inf", [0], [ulp_below(_T)], [1]),
    # all-equal costs: m = +0 (rejected by any tau > 0, kept by tau = 0)
    ("all-equal", [[2.0, 2.0, 2.0, 2.0]], 1e-30, "inf", [0], [0.0], [1]),
    ("all-equal-tau0", [[2.0, 2.0, 2.0, 2.0]], 0.0, "inf", [0], [0.0], [0]),
    ("all-fill", [[-0.0, -0.0, -0.0]], 0.5, "inf", [0], [0.0], [1]),
    # NaN never wins either scan; +inf can be the runner-up; -inf - -inf is the c2 == c1 case
    ("nan-skipped", [[NAN, 2.0, NAN, 3.0, NAN]], 0.5, "inf", [1], [1.0], [0]),
    ("nan-runner-up", [[1.0, 0.5, NAN, NAN]], 1.0, "inf", [1], [np.inf], [0]),
    ("inf-runner-up", [[1.0, INF, INF, INF]], 1e38, "inf", [0], [np.inf], [0]),
    ("minus-inf-tie", [[-INF, 0.0, -INF]], 0.5, "inf", [0], [0.0], [1]),
    ("minus-inf-winner", [[-INF, 0.0, 7.0]], 3e38, "inf", [0], [np.inf], [0]),
    ("no-winner", [[NAN, INF, NAN, INF]], 1.0, "inf", [-1], [0.0], [0]),
    # rule d0: the same scan from c[0]; "no winner" reads 0, a NaN at d = 0 is never replaced (m = NaN: kept)
    ("d0-plain", [[1.5, 3.0, 1.0, 1.01, 2.0]], 0.75, "d0", [2], [0.5], [1]),
    ("d0-all-inf", [[INF, INF, INF]], 1.0, "d0", [0], [0.0], [1]),
    ("d0-nan-first", [[NAN, 1.0, 2.0, 3.0]], 1.0, "d0", [0], [np.nan], [0]),
    ("d0-nan-later", [[4.0, NAN, 6.0, 5.0]], 1.5, "d0", [0], [1.0], [1]),
    ("d0-tie-keeps-first", [[1.0, 5.0, 1.0, 1.0]], 0.5, "d0", [0], [0.0], [1]),
]


def literal_arrays(name):
    for n, c, tau, rule, i, m, rej in LITERALS:
        if n == name:
            return (np.array(c, F), F(tau), rule, np.array(i, np.int32), np.array(m, F), np.array(rej, np.uint8))
    raise KeyError(name)


LITERAL_NAMES = [lit[0] for lit in LITERALS]
