"""Inputs of the SGM form tests, shared by test_sgm_cases_host.py (CPU: every builder's condition, asserted on the
oracle alone) and test_gpu_sgm_forms.py (sgm_scan_kernel's forms against the oracle).  numpy only.  Inputs are
built once per case and handed out read-only.

sgm_scan_kernel exists once per (DPL, load kind, form): DPL = ceil(D / 64) disparities per lane, full-D (D = 64 DPL
a compile-time constant), vector loads (DPL divides D) or scalar loads, and the forms A..G of csrc/sgm.hip.  PF is
the prefetch ring's depth and the block size of the fused WTA: 8 up to DPL 4, then 4.
"""
import functools

import numpy as np

KINDS = ("full", "vector", "scalar")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- which kernel a D reaches (launch_dpl and launch_form of csrc/sgm.hip, restated) --------------------------
def dpl_of(D):
    return (D + 63) // 64


def pf_of(D):
    return 8 if dpl_of(D) <= 4 else 4


def launch_cell(D):
    """(DPL, kind) of the kernels a call with this D launches."""
    k = dpl_of(D)
    if D == 64 * k:
        return k, "full"
    return k, "vector" if D % k == 0 else "scalar"


# every cell but (1, scalar): D % 1 == 0
REACHABLE_CELLS = frozenset((k, kind) for k in range(1, 9) for kind in KINDS) - {(1, "scalar")}


def form_ds(k):
    """Family 1's D values at DPL k: 64k (full-D), 64k - k and the smallest multiple of k above 64(k - 1) (vector
    loads, one invalid lane / nearly all lanes invalid), 64k - 1 and the smallest non-multiple above 64(k - 1)
    (scalar loads, one invalid disparity / nearly all)."""
    if k == 1:
        return (64, 63, 1, 2, 3, 5)
    lo = 64 * (k - 1)
    mult = next(d for d in range(lo + 1, 64 * k) if d % k == 0)
    non = next(d for d in range(lo + 1, 64 * k) if d % k != 0)
    return (64 * k, 64 * k - k, mult, 64 * k - 1, non)


# ---- volumes, penalty maps, seeds of S ------------------------------------------------------------------------
def mixed_costs(rng, H, W, D):
    """The mix of the older SGM tests: normal x 0.5, 10 % at 1.0 (the invalid voxels), some zeros of both signs."""
    cv = (rng.standard_normal((H, W, D)) * 0.5).astype(np.float32)
    cv[rng.random(cv.shape) < 0.10] = 1.0
    cv[rng.random(cv.shape) < 0.03] = 0.0
    cv[rng.random(cv.shape) < 0.03] = -0.0
    return cv


def seed_s(rng, H, W, D):
    """An accumulate input: nonzero normals (no zero of either sign)."""
    s = (rng.standard_normal((H, W, D)) * 0.25).astype(np.float32)
    s[s == 0] = 0.5
    return s


PENALTY_CLASSES = ("positive", "zeros", "neg_p1", "neg_p2", "neg_both", "extreme")


def penalty_map(rng, H, W, kind):
    """f32 [H, W, 16], random per pixel and channel, channels 0/1 (direction DU's) live.  Even channels are P1,
    odd ones P2.  positive: P1 in (0.1, 1.1), P2 in (0.5, 4.5); zeros: the same with 20 % exact zeros; neg_p1 /
    neg_p2 / neg_both: half of the even / odd / all channels' values negated; extreme: a third of the values 1e30,
    a third float32 subnormals."""
    pen = np.empty((H, W, 16), np.float32)
    pen[..., 0::2] = 0.1 + rng.random((H, W, 8))
    pen[..., 1::2] = 0.5 + 4.0 * rng.random((H, W, 8))
    flip = rng.random(pen.shape) < 0.5
    if kind == "zeros":
        pen[rng.random(pen.shape) < 0.2] = 0.0
    elif kind == "neg_p1":
        flip[..., 1::2] = False
        pen[flip] *= -1
    elif kind == "neg_p2":
        flip[..., 0::2] = False
        pen[flip] *= -1
    elif kind == "neg_both":
        pen[flip] *= -1
    elif kind == "extreme":
        u = rng.random(pen.shape)
        pen[u < 1 / 3] = 1e30
        sub = (u >= 1 / 3) & (u < 2 / 3)
        pen[sub] = (rng.integers(1, 1 << 23, pen.shape).astype(np.uint32).view(np.float32))[sub]
    else:
        assert kind == "positive"
    return pen


def zero_du(pen):
    """The map a call with the DU fold gets: channels 0/1 zero (the flag's contract)."""
    out = np.array(pen, copy=True)
    out[..., 0:2] = 0.0
    return out


def default_penalties(oracle, rng, H, W):
    """What sgm_penalties gives for a random image with runs of equal intensity: two values per channel, channels
    0/1 zero."""
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    img[rng.random((H, W)) < 0.3] = 128
    return oracle.sgm_penalties(img)


class Case:
    """Two image sides with different data: cost volumes, penalty maps, seeds of S (accumulate inputs)."""

    def __init__(self, cv, pen, S0, nonfinite=False):
        self.cv, self.pen, self.S0, self.nonfinite = cv, pen, S0, nonfinite
        _frozen(*cv, *pen, *S0)
        self.shape = cv[0].shape


# ---- family 1: the form matrix; family 4: general penalties ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix_case(H, W, D, kind="positive"):
    rng = np.random.default_rng([H, W, D, PENALTY_CLASSES.index(kind)])
    return Case([mixed_costs(rng, H, W, D) for _ in range(2)], [penalty_map(rng, H, W, kind) for _ in range(2)],
                [seed_s(rng, H, W, D) for _ in range(2)])


def ud_dropped_neighbour(cv, pen):
    """Direction UD from S = 0 as the fast recurrence states it, in float64 NumPy: the minimum over L'(d),
    L'(d-1) + P1, L'(d+1) + P1 and m' + P2 with the terms of the neighbours d = -1 and d = D dropped, where the
    reference takes L'(d) + P1.  Equal to the reference for P1 >= 0 only: what the negative-P1 cases must tell
    apart.  Finite inputs."""
    H, W, D = cv.shape
    S = np.zeros(cv.shape, np.float32)
    n = max(H - 1, 2)
    L = cv[0].astype(np.float64)
    S[0] = (0.0 + L).astype(np.float32)         # S = f32(0 + L): a -0.0 in L does not reach S
    for r in range(1, n):
        p1 = pen[r - 1, :, 2].astype(np.float64)[:, None]
        p2 = pen[r - 1, :, 3].astype(np.float64)[:, None]      # P2 read at the previous step
        m = L.min(axis=1, keepdims=True)
        b = np.minimum(L, m + p2)
        b[:, 1:] = np.minimum(b[:, 1:], L[:, :-1] + p1)
        b[:, :-1] = np.minimum(b[:, :-1], L[:, 1:] + p1)
        L = cv[r].astype(np.float64) + (b - m)
        S[r] = (0.0 + L).astype(np.float32)
    return S


# ---- family 2: block edges ------------------------------------------------------------------------------------
def block_edge_shapes(PF):
    """(H, W) with n = max(length - 1, 2) steps per line at 2, PF-1, PF, PF+1, 2PF-1, 2PF, 2PF+1 and 3PF+1: as H
    (vertical and diagonal lines, the fused WTA) crossed with W in {2, 3, H, 2H+1} (a restart every other step, a
    few wraps, one wrap, none), and as W with H = 3 (horizontal lines)."""
    ns = sorted({2, PF - 1, PF, PF + 1, 2 * PF - 1, 2 * PF, 2 * PF + 1, 3 * PF + 1})
    shapes = []
    for n in ns:
        H = n + 1
        shapes += [(H, W) for W in (2, 3, H, 2 * H + 1)]
    shapes += [(3, n + 1) for n in ns]
    return sorted(set(shapes))


def steps_of(length):
    return max(length - 1, 2)


@functools.lru_cache(maxsize=None)
def block_edge_case(oracle, H, W, D):
    rng = np.random.default_rng([H, W, D, 2])
    return Case([mixed_costs(rng, H, W, D) for _ in range(2)], [default_penalties(oracle, rng, H, W) for _ in range(2)],
                [seed_s(rng, H, W, D) for _ in range(2)])


# ---- family 3a: integer volumes (exact ties in S) -------------------------------------------------------------
def integer_penalties(H, W):
    pen = np.zeros((H, W, 16), np.float32)
    pen[..., 2::2] = 1.0
    pen[..., 3::2] = 2.0
    return pen


@functools.lru_cache(maxsize=None)
def integer_case(H, W, D):
    """Costs in {0, 1, 2}, P1 = 1 and P2 = 2 on channels 2..15, S seeded with integers in {0, 1}: every value of
    the recurrence is a small integer, so S ties exactly at many disparities."""
    rng = np.random.default_rng([H, W, D, 3])
    return Case([rng.integers(0, 3, (H, W, D)).astype(np.float32) for _ in range(2)],
                [integer_penalties(H, W) for _ in range(2)],
                [rng.integers(0, 2, (H, W, D)).astype(np.float32) for _ in range(2)])


def tie_share(S, D):
    """Share of the pixels whose minimum of S is attained at disparities owned by more than one lane."""
    k = dpl_of(D)
    at_min = S == S.min(axis=-1, keepdims=True)
    lanes = np.zeros(S.shape[:2] + (64,), bool)
    for d in range(D):
        lanes[..., d // k] |= at_min[..., d]
    return float((lanes.sum(axis=-1) > 1).mean())


# ---- family 3b: crafted rows of S under zero costs ------------------------------------------------------------
def wta_patterns(D):
    """[(name, row of D float32, first-min disparity under the reference's rule)]: a background of distinct values
    in (1, 2) with the named feature.  Pairs of equal minima straddle every boundary of the fused WTA: between two
    lanes, between two chunks of DPL PF disparities (one scanning lane's share), between two groups of 64 / PF
    parking lanes, between two DPP rows of 16 lanes, and the row's two ends."""
    k, PF = dpl_of(D), pf_of(D)
    rng = np.random.default_rng([D, 31])
    base = (1.0 + (1 + rng.permutation(D)) / (D + 1.0)).astype(np.float32)
    pats = []

    def add(name, edits, want):
        row = base.copy()
        for d, v in edits:
            row[d] = v
        pats.append((name, row, want))

    pairs = {"lane": (k - 1, k), "lane_far": (k * (D // k - 1) - 1, k * (D // k - 1)), "chunk": (k * PF - 1, k * PF),
             "group": (k * (64 // PF) - 1, k * (64 // PF)), "row": (16 * k - 1, 16 * k), "ends": (0, D - 1),
             "chunk_far": (k * PF - 1, D - 1), "mid_last": (D // 2, D - 1)}
    for name, (d1, d2) in pairs.items():
        if 0 <= d1 < d2 < D:
            add("tie_" + name, [(d1, 0.25), (d2, 0.25)], d1)
    add("all_inf", [(d, np.inf) for d in range(D)], 0)
    add("nan_at_0", [(0, np.nan), (D - 1, 0.25)], 0)
    add("min_last", [(D - 1, 0.25)], D - 1)
    add("neg_inf", [(D // 3, -np.inf), (D - 1, -np.inf)] if D > 3 else [(D - 1, -np.inf)], D // 3 if D > 3 else D - 1)
    if D >= 3:
        add("nan_then_min", [(D // 2 - 1, np.nan), (D // 2, 0.25), (D - 1, np.nan)], D // 2)
        add("inf_head", [(d, np.inf) for d in range(D - 1)], D - 1)
    return pats


@functools.lru_cache(maxsize=None)
def wta_pattern_case(oracle, H, W, D):
    """Zero costs, default penalties, S0 = one pattern per pixel in row-major rotation (W > the number of patterns:
    every pattern falls in row 0, which the last direction never visits, and in visited rows).  Returns the case
    and the expected disparities by the patterns' own closed form."""
    pats = wta_patterns(D)
    assert W > len(pats) and H >= 3
    rng = np.random.default_rng([H, W, D, 32])
    S0, want = [], []
    for side in range(2):
        s = np.empty((H, W, D), np.float32)
        w = np.empty((H, W), np.float32)
        for p in range(H * W):
            _, row, d = pats[(p + side) % len(pats)]
            s[p // W, p % W] = row
            w[p // W, p % W] = d
        S0.append(s)
        want.append(w)
    case = Case([np.zeros((H, W, D), np.float32) for _ in range(2)],
                [default_penalties(oracle, rng, H, W) for _ in range(2)], S0, nonfinite=True)
    return case, _frozen(*want)


# ---- family 5: signed zeros onto -0.0 -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signed_zero_case(oracle, H, W, D, mixed):
    """Costs from {-0.0, +0.0, |normal|}; S0 all -0.0, or (mixed) a random mix of both zeros; default penalties
    (channels 0/1 zero: direction DU runs on zero penalties, where zeros of both signs tie)."""
    rng = np.random.default_rng([H, W, D, 5, int(mixed)])
    cv, S0 = [], []
    for _ in range(2):
        c = np.abs(rng.standard_normal((H, W, D)) * 0.5).astype(np.float32)
        u = rng.random(c.shape)
        c[u < 0.35] = -0.0
        c[(u >= 0.35) & (u < 0.7)] = 0.0
        cv.append(c)
        s = np.full((H, W, D), -0.0, np.float32)
        if mixed:
            s[rng.random(s.shape) < 0.5] = 0.0
        S0.append(s)
    return Case(cv, [default_penalties(oracle, rng, H, W) for _ in range(2)], S0)


def neg_zeros(a):
    return int((np.asarray(a, np.float32).view(np.uint32) == 0x80000000).sum())


# ---- family 6: finite extremes --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extreme_case(oracle, H, W, D):
    """Per pixel one of: costs in +(1.7e38, 3.4e38), the same negated, float32 subnormals of both signs.  All
    finite, so every line stays on the fast path; S overflows float32 to +-inf from the second pass on at the huge
    pixels, and stays subnormal at the others (next to a huge pixel, min - m' is exactly 0).  S0 holds subnormals."""
    rng = np.random.default_rng([H, W, D, 6])
    cv, S0 = [], []
    for _ in range(2):
        sub = rng.integers(1, 1 << 23, (H, W, D)).astype(np.uint32)
        sub |= (rng.integers(0, 2, (H, W, D)).astype(np.uint32) << 31)
        c = sub.view(np.float32).copy()
        cls = rng.integers(0, 3, (H, W))
        huge = (np.float32(1.7e38) * (1 + rng.random((H, W, D)))).astype(np.float32)
        c[cls == 0] = huge[cls == 0]
        c[cls == 1] = -huge[cls == 1]
        assert np.isfinite(c).all()
        cv.append(c)
        S0.append(rng.integers(1, 1 << 22, (H, W, D)).astype(np.uint32).view(np.float32).copy())
    return Case(cv, [default_penalties(oracle, rng, H, W) for _ in range(2)], S0)


def subnormals(a):
    a = np.abs(np.asarray(a, np.float32))
    return int(((a > 0) & (a < np.finfo(np.float32).tiny)).sum())
