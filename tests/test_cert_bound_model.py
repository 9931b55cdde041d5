"""CPU checks behind tests/test_gpu_certificate.py: the certificate's error bound against a NumPy model of
the row sweep's fast scores, and the adversarial inputs' own conditions against the oracle alone.

The model restates cv_row.hip's arithmetic: operands scaled by 2^RW_S and split into two fp16 parts
(rw_split), the three partial products accumulated in fp32 one product at a time -- the per-add model the
bound's derivation assumes -- with the eight small-term blocks of 16 channels (l h', h l' per block)
before the four leading ones (h h').  The MFMA's internal order is not documented; any order's error is
within the per-add model's bound, which is what RW_K is derived from.
"""
import numpy as np
import pytest

import cert_cases as cc


def rw_split_np(x, S):
    xs = x.astype(np.float32) * np.float32(2.0 ** S)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float32), l.astype(np.float32)


def fast_score_model(right, left, S):
    """[N, 64] x [N, 64] fp32 -> the kernel's fast scores, unscaled, as fp64."""
    ah, al = rw_split_np(right, S)
    bh, bl = rw_split_np(left, S)
    assert np.isfinite(ah).all() and np.isfinite(bh).all(), "model inputs must stay below the fp16 range guard"
    acc = np.zeros(right.shape[0], np.float32)
    for s in range(4):
        for x, y in ((al, bh), (ah, bl)):
            for c in range(16 * s, 16 * s + 16):
                acc = acc + x[:, c] * y[:, c]          # fp16 x fp16 is exact in fp32; one fp32 add each
    for c in range(64):
        acc = acc + ah[:, c] * bh[:, c]
    assert acc.dtype == np.float32
    return acc.astype(np.float64) / 4.0 ** S


def _with_norm(rng, v, lo, hi):
    """Rows of v rescaled to norms log-uniform in [2^lo, 2^hi]."""
    n = np.sqrt((v.astype(np.float64) ** 2).sum(-1, keepdims=True))
    return (v / np.maximum(n, 1e-300) * 2.0 ** rng.uniform(lo, hi, (v.shape[0], 1))).astype(np.float32)


def _families():
    rng = np.random.default_rng(5)
    N = 4000
    out = {}
    fl, fr, info = cc.build_case("loud-up-D192")
    ys, xs = np.nonzero(info["built"])
    out["builder pairs"] = (np.concatenate([fr[ys, xs - info["dA"][ys, xs]], fr[ys, xs - info["dB"][ys, xs]]]),
                            np.concatenate([fl[ys, xs], fl[ys, xs]]))
    a = np.zeros((N, 64), np.float32)
    b = np.zeros((N, 64), np.float32)
    i, j = rng.integers(0, 64, N), rng.integers(0, 64, N)
    j[: N // 2] = i[: N // 2]
    a[np.arange(N), i] = (2.0 ** rng.uniform(-20, 6.9, N) * rng.choice([-1, 1], N)).astype(np.float32)
    b[np.arange(N), j] = (2.0 ** rng.uniform(-20, 6.9, N) * rng.choice([-1, 1], N)).astype(np.float32)
    out["one-hot"] = (a, b)
    sgn = np.where(np.arange(64) % 2, -1.0, 1.0)
    g = np.abs(rng.standard_normal((N, 64)))
    out["sign-alternating"] = (_with_norm(rng, g * sgn, -8, 6.9), _with_norm(rng, np.abs(rng.standard_normal((N, 64))), -8, 6.9))
    out["all-positive"] = (_with_norm(rng, g + 0.5, -8, 6.9), _with_norm(rng, np.abs(rng.standard_normal((N, 64))) + 0.5, -8, 6.9))
    out["constant"] = (_with_norm(rng, np.ones((N, 64)), -8, 6.9), _with_norm(rng, np.ones((N, 64)), -8, 6.9))
    out["heavy-tailed"] = (_with_norm(rng, rng.standard_cauchy((N, 64)), -10, 6.9),
                           _with_norm(rng, rng.standard_cauchy((N, 64)), -10, 6.9))
    # parts in fp16's subnormal range: scaled elements below 2^-14, i.e. |x| < 2^-22 -- whole vectors, and
    # vectors with a few ordinary channels (whose low parts and small channels land there)
    out["fp16-subnormal"] = (_with_norm(rng, rng.standard_normal((N, 64)), -30, -17),
                             _with_norm(rng, rng.standard_normal((N, 64)), -30, -17))
    m = rng.standard_normal((N, 64)) * np.where(rng.random((N, 64)) < 0.05, 1.0, 2.0 ** -20)
    out["mixed subnormal"] = (_with_norm(rng, m, -12, 0), _with_norm(rng, rng.standard_normal((N, 64)), -24, 0))
    return out


def test_constants_are_read_from_the_sources():
    C = cc.cert_constants()
    assert C["RW_S"] == 8 and C["RW_ABS"] == pytest.approx(2.0 ** -30, rel=1e-6)
    assert C["RW_NMAX"] * 2.0 ** C["RW_S"] < 65504.0       # a certified operand's parts cannot overflow fp16
    assert 0 < C["RW_K"] < C["FX_K"] and C["FX_NORM_UP"] > 1.0


def test_constants_cover_the_derived_bounds():
    """RW_K and FX_K may not sink below the bounds their comments derive (the measured errors are far smaller,
    so no output would show it): split 3.001 * 2^-22, accumulation (64 * 1.002 + 0.13) * 2^-23, NumPy's
    pairwise order 10 * 2^-24 for the fp16 row sweep; (3 * 2^-16 + 192 * 2^-23) + 10 * 2^-24 for bf16."""
    C = cc.cert_constants()
    rw = 3.001 * 2.0 ** -22 + (64 * 1.002 + 0.13) * 2.0 ** -23 + 10 * 2.0 ** -24
    fx = 3 * 2.0 ** -16 + 192 * 2.0 ** -23 + 10 * 2.0 ** -24
    print(f"derived bounds: row sweep {rw:.3e} (RW_K {C['RW_K']:.1e}), bf16 {fx:.3e} (FX_K {C['FX_K']:.1e})")
    assert 8.9e-6 < rw < 9.0e-6 and 6.9e-5 < fx < 7.0e-5
    # the GPU tests' must-be-listed rule leans on these margins: err <= 0.6 RW_K, 0.7 FX_K of |a| |b|
    assert rw <= 0.6 * C["RW_K"] and fx <= 0.7 * C["FX_K"]
    # 64 elements, absolute error 2^-25 per scaled element, against each operand's 1-norm <= 8 |.|_2
    assert C["RW_ABS"] >= 8 * 2.0 ** -25 / 2.0 ** C["RW_S"] * (1 - 1e-6)


def test_fast_score_model_within_the_certified_bound():
    """|s_model - s_fp64| <= RW_K |a| |b| + RW_ABS (|a| + |b|) on every family; prints the worst ratios."""
    C = cc.cert_constants()
    S = int(C["RW_S"])
    worst_all = 0.0
    for name, (a, b) in _families().items():
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        na, nb = np.sqrt((a64 ** 2).sum(-1)), np.sqrt((b64 ** 2).sum(-1))
        assert na.max() < C["RW_NMAX"] and nb.max() < C["RW_NMAX"], name
        err = np.abs(fast_score_model(a, b, S) - (a64 * b64).sum(-1))
        bound = C["RW_K"] * na * nb + C["RW_ABS"] * (na + nb)
        ratio = (err / np.maximum(bound, 1e-300)).max()
        rel = (err / np.maximum(na * nb, 1e-300))[na * nb > 1e-6].max() if (na * nb > 1e-6).any() else 0.0
        print(f"bound model, {name}: worst err / bound = {ratio:.4f}, worst err / (|a| |b|) = {rel:.3e} "
              f"(derived 9.0e-6, RW_K {C['RW_K']:.1e})")
        assert np.all(err <= bound), (name, ratio)
        worst_all = max(worst_all, ratio)
    print(f"bound model: worst err / bound over all families = {worst_all:.4f}")


def test_builder_places_the_requested_near_tie():
    """fl[x]'s two candidate scores differ by 2 t relative to their mean (fp32 rounding of fl aside), whatever
    the candidates' norms."""
    fl, fr, info = cc.build_case("loud-up-D192")
    ys, xs = np.nonzero(info["built"])
    f = fl[ys, xs].astype(np.float64)
    sa = (f * fr[ys, xs - info["dA"][ys, xs]]).sum(-1)
    sb = (f * fr[ys, xs - info["dB"][ys, xs]]).sum(-1)
    t = info["t"][ys, xs]
    assert np.all(np.abs((sb - sa) / (sb + sa) - t) <= 64 * 2.0 ** -24)
    assert np.all(info["dA"][ys, xs] < info["dB"][ys, xs]) and np.all(info["dB"][ys, xs] <= np.minimum(xs, 191))
    # at most one loud pixel in any left pixel's disparity range
    cs = np.concatenate([np.zeros((cc.H, 1)), np.cumsum(info["loud"], 1)], 1)
    assert (cs[:, 192:] - cs[:, :-192]).max() == 1


@pytest.fixture(scope="module")
def built(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            fl, fr, info = cc.build_case(name)
            cache[name] = (fl, fr, info, oracle.compute_cost_volume(fl, fr, info["D"]))
        return cache[name]
    return get


@pytest.mark.parametrize("name", cc.SHARE_CASES)
def test_case_inputs_are_adversarial(built, name):
    """From the oracle's cost volume alone: enough pixels near eps, in the band a lost window norm would
    wrongly certify, and across the 256-disparity chunk boundary."""
    C = cc.cert_constants()
    fl, fr, info, cv = built(name)
    sh = cc.shares(cc.analyse(cv, fl, fr, info, C["RW_K"], C["RW_ABS"]), info)
    print(name, {k: (round(float(v), 3) if not isinstance(v, tuple) else v) for k, v in sh.items()})
    cc.check_shares(name, sh)
    assert np.isfinite(cv).all()


def test_power_of_two_scales_leave_the_exact_map_alone(built, oracle):
    """The scaled cases' premise: no exact cost under- or overflows at 2^-20 .. 2^12, so the oracle's map is
    the unscaled one (2^-40 is past that: products reach fp32's subnormals)."""
    fl, fr, info, cv = built("unit-D192-d0")
    ref = oracle.WTA1(cv)
    for e in cc.SCALES:
        sfl, sfr, _ = cc.build_case(f"scale-2^{e}")
        assert np.array_equal(sfl, fl * np.float32(2.0 ** e)) and np.array_equal(sfr, fr * np.float32(2.0 ** e))
        if e in cc.SCALE_INVARIANT:
            scv = oracle.compute_cost_volume(sfl, sfr, info["D"])
            assert np.array_equal(scv.astype(np.float64), cv.astype(np.float64) * 4.0 ** e), e
            assert np.array_equal(oracle.WTA1(scv), ref), e
