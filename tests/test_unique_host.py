"""CPU: the uniqueness check's restatement (tests/unique_literal.py) held to hand-written literals, the adversarial
builder's own conditions (tests/unique_cases.py) asserted from the oracle's volume alone, the integer-feature
case, the header's boundary and the argument checks that return before any launch."""
import ctypes

import numpy as np
import pytest

import cert_cases as cc
import unique_cases as uc
import unique_literal as ul


@pytest.mark.parametrize("name", ul.LITERAL_NAMES)
def test_restatement_matches_literals(name):
    """The restatement against expected maps written by hand from the text of the definition."""
    c, tau, rule, i, m, rej = ul.literal_arrays(name)
    u = ul.unique(c, tau, rule)
    assert np.array_equal(u["i"], i), (name, u["i"])
    assert u["m"].tobytes() == m.tobytes(), (name, u["m"])
    assert np.array_equal(u["reject"], rej), (name, u["reject"])
    want = np.where(rej == 1, np.float32(-1), i.astype(np.float32))
    assert u["disp"].tobytes() == want.tobytes(), (name, u["disp"])


def test_restatement_layout_and_range_helpers():
    """right_volume shears the left volume (fill where x' + d >= W); fused() offsets indices by d0 and scans
    [d0, D) only."""
    rng = np.random.default_rng(3)
    cv = rng.standard_normal((6, 2, 9)).astype(np.float32)
    R = ul.right_volume(cv)
    for d in range(6):
        for x in range(9):
            want = cv[d, :, x + d] if x + d < 9 else np.float32(-0.0)
            assert np.array_equal(R[d, :, x], np.broadcast_to(want, (2,)))
    assert np.signbit(R[5, 0, 8])
    f = ul.fused(cv, 0.5, d0=2)
    assert np.array_equal(f["argmin"], cv[2:].argmin(0) + 2)
    assert f["min_cost"].tobytes() == cv[2:].min(0).tobytes()
    # tau = 0 rejects nothing: the plain entry point's map
    f0 = ul.fused(cv, 0.0)
    assert not f0["reject"].any() and np.array_equal(f0["disp"], cv.argmin(0).astype(np.float32))


@pytest.fixture(scope="module")
def analysed(oracle):
    C = cc.cert_constants()
    cache = {}

    def get(name):
        if name not in cache:
            fl, fr, info = uc.build_case(name)
            cv = oracle.compute_cost_volume(fl, fr, info["D"])
            f = ul.fused(cv, info["tau"], info["d0"])
            cache[name] = (fl, fr, info, cv, f, uc.analyse(cv, fl, fr, info, C["RW_K"], C["RW_ABS"], f))
        return cache[name]
    return get


@pytest.mark.parametrize("name", uc.SHARE_CASES)
def test_builder_is_adversarial(analysed, name):
    """From the oracle's volume, for the reference alone: the planted pair is what the definition sees, and the
    shares of pixels near tau, on each side of it, with an adjacent plain runner-up, rejected and kept hold."""
    fl, fr, info, cv, f, an = analysed(name)
    b = info["built"]
    assert b.sum() >= 0.9 * (b.size - b.shape[0] * (info["d0"] + 2))
    # the planted winner and margin survive: the winner is dA and m = tau + t within the float32 rounding of the
    # features (|fl| <= ~3, 64 products: a few 1e-6) almost everywhere (noise may beat the planted pair rarely)
    hit = (f["argmin"] == info["dA"]) & (np.abs(an["m"] - (float(info["tau"]) + info["t"])) < 1e-5)
    assert hit[b].mean() >= 0.95, (name, hit[b].mean())
    sh = uc.shares(an, info)
    print(name, {k: round(float(v), 3) for k, v in sh.items()})
    uc.check_shares(name, sh)


def test_integer_features_sit_on_tau(oracle):
    """Entries 0..3: every dot product is exact, so margins are small integers; at tau = 2 some pixels sit at
    m == tau (kept) and some one step below (rejected)."""
    fl, fr = uc.integer_pair(np.random.default_rng(5), 4, 200)
    cv = oracle.compute_cost_volume(fl, fr, 32)
    assert np.array_equal(cv, np.round(cv))
    f = ul.fused(cv, 2.0)
    at, below = f["m"] == 2.0, f["m"] == 1.0
    assert at.any() and below.any(), (int(at.sum()), int(below.sum()))
    assert not f["reject"][at].any() and f["reject"][below].all()
    assert (f["disp"][below] == -1).all() and (f["disp"][at] == f["argmin"][at]).all()


def test_header_boundary():
    """include/sde_unique.h beside the other three: its two functions are declared, bound with the right types and
    exported; sde.h and the other headers keep what they had."""
    from ctypes import c_float, c_int, c_int64
    from ctypes import c_void_p as p

    from scenedepthestimation_amd import _lib
    declared = set(_lib.header_functions(prefix="sdu"))
    assert declared == set(_lib.UNIQUE_SIGNATURES) == {"sdu_wta_unique", "sdu_cv_wta_unique"}
    assert _lib.HEADER_NAMES["sdu"] == "sde_unique.h" and _lib.UNIQUE_CONSTANTS == {}
    want = {"sdu_wta_unique": (c_int, [p, c_int, c_int, c_int, c_int, c_int, c_float, p, p, p, p]),
            "sdu_cv_wta_unique": (c_int, [p, p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, p, p, p, p, c_int,
                                          p, c_int64, p])}
    assert _lib.UNIQUE_SIGNATURES == want
    for name, (res, args) in want.items():
        fn = getattr(_lib.lib, name)
        assert (fn.restype, list(fn.argtypes)) == (res, args), name
    with open(_lib.UNIQUE_HEADER) as fh:
        text = fh.read()
    for prefix in ("sde", "sdg", "sdf"):
        assert _lib.parse_header(text, prefix=prefix) == ({}, {})
    assert _lib.SDE_ABI_VERSION == 4 == _lib.lib.sde_abi_version()


BAD_TAUS = (-1.0, -1e-45, float("nan"), float("inf"), -float("inf"))


def test_argument_checks_return_before_any_launch():
    """A negative, NaN or infinite tau, null outputs and bad sizes are SDE_ERR_ARG; the pointers are never
    dereferenced (they are not device memory), so nothing was launched."""
    import torch

    from scenedepthestimation_amd import _lib
    if torch.cuda.is_available():
        # as tests/test_capi.py: host addresses are only safe while no device can be launched on; with a GPU the
        # same checks run on device pointers (tests/test_gpu_unique.py::test_bad_arguments_launch_nothing)
        pytest.skip("passes host addresses, which is only safe while no device can be launched on")
    lib, ERR = _lib.lib, _lib.SDE_ERR_ARG
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    f = ctypes.c_float
    DHW, HWD, INFR = _lib.SDE_LAYOUT_DHW, _lib.SDE_LAYOUT_HWD, _lib.SDE_WTA_INIT_INF
    for tau in BAD_TAUS:
        assert lib.sdu_wta_unique(a, 2, 2, 4, DHW, INFR, f(tau), a, a, a, None) == ERR, tau
        assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, 0, 4, _lib.SDE_SIDE_LEFT, f(tau), a, a, a, a, _lib.SDE_CV_EXACT,
                                     None, 0, None) == ERR, tau
    ok = f(0.5)
    assert lib.sdu_wta_unique(a, 2, 2, 4, HWD, INFR, ok, None, None, None, None) == ERR      # no output
    assert lib.sdu_wta_unique(None, 2, 2, 4, HWD, INFR, ok, a, a, a, None) == ERR
    assert lib.sdu_wta_unique(a, 0, 2, 4, HWD, INFR, ok, a, a, a, None) == ERR
    assert lib.sdu_wta_unique(a, 2, 2, 0, HWD, INFR, ok, a, a, a, None) == ERR
    assert lib.sdu_wta_unique(a, 2, 2, 4, 7, INFR, ok, a, a, a, None) == ERR                 # layout
    assert lib.sdu_wta_unique(a, 2, 2, 4, HWD, 9, ok, a, a, a, None) == ERR                  # rule
    L, EX, CE = _lib.SDE_SIDE_LEFT, _lib.SDE_CV_EXACT, _lib.SDE_CV_CERTIFIED
    assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, 0, 4, L, ok, None, None, None, None, EX, None, 0, None) == ERR
    assert lib.sdu_cv_wta_unique(None, a, 1, 1, 64, 0, 4, L, ok, a, a, a, a, EX, None, 0, None) == ERR
    assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, 4, 4, L, ok, a, a, a, a, EX, None, 0, None) == ERR     # d1 <= d0
    assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, -1, 4, L, ok, a, a, a, a, EX, None, 0, None) == ERR
    assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, 0, 4, 3, ok, a, a, a, a, EX, None, 0, None) == ERR     # side
    assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, 0, 4, L, ok, a, a, a, a, 5, None, 0, None) == ERR      # mode
    # certified mode needs the workspace sde_cv_wta needs
    assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, 0, 4, L, ok, a, a, a, a, CE, None, 0, None) == _lib.SDE_ERR_WORKSPACE
    assert lib.sdu_cv_wta_unique(a, a, 1, 1, 64, 0, 4, L, ok, a, a, a, a, CE, a, 16, None) == _lib.SDE_ERR_WORKSPACE


def test_host_layer_refuses_bad_margins():
    from scenedepthestimation_amd import local_method, match_single, ops
    for tau in BAD_TAUS + (1e39,):
        with pytest.raises(ValueError):
            ops.unique_tau(tau)
    assert ops.unique_tau(0) == 0.0 and ops.unique_tau(np.float32(0.1)) == float(np.float32(0.1))
    assert match_single.parse_args(["--unique", "0.25"]).unique == 0.25
    assert match_single.parse_args([]).unique is None and local_method.parse_args([]).unique is None
    with pytest.raises(SystemExit):
        match_single.parse_args(["--unique", "-1"])
    with pytest.raises(SystemExit):
        local_method.parse_args(["--unique", "nan"])
