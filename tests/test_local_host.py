"""CPU-side checks of the local matcher (SAD+SSD, rank, census): the NumPy restatement's check values and the
agreement of its loop and vectorised forms, the six entry points' argument validation through the C ABI, the ops'
refusal of CPU tensors and the CLI parser."""
import ctypes

import numpy as np
import pytest

import local_literal as ll


def images(rng, H, W, hi=256):
    return rng.integers(0, hi, (H, W), dtype=np.uint8), rng.integers(0, hi, (H, W), dtype=np.uint8)


def test_invalid_is_the_float32_of_the_reference_literal():
    from scenedepthestimation_amd import _lib
    assert np.float32(999999999999).view(np.uint32) == 0x5368d4a5
    assert float(np.float32(999999999999)) == 999999995904.0 == _lib.SDE_LOCAL_INVALID
    assert ll.INVALID.view(np.uint32) == 0x5368d4a5
    import re
    with open(_lib.os.path.join(_lib.INCLUDE, "sde.h")) as fh:
        text = fh.read()
    assert float(re.search(r"#define SDE_LOCAL_INVALID ([0-9.]+)f", text).group(1)) == _lib.SDE_LOCAL_INVALID
    assert int(re.search(r"#define SDE_LOCAL_MAX_RADIUS (\d+)", text).group(1)) == _lib.SDE_LOCAL_MAX_RADIUS == 32


def test_census_check_values():
    img = np.zeros((7, 9), np.uint8)
    img[0, 0] = 1
    for fn in (ll.census_loop, ll.census):
        assert fn(img)[3, 4] == 0x40000                      # the first bit appended is the most significant
        assert fn(np.ascontiguousarray(img[::-1, ::-1]))[3, 4] == 0
    # not symmetric under a horizontal flip
    rng = np.random.default_rng(2)
    a, _ = images(rng, 9, 23)
    assert not np.array_equal(ll.census(a), ll.census(np.ascontiguousarray(a[:, ::-1]))[:, ::-1])
    assert ll.census(a).max() < 1 << 19


def test_rank_of_a_constant_image_is_49():
    for fn in (ll.rank_loop, ll.rank):
        assert (fn(np.full((5, 8), 7, np.uint8)) == 49).all()        # corners included: outside reads 0
    assert (ll.rank(np.zeros((4, 4), np.uint8)) == 49).all()


def test_vectorised_forms_equal_loop_forms():
    rng = np.random.default_rng(5)
    H, W, D = 9, 23, 8
    a, b = images(rng, H, W)
    assert np.array_equal(ll.census(a), ll.census_loop(a))
    assert np.array_equal(ll.rank(a), ll.rank_loop(a))
    r = ll.rank(a)
    assert r.min() >= 1 and r.max() <= 49
    cl, cr = ll.census(a), ll.census(b)
    for got, want in zip(ll.census_cost(cl, cr, D), ll.census_cost_loop(cl, cr, D)):
        assert got.tobytes() == want.tobytes()
    for k in (0, 2, 7):
        assert np.array_equal(ll.ad_sums(a, b, D, k), ll.ad_sums_loop(a, b, D, k)), k
        assert ll.ad_cost(a, b, D, k).tobytes() == ll.ad_cost_loop(a, b, D, k).tobytes()
    # D > W for the census cost
    for got, want in zip(ll.census_cost(cl[:2, :5], cr[:2, :5], 9), ll.census_cost_loop(cl[:2, :5], cr[:2, :5], 9)):
        assert got.tobytes() == want.tobytes()


def test_right_volume_is_the_shear_of_the_left():
    rng = np.random.default_rng(6)
    a, b = images(rng, 4, 19)
    L, R = ll.census_cost(ll.census(a), ll.census(b), 8)
    H, W, D = L.shape
    n = 0
    for x in range(W):
        for d in range(D):
            if x + d < W:
                assert np.array_equal(R[:, x, d], L[:, x + d, d])
                n += 1
            else:
                assert (R[:, x, d] == ll.INVALID).all()
    assert n > 0 and (L[:, 0, 1:] == ll.INVALID).all()


def test_first_minimum_wta_equals_argmin():
    rng = np.random.default_rng(7)
    cl = rng.integers(0, 1 << 19, (6, 40), dtype=np.uint32)
    cr = rng.integers(0, 1 << 19, (6, 40), dtype=np.uint32)
    for vol in ll.census_cost(cl, cr, 16):
        assert ll.tie_share(vol) > 0.1                      # ties are common: the first-minimum rule matters
        for got, want in zip(ll.wta(vol), ll.wta_loop(vol)):
            assert got.tobytes() == want.tobytes()
        assert (ll.wta(vol)[1] < ll.INVALID).all()          # d = 0 is always valid


def test_argument_validation_without_gpu():
    """Every refusal comes from the argument checks (SDE_ERR_ARG, before any launch).  The accepted shape is
    launched on real buffers where a GPU is present; without one the launch itself fails (not SDE_ERR_ARG)."""
    import torch

    from scenedepthestimation_amd import _lib
    lib = _lib.lib
    ERR, N = -1, None
    inv = ctypes.c_float(_lib.SDE_LOCAL_INVALID)
    D, k = 8, 2
    assert lib.sde_ad_wta(1, 2, 3, D + 2 * k - 1, D, k, 3, N, N) == ERR          # W = D + 2k - 1
    assert lib.sde_ad_cost(1, 2, 3, D + 2 * k - 1, D, k, inv, 3, N) == ERR
    W = D + 2 * k
    if torch.cuda.is_available():
        il = torch.zeros((3, W), dtype=torch.uint8, device="cuda")
        out = torch.empty((3, W), dtype=torch.float32, device="cuda")
        assert lib.sde_ad_wta(il.data_ptr(), il.data_ptr(), 3, W, D, k, out.data_ptr(), N, N) == 0
        torch.cuda.synchronize()
        assert (out == 0).all()
    else:
        assert lib.sde_ad_wta(1, 2, 3, W, D, k, 3, N, N) not in (ERR, 0)        # W = D + 2k passes the checks
    assert lib.sde_ad_wta(1, 2, 3, 200, D, 33, 3, N, N) == ERR                   # radius > SDE_LOCAL_MAX_RADIUS
    assert lib.sde_ad_wta(1, 2, 3, 200, D, -1, 3, N, N) == ERR
    assert lib.sde_ad_wta(1, 2, 3, 2000, 0, k, 3, N, N) == ERR                   # D = 0
    assert lib.sde_ad_wta(1, 2, 3, 2000, 513, k, 3, N, N) == ERR                 # D = 513
    assert lib.sde_ad_wta(1, 2, 0, 200, D, k, 3, N, N) == ERR                    # H = 0
    assert lib.sde_ad_wta(N, 2, 3, 200, D, k, 3, N, N) == ERR
    assert lib.sde_ad_wta(1, 2, 3, 200, D, k, N, 3, N) == ERR                    # min without disp
    assert lib.sde_ad_cost(1, 2, 3, 200, D, 33, inv, 3, N) == ERR
    assert lib.sde_ad_cost(1, 2, 3, 2000, 513, k, inv, 3, N) == ERR
    assert lib.sde_ad_cost(1, 2, 3, 200, D, k, inv, N, N) == ERR
    for fn in (lib.sde_census_transform, lib.sde_rank_transform):
        assert fn(1, 0, 4, 4, 2, N) == ERR                                       # nimg = 0
        assert fn(1, 2, 0, 4, 2, N) == ERR
        assert fn(1, 2, 4, 0, 2, N) == ERR
        assert fn(N, 2, 4, 4, 2, N) == ERR and fn(1, 2, 4, 4, N, N) == ERR
    assert lib.sde_census_wta(1, 2, 4, 4, 4, N, N, N, N, N) == ERR               # both disp NULL
    assert lib.sde_census_wta(1, 2, 4, 4, 4, N, 3, N, 4, N) == ERR               # mins alone are no request
    assert lib.sde_census_wta(1, 2, 4, 4, 4, 3, N, N, 4, N) == ERR               # min_r without disp_r
    assert lib.sde_census_wta(1, 2, 4, 4, 0, 3, N, N, N, N) == ERR
    assert lib.sde_census_wta(1, 2, 4, 4, 513, 3, N, N, N, N) == ERR
    assert lib.sde_census_wta(N, 2, 4, 4, 4, 3, N, N, N, N) == ERR
    assert lib.sde_census_cost(1, 2, 4, 4, 4, inv, N, N, N) == ERR               # both outputs NULL
    assert lib.sde_census_cost(1, 2, 4, 4, 0, inv, 3, N, N) == ERR
    assert lib.sde_census_cost(1, 2, 4, 4, 513, inv, 3, N, N) == ERR
    assert lib.sde_census_cost(1, N, 4, 4, 4, inv, 3, N, N) == ERR
    assert lib.sde_abi_version() == 4


def test_header_declares_and_binding_covers_local_matcher():
    from scenedepthestimation_amd import _lib
    declared = set(_lib.header_functions())
    for name in ("sde_census_transform", "sde_rank_transform", "sde_census_cost", "sde_census_wta", "sde_ad_cost",
                 "sde_ad_wta"):
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_ops_refuse_cpu_tensors():
    import torch

    from scenedepthestimation_amd import ops
    u8 = torch.zeros((4, 30), dtype=torch.uint8)
    i32 = torch.zeros((4, 30), dtype=torch.int32)
    calls = [lambda: ops.census_transform(u8), lambda: ops.rank_transform(u8),
             lambda: ops.census_cost(i32, i32, 4), lambda: ops.census_wta(i32, i32, 4),
             lambda: ops.ad_cost(u8, u8, 4, 2), lambda: ops.ad_wta(u8, u8, 4, 2)]
    for call in calls:
        with pytest.raises(ValueError, match="GPU"):
            call()


def test_cli_parser(capsys):
    from scenedepthestimation_amd import local_method
    a = local_method.parse_args([])
    assert (a.kernel, a.method, a.ndisp, a.lr_check, a.image_dir, a.out_dir, a.num) == \
        (5, "ad", 200, False, "./eval", "./result/SAD", 5)
    a = local_method.parse_args(["-k", "3", "--method", "census", "--lr-check", "-n", "1"])
    assert (a.kernel, a.method, a.lr_check, a.num) == (3, "census", True, 1)
    for method in ("ad", "rank"):
        with pytest.raises(SystemExit) as e:
            local_method.parse_args(["--method", method, "--lr-check"])
        assert e.value.code == 2
        assert "--lr-check needs --method census" in capsys.readouterr().err
    assert "W >= D + 2k" in local_method.window_rule(100, 200, 5)
