"""CPU: the filter header's boundary (include/sde_filter.h beside the other two), sdf_speckle's argument checks, the
flood-fill restatement against hand-drawn pictures and against a second, independently written formulation, the
non-vacuity of the GPU tests' cases, and the command lines' parser errors.  No GPU needed, and safe with one: every
library call here is refused by the argument checks, before any launch, and the pointers it passes are real host
arrays that are never followed."""
import ctypes
import subprocess

import numpy as np
import pytest

import speckle_cases as sc
import speckle_literal as sl

CASES = {c["name"]: c for c in sc.all_cases()}


# ----------------------------------------------------------------------------
# (a) the third header
# ----------------------------------------------------------------------------
def test_filter_header_binding_and_exports():
    from ctypes import c_float, c_int, c_int64
    from ctypes import c_void_p as p

    from scenedepthestimation_amd import _lib
    from scenedepthestimation_amd._build import LIB
    declared = set(_lib.header_functions(prefix="sdf"))
    assert declared == set(_lib.FILTER_SIGNATURES) == {"sdf_speckle_workspace_bytes", "sdf_speckle"}
    assert declared == set(_lib.header_functions(_lib.FILTER_HEADER, prefix="sdf"))
    with open(_lib.FILTER_HEADER) as fh:
        text = fh.read()
    assert _lib.parse_header(text, prefix="sdf") == (_lib.FILTER_SIGNATURES, _lib.FILTER_CONSTANTS)
    want = {"sdf_speckle_workspace_bytes": (c_int64, [c_int, c_int]),
            "sdf_speckle": (c_int, [p, c_int, c_int, c_int, c_float, c_float, p, p, p, p, c_int64, p])}
    assert _lib.FILTER_SIGNATURES == want
    for name, sig in want.items():
        fn = getattr(_lib.lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    assert _lib.FILTER_CONSTANTS == {}
    assert _lib.HEADER_NAMES["sdf"] == "sde_filter.h"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {s for s in exported if s.startswith("sdf_")} == declared


def test_other_headers_are_unchanged_by_the_third_one():
    from scenedepthestimation_amd import _lib
    with open(_lib.HEADER) as fh:
        text = fh.read()
    assert _lib.parse_header(text) == (_lib.SIGNATURES, _lib.CONSTANTS)
    assert len(_lib.SIGNATURES) == 60 and _lib.SDE_ABI_VERSION == 4 == _lib.lib.sde_abi_version()
    assert len(_lib.GEOM_SIGNATURES) == 3
    for sigs in (_lib.SIGNATURES, _lib.GEOM_SIGNATURES):
        assert not any(k.startswith("sdf_") for k in sigs)
    with open(_lib.FILTER_HEADER) as fh:
        filt = fh.read()
    assert _lib.parse_header(filt) == ({}, {}) and _lib.parse_header(filt, prefix="sdg") == ({}, {})
    assert "sdf_" not in text and "SDF_" not in text
    with pytest.raises(TypeError, match="sde_filter.h"):
        _lib.parse_header("int sdf_f(long n);", prefix="sdf")


# ----------------------------------------------------------------------------
# (b) argument checks: every call below is refused before any launch
# ----------------------------------------------------------------------------
def test_speckle_argument_checks():
    from scenedepthestimation_amd import _lib
    lib, ARG, WS, N = _lib.lib, _lib.SDE_ERR_ARG, _lib.SDE_ERR_WORKSPACE, None
    # real host arrays stand in for the device pointers (never followed: each call returns before a launch)
    H, W = 4, 6
    disp, out = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    mask, sizes = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int32)
    ws = np.zeros(H * W * 8 + 8, np.uint8)
    need = lib.sdf_speckle_workspace_bytes(H, W)
    assert need == H * W * 8 <= ws.nbytes and ws.ctypes.data % 4 == 0
    f = ctypes.c_float

    def call(d=disp.ctypes.data, h=H, w=W, max_size=3, max_diff=1.0, fill=-1.0, o=out.ctypes.data,
             m=mask.ctypes.data, s=sizes.ctypes.data, work=ws.ctypes.data, nbytes=None):
        nbytes = need if nbytes is None else nbytes
        return lib.sdf_speckle(d, h, w, max_size, f(max_diff), f(fill), o, m, s, work, nbytes, N)

    assert call(d=N) == ARG and call(o=N) == ARG and call(work=N) == ARG
    assert call(h=0) == ARG and call(w=0) == ARG and call(h=-3) == ARG and call(w=-1) == ARG
    assert call(h=1 << 16, w=1 << 15, nbytes=1 << 62) == ARG            # 2^31 pixels
    assert call(h=46341, w=46341, nbytes=1 << 62) == ARG                # 2147488281 > 2^31 - 1
    assert call(max_size=-1) == ARG
    assert call(max_diff=-0.5) == ARG and call(max_diff=float("nan")) == ARG and call(max_diff=float("inf")) == ARG
    assert call(max_diff=-float("inf")) == ARG
    assert call(work=ws.ctypes.data + 1) == ARG and call(work=ws.ctypes.data + 2) == ARG
    assert call(nbytes=need - 1) == WS and call(nbytes=0) == WS and call(nbytes=-8) == WS
    # the argument checks come first: a short workspace with a bad argument is a bad argument
    assert call(nbytes=0, max_size=-1) == ARG
    # 2^31 - 1 pixels is a legal shape: its workspace is the first thing found wanting
    assert lib.sdf_speckle_workspace_bytes(1, 2147483647) == 8 * 2147483647
    assert call(h=1, w=2147483647, nbytes=need) == WS
    assert call(h=2147483647, w=1, nbytes=8 * 2147483647 - 1) == WS
    for h, w in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15)):
        assert lib.sdf_speckle_workspace_bytes(h, w) == 0
    assert not disp.any() and not out.any() and not mask.any() and not sizes.any() and not ws.any()


def test_speckle_ops_refuse_cpu_tensors_and_bad_options():
    import torch

    from scenedepthestimation_amd import ops
    from scenedepthestimation_amd.pipeline import SpeckleStage
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        ops.speckle(torch.zeros((3,)), 2)
    with pytest.raises(ValueError, match="max_size"):
        SpeckleStage(4, 4, "cpu", -1)
    with pytest.raises(ValueError, match="max_diff"):
        SpeckleStage(4, 4, "cpu", 3, float("inf"))
    with pytest.raises(ValueError, match="max_diff"):
        SpeckleStage.make(4, 4, "cpu", (3, -1.0))
    assert SpeckleStage.make(4, 4, "cpu", None) is None
    stage = SpeckleStage.make(4, 4, "cpu", (3, 0.5))
    assert (stage.max_size, stage.max_diff, stage.mask, stage.sizes, stage.ws) == (3, 0.5, None, None, None)
    assert SpeckleStage.make(4, 4, "cpu", stage) is stage


# ----------------------------------------------------------------------------
# (c) the restatement against hand-drawn pictures
# ----------------------------------------------------------------------------
def picture(rows, values):
    """Rows of characters -> float32 map through `values` (a dict from character to number)."""
    return np.array([[values[ch] for ch in row] for row in rows], np.float32)


def test_literal_hand_drawn_regions():
    V = {".": -1.0, "a": 5.0, "b": 5.5, "c": 9.0, "n": np.nan, "z": -0.0, "o": 0.0, "i": np.inf}
    d = picture(["aa.c.",
                 "a.bc.",
                 "..b.z",
                 "cn.ao",
                 "c.iaa"], V)
    # counted by hand: the three a at the top left; b above b (they touch no a, and c is 3.5 away); c above c in
    # column 3; -0.0 above 0.0 (0 apart; the a beside and below the 0.0 are 5 away); c above c in column 0; the
    # three a at the bottom right.  NaN, inf and -1 belong to nothing.
    want = np.array([[3, 3, 0, 2, 0],
                     [3, 0, 2, 2, 0],
                     [0, 0, 2, 0, 2],
                     [2, 0, 0, 3, 2],
                     [2, 0, 0, 3, 3]], np.int32)
    out, mask, sizes = sl.speckle(d, 2, 1.0, -1.0)
    assert (sizes == want).all()
    assert (mask == ((want > 0) & (want <= 2))).all()
    keep = mask == 0
    assert out[keep].tobytes() == d[keep].tobytes() and (out[mask == 1] == -1.0).all()
    # max_size = 0: a copy, bit for bit (the NaN and -0.0 included)
    out0, mask0, sizes0 = sl.speckle(d, 0, 1.0, 7.0)
    assert out0.tobytes() == d.tobytes() and not mask0.any() and (sizes0 == want).all()
    # max_size = 3: every valid pixel goes, invalid ones stay as they are
    out3, mask3, _ = sl.speckle(d, 3, 1.0, 7.0)
    assert (mask3 == (want > 0)).all() and (out3[want > 0] == 7.0).all()
    assert out3[want == 0].tobytes() == d[want == 0].tobytes()


def test_literal_ramp_and_threshold():
    up = np.nextafter(np.float32(9.0), np.float32(np.inf))
    d = np.array([[8.0, 9.0, -1.0, 8.0, up, -1.0, 0.0, 0.75, 1.5, 2.25, 3.0]], np.float32)
    _, _, sizes = sl.speckle(d, 0, 1.0, -1.0)
    assert sizes.tolist() == [[2, 2, 0, 1, 1, 0, 5, 5, 5, 5, 5]]
    # transitive closure: the ends of the ramp differ by 3
    _, _, sizes = sl.speckle(d, 0, 0.5, -1.0)
    assert sizes.tolist() == [[1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1]]
    # one pass: the fill takes no part, even when it would link what is left
    d = np.array([[1.0, 2.0, 2.0, 3.0, 5.0, 5.0, 5.0]], np.float32)
    out, mask, sizes = sl.speckle(d, 3, 0.0, 5.0)
    assert sizes.tolist() == [[1, 2, 2, 1, 3, 3, 3]] and mask.all() and (out == 5.0).all()
    out, mask, _ = sl.speckle(d, 2, 0.0, 5.0)
    assert mask.tolist() == [[1, 1, 1, 1, 0, 0, 0]] and (out == 5.0).all()


def test_literal_nan_payload_and_negative_zero_survive():
    d = np.array([[sc.NAN_PAYLOAD, -0.0, 0.0], [sc.NEG_NAN, -np.inf, np.inf]], np.float32)
    out, mask, sizes = sl.speckle(d, 1, 1.0, np.nan)
    assert sizes.tolist() == [[0, 2, 2], [0, 0, 0]] and not mask.any()
    assert out.tobytes() == d.tobytes()
    assert out.view(np.uint32)[0, 0] == 0x7FC12345 and out.view(np.uint32)[0, 1] == 0x80000000


# ----------------------------------------------------------------------------
# (d) a second formulation: union-find over the list of links (shares nothing with the flood fill)
# ----------------------------------------------------------------------------
def sizes_by_union_find(disp, max_diff):
    d = np.asarray(disp, np.float32)
    H, W = d.shape
    ok = np.isfinite(d) & ~np.signbit(np.where(d == 0, np.float32(0.0), d))    # finite, and >= 0 with -0.0 in
    with np.errstate(invalid="ignore", over="ignore"):
        right = ok[:, :-1] & ok[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= np.float32(max_diff))
        down = ok[:-1, :] & ok[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= np.float32(max_diff))
    idx = np.arange(H * W).reshape(H, W)
    links = np.concatenate([np.stack([idx[:, :-1][right], idx[:, 1:][right]], 1),
                            np.stack([idx[:-1, :][down], idx[1:, :][down]], 1)])
    parent = list(range(H * W))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in links.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(a) for a in range(H * W)])
    counts = np.bincount(roots[ok.reshape(-1)], minlength=H * W)
    return np.where(ok, counts[roots].reshape(H, W), 0).astype(np.int32)


@pytest.mark.parametrize("name", ["random", "random_subpixel", "random_small", "random_narrow", "invalid_kinds",
                                  "threshold", "threshold_tenth", "spiral", "rings"])
def test_literal_against_union_find(name):
    c = CASES[name]
    _, _, sizes = sc.expected(c)
    assert (sizes == sizes_by_union_find(c["disp"], c["max_diff"])).all()


# ----------------------------------------------------------------------------
# (e) the cases say what they claim
# ----------------------------------------------------------------------------
def spans(sizes, mask):
    """Largest height and width of the bounding box of a kept region (by its size: regions of equal size are taken
    together, which can only widen the box of cases whose kept regions have distinct sizes)."""
    best = (0, 0)
    kept = (sizes > 0) & (mask == 0)
    for n in np.unique(sizes[kept]):
        ys, xs = np.nonzero(kept & (sizes == n))
        box = (ys.max() - ys.min() + 1, xs.max() - xs.min() + 1)
        if min(box) > min(best):
            best = box
    return best


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["full"]))
def test_cases_are_not_vacuous(name):
    c = CASES[name]
    out, mask, sizes = sc.expected(c)
    valid = sizes > 0
    assert (mask == 1).any(), "nothing is removed"
    assert (valid & (mask == 0)).any(), "nothing is kept"
    assert (~valid).any(), "no invalid pixel"
    h, w = spans(sizes, mask)
    assert h > 64 and w > 64, f"no kept region spans more than 64 pixels each way ({h} x {w})"
    assert max(c["disp"].shape) <= 200


def test_case_list_covers_the_shapes():
    shapes = {c["disp"].shape for c in CASES.values()}
    assert {(150, 199), (70, 131), (1, 1), (1, 199), (150, 1), (37, 19)} <= shapes
    fills = [c["fill"] for c in CASES.values()]
    assert -1.0 in fills and 7.0 in fills and any(np.isnan(f) for f in fills)
    assert any(c["max_size"] == 0 for c in CASES.values())
    assert len(CASES) == len(sc.all_cases())               # names are unique


def is_chain(path):
    cells = set(path)
    for k, (y, x) in enumerate(path):
        near = sum((y + dy, x + dx) in cells for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)))
        if near != (1 if k in (0, len(path) - 1) else 2):
            return False
    return len(cells) == len(path)


def test_spiral_and_serpentine_are_single_chains():
    """One-pixel-wide paths that touch themselves nowhere: one region whose only route is the whole path."""
    for name, path in (("spiral", sc.spiral_path(*sc.BIG)), ("serpentine", sc.serpentine_path(*sc.BIG))):
        assert is_chain(path), name
        assert len(path) > 14000
        _, _, sizes = sc.expected(CASES[name])
        on = np.zeros(sc.BIG, bool)
        on[tuple(np.array(path).T)] = True
        assert (sizes[on] == len(path)).all(), name
        # it crosses every 16-aligned seam of the image, both ways
        ys, xs = np.array(path).T
        for n, seen in ((sc.BIG[0], set(ys.tolist())), (sc.BIG[1], set(xs.tolist()))):
            assert all(k in seen and k - 1 in seen for k in range(16, n, 16)), name


def test_structured_cases_hand_counts():
    _, _, s = sc.expected(CASES["u_through_neighbour"])
    assert s[66, 66] == s[66, 70] == 75 + 75 + 3 and s[66, 74] == 75 and s[10, 10] == 110
    # in the tile of rows and columns 64..79 the two arms touch nothing that joins them
    d = CASES["u_through_neighbour"]["disp"][64:80, 64:80]
    tile_sizes = sl.region_sizes(d, 1.0)
    assert tile_sizes[2, 2] == tile_sizes[2, 6] == 14
    out, mask, s = sc.expected(CASES["blobs_at_corners"])
    assert s[64, 64] == 12 and mask[64, 64] == 1 and s[64, 128] == 13 and mask[64, 128] == 0
    assert s[128, 64] == 13 and mask[128, 64] == 0 and s[128, 128] == 12 and mask[128, 128] == 1
    assert s[0, 0] == 12 and mask[0, 0] == 1 and s[-1, -1] == 13 and mask[-1, -1] == 0
    assert s[0, -1] == 12 and mask[0, -1] == 1 and s[-1, 0] == 13 and mask[-1, 0] == 0
    _, mask, s = sc.expected(CASES["comb_rows"])
    assert s[0, 0] == s[99, 198] == s[64, 1] and s[0, 0] > 5000 and mask[0, 0] == 0
    assert s[101, 0] == 49 and mask[101, 0] == 1
    _, mask, s = sc.expected(CASES["comb_cols"])
    assert s[0, 0] == s[148, 179] == s[1, 63] and mask[0, 0] == 0 and s[0, 181] == 18 and mask[0, 181] == 1
    _, mask, s = sc.expected(CASES["invalid_kinds"])
    assert s[31, 6] == 12 and s[30, 5] == 12 and mask[30, 5] == 1 and s[104, 114] == s[100, 110]
    _, mask, s = sc.expected(CASES["threshold"])
    assert s[0, :9].tolist() == [2, 2, 0, 1, 1, 0, 3, 3, 3] and s[2:4, 0].tolist() == [2, 2]
    assert s[2:4, 3].tolist() == [1, 1] and (s[2, 60:67] == 7).all() and s[4, 10:13].tolist() == [2, 2, 1]
    _, mask, s = sc.expected(CASES["constant_kept"])
    assert (s == 70 * 131).all() and not mask.any()
    assert sc.expected(CASES["constant_gone"])[1].all()
    assert sc.expected(CASES["checkerboard_gone"])[1].all() and not sc.expected(CASES["checkerboard_kept"])[1].any()
    assert (sc.expected(CASES["ramp_1xW"])[2] == 199).all()
    assert sc.expected(CASES["ramp_Hx1"])[2][:, 0].tolist()[:52] == [40] * 40 + [0] + [9] * 9 + [0, 69]


# ----------------------------------------------------------------------------
# (f) the command lines
# ----------------------------------------------------------------------------
def test_cli_speckle_flags(capsys):
    from scenedepthestimation_amd import local_method, match, match_single
    assert match_single.parse_args([]).speckle is None
    assert match_single.parse_args(["--speckle-size", "40"]).speckle == (40, 1.0)
    assert match_single.parse_args(["--speckle-size", "40", "--speckle-range", "2.5"], ui=True).speckle == (40, 2.5)
    assert local_method.parse_args(["--speckle-size", "9", "--speckle-range", "0"]).speckle == (9, 0.0)
    assert local_method.parse_args([]).speckle is None
    args = match.build_parser().parse_args(["--speckle-size", "7"])
    assert local_method.speckle_option(match.build_parser(), args) == (7, 1.0)
    for parse in (match_single.parse_args, local_method.parse_args, match.main):
        for argv, msg in ((["--speckle-range", "2"], "needs --speckle-size"),
                          (["--speckle-size", "-1"], ">= 0"),
                          (["--speckle-size", "5", "--speckle-range", "-1"], "finite"),
                          (["--speckle-size", "5", "--speckle-range", "nan"], "finite")):
            with pytest.raises(SystemExit) as e:
                parse(argv)
            assert e.value.code == 2
            assert msg in capsys.readouterr().err
