"""GPU: sgm_scan_kernel at every lane width, load kind and form, at the fused WTA's block edges, on ties, under
general penalty maps, on signed zeros and at the ends of float32 -- against the C oracle (oracle/sde_oracle.c, pinned
to tests/sgm_literal.py by test_oracle_sgm.py and test_sgm_cases_host.py, which also asserts every case's
condition).  S is compared by bytes, disparities exactly; outputs that a call overwrites arrive filled with NaN or
0xA5 bytes, accumulate inputs are seeded data.

The calls of one case (Calls.run), each on both image sides with different data:
    sgm_8path                                   form A in all eight directions
    sgm_direction x 8 (where the family says)   form A
    sgm_8path_pair overwrite                    forms C, B;  with the DU fold D, B
    sgm_8path_pair accumulate                   form A;      with the DU fold E, A
    sgm_8path_wta_pair overwrite                ... G, with and without the fold
    sgm_8path_wta_pair accumulate               ... F, with and without the fold
A call with the DU fold gets the case's penalty map with channels 0/1 zeroed (the flag's contract) and must give what
the oracle's eight unfolded directions give for that map.

Before the fixes of this test set two families failed (MI355X, recorded in DESIGN.md 3.3): negative P1 (family 4; the
fast recurrence drops the reference's L'(d) + P1 term at d = 0 and D-1) and zero signs when accumulating onto a -0.0
(family 5; the select chain's tie order is not the reference's).
"""
import numpy as np
import pytest
import torch

import sgm_cases as sc

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()      # (the cases' arrays are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def filled(shape, byte=None):
    """An output buffer: NaN, or every byte `byte`."""
    if byte is None:
        return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    return torch.full((4 * int(np.prod(shape)),), byte, dtype=torch.uint8, device="cuda").view(torch.float32) \
        .reshape(tuple(shape))


def same(got, want, what, nonfinite=False):
    """Byte equality (NaNs canonicalised where the case holds non-finite values), naming the first difference."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if nonfinite:
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        got, want = np.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if diff.any():
        at = tuple(int(i) for i in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} differ, first at {at}: got {got[at]!r} "
                             f"(0x{int(got.view(np.uint32)[at]):08x}), want {want[at]!r} "
                             f"(0x{int(want.view(np.uint32)[at]):08x})")


class Calls:
    """One case's expectations (computed once, by the oracle) and the GPU calls checked against them."""

    def __init__(self, ops, oracle, case):
        self.ops, self.o, self.case = ops, oracle, case
        self.shape = case.shape
        self.nf = case.nonfinite
        self.pen = {False: case.pen, True: [sc.zero_du(p) for p in case.pen]}      # by `fold`
        self._want = {}

    def want(self, fold, acc):
        """The oracle's S of both sides: all eight directions, from zero or onto the seed."""
        key = (fold, acc)
        if key not in self._want:
            c = self.case
            self._want[key] = [self.o.sgm_8path(c.cv[i], self.pen[fold][i], c.S0[i].copy() if acc else None)
                               for i in range(2)]
        return self._want[key]

    def _args(self, fold, S, disp=None):
        c, p = self.case, self.pen[fold]
        if disp is None:
            return dev(c.cv[0]), dev(p[0]), S[0], dev(c.cv[1]), dev(p[1]), S[1]
        return dev(c.cv[0]), dev(p[0]), S[0], disp[0], dev(c.cv[1]), dev(p[1]), S[1], disp[1]

    def eight_path(self, tag=""):
        c = self.case
        for i in range(2):
            same(host(self.ops.sgm_8path(dev(c.cv[i]), dev(c.pen[i]))), self.want(False, False)[i],
                 f"{tag}sgm_8path side {i}", self.nf)
            same(host(self.ops.sgm_8path(dev(c.cv[i]), dev(c.pen[i]), dev(c.S0[i]))), self.want(False, True)[i],
                 f"{tag}sgm_8path onto a seed, side {i}", self.nf)

    def directions(self, tag=""):
        c = self.case
        for i in range(2):
            for d in range(8):
                want = self.o.sgm_direction(c.cv[i], c.pen[i], d, c.S0[i].copy())
                got = host(self.ops.sgm_direction(dev(c.cv[i]), dev(c.pen[i]), d, dev(c.S0[i])))
                same(got, want, f"{tag}sgm_direction {d} side {i}", self.nf)

    def pair(self, fold, acc, tag=""):
        S = [dev(s) for s in self.case.S0] if acc else [filled(self.shape) for _ in range(2)]
        self.ops.sgm_8path_pair(*self._args(fold, S), accumulate=acc, zero_du_penalties=fold)
        for i in range(2):
            same(host(S[i]), self.want(fold, acc)[i], f"{tag}pair fold={fold} accumulate={acc} side {i}", self.nf)

    def wta(self, fold, acc, tag="", want_disp=None):
        S = [dev(s) for s in self.case.S0] if acc else [filled(self.shape, 0xA5) for _ in range(2)]
        disp = [filled(self.shape[:2]) for _ in range(2)]
        self.ops.sgm_8path_wta_pair(*self._args(fold, S, disp), accumulate=acc, zero_du_penalties=fold)
        for i in range(2):
            want = self.o.wta_sgm(self.want(fold, acc)[i])
            if want_disp is not None:
                assert np.array_equal(want, want_disp[i])
            same(host(disp[i]), want, f"{tag}wta pair fold={fold} accumulate={acc} side {i}")
        return S

    def run(self, tag="", directions=False):
        self.eight_path(tag)
        if directions:
            self.directions(tag)
        for fold in (False, True):
            for acc in (False, True):
                self.pair(fold, acc, tag)
                self.wta(fold, acc, tag)


@pytest.fixture(scope="module")
def ops(gpu):
    from scenedepthestimation_amd import ops
    return ops


# ---- 1. the form matrix ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_form_matrix(ops, oracle, k):
    """Every (DPL, load kind) cell at DPL k in every form: D = 64k, one lane / nearly all lanes invalid (vector
    loads), one disparity / nearly all of the last lane's invalid (scalar loads).  11 x 5: ten steps (blocks of
    both ring depths), W < H (the diagonals wrap); positive per-pixel penalties with channels 0/1 live."""
    for D in sc.form_ds(k):
        Calls(ops, oracle, sc.matrix_case(11, 5, D)).run(f"D={D} {sc.launch_cell(D)}: ")


# ---- 2. block edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 97, 320, 321])
def test_block_edges(ops, oracle, D):
    """Lines of 2, PF-1, PF, PF+1, 2PF-1, 2PF, 2PF+1 and 3PF+1 steps against the fused WTA's double-buffered blocks
    of PF steps and the prefetch ring: the hot forms D, B, G (overwrite WTA, folded), A and F (accumulate WTA),
    C and B (the unfolded pair)."""
    for H, W in sc.block_edge_shapes(sc.pf_of(D)):
        calls = Calls(ops, oracle, sc.block_edge_case(oracle, H, W, D))
        tag = f"{H}x{W}x{D}: "
        calls.wta(True, False, tag)
        calls.wta(False, True, tag)
        calls.pair(False, False, tag)


# ---- 3. fused-WTA ties ----------------------------------------------------------------------------------------
WTA_DS = [64, 192, 97, 320, 321, 512]


@pytest.mark.parametrize("H,W,D", [(9, 11, D) if D != 97 else (10, 9, 97) for D in WTA_DS])
def test_wta_integer_ties(ops, oracle, H, W, D):
    """Integer volumes: S ties exactly across lanes at a quarter of the pixels at least (asserted on the CPU); the
    first minimum must win in form G and, onto an integer seed, form F."""
    calls = Calls(ops, oracle, sc.integer_case(H, W, D))
    for fold in (False, True):
        calls.wta(fold, False)
        calls.wta(fold, True)
        calls.pair(fold, False)


@pytest.mark.parametrize("D", WTA_DS)
def test_wta_crafted_rows(ops, oracle, D):
    """Zero costs, accumulating onto a crafted S0 (forms A x 7 and F; E with the fold): S0 comes back unchanged and
    each pixel's disparity is its pattern's -- ties across lane, chunk, lane-group and DPP-row boundaries and the
    row's ends, rows of +inf, NaN at d = 0 and elsewhere, -inf, the minimum at the last valid d -- in row 0 (never
    visited by the last direction) and in visited rows."""
    case, want = sc.wta_pattern_case(oracle, 6, 17, D)
    calls = Calls(ops, oracle, case)
    for fold in (False, True):
        S = calls.wta(fold, True, want_disp=want)
        for i in range(2):
            same(host(S[i]), case.S0[i], f"S after the WTA pair, fold={fold}, side {i}", nonfinite=True)
        calls.pair(fold, True)


# ---- 4. general penalties -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sc.PENALTY_CLASSES)
@pytest.mark.parametrize("D", [64, 100, 192, 321])
def test_general_penalties(ops, oracle, D, kind):
    """Per-pixel, per-channel penalty maps with channels 0/1 live: positive, with zeros, negative P1, negative P2,
    both, huge and subnormal.  A negative P1 leaves the fast path (the reference's chain holds L'(d) + P1 at d = 0
    and D-1); under the fold a negative channel 2 still gives the unfolded values."""
    Calls(ops, oracle, sc.matrix_case(9, 7, D, kind)).run(directions=True)


# ---- 5. signed zeros onto -0.0 --------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("D", [16, 192, 97])
def test_signed_zeros_onto_negative_zero(ops, oracle, D, mixed):
    """Costs from {-0.0, +0.0, |x|} accumulated onto S0 = -0.0 (or a mix of both zeros): S keeps a -0.0 exactly where
    the reference's minima (left, self, right, m + P2; one per reference lane) say so -- direction DU runs on zero
    penalties, where zeros of both signs tie."""
    calls = Calls(ops, oracle, sc.signed_zero_case(oracle, 6, 8, D, mixed))
    calls.directions()
    calls.eight_path()
    calls.pair(False, True)
    calls.pair(True, True)
    calls.wta(False, True)
    calls.wta(True, True)


# ---- 6. finite extremes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 97, 320])
def test_finite_extremes(ops, oracle, D):
    """Subnormal costs and seeds (a flush in either conversion shows), and costs near +-3e38: all finite, so the
    fast path runs; S overflows to +-inf part way through the eight passes, and the later passes and the WTA meet
    it."""
    Calls(ops, oracle, sc.extreme_case(oracle, 9, 7, D)).run(directions=True)
