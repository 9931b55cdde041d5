"""CPU: the conditions of the SGM form tests' inputs (sgm_cases.py), asserted on the oracle and the literal alone,
so that no case of test_gpu_sgm_forms.py can pass vacuously."""
import numpy as np
import pytest

import post_literal
import sgm_cases as sc
from sgm_literal import sgm_8path_literal


def test_form_matrix_reaches_every_cell():
    """Family 1's D list launches every (DPL, load kind) cell that launch_dpl can choose: 8 x 3 minus (1, scalar)."""
    cells = {}
    for k in range(1, 9):
        for D in sc.form_ds(k):
            assert sc.dpl_of(D) == k and 1 <= D <= 512
            cells.setdefault(sc.launch_cell(D), []).append(D)
    assert set(cells) == sc.REACHABLE_CELLS and len(sc.REACHABLE_CELLS) == 23
    assert (1, "scalar") not in {sc.launch_cell(D) for D in range(1, 513)}
    assert {sc.launch_cell(D) for D in range(1, 513)} == sc.REACHABLE_CELLS
    # the lists of the issue, spelled out
    assert sc.form_ds(2) == (128, 126, 66, 127, 65) and sc.form_ds(3) == (192, 189, 129, 191, 130)
    assert sc.form_ds(4) == (256, 252, 196, 255, 193) and sc.form_ds(5) == (320, 315, 260, 319, 257)
    assert sc.form_ds(6) == (384, 378, 324, 383, 321) and sc.form_ds(7) == (448, 441, 385, 447, 386)
    assert sc.form_ds(8) == (512, 504, 456, 511, 449)
    # both ring depths
    assert {sc.pf_of(D) for k in range(1, 9) for D in sc.form_ds(k)} == {4, 8}


@pytest.mark.parametrize("PF", [8, 4])
def test_block_edge_shapes_cover_every_step_count(PF):
    want = {2, PF - 1, PF, PF + 1, 2 * PF - 1, 2 * PF, 2 * PF + 1, 3 * PF + 1}
    shapes = sc.block_edge_shapes(PF)
    for n in want:
        Hs = [s for s in shapes if sc.steps_of(s[0]) == n]
        assert {2, 3} <= {W for _, W in Hs} and any(W == H for H, W in Hs) and any(W == 2 * H + 1 for H, W in Hs)
        assert any(H == 3 and sc.steps_of(W) == n for H, W in shapes)
    assert max(H * W for H, W in shapes) <= 27 * 55


@pytest.mark.parametrize("H,W,D", [(5, 6, 8), (3, 7, 12), (6, 3, 16)])
@pytest.mark.parametrize("kind", sc.PENALTY_CLASSES)
def test_oracle_matches_literal_general_penalties(oracle, H, W, D, kind):
    """Random per-pixel, per-channel penalty maps with negatives, zeros, huge and subnormal values and live
    channels 0/1: the oracle is the literal, bit for bit."""
    case = sc.matrix_case(H, W, D, kind)
    pen = case.pen[0]
    assert (pen[..., :2] != 0).any() and np.isfinite(pen).all()
    if kind.startswith("neg"):
        assert (pen < 0).any()
    if kind == "zeros":
        assert (pen == 0).any()
    assert oracle.sgm_8path(case.cv[0], pen).tobytes() == sgm_8path_literal(case.cv[0], pen).tobytes()


def test_oracle_matches_literal_signed_zeros(oracle):
    """Family 5 at D = 16: S0 = -0.0 survives where the literal says so.  (The literal starts from zero: its S is
    compared after one more accumulation of both onto the same seed, direction by direction.)"""
    case = sc.signed_zero_case(oracle, 6, 8, 16, False)
    cv, pen = case.cv[0], case.pen[0]
    assert oracle.sgm_8path(cv, pen).tobytes() == sgm_8path_literal(cv, pen).tobytes()
    import sgm_literal as lit
    S = case.S0[0].copy()
    lit.vertical(cv, pen, S, True)
    lit.vertical(cv, pen, S, False)
    lit.horizontal(cv, pen, S, True)
    lit.horizontal(cv, pen, S, False)
    lit.diagonal(cv, pen, S, True, True)
    lit.diagonal(cv, pen, S, False, True)
    lit.diagonal(cv, pen, S, True, False)
    lit.diagonal(cv, pen, S, False, False)
    assert oracle.sgm_8path(cv, pen, case.S0[0].copy()).tobytes() == S.tobytes()


@pytest.mark.parametrize("H,W,D", [(9, 7, 64), (9, 7, 100), (6, 5, 8)])
def test_negative_p1_case_discriminates(oracle, H, W, D):
    """The recurrence with the missing neighbours' terms dropped is the oracle's for positive penalties and is not
    for negative P1: a kernel that drops them cannot pass the negative-P1 cases."""
    pos, neg = sc.matrix_case(H, W, D, "positive"), sc.matrix_case(H, W, D, "neg_p1")
    for side in range(2):
        assert sc.ud_dropped_neighbour(pos.cv[side], pos.pen[side]).tobytes() == \
            oracle.sgm_direction(pos.cv[side], pos.pen[side], 0).tobytes()
        assert (neg.pen[side][..., 2] < 0).any()
        assert not np.array_equal(sc.ud_dropped_neighbour(neg.cv[side], neg.pen[side]),
                                  oracle.sgm_direction(neg.cv[side], neg.pen[side], 0))
    # negative P2 alone keeps the dropped-term form exact: those cases stay on the fast path
    n2 = sc.matrix_case(H, W, D, "neg_p2")
    assert sc.ud_dropped_neighbour(n2.cv[0], n2.pen[0]).tobytes() == oracle.sgm_direction(n2.cv[0], n2.pen[0], 0).tobytes()


@pytest.mark.parametrize("H,W,D", [(9, 11, 64), (9, 11, 192), (10, 9, 97), (9, 11, 320), (9, 11, 321), (9, 11, 512)])
def test_integer_volumes_tie_across_lanes(oracle, H, W, D):
    case = sc.integer_case(H, W, D)
    for side in range(2):
        for S0 in (None, case.S0[side].copy()):
            S = oracle.sgm_8path(case.cv[side], case.pen[side], S0)
            assert np.array_equal(S, np.rint(S)) and np.isfinite(S).all()
            share = sc.tie_share(S, D)
            print(f"tie share {share:.3f} at {(H, W, D)}")
            assert share >= 0.25


@pytest.mark.parametrize("D", [64, 192, 97, 320, 321, 512])
def test_zero_costs_leave_seed_alone(oracle, D):
    """Zero costs under the default penalties add +0.0 everywhere: S comes back as it went in (no -0.0 in it), so
    the fused WTA's input is the caller's to craft; and the patterns' closed-form disparities are the literal's and
    the oracle's."""
    case, want = sc.wta_pattern_case(oracle, 6, 17, D)
    names = [n for n, _, _ in sc.wta_patterns(D)]
    assert len(names) < 17 and {"tie_lane", "tie_chunk", "tie_group", "tie_ends", "all_inf", "nan_at_0",
                                "nan_then_min", "neg_inf", "min_last"} <= set(names)
    for side in range(2):
        S0 = case.S0[side]
        assert sc.neg_zeros(S0) == 0
        S = oracle.sgm_8path(case.cv[side], case.pen[side], S0.copy())
        assert S.tobytes() == S0.tobytes()
        assert np.array_equal(post_literal.wta(S0, "HWD", "d0"), want[side])
        assert np.array_equal(oracle.wta_sgm(S0), want[side])


@pytest.mark.parametrize("D", [16, 192, 97])
@pytest.mark.parametrize("mixed", [False, True])
def test_signed_zero_cases_keep_negative_zeros(oracle, D, mixed):
    case = sc.signed_zero_case(oracle, 6, 8, D, mixed)
    for side in range(2):
        S = oracle.sgm_8path(case.cv[side], case.pen[side], case.S0[side].copy())
        nz, z = sc.neg_zeros(S), int((S == 0).sum())
        print(f"-0.0 in {nz} of {z} zeros, D = {D}, mixed = {mixed}")
        assert 0 < nz < z
        one = oracle.sgm_direction(case.cv[side], case.pen[side], 1, case.S0[side].copy())
        assert 0 < sc.neg_zeros(one) < int((one == 0).sum())


@pytest.mark.parametrize("D", [64, 97, 320])
def test_extreme_case_overflows_without_nan(oracle, D):
    case = sc.extreme_case(oracle, 9, 7, D)
    for side in range(2):
        assert sc.subnormals(case.cv[side]) > 0 and sc.subnormals(case.S0[side]) > 0
        for S0 in (None, case.S0[side].copy()):
            S = oracle.sgm_8path(case.cv[side], case.pen[side], S0)
            assert not np.isnan(S).any()
            assert (S == np.inf).any() and (S == -np.inf).any() and sc.subnormals(S) > 0
        # part way through: still finite after the first direction
        assert np.isfinite(oracle.sgm_direction(case.cv[side], case.pen[side], 0)).all()
