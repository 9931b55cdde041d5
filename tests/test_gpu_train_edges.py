"""The training kernels where test_gpu_train.py does not go: weight-gradient chunks above 256 pixels (B = 259 and
440 at L = 5), batches past the 256 lanes of the loss mean, and batches in which one triplet alone is live, so that
a single pixel lost or repeated at a chunk, tile or sub-step edge is large against the bar (train_cases.py;
test_train_cases_host.py asserts the inputs' conditions on the CPU).

Every gradient comparison is test_gpu_train.compare_gradients: err_gpu <= 8 * err_cpu32 per parameter tensor."""
import numpy as np
import pytest
import torch

import test_gpu_train as tg
import train_cases as tc
import train_literal as tl

pytestmark = pytest.mark.gpu

L = tc.L
ACTIVE = {259: 164, 440: 306}           # active triplets of the dense batches' float64 literal (tg.SEEDS)


def forward_only(p, nlayers, margin):
    """-> the loss words [1 + B] of a run without gradients."""
    from scenedepthestimation_amd import ops, training
    B = p.shape[1]
    ws = tg.junk((ops.train_workspace_bytes(B, nlayers),), torch.uint8)
    w = tg.weights(nlayers)
    loss, none = ops.train_loss_grad(tg.dev(p), tg.dev(training.flatten(w, nlayers)), nlayers, margin,
                                     loss=tg.junk((1 + B,)), workspace=ws, want_grads=False)
    assert none is None
    return tg.host(loss)


def check_mean(loss, B):
    """loss[0] against the float64 mean of max(h, 0) over the GPU's own h words, within the bound the kernel's
    summation shape gives (train_cases.loss_mean_bound).  -> that mean."""
    mean = np.maximum(loss[1:].astype(np.float64), 0).sum() / B
    assert mean > 0, "the mean of no active triplet checks nothing"
    assert abs(float(loss[0]) - mean) <= tc.loss_mean_bound(B, mean), (float(loss[0]), mean)
    return mean


# ---------------------------------------------------------------------------------------------------------
# A. one live triplet, swept over the positions
# ---------------------------------------------------------------------------------------------------------
def live_run(B, i):
    """The batch with triplet i alone live, on the GPU (0xA5-filled outputs and workspace).  -> (loss [1 + B],
    gradient blob, the post-ReLU outputs of layers 1..L-1 of patches i, B + i and 2B + i)."""
    from scenedepthestimation_amd import ops, training
    q = tc.plan(B).batch(i)
    ws = tg.junk((ops.train_workspace_bytes(B, L),), torch.uint8)
    loss, grads = ops.train_loss_grad(tg.dev(q), tg.dev(training.flatten(tc.weights(), L)), L, tc.MARGIN,
                                      loss=tg.junk((1 + B,)), grads=tg.junk((ops.train_param_floats(L),)), workspace=ws)
    rows = torch.tensor(tc.live_patches(B, i), device="cuda")
    acts = [tg.host(ops.train_export_activations(ws, B, L, k)[rows]) for k in range(1, L)]
    return tg.host(loss), tg.host(grads), acts


def check_position(B, i):
    """One live-triplet run against the float64 literal of the live triplet alone (train_cases.reduced_runs; the
    whole batch's gradient is that one's over B, so the GPU's is multiplied by B, exactly, in float64).
    -> the worst err_gpu / err_cpu32."""
    from scenedepthestimation_amd import training
    pl = tc.plan(B)
    loss, blob, acts = live_run(B, i)
    h = loss[1:]
    assert np.flatnonzero(h > 0).tolist() == [i]
    assert np.abs(h - pl.expected_h(i)).max() <= 1e-5
    mean = check_mean(loss, B)
    assert mean == float(h[i]) / B
    assert np.isfinite(blob).all()
    g = {"acts": acts, "loss": np.array([loss[0], h[i]]),
         "grads": {k: v.astype(np.float64) * B for k, v in training.unflatten(blob, L).items()}}
    return tg.compare_gradients(g, tc.reduced(pl.batch(i), i), tc.weights(), L, tc.MARGIN, f"B={B} live {i}")


def check_positions(B, where):
    assert where
    worst = max(check_position(B, i) for i in where)
    print(f"B={B}, {len(where)} positions {where[0]}..{where[-1]}: worst err_gpu / err_cpu32 = {worst:.2f}")


@pytest.mark.parametrize("residue", range(8))
def test_one_live_triplet_every_position_b259(gpu, residue):
    """B = 259: chunks of 512 and 320 pixels in layers 1 and 2, 256 in layers 3-5 (9 pixels in layer 5's last),
    B > 256 and B mod 4 = 3.  Every patch is live in exactly one run, so the sweep crosses every chunk bound,
    every 64-pixel tile tail of the forward and backward-data kernels and every 32-pixel sub-step tail."""
    check_positions(259, [i for i in tc.sweep(259) if i % 8 == residue])


@pytest.mark.parametrize("B", [440, 130])
def test_one_live_triplet_sampled_positions(gpu, B):
    """B = 440: chunks of 864, 512 and 288 pixels in layers 1-3, every 16th position and the last.  B = 130: the
    256-pixel chunks of test_gpu_train.py, every 8th position and the last."""
    check_positions(B, tc.sweep(B))


# ---------------------------------------------------------------------------------------------------------
# B. dense batches in the capped regime
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [259, 440])
def test_dense_gradients_capped_chunks(gpu, B):
    g, ref = tg.case(B, L)
    assert int((ref["h"] > 0).sum()) == ACTIVE[B] and tg.SEEDS[B] == 100 + B
    tg.compare_gradients(g, tg.batch(tg.SEEDS[B], B, L), tg.weights(L), L, 0.3, f"B={B} L={L}")


@pytest.mark.parametrize("check", [tg.test_forward, tg.test_masks, tg.test_deterministic], ids=lambda f: f.__name__[5:])
def test_dense_b259(gpu, check):
    """test_gpu_train's own forward, mask and determinism checks (two runs, identical bytes) at B = 259, L = 5."""
    check(gpu, 259) if check is tg.test_deterministic else check(gpu, 259, L)


# ---------------------------------------------------------------------------------------------------------
# C. the loss mean past 256 triplets
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nlayers", [(256, 1), (257, 1), (300, 1), (1000, 1), (259, 5)])
def test_loss_mean_past_256(gpu, B, nlayers):
    """Forward only.  B = 256 fills the 256 lanes once; past it the lane-strided loop takes a second trip (a
    fourth at B = 1000)."""
    p = tg.batch(100 + B, B, nlayers)
    loss = forward_only(p, nlayers, 0.3)
    ref = tl.run(p, tg.weights(nlayers), nlayers, 0.3, grads=False)
    assert np.abs(loss[1:] - ref["h"]).max() <= 1e-5
    mean = check_mean(loss, B)
    late = np.maximum(loss[1 + 256:].astype(np.float64), 0).sum() / B
    print(f"B={B} L={nlayers}: loss {float(loss[0]):.9g}, float64 mean of the GPU's h {mean:.9g}, difference "
          f"{abs(float(loss[0]) - mean):.3g} (bound {tc.loss_mean_bound(B, mean):.3g}); "
          f"triplets 256.. carry {late / mean:.3f}")
    if B >= 300:
        assert late > tc.loss_mean_bound(B, mean), "the later trips must matter to the mean"


@pytest.mark.parametrize("i", [256, 258])
def test_loss_mean_second_trip_alone(gpu, i):
    """B = 259 with triplet i >= 256 alone active: the loop's second trip carries the whole sum."""
    B = 259
    loss = forward_only(tc.plan(B).batch(i), L, tc.MARGIN)
    assert np.flatnonzero(loss[1:] > 0).tolist() == [i]
    assert np.abs(loss[1:] - tc.plan(B).expected_h(i)).max() <= 1e-5
    mean = check_mean(loss, B)
    assert mean == float(loss[1 + i]) / B
