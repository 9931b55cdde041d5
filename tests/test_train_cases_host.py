"""CPU: the conditions of the training edge tests' inputs (train_cases.py), asserted on the float64 literal alone,
so that no case of test_gpu_train_edges.py can pass vacuously: one live triplet per batch and hinge decisions no
fp32 rounding can flip, the reduced literal standing for the whole batch's, and every pixel of the live patches
large enough against the bar that losing or repeating it would fail."""
import numpy as np
import pytest

import train_cases as tc
import train_literal as tl

BS = (130, 259, 440)


def spread(B, n=8):
    """About n swept positions, first and last included."""
    sw = tc.sweep(B)
    return sorted({sw[round(j * (len(sw) - 1) / (n - 1))] for j in range(n)})


def test_chunk_table():
    """The capped layers of each batch size, spelled out, and the library's workspace size follows from them (the
    partial-sum region is the widest nchunks * (weights + biases))."""
    from scenedepthestimation_amd import ops
    for B in BS:
        assert tuple(tc.chunking(B)) == tc.CHUNKS[B]
    assert [c for c, _ in tc.chunking(259)] == [512, 320, 256, 256, 256]
    assert [c for c, _ in tc.chunking(440)] == [864, 512, 288, 256, 256]
    assert 3 * 259 * 1 - 3 * 256 == 9                  # layer 5's last chunk at B = 259 holds 9 pixels
    assert all(c == 256 for B in (128, 130) for c, _ in tc.chunking(B))
    assert [c > 256 for c, _ in tc.chunking(4096)] == [True] * 4 + [False]
    for B in BS + (128, 4096):
        assert tc.workspace_floats(B) * 4 == ops.train_workspace_bytes(B, tc.L)


@pytest.mark.parametrize("B", BS)
def test_one_live_conditions(B):
    """Per position, from one float64 forward pass of the drawn batch: dead triplets at h <= -0.02, the live one at
    h >= 0.05 in its better role order, skips within the cap and away from every last chunk."""
    pl = tc.plan(B)
    assert tc.conditions_hold(pl)
    assert pl.h_dead.max() <= tc.H_DEAD
    skipped = [i for i in tc.positions(B) if not pl.ok[i]]
    print(f"B={B} seed {tc.SEEDS[B]}: {len(skipped)} of {len(tc.positions(B))} swept positions skipped {skipped}; "
          f"max dead h {pl.h_dead.max():.3f}, min live h of the sweep {pl.h_live[tc.sweep(B)].min():.3f}, "
          f"{int(pl.swapped.sum())} positions with the roles swapped")
    assert len(skipped) <= 0.05 * B
    assert B - 1 in tc.sweep(B) and 0 in tc.sweep(B)
    assert (pl.h_live[tc.sweep(B)] >= tc.H_LIVE).all()
    assert pl.swapped.any() and not pl.swapped.all()          # both role orders occur
    if B == 259:
        assert sorted(tc.sweep(B) + skipped) == list(range(B))
        assert {256, 258} <= set(tc.sweep(B))                 # the loss-mean cases of the second loop trip
    # the seed is the first from 100 + B on that meets the conditions
    for seed in range(100 + B, tc.SEEDS[B]):
        assert not tc.conditions_hold(tc.Plan(B, seed)), seed


@pytest.mark.parametrize("B", BS)
def test_one_live_batches_as_built(B):
    """The batches themselves, through the whole float64 literal: exactly one active triplet, the h the plan says,
    the live triplet's three patches distinct and its negative not its left patch."""
    pl = tc.plan(B)
    for i in spread(B, 4):
        q = pl.batch(i)
        assert not np.array_equal(q[0, i], q[1, i]) and not np.array_equal(q[0, i], q[2, i])
        assert not np.array_equal(q[1, i], q[2, i])
        dead = np.arange(B) != i
        assert np.array_equal(q[0, dead], q[1, dead])
        h = tl.run(q, tc.weights(), tc.L, tc.MARGIN, grads=False)["h"]
        assert np.abs(h - pl.expected_h(i)).max() <= 1e-12
        assert (h > 0).sum() == 1 and h[i] >= tc.H_LIVE and h[dead].max() <= tc.H_DEAD


@pytest.mark.parametrize("B,i", [(259, 0), (259, 258), (440, 439)])
def test_reduced_literal_is_the_full_literal(B, i):
    """The literal on the live triplet alone (a batch of one, hinge forced, the full run's ReLU masks of its three
    patches), divided by B, is the literal on the whole batch: 1e-13 of each tensor's maximum."""
    pl = tc.plan(B)
    q = pl.batch(i)
    full = tl.run(q, tc.weights(), tc.L, tc.MARGIN)
    rm = [m[tc.live_patches(B, i)] for m in tc.relu_masks_of(full)]
    r64, _ = tc.reduced_runs(q, i, rm)
    assert abs(r64["loss"] - full["h"][i]) <= 1e-14
    assert abs(r64["loss"] / B - full["loss"]) <= 1e-15
    for k, g in full["grads"].items():
        assert np.abs(g).max() > 0, k
        assert np.abs(r64["grads"][k] / B - g).max() <= 1e-13 * np.abs(g).max(), k
    # and the dead patches' dz is exactly zero in the full run
    live = tc.live_patches(B, i)
    for d in full["dpre"]:
        assert not np.delete(d, live, axis=0).any()


@pytest.mark.parametrize("B", BS)
def test_every_pixel_is_visible(B):
    """At about 8 swept positions, in every layer, for every pixel of the three live patches (243, 147, 75, 27 and
    3 of them): the largest term the pixel adds to the layer's weight gradient exceeds 8 * err_cpu32 of that
    tensor, and so does its bias term -- dropping or repeating any one pixel fails compare_gradients' bar; in the
    64-channel layers that holds of each of the nine taps separately.  The
    literal's own ReLU masks stand in for the GPU's here."""
    pl = tc.plan(B)
    worst = {}
    for i in spread(B, 8):
        q = pl.batch(i)
        r = tc.reduced(q, i)
        rm = tc.relu_masks_of(tl.run(r, tc.weights(), tc.L, tc.MARGIN, grads=False))
        r64, r32 = tc.reduced_runs(q, i, rm)
        for k, v in enumerate(tc.pixel_visibility(r64, r32, r, rm), start=1):
            print(f"B={B} i={i} layer {k}: window {v['window']:.3g} (one tap {v['tap']:.3g}) against {v['bar_w']:.3g}; "
                  f"bias {v['bias']:.3g} against {v['bar_b']:.3g}")
            assert v["window"] > v["bar_w"], (i, k)
            assert v["bias"] > v["bar_b"], (i, k)
            if k > 1:       # 64 input channels: each tap's block on its own sees the pixel (layer 1 has one channel,
                assert v["tap"] > v["bar_w"], (i, k)          # and a single image value can be near zero)
            worst[k] = min(worst.get(k, np.inf), v["window"] / v["bar_w"])
            scale = np.abs(r64["grads"][tl.var_names(tc.L)[k - 1][0]]).max()
            assert 1e-7 <= v["bar_w"] / 8 / scale <= 3e-6       # the yardstick is an fp32 rounding error, no more
    print(f"B={B}: smallest window / bar per layer {[round(worst[k], 1) for k in sorted(worst)]}")
