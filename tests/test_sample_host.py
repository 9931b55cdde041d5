"""Scene training and evaluation, the parts that need no GPU: the literal against known answers and against
training.TripletSampler, the C ABI's argument checks, the CLIs and the file handling."""
import ctypes
import os

import numpy as np
import pytest

import sample_literal as sl

SYNTHETIC = [(11, 23, 4, 5), (12, 24, 6, 5), (13, 40, 8, 5), (17, 70, 16, 5), (64, 160, 32, 5), (3, 15, 4, 1)]


# ---------------------------------------------------------------------------------------------------------
# the literal
# ---------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    def hexs(t):
        return " ".join(f"{v:08x}" for v in t)
    assert hexs(sl.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert hexs(sl.philox4x32_10((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexs(sl.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_unit_is_53_bits_in_the_half_open_interval():
    assert sl.unit((0, 0, 0, 0)) == 0.0
    top = sl.unit((0xFFFFFFFF, 0xFFFFFFFF, 0, 0))
    assert top == 1.0 - 2.0 ** -53 and top < 1.0
    assert sl.unit((1, 1 << 11, 0, 0)) == (2 ** 21 + 1) * 2.0 ** -53


def _sampler_centres(left, right, L, zero_is_invalid):
    from scenedepthestimation_amd.training import TripletSampler
    c = TripletSampler(left, right, patch=2 * L + 1, zero_is_invalid=zero_is_invalid).centres
    return (c[:, 0] * left.shape[1] + c[:, 1]).astype(np.int32)


@pytest.mark.parametrize("H,W,D,L", SYNTHETIC)
def test_literal_centres_equal_the_sampler_on_synthetic_scenes(H, W, D, L):
    from scenedepthestimation_amd.synthetic import stereo_pair
    _, _, gt = stereo_pair(H, W, D, 1)
    rgt = sl.right_map(gt)
    for right in (rgt, None):
        assert np.array_equal(sl.centres(gt, right, L, False), _sampler_centres(gt, right, L, False))


@pytest.mark.parametrize("zero_is_invalid", [True, False])
def test_literal_centres_equal_the_sampler_on_the_handmade_map(zero_is_invalid):
    left, right = sl.handmade_maps()
    W = left.shape[1]
    for r in (right, None):
        assert np.array_equal(sl.centres(left, r, 5, zero_is_invalid), _sampler_centres(left, r, 5, zero_is_invalid))
    got = set(sl.centres(left, right, 5, zero_is_invalid).tolist())
    yes = [(5, 12), (7, 20), (5, 20)] + ([] if zero_is_invalid else [(6, 12), (6, 23)])
    no = [(5, 11), (7, 25), (7, 30), (5, 22), (6, 10), (6, 11), (6, 13), (6, 14), (6, 29), (6, 30), (7, 33)] + \
        ([(6, 12), (6, 23)] if zero_is_invalid else [])
    assert all(y * W + x in got for y, x in yes) and not any(y * W + x in got for y, x in no)


@pytest.mark.parametrize("L", [1, 5])
def test_literal_triplets_keep_the_sampler_invariants(L):
    from scenedepthestimation_amd.synthetic import stereo_pair
    scenes = []
    for H, W, D in ((13, 40, 8), (17, 70, 16), (64, 160, 32)):
        _, _, gt = stereo_pair(H, W, D, 1)
        scenes.append((gt.astype(np.float32), sl.centres(gt, sl.right_map(gt), L, False)))
    idx, scene, rounds = sl.draw(scenes, L, seed=9, step=2, B=400)
    assert (rounds >= 1).all() and rounds.max() > 1
    both = set()
    for (y, x, pos, neg), s, (rp, rn) in zip(idx.tolist(), scene.tolist(), rounds.tolist()):
        dl, cs = scenes[s]
        W = dl.shape[1]
        assert y * W + x in set(cs.tolist())
        rc = x - float(dl[y, x])
        assert L <= pos < W - L and L <= neg < W - L
        assert rc - 0.501 - 1 < pos <= rc + 0.501
        if rn <= 32:
            assert rc - 6 - 1 < neg <= rc - 1.5 or rc + 1.5 - 1 < neg <= rc + 6
        both.add(neg > rc)
    assert both == {True, False}


def test_fallbacks_fire_and_stay_inside():
    (_, _), dl = sl.reject_scene()
    cs = sl.centres(dl, None, 5, False)
    idx, _, rounds = sl.draw([(dl, cs)], 5, seed=1, step=4, B=67, max_rounds=1)
    assert (rounds[:, 0] == 2).any() and (rounds[:, 1] == 2).any()
    assert ((idx[:, 2:] >= 5) & (idx[:, 2:] < 23 - 5)).all()
    fell = rounds[:, 0] == 2
    assert (idx[fell, 2] == (idx[fell, 1] - dl[idx[fell, 0], idx[fell, 1]]).astype(np.int32)).all()


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
NEW_FUNCS = ["sde_triplet_centres", "sde_train_sample_gather", "sde_bad_pixels"]


def test_abi_declares_and_binds_the_new_entry_points():
    from scenedepthestimation_amd import _lib
    declared = set(_lib.header_functions())
    for f in NEW_FUNCS:
        assert f in declared and f in _lib.SIGNATURES, f
    assert _lib.lib.sde_abi_version() == 4 == _lib.SDE_ABI_VERSION


def test_abi_refuses_bad_arguments():
    """Every refusal comes before any launch, so a host address (never dereferenced) stands in for device ones."""
    from scenedepthestimation_amd import _lib
    lib, ARG = _lib.lib, -1
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # centres: H < P, W < P + 12, H*W >= 2^31, nlayers outside 1..5, unknown flags, null pointers
    assert lib.sde_triplet_centres(p, p, 10, 40, 5, 0, p, p, None) == ARG
    assert lib.sde_triplet_centres(p, p, 13, 22, 5, 0, p, p, None) == ARG
    assert lib.sde_triplet_centres(p, p, 2, 15, 1, 0, p, p, None) == ARG
    assert lib.sde_triplet_centres(p, p, 3, 14, 1, 0, p, p, None) == ARG
    assert lib.sde_triplet_centres(p, p, 1 << 16, 1 << 15, 5, 1, p, p, None) == ARG
    for L in (0, 6, -1):
        assert lib.sde_triplet_centres(p, p, 64, 160, L, 1, p, p, None) == ARG
    for flags in (2, 3, -1):
        assert lib.sde_triplet_centres(p, p, 64, 160, 5, flags, p, p, None) == ARG
    for hole in (0, 2, 3):
        a = [p, p, p, p]
        a[hole] = None
        assert lib.sde_triplet_centres(a[0], a[1], 64, 160, 5, 1, a[2], a[3], None) == ARG
    # sample + gather: the scalars
    ok = dict(S=1, N=10, B=4, L=5, rounds=32)

    def sample(table=p, patches=p, **kw):
        v = dict(ok, **kw)
        return lib.sde_train_sample_gather(table, v["S"], v["N"], v["B"], v["L"], 1, 2, v["rounds"], patches, None,
                                           None, None)
    assert sample(table=None) == ARG and sample(patches=None) == ARG
    for kw in (dict(S=0), dict(S=-1), dict(N=0), dict(N=1 << 31), dict(N=-5), dict(B=0), dict(B=-1), dict(B=1 << 30),
               dict(L=0), dict(L=6), dict(rounds=0), dict(rounds=33), dict(rounds=-1)):
        assert sample(**kw) == ARG, kw
    # bad pixels
    d = ctypes.c_double
    assert lib.sde_bad_pixels(None, p, 4, 4, d(1), p, None, None) == ARG
    assert lib.sde_bad_pixels(p, None, 4, 4, d(1), p, None, None) == ARG
    assert lib.sde_bad_pixels(p, p, 4, 4, d(1), None, None, None) == ARG
    for H, W in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15)):
        assert lib.sde_bad_pixels(p, p, H, W, d(1), p, None, None) == ARG
    for thr in (-1.0, float("nan")):
        assert lib.sde_bad_pixels(p, p, 4, 4, d(thr), p, None, None) == ARG


def test_ops_refuse_cpu_tensors():
    import torch

    from scenedepthestimation_amd import ops
    f = torch.zeros((13, 40))
    with pytest.raises(ValueError, match="GPU"):
        ops.triplet_centres(f, None, 5)
    with pytest.raises(ValueError, match="GPU"):
        ops.train_sample_gather(torch.zeros((1, 8), dtype=torch.int64), 10, 4, 5, 0, 0,
                                out=torch.zeros((3, 4, 11, 11)))
    with pytest.raises(ValueError, match="GPU"):
        ops.bad_pixels(f, f, counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.triplet_centres(f, torch.zeros((13, 41)), 5)
    with pytest.raises(ValueError):
        ops.train_sample_gather(torch.zeros((1, 7), dtype=torch.int64), 10, 4, 5, 0, 0)
    with pytest.raises(ValueError):
        ops.bad_pixels(f, torch.zeros((13, 41)))


# ---------------------------------------------------------------------------------------------------------
# CLIs and files
# ---------------------------------------------------------------------------------------------------------
def test_train_cli_scene_flags():
    from scenedepthestimation_amd import train
    a = train.make_parser().parse_args([])
    assert (a.scene_files, a.half, a.val_scenes, a.val_ndisp, a.seed) == \
        ("im0.png,im1.png,disp0.pfm,disp1.pfm", False, 0, 128, 0)
    b = train.make_parser().parse_args("--data scenes:list.txt --scene-files a.png,b.png,c.pfm, --half --val-scenes 2 "
                                       "--val-ndisp 64 --seed 7 --steps-per-epoch 3".split())
    assert (b.data, b.scene_files.split(","), b.half, b.val_scenes, b.val_ndisp, b.seed, b.steps_per_epoch) == \
        ("scenes:list.txt", ["a.png", "b.png", "c.pfm", ""], True, 2, 64, 7, 3)


def test_scene_source_steps():
    """Epoch e, batch k is step e * size + k; the training stream runs on, the validation stream restarts."""
    from scenedepthestimation_amd import train

    class Set:
        def batch(self, step, B):
            return step, B

    tr = train._SceneSource(Set(), 16, 3, first_step=2 * 3, restart=False)
    va = train._SceneSource(Set(), 16, 2, first_step=0, restart=True)
    seen = []
    for _ in range(2):
        seen.append(([tr.next_batch() for _ in range(3)], [va.next_batch() for _ in range(2)]))
        tr.reset_pointer()
        va.reset_pointer()
    assert seen[0] == ([(6, 16), (7, 16), (8, 16)], [(0, 16), (1, 16)])
    assert seen[1] == ([(9, 16), (10, 16), (11, 16)], [(0, 16), (1, 16)])


def test_halve_is_the_2x2_mean():
    from scenedepthestimation_amd.evaluation import halve, halve_u8
    a = np.arange(24, dtype=np.float32).reshape(4, 6)
    a[0, 0] = 0.5
    assert np.array_equal(halve(a), np.float32([[(0.5 + 1 + 6 + 7) / 4, 5.5, 7.5], [15.5, 17.5, 19.5]]))
    assert halve(a).dtype == np.float32
    assert halve(np.ones((5, 7))).shape == (2, 3)
    b = a.copy()
    b[3, 5] = np.inf
    assert np.isinf(halve(b)[1, 2]) and np.array_equal(halve(b)[0], halve(a)[0])
    u = np.array([[1, 2, 255, 255], [2, 2, 255, 254]], np.uint8)
    assert halve_u8(u).tolist() == [[2, 255]] and halve_u8(u).dtype == np.uint8      # 1.75 -> 2, 254.75 -> 255
    assert halve_u8(np.array([[1, 2], [1, 2]], np.uint8)).tolist() == [[2]]           # 1.5 rounds up


def test_load_scene_reads_and_halves(tmp_path):
    from scenedepthestimation_amd import train
    from scenedepthestimation_amd.evaluation import halve, halve_u8
    from scenedepthestimation_amd.imageio import imwrite
    from scenedepthestimation_amd.pfm import save_pfm
    rng = np.random.default_rng(3)
    il, ir = rng.integers(0, 256, (2, 6, 8)).astype(np.uint8)
    dl = rng.uniform(1, 9, (6, 8)).astype(np.float32)
    dl[2, 3] = np.inf
    d = str(tmp_path / "scene")
    imwrite(os.path.join(d, "l.png"), il)
    imwrite(os.path.join(d, "r.png"), ir)
    save_pfm(os.path.join(d, "d.pfm"), dl)
    (tmp_path / "list.txt").write_text(f"{d}\n\n")
    assert train.read_scene_list(str(tmp_path / "list.txt")) == [d]
    a = train.load_scene(d, ["l.png", "r.png", "d.pfm", ""], half=False)
    assert np.array_equal(a[0], il) and np.array_equal(a[1], ir) and a[3] is None
    assert a[2].tobytes() == dl.tobytes() and a[2].dtype == np.float32
    h = train.load_scene(d, ["l.png", "r.png", "d.pfm", "d.pfm"], half=True)
    assert np.array_equal(h[0], halve_u8(il)) and h[0].shape == (3, 4)
    assert np.array_equal(h[2], halve(dl) / 2) and np.array_equal(h[2], h[3]) and np.isinf(h[2][1, 1])


def test_error_calculate_end_to_end(tmp_path, monkeypatch, capsys):
    """Tiny files on disk, the device count replaced by the literal: the reference's lines and pictures."""
    from PIL import Image

    from scenedepthestimation_amd import error_calculate, evaluation
    from scenedepthestimation_amd.imageio import imwrite
    from scenedepthestimation_amd.pfm import save_pfm

    def literal_counts(disp, gt, threshold, want_area):
        ev, bad, area = sl.bad_pixels(np.asarray(disp, np.float32), gt, threshold)
        return ev, bad, (area if want_area else None)
    monkeypatch.setattr(evaluation, "_device_counts", literal_counts)
    res, tru, out = tmp_path / "res", tmp_path / "gt", tmp_path / "area"
    os.makedirs(tru)
    disp0 = np.array([[3, 4, 5], [6, 7, 8]], np.uint8)
    gt0 = np.float32([[6, 12, np.inf], [0, 14, 16.5]])                   # * 0.5: 3, 6 (bad), skip, skip, 7, 8.25
    disp1 = np.array([[10, 20]], np.uint8)
    gt1 = np.float32([[24, 24, 46, 46], [24, 24, 46, 46]])               # twice the size: halved to 24, 46; bad, bad
    for i, (d, g) in enumerate(((disp0, gt0), (disp1, gt1))):
        imwrite(str(res / f"ld{i}.png"), d)
        save_pfm(str(tru / f"disp{i}.pfm"), g)
    assert error_calculate.main(["--result", str(res), "--truth", str(tru), "--count", "2", "--area", str(out)]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines == [f"error rate of disp0: {1 / 6}", "error rate of disp1: 1.0", f"mean error rate: {(1 / 6 + 1) / 2}"]
    pic = np.asarray(Image.open(out / "area0.png").convert("RGB"))
    assert pic[0, 0].tolist() == [0, 255, 0] and pic[0, 1].tolist() == [255, 0, 0] and pic[0, 2].tolist() == [0, 0, 0]
    # any other size is an error; a scale of 1 changes the verdicts
    with pytest.raises(ValueError):
        error_calculate.fit_truth(np.zeros((3, 3), np.float32), (2, 3), 0.5)
    assert error_calculate.main(["--result", str(res), "--truth", str(tru), "--count", "1", "--gt-scale", "1"]) == 0
    assert capsys.readouterr().out.splitlines()[0] == f"error rate of disp0: {4 / 6}"   # 6, 12, 14, 16.5 against 3, 4, 7, 8
    r = evaluation.bad_pixel_rate(disp0, error_calculate.fit_truth(gt0, (2, 3), 0.5))
    assert (r["evaluated"], r["bad"]) == (4, 1) and r["rate_over_evaluated"] == 0.25
    a = error_calculate.make_parser().parse_args([])
    assert (a.count, a.gt_scale, a.area) == (5, 0.5, None)
