"""Training, the parts that need no GPU: the float64 literal checks itself against finite differences, the PFM
reader / writer, the patch-file dataset, the triplet sampler, the CLI defaults, the C ABI's argument checks and
the NumPy statement of the momentum rule."""
import ctypes
import os

import numpy as np
import pytest

import train_literal as tl

NF = 64


def synthetic_batch(seed, B, nlayers):
    from scenedepthestimation_amd import training
    il, ir, idx = training.synthetic_triplets(seed, B, patch=2 * nlayers + 1)
    return tl.gather_host(il, ir, idx, 2 * nlayers + 1)


# ---------------------------------------------------------------------------------------------------------
# the literal
# ---------------------------------------------------------------------------------------------------------
def test_literal_gradient_matches_finite_differences():
    """Central differences in float64 on 20 seeded parameter entries at B = 4, nlayers = 5, with the base run's
    masks forced (the loss is then smooth): 1e-6 relative to the entry's own gradient."""
    from scenedepthestimation_amd import mc_cnn
    L, B = 5, 4
    patches = synthetic_batch(3, B, L)
    w = {k: v.astype(np.float64) for k, v in mc_cnn.synthetic_weights(L).items()}
    base = tl.run(patches, w, L)
    rm, hm = tl.masks_of(base)
    assert hm.any(), "no active triplet: the check would be vacuous"
    rng = np.random.default_rng(0)
    names = sorted(w)
    eps = 1e-5
    for _ in range(20):
        name = names[rng.integers(len(names))]
        pos = tuple(rng.integers(s) for s in w[name].shape)
        vals = []
        for sign in (1, -1):
            w2 = {k: v.copy() for k, v in w.items()}
            w2[name][pos] += sign * eps
            vals.append(tl.run(patches, w2, L, relu_masks=rm, hinge_mask=hm, grads=False)["loss"])
        fd = (vals[0] - vals[1]) / (2 * eps)
        g = base["grads"][name][pos]
        assert abs(fd - g) <= 1e-6 * abs(g) + 1e-13, (name, pos, fd, g)


def test_literal_forced_masks_reproduce_the_free_run():
    from scenedepthestimation_amd import mc_cnn
    L = 2
    patches = synthetic_batch(4, 3, L)
    w = mc_cnn.synthetic_weights(L)
    a = tl.run(patches, w, L)
    b = tl.run(patches, w, L, relu_masks=tl.masks_of(a)[0], hinge_mask=tl.masks_of(a)[1])
    assert a["loss"] == b["loss"]
    for k in a["grads"]:
        assert np.array_equal(a["grads"][k], b["grads"][k]), k


# ---------------------------------------------------------------------------------------------------------
# PFM, PatchFileDataset
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("shape", [(3, 5), (4, 2, 1), (2, 3, 3)])
def test_pfm_round_trip(tmp_path, big_endian, shape):
    from scenedepthestimation_amd.pfm import load_pfm, save_pfm
    rng = np.random.default_rng(1)
    img = rng.standard_normal(shape).astype(np.float32)
    img.flat[0] = np.float32(-0.0)
    path = str(tmp_path / "a.pfm")
    save_pfm(path, img, big_endian=big_endian)
    back, scale = load_pfm(path)
    assert scale == 1.0
    assert back.shape == (shape[0], shape[1], 3 if len(shape) == 3 and shape[2] == 3 else 1)
    assert back.astype("<f4").tobytes() == img.reshape(back.shape).astype("<f4").tobytes()
    # rows are stored bottom-up: the file's first row is the image's last
    with open(path, "rb") as fh:
        raw = fh.read()
    body = raw.split(b"\n", 3)[3]
    first = np.frombuffer(body, ">f4" if big_endian else "<f4")[:back.shape[1] * back.shape[2]]
    assert np.array_equal(first, img.reshape(back.shape)[-1].ravel())
    assert raw.startswith(b"PF\n" if back.shape[2] == 3 else b"Pf\n")
    assert (float(raw.split(b"\n")[2]) > 0) == big_endian


def test_pfm_rejects_other_files(tmp_path):
    from scenedepthestimation_amd.pfm import load_pfm
    p = tmp_path / "x.pfm"
    p.write_bytes(b"P5\n2 2\n255\n\0\0\0\0")
    with pytest.raises(ValueError):
        load_pfm(str(p))


def _write_patches(root, numbers, size=3):
    from scenedepthestimation_amd.pfm import save_pfm
    vals = {}
    for s, sub in enumerate(("left", "right_pos", "right_neg")):
        os.makedirs(os.path.join(root, sub))
        for n in numbers:
            rng = np.random.default_rng(1000 * s + n)
            vals[sub, n] = rng.standard_normal((size, size)).astype(np.float32)
            save_pfm(os.path.join(root, sub, f"{n}.pfm"), vals[sub, n])
    return vals


def test_patch_file_dataset_order_and_pointer(tmp_path):
    """6 patches numbered 3..8, batches of 2: unshuffled batches walk the numbers in order, the pointer advances
    by the batch size and reset_pointer starts over (data_generator.py:47-60, 105-116)."""
    from scenedepthestimation_amd.training import PatchFileDataset
    root = str(tmp_path)
    vals = _write_patches(root, range(3, 9))
    paths = [os.path.join(root, sub, "{}.pfm") for sub in ("left", "right_pos", "right_neg")]
    ds = PatchFileDataset(*paths, 3, 9, patch_size=(3, 3), batch_size=2, shuffle=False)
    assert ds.dataset_size == 3 and ds.pointer == 0
    assert list(ds.patches_list) == [0, 1, 2, 3, 4, 5]
    for b in range(3):
        batch = ds.next_batch()
        assert ds.pointer == 2 * (b + 1)
        for arr, sub in zip(batch, ("left", "right_pos", "right_neg")):
            assert arr.shape == (2, 3, 3, 1) and arr.dtype == np.float32
            for i in range(2):
                assert np.array_equal(arr[i, :, :, 0], vals[sub, 3 + 2 * b + i])
    ds.reset_pointer()
    assert ds.pointer == 0
    assert np.array_equal(ds.next_batch()[0][0, :, :, 0], vals["left", 3])
    # shuffled: a permutation from NumPy's global state, redrawn by reset_pointer
    np.random.seed(5)
    expect = np.random.permutation(6)
    np.random.seed(5)
    sh = PatchFileDataset(*paths, 3, 9, patch_size=(3, 3), batch_size=2, shuffle=True)
    assert np.array_equal(sh.patches_list, expect)
    assert np.array_equal(sh.next_batch()[2][1, :, :, 0], vals["right_neg", 3 + expect[1]])


# ---------------------------------------------------------------------------------------------------------
# TripletSampler
# ---------------------------------------------------------------------------------------------------------
def _check_rows(rows, left, half, zero_is_invalid, right=None):
    H, W = left.shape
    for y, x, xp, xn in rows:
        d = left[y, x]
        assert np.isfinite(d) and (d != 0 or not zero_is_invalid)
        assert half <= y < H - half and half <= x < W - half
        assert d + half <= x
        rc = x - d
        for c in (xp, xn):
            assert half <= c < W - half
        assert rc - 0.501 - 1 < xp <= rc + 0.501
        assert (rc + 1.5 - 1 < xn <= rc + 6) or (rc - 6 - 1 < xn <= rc - 1.5)
        if right is not None:
            rd = right[y, int(rc)]
            assert np.isfinite(rd) and (rd != 0 or not zero_is_invalid) and abs(rd - d) <= 1


def test_triplet_sampler_rule_and_seed():
    from scenedepthestimation_amd.synthetic import stereo_pair
    from scenedepthestimation_amd.training import TripletSampler
    _, _, gt = stereo_pair(64, 160, 32, 7)
    a = TripletSampler(gt, patch=11, seed=3, zero_is_invalid=False).sample(300)
    b = TripletSampler(gt, patch=11, seed=3, zero_is_invalid=False).sample(300)
    c = TripletSampler(gt, patch=11, seed=4, zero_is_invalid=False).sample(300)
    assert a.dtype == np.int32 and a.shape == (300, 4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    _check_rows(a, gt.astype(np.float64), 5, False)
    # both signs of the negative offset occur
    rc = a[:, 1] - gt[a[:, 0], a[:, 1]]
    assert (a[:, 3] > rc).any() and (a[:, 3] < rc).any()


def test_triplet_sampler_sentinels_and_right_map():
    """Zero / infinite disparities are never centres; with a right map, only centres whose right disparity is
    known and within 1."""
    from scenedepthestimation_amd.training import TripletSampler
    H, W = 30, 90
    left = np.full((H, W), 6.5)
    left[:, 40:50] = 0
    left[:, 50:55] = np.inf
    right = np.full((H, W), 6.0)
    right[:, 60:70] = 9.0          # disagrees by more than 1
    right[:, 70:75] = 0            # unknown
    s = TripletSampler(left, right, patch=7, seed=1)
    rows = s.sample(400)
    _check_rows(rows, left, 3, True, right)
    xs = set(rows[:, 1].tolist())
    assert not xs & set(range(40, 55))
    assert not {x for x in xs if 60 <= int(x - 6.5) < 75}
    assert xs - set(range(0, 40)), "centres right of the masked band exist"
    with pytest.raises(ValueError):
        TripletSampler(np.zeros((H, W)), patch=7)


# ---------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------
def test_cli_defaults_equal_the_reference():
    from scenedepthestimation_amd import train
    a = train.make_parser().parse_args([])
    assert (a.gpu, a.patch_size, a.batch_size, a.margin, a.learning_rate, a.beta) == ("0,1,2,3,4,5,6", 11, 128, 0.3,
                                                                                    0.001, 0.9)
    assert (a.resume, a.start_epoch, a.end_epoch, a.print_freq, a.save_freq, a.val_freq) == (None, 3, 14, 1, 1, 1)
    assert (a.data, a.steps_per_epoch, a.checkpoint_dir) == ("pfm:./training_data_set", None, "./check_points_mr30")
    b = train.make_parser().parse_args("-g 2 -ps 7 -bs 16 -mr 0.2 -lr 0.01 -bt 0.5 --resume x.npz".split())
    assert (b.gpu, b.patch_size, b.batch_size, b.margin, b.learning_rate, b.beta, b.resume) == ("2", 7, 16, 0.2, 0.01,
                                                                                              0.5, "x.npz")
    assert (train.TRAIN_HEAD, train.TRAIN_TAIL, train.VAL_HEAD, train.VAL_TAIL) == (0, 1898240, 1898359, 2089591)


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
TRAIN_FUNCS = ["sde_train_param_floats", "sde_train_workspace_bytes", "sde_train_gather", "sde_train_loss_grad",
               "sde_train_export_activations", "sde_train_momentum"]


def test_abi_declares_and_binds_training():
    from scenedepthestimation_amd import _lib
    declared = set(_lib.header_functions())
    for f in TRAIN_FUNCS:
        assert f in declared and f in _lib.SIGNATURES, f
    assert _lib.lib.sde_abi_version() == 4 == _lib.SDE_ABI_VERSION


def test_param_blob_size_and_order():
    from scenedepthestimation_amd import _lib, mc_cnn, training
    lib = _lib.lib
    for L in range(1, 6):
        assert lib.sde_train_param_floats(L, NF) == 640 + (L - 1) * (9 * NF * NF + NF)
    w = mc_cnn.synthetic_weights(3, seed=2)
    blob = training.flatten(w, 3)
    assert blob.size == lib.sde_train_param_floats(3, NF)
    assert np.array_equal(blob[:576], w["conv1/weights:0"].ravel())
    assert np.array_equal(blob[576:640], w["conv1/biases:0"])
    assert np.array_equal(blob[640:640 + 36864], w["conv2/weights:0"].ravel())
    back = training.unflatten(blob, 3)
    assert all(np.array_equal(back[k], w[k]) for k in w)


def test_abi_refuses_bad_arguments():
    """Every refusal comes before any launch, so host addresses (never dereferenced) stand in for device ones."""
    from scenedepthestimation_amd import _lib
    lib, ARG = _lib.lib, -1
    buf = np.zeros(64, np.float32)
    p = (buf.ctypes.data + 15) & ~15                      # 16-byte aligned, inside buf
    f = ctypes.c_float
    for L, nf in ((0, NF), (6, NF), (5, 32), (5, 128)):
        assert lib.sde_train_param_floats(L, nf) == -1
        assert lib.sde_train_workspace_bytes(4, L, nf) == -1
        assert lib.sde_train_loss_grad(p, 4, p, L, nf, f(0.3), p, p, p, 1 << 40, None) == ARG
        assert lib.sde_train_export_activations(p, 4, L, nf, 1, p, None) == ARG
    for L in (0, 6):
        assert lib.sde_train_gather(p, p, 8, 8, p, 4, L, p, None) == ARG
    for B in (0, -3, 1 << 30):            # B = 2^30: offsets past 2^31
        assert lib.sde_train_workspace_bytes(B, 5, NF) == -1
        assert lib.sde_train_gather(p, p, 8, 8, p, B, 5, p, None) == ARG
        assert lib.sde_train_loss_grad(p, B, p, 5, NF, f(0.3), p, p, p, 1 << 40, None) == ARG
        assert lib.sde_train_export_activations(p, B, 5, NF, 1, p, None) == ARG
    need = lib.sde_train_workspace_bytes(4, 5, NF)
    assert need > 0
    assert lib.sde_train_loss_grad(p, 4, p, 5, NF, f(0.3), p, p, p, need - 1, None) == ARG       # short workspace
    for off in (4, 8, 12):                               # params / workspace not 16-byte aligned (float4 loads)
        assert lib.sde_train_loss_grad(p, 4, p + off, 5, NF, f(0.3), p, p, p, need, None) == ARG
        assert lib.sde_train_loss_grad(p, 4, p, 5, NF, f(0.3), p, p, p + off, need + 16, None) == ARG
    for hole in range(4):                                                                        # null pointers
        a = [p, p, p, p]
        a[hole] = None
        assert lib.sde_train_loss_grad(a[0], 4, a[1], 5, NF, f(0.3), a[2], p, a[3], need, None) == ARG
        g = [p, p, p, p]
        g[hole] = None
        assert lib.sde_train_gather(g[0], g[1], 8, 8, g[2], 4, 5, g[3], None) == ARG
    assert lib.sde_train_gather(p, p, 0, 8, p, 4, 5, p, None) == ARG
    assert lib.sde_train_export_activations(None, 4, 5, NF, 1, p, None) == ARG
    assert lib.sde_train_export_activations(p, 4, 5, NF, 1, None, None) == ARG
    for layer in (0, 6):
        assert lib.sde_train_export_activations(p, 4, 5, NF, layer, p, None) == ARG
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert lib.sde_train_momentum(a[0], a[1], a[2], 8, f(1e-3), f(0.9), None) == ARG
    assert lib.sde_train_momentum(p, p, p, 0, f(1e-3), f(0.9), None) == ARG


# ---------------------------------------------------------------------------------------------------------
# the momentum rule the GPU test compares against
# ---------------------------------------------------------------------------------------------------------
def fma_sensitive_case():
    """(p, v, g, lr, beta) where contracting beta*v + g into one FMA changes the result: g cancels the ROUNDED
    product, so the separately rounded sum is exactly 0 and the fused one is the product's rounding error (about
    2^-25 here).  p = 2^-20 has an ulp of 2^-43, so lr times that error moves p as well."""
    beta, v = np.float32(0.9), np.float32(3.0000002)
    g = -np.float32(beta * v)
    return np.float32(2.0 ** -20), v, g, np.float32(0.25), beta


def test_momentum_rule_is_separately_rounded():
    p, v, g, lr, beta = fma_sensitive_case()
    exact = np.float64(beta) * np.float64(v)           # 48 significant bits at most: exact in float64
    assert np.float64(np.float32(exact)) != exact, "the product must need rounding"
    fused_v = np.float32(exact + np.float64(g))        # the cancellation leaves few bits: exact, then one rounding
    p1, v1 = tl.momentum_np(p, v, g, lr, beta)
    assert v1 == np.float32(0) and fused_v != 0
    assert p1 == p
    assert np.float32(p - np.float32(lr * fused_v)) != p1, "a fused update must move p too"
    # hand-made values, every intermediate written out
    p, v, g = np.float32([1.0, -2.0, 0.5]), np.float32([0.5, 0.25, -1.0]), np.float32([0.125, 1.0, 0.3])
    p1, v1 = tl.momentum_np(p, v, g, 0.1, 0.9)
    b, l = np.float32(0.9), np.float32(0.1)
    for i in range(3):
        vi = np.float32(np.float32(b * v[i]) + g[i])
        assert v1[i] == vi and p1[i] == np.float32(p[i] - np.float32(l * vi))
    assert p1.dtype == v1.dtype == np.float32
