"""GPU tests of the device-resident dataset (blurred_gan_amd/data.py, include/bgan.h bg_u8_gather_normalize_resize_f32): the
one-launch gather -> normalise -> bilinear resize -> mirror kernel against the oracle and, bit for bit, against itself on a
pre-gathered batch and against the dense kernel it extends; DeviceDataset's epochs, sharding-free single-rank order, flip flags,
chunked upload and ring contract; and a two-epoch ``fit`` that must leave exactly the weights ``train_on_batch`` leaves."""
import math

import numpy as np
import pytest
import torch

from oracle import np_ops as O

pytestmark = pytest.mark.gpu

# (Hs, Ws) -> (Hd, Wd), C
GEOMETRIES = [
    ((218, 178), (128, 128), 3),      # CelebA's own non-integer downscale
    ((28, 28), (28, 28), 1),          # identity
    ((16, 20), (40, 33), 3),          # upscale, odd width
    ((9, 11), (5, 7), 3),             # 315 output floats: the 16-byte path has a 3-element tail (one pixel)
    ((9, 11), (5, 7), 2),             # a channel count without a 16-byte path: the one-pixel-per-thread kernel
]
N, B, IDX, FLIP = 4, 3, [3, 0, 3], [1, 0, 1]
MARGIN = 64                           # floats on either side of dst: 256 bytes, so dst stays 16-byte aligned


def _run(src_d, idx, shape, flip=None):
    """One launch into the middle of a zero-filled buffer; returns (dst view, whole buffer)."""
    from blurred_gan_amd import ops
    n = math.prod(shape)
    big = torch.zeros(n + 2 * MARGIN, device="cuda")
    dst = big[MARGIN:MARGIN + n].view(shape)
    assert dst.data_ptr() % 16 == 0
    ops.u8_gather_normalize_resize(src_d, torch.tensor(idx, dtype=torch.int32, device="cuda"), dst,
                                   None if flip is None else torch.tensor(flip, dtype=torch.uint8, device="cuda"))
    return dst, big


@pytest.mark.parametrize("src_hw,dst_hw,C", GEOMETRIES)
def test_kernel_parity_gather_mirror_and_bounds(src_hw, dst_hw, C):
    from blurred_gan_amd import ops
    src = np.random.default_rng(9).integers(0, 256, size=(N, *src_hw, C), dtype=np.uint8)
    src_d = torch.from_numpy(src).cuda()
    shape = (B, *dst_hw, C)
    out, big = _run(src_d, IDX, shape)
    # 1. the oracle, at the tolerance the dense kernel is held to (tests/test_misc_gpu.py), and the value range
    ref = O.normalize_resize_bilinear(src[IDX], dst_hw)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=2e-6)
    assert float(out.min()) >= -1 - 1e-6 and float(out.max()) <= 1 + 1e-6
    if src_hw == dst_hw:
        assert torch.equal(out.cpu(), (torch.from_numpy(src[IDX]).float() - 127.5) / 127.5)
    # 4. nothing outside dst
    assert not big[:MARGIN].any() and not big[-MARGIN:].any()
    # 2. the gather is exact: the same entry point on the pre-gathered batch, and the dense kernel on it
    gathered = torch.from_numpy(np.ascontiguousarray(src[IDX])).cuda()
    dense, _ = _run(gathered, list(range(B)), shape)
    assert torch.equal(out, dense)
    assert torch.equal(out, ops.u8_normalize_resize(gathered, torch.empty(shape, device="cuda")))
    # 3. the mirror is exact, and no flags = all-zero flags
    flipped, big_f = _run(src_d, IDX, shape, FLIP)
    mirror = torch.flip(out, dims=[2])
    assert torch.equal(flipped[0], mirror[0]) and torch.equal(flipped[2], mirror[2]) and torch.equal(flipped[1], out[1])
    assert not big_f[:MARGIN].any() and not big_f[-MARGIN:].any()
    zeros, _ = _run(src_d, IDX, shape, [0, 0, 0])
    assert torch.equal(zeros, out)


def test_normalisation_is_the_ieee_quotient_for_every_byte():
    """The kernel forms (x - 127.5) / 127.5 without a division instruction sequence; every one of the 256 bytes must come out as
    the correctly rounded float32 quotient (what the dense kernel's division and the host's give), at the identity size."""
    from blurred_gan_amd import ops
    src = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1)
    out, _ = _run(src.cuda(), [0], (1, 16, 16, 1))
    assert torch.equal(out.cpu(), (src.float() - 127.5) / 127.5)
    assert torch.equal(out, ops.u8_normalize_resize(src.cuda(), torch.empty(1, 16, 16, 1, device="cuda")))


def test_image_offsets_are_formed_in_64_bits():
    """A dataset of more than 2^31 bytes: the last image starts past the reach of a 32-bit byte offset."""
    Hs, Ws, C, n = 256, 256, 4, 8200
    assert (n - 1) * Hs * Ws * C > 2 ** 31
    data = torch.empty((n, Hs, Ws, C), dtype=torch.uint8, device="cuda")
    pick = [n - 1, 0, 8192]                                   # 8192 * 262144 = 2^31 exactly
    imgs = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=(3, Hs, Ws, C), dtype=np.uint8)).cuda()
    for i, p in enumerate(pick):
        data[p].copy_(imgs[i])
    out, _ = _run(data, pick, (3, 8, 8, C))
    dense, _ = _run(imgs, [0, 1, 2], (3, 8, 8, C))
    assert torch.equal(out, dense)


# ------------------------------------------------------------------ DeviceDataset
def _ids(batch):
    """Images filled with their own index: the index back out of a normalised batch."""
    return torch.round(batch[:, 0, 0, 0] * 127.5 + 127.5).to(torch.int64).cpu().tolist()


def _self_naming(n, h=4, w=5, c=3):
    return np.broadcast_to(np.arange(n, dtype=np.uint8)[:, None, None, None], (n, h, w, c)).copy()


def test_epochs_cover_the_dataset_reshuffle_and_repeat():
    from blurred_gan_amd import DeviceDataset, EpochPlan
    imgs = _self_naming(10)
    ds = DeviceDataset(imgs, batch_size=4, seed=3)
    assert len(ds) == 3 and ds.samples_per_epoch == 10 and ds.epoch == 0
    epochs = []
    for _ in range(2):
        batches = [b.clone() for b in ds]
        assert [b.shape[0] for b in batches] == [4, 4, 2] and tuple(batches[0].shape[1:]) == (4, 5, 3)
        epochs.append(batches)
    assert ds.epoch == 2
    order = [sum((_ids(b) for b in e), []) for e in epochs]
    assert sorted(order[0]) == list(range(10)) and sorted(order[1]) == list(range(10)) and order[0] != order[1]
    for e in (0, 1):
        assert order[e] == EpochPlan(10, 4, seed=3, epoch=e).indices.tolist()
    again = DeviceDataset(imgs, batch_size=4, seed=3)
    for e in range(2):
        for a, b in zip(epochs[e], again):
            assert torch.equal(a, b)
    again.epoch = 0                                           # a resumed run sets the epoch
    assert torch.equal(next(iter(again)), epochs[0][0])
    assert len(DeviceDataset(imgs, batch_size=4, drop_remainder=True)) == 2
    unshuffled = DeviceDataset(torch.from_numpy(imgs).cuda(), batch_size=4, shuffle=False)      # a device tensor is used in place
    assert sum((_ids(b) for b in unshuffled), []) == list(range(10))


def test_flip_flags_are_the_documented_keep_mask_draw():
    from blurred_gan_amd import DeviceDataset, ops
    imgs = _self_naming(10, 4, 6, 1)
    imgs[:, :, 3:] += 100                                     # right half = index + 100: a mirrored sample starts with it
    ds = DeviceDataset(imgs, batch_size=4, seed=11, flip=True, shuffle=False)
    assert ds.flip_seed == 11 and ds.flip_offset(0) == 0 and ds.flip_offset(1) == 3      # ceil(10 / 4) Philox blocks per epoch
    for epoch in range(2):
        first = sum((_ids(b) for b in ds), [])
        want = ops.keep_mask(torch.empty(10, dtype=torch.uint8, device="cuda"), 0.5, ds.flip_seed, ds.flip_offset(epoch)).cpu().tolist()
        assert [f - i for i, f in enumerate(first)] == [100 * int(w != 0) for w in want], epoch


def test_chunked_upload_from_a_file_equals_the_array(tmp_path):
    from blurred_gan_amd import DeviceDataset
    arr = np.random.default_rng(2).integers(0, 256, size=(10, 5, 6, 3), dtype=np.uint8)
    path = tmp_path / "images.npy"
    np.save(path, arr)
    by_path = DeviceDataset(str(path), batch_size=4, chunk_bytes=4 * 90)      # 4 images per chunk: 4 + 4 + 2
    direct = DeviceDataset(arr, batch_size=4)
    assert by_path.data.dtype == torch.uint8 and torch.equal(by_path.data, direct.data)
    assert torch.equal(by_path.data.cpu(), torch.from_numpy(arr))
    for a, b in zip(by_path, direct):
        assert torch.equal(a, b)
    grey = DeviceDataset(arr[..., 0], batch_size=4, chunk_bytes=1)            # [N,H,W]: one channel; a chunk is at least one image
    assert tuple(grey.data.shape) == (10, 5, 6, 1) and torch.equal(grey.data.cpu()[..., 0], torch.from_numpy(arr[..., 0]))


def test_size_limit_raises():
    from blurred_gan_amd import DeviceDataset
    with pytest.raises(ValueError, match=r"needs 300 bytes .* at most 1 "):
        DeviceDataset(np.zeros((4, 5, 5, 3), np.uint8), batch_size=2, max_bytes=1)


def test_ring_contract():
    from blurred_gan_amd import DeviceDataset
    ds = DeviceDataset(_self_naming(10), batch_size=4, buffers=2, seed=1)
    it = iter(ds)
    b0 = next(it)
    keep0 = b0.clone()
    b1 = next(it)
    keep1 = b1.clone()
    assert torch.equal(b0, keep0) and b1.data_ptr() != b0.data_ptr()           # batch k is untouched after batch k + 1 ...
    b2 = next(it)
    assert b2.shape[0] == 2 and b2.data_ptr() == b0.data_ptr()                  # ... and shares storage with batch k + 2 (short: a leading view)
    assert torch.equal(b1, keep1)
    with pytest.raises(StopIteration):
        next(it)
    b3 = next(iter(ds))                                                         # the ring goes on across epochs
    assert b3.data_ptr() == b1.data_ptr()


# ------------------------------------------------------------------ through fit
def _gan(tmp_path, tag, **kw):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(77)
    gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=4, batch_size=4)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir=str(tmp_path / tag)), **kw)


@pytest.mark.parametrize("persistent_input", [False, True])
def test_fit_trains_every_epoch_and_equals_train_on_batch(tmp_path, persistent_input):
    from blurred_gan_amd import DeviceDataset
    imgs = np.random.default_rng(4).integers(0, 256, size=(12, 11, 9, 3), dtype=np.uint8)
    make = lambda: DeviceDataset(imgs, image_size=8, batch_size=4, seed=5)
    gan = _gan(tmp_path, "fit", persistent_input=persistent_input)
    history = gan.fit(make(), epochs=2)
    assert int(gan.n_img) == 24 and int(gan.n_batches) == 6 and len(history) == 2
    for logs in history:
        assert all(math.isfinite(float(logs[k])) for k in gan.metrics_names), logs
    assert gan._programs.stats["replayed"] >= 2, gan._programs.stats
    if persistent_input:
        assert gan._reals_stage is None
    ref = _gan(tmp_path, "ref")
    ds = make()
    for _ in range(2):
        for batch in ds:
            ref.train_on_batch(batch.clone())
    assert int(ref.n_batches) == 6
    for a, b in ((gan.generator, ref.generator), (gan.discriminator, ref.discriminator)):
        for name in ("theta", "state"):
            assert torch.equal(getattr(a.store, name), getattr(b.store, name)), name


def test_demo_trains_from_a_dataset_file(tmp_path):
    """demo_mnist --dataset PATH --flip: a uint8 [N,H,W] file, resized to the model's 28x28 input; both epochs train."""
    import demo_mnist
    path = tmp_path / "digits.npy"
    np.save(path, np.random.default_rng(6).integers(0, 256, size=(10, 20, 24), dtype=np.uint8))
    gan = demo_mnist.main(["--dataset", str(path), "--flip", "--batch_size", "4", "--epochs", "2", "--max_batches", "2",
                           "--results_dir", str(tmp_path / "results")])
    assert int(gan.n_batches) == 4 and int(gan.n_img) == 16 and gan.persistent_input
    assert tuple(gan.images[1].shape[1:]) == (28, 28, 1)
