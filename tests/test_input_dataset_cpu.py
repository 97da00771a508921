"""CPU tests of the device-resident dataset: the gather/normalise/resize entry point is exported, bound and reports argument
errors as statuses before any HIP call; EpochPlan (pure host code) orders, shards and batches an epoch; DeviceDataset refuses to
run without a GPU.  No device work is launched here."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bg_u8_gather_normalize_resize_f32"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge._load_build_module().build_lib(verbose=False)
    from blurred_gan_amd import _lib
    return _lib.load()


def test_symbol_is_exported_declared_and_bound(lib):
    from blurred_gan_amd import _lib
    assert hasattr(lib, NAME)
    assert NAME in open(os.path.join(ROOT, "include", "bgan.h")).read()
    res, args = _lib.SIGNATURES[NAME]
    p, i = _lib._p, _lib._i
    assert res is i and args == [p, i, p, p, p, i, i, i, i, i, i, p]     # src, N, idx_d, flip_d, dst, B, Hs, Ws, C, Hd, Wd, stream
    assert lib.bg_version() == 5 and _lib.ABI_VERSION == 5               # an addition: the ABI version stays


def test_argument_errors_are_statuses(lib):
    fn = getattr(lib, NAME)
    src, idx, dst = 0x1000, 0x2000, 0x3000          # never dereferenced: every check below fails before the first HIP call
    ok = (4, idx, None, dst, 3, 9, 11, 3, 5, 7, None)
    for k in (1, 3):                                 # idx_d, dst
        a = list(ok)
        a[k] = None
        assert fn(src, *a) == -6
        assert NAME.encode() in lib.bg_last_error()
    assert fn(None, *ok) == -6
    for k in (0, 4, 5, 6, 7, 8, 9):                  # N, B, Hs, Ws, C, Hd, Wd
        for bad in (0, -1):
            a = list(ok)
            a[k] = bad
            assert fn(src, *a) == -1, k
            assert NAME.encode() in lib.bg_last_error()
    a = list(ok)
    a[3] = dst + 4                                   # the 16-byte stores need an aligned destination
    assert fn(src, *a) == -2
    assert b"16-byte" in lib.bg_last_error()


def test_epoch_plan_batches_and_coverage():
    from blurred_gan_amd import EpochPlan
    p = EpochPlan(10, 4, shuffle=True, seed=3, epoch=0)
    assert p.batch_sizes == [4, 4, 2] and len(p) == 3
    assert p.bounds == [(0, 4), (4, 8), (8, 10)]
    assert p.indices.dtype == np.int32 and sorted(p.indices.tolist()) == list(range(10))
    q = EpochPlan(10, 4, shuffle=True, seed=3, epoch=0, drop_remainder=True)
    assert q.batch_sizes == [4, 4] and np.array_equal(q.indices, p.indices)
    assert EpochPlan(8, 4, drop_remainder=False).batch_sizes == [4, 4]


def test_epoch_plan_epochs_differ_and_repeat():
    from blurred_gan_amd import EpochPlan
    e0, e1 = EpochPlan(10, 4, seed=5, epoch=0), EpochPlan(10, 4, seed=5, epoch=1)
    assert not np.array_equal(e0.indices, e1.indices)
    assert np.array_equal(e0.indices, EpochPlan(10, 4, seed=5, epoch=0).indices)
    assert np.array_equal(e1.indices, EpochPlan(10, 4, seed=5, epoch=1).indices)
    assert np.array_equal(e1.indices, np.random.default_rng([5, 1]).permutation(10))
    assert not np.array_equal(e0.indices, EpochPlan(10, 4, seed=6, epoch=0).indices)


def test_epoch_plan_shards_are_disjoint_slices_of_one_permutation():
    from blurred_gan_amd import EpochPlan
    perm = np.random.default_rng([7, 2]).permutation(10)
    shards = [EpochPlan(10, 2, seed=7, epoch=2, rank=r, world_size=3).indices for r in range(3)]
    for r, s in enumerate(shards):
        assert len(s) == 3 and np.array_equal(s, perm[3 * r:3 * r + 3])
    sets = [set(s.tolist()) for s in shards]
    assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])
    assert EpochPlan(10, 2, seed=7, epoch=2, rank=1, world_size=3).batch_sizes == [2, 1]


def test_epoch_plan_unshuffled_is_arange_and_bad_arguments_raise():
    from blurred_gan_amd import EpochPlan
    assert np.array_equal(EpochPlan(10, 4, shuffle=False, epoch=3).indices, np.arange(10))
    assert np.array_equal(EpochPlan(10, 4, shuffle=False, rank=1, world_size=2).indices, np.arange(5, 10))
    for kw in (dict(N=0, batch_size=4), dict(N=4, batch_size=0), dict(N=4, batch_size=2, rank=2, world_size=2),
               dict(N=2, batch_size=1, rank=0, world_size=3)):
        with pytest.raises(ValueError):
            EpochPlan(**kw)


def test_device_dataset_needs_a_gpu(monkeypatch):
    from blurred_gan_amd import DeviceDataset, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # what a machine without a GPU answers
    with pytest.raises(ops.BgDeviceError, match="no host-side fallback"):
        DeviceDataset(np.zeros((4, 8, 8, 3), np.uint8), batch_size=2)


def test_device_dataset_rejects_host_tensors_and_other_dtypes():
    from blurred_gan_amd import DeviceDataset, ops
    with pytest.raises(ops.BgDeviceError):
        DeviceDataset(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), batch_size=2)
    with pytest.raises(ValueError, match="uint8"):
        DeviceDataset(np.zeros((4, 8, 8, 3), np.float32), batch_size=2)
    with pytest.raises(ValueError, match="shape"):
        DeviceDataset(np.zeros((4, 8), np.uint8), batch_size=2)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gather_kernels_do_not_spill_and_store_16_bytes(tmp_path):
    import re
    import subprocess
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "input.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "blurred-gan_amd", "csrc", "input.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    names = sorted(set(re.findall(r"\.name:\s+(\S*u8_gather_resize_\w+_kernel\S*)\n", isa)))
    assert len(names) == 4, names                  # 16-byte paths for C = 1, 3, 4 and the any-C kernel
    for m in re.finditer(r"\.name:\s+(\S*_kernel\S*)\n(.*?)\.wavefront_size", isa, flags=re.S):
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
            assert v and int(v.group(1)) == 0, (m.group(1), key)       # no spills, no scratch
    assert set(re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa)) == {"0"}      # and no LDS
    for name in names:
        body = re.search(r"^" + re.escape(name) + r":(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
        assert ("global_store_dwordx4" in body) == ("vec_kernel" in name), name
