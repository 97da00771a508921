"""Host side of the opt-in split-bf16 conv math: the C ABI entries and the dispatch query, the Python surface (ops, WGAN keyword,
step key), and the split kernel's code object (bf16 MFMAs only, no fp32 MFMA)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# celeba64 (C2) conv geometries at B 256: (H, W, Cin, Cout), stride 2
C2_CONVS = [(64, 64, 3, 32), (32, 32, 32, 64), (16, 16, 64, 128), (8, 8, 128, 256), (4, 4, 256, 512), (8, 8, 256, 512),
            (16, 16, 128, 256), (32, 32, 64, 128), (64, 64, 32, 64)]


@pytest.fixture(scope="module")
def lib():
    from blurred_gan_amd import _lib
    return _lib.load()


def test_new_symbols_are_exported_declared_and_bound(lib):
    from blurred_gan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bgan.h")).read()
    for name in ("bg_conv2d_fwd_math", "bg_conv2d_bwd_data_math", "bg_conv2d_math_taken"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "BG_CONV_MATH_FP32 = 0" in hdr and "BG_CONV_MATH_BF16X6 = 1" in hdr
    assert lib.bg_version() == 5


def test_math_taken_answers_for_the_c2_layers(lib):
    from blurred_gan_amd import ops
    taken = set()
    for bwd in (0, 1):
        for (H, W, Ci, Co) in C2_CONVS:
            assert lib.bg_conv2d_math_taken(bwd, 256, H, W, Ci, Co, 5, 2, 0) == 0
            assert not ops.conv2d_math_taken(bwd, 256, H, W, Ci, Co, 5, 2, "fp32")
            t = lib.bg_conv2d_math_taken(bwd, 256, H, W, Ci, Co, 5, 2, 1)
            assert t in (0, 1)
            if t:
                taken.add((bwd, H, W, Ci, Co))
    # the measured table: the data gradients of the G4 and G5 transposed convs; every other layer stays fp32
    assert taken == {(0, 32, 32, 64, 128), (0, 64, 64, 32, 64)}
    assert lib.bg_conv2d_math_taken(0, 256, 32, 32, 64, 128, 5, 2, 7) == 0
    assert lib.bg_conv2d_math_taken(0, 0, 32, 32, 64, 128, 5, 2, 1) == 0


def test_unknown_math_is_an_error(lib):
    from blurred_gan_amd import ops
    for bad in ("bf16", "fp16", "", None, 1):
        with pytest.raises(ValueError):
            ops.conv_math_code(bad)
    # the C entries refuse an unknown mode with a status before touching any pointer
    assert lib.bg_conv2d_fwd_math(None, None, None, 2, 8, 8, 32, 32, 5, 2, None, None, 5) != 0
    assert lib.bg_conv2d_bwd_data_math(None, None, None, 2, 8, 8, 32, 32, 5, 2, None, None, -1) != 0
    # a null pointer in the split mode is the plain entry's error, not a crash
    assert lib.bg_conv2d_fwd_math(None, None, None, 2, 32, 32, 64, 128, 5, 2, None, None, 1) != 0


def _wgan(**kw):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=1.0, batch_size=4, global_batch_size=4)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), **kw)


def test_wgan_rejects_an_unknown_conv_math():
    with pytest.raises(ValueError):
        _wgan(conv_math="bf16")
    gan = _wgan()
    assert gan.conv_math == "fp32"
    with pytest.raises(ValueError):
        gan.conv_math = "tf32"
    assert gan.conv_math == "fp32"


def test_step_key_differs_between_modes():
    import torch
    gan = _wgan()
    from blurred_gan_amd.models import IMAGE_SHAPE
    reals = torch.zeros((4,) + tuple(IMAGE_SHAPE["tiny"]))
    k32 = gan._step_key("d", reals)
    gan.conv_math = "bf16x6"
    kx6 = gan._step_key("d", reals)
    assert k32 != kx6
    assert gan.generator.net().conv_math == "bf16x6" and gan.discriminator.net().conv_math == "bf16x6"
    gan.conv_math = "fp32"
    assert gan._step_key("d", reals) == k32


@pytest.fixture(scope="module")
def x6_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "x6.s")
    src = os.path.join(ROOT, "blurred-gan_amd", "csrc", "conv_igemm_x6.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", src, "-o", out],
                   check=True, capture_output=True)
    return open(out).read()


def test_split_kernel_runs_on_bf16_mfma_only(x6_isa):
    bodies = re.findall(r"^(_Z\S*conv_igemm_x6\S*):[^\n]*\n(.*?)\n\.Lfunc_end", x6_isa, re.S | re.M)
    assert len(bodies) >= 3, [b[0] for b in bodies]
    for name, body in bodies:
        bf16 = re.findall(r"v_mfma_f32_(?:32x32x16|16x16x32)_bf16\b", body)
        assert bf16, name
        assert len(bf16) % 6 == 0, (name, len(bf16))          # six products per operand pair
        every = re.findall(r"\bv_mfma\w*", body)
        assert every == bf16, (name, sorted(set(every) - set(bf16)))      # no fp32 (v_mfma_f32_32x32x2_f32 ...) nor any other MFMA
