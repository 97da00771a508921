"""GPU parity of the conv family at kernel sizes 1 and 3 (include/bgan.h promises every odd k with k*k <= 25; every other conv test
passes 5): forward / data gradient / filter gradient against the float64 oracle with the bounds of tests/test_conv_gpu.py, on a
hand-written table that reaches every kernel family the dispatcher can send k != 5 to and every shape where a 5x5-only fast path must
step aside.  Each hand-written case also PINS ITS ROUTE: the launches are recorded (ops.prof_*) and their names must be the ones the
dispatcher is expected to pick, so the table cannot drift onto one family unnoticed.

Routes are derived from the dispatch code (conv_igemm.hip run_gather / bg_conv2d_fwd / bg_conv2d_bwd_data, conv_rows.hip
try_conv_rows / try_conv_rows_gather, conv_wgrad.hip plan_wgrad).  The profile names do not tell every variant apart: all gather-GEMM
tiles / K steps / orders are "conv_igemm_*" (split-K shows as the extra "conv_igemm_splitk_reduce" launch), the generic filter
gradient modes 1..5 are all "conv_wgrad_mfma", and the row-MFMA filter gradients (modes 31 / 30) share their name with the generic thin
kernels (modes 10..12 / 20..22).  Modes 31 / 30 are therefore pinned by their name AND by the number of slabs the workspace query
plans for them (one per workgroup: max(2, min(blocks, 1024))), which the generic plans do not produce on these shapes."""
import numpy as np
import pytest
import torch

from oracle import np_ops as O
from helpers import dev, conv_tol

pytestmark = pytest.mark.gpu

IGF, IGD = "conv_igemm_fwd", "conv_igemm_dgrad"
SPLIT = "+splitk"                   # suffix: the gather-GEMM runs split-K (slabs + "conv_igemm_splitk_reduce")
RF, RD = "conv_rows_fwd", "conv_rows_dgrad"                       # scatter-form row kernels (thin output side)
GF, GD = "conv_rows_thin_k_fwd", "conv_rows_thin_k_dgrad"         # gather-form row kernels (thin contraction side)
WG = "conv_wgrad_mfma"              # conv_wgrad_v3_kernel, modes 1..5
WTI, WTO = "conv_wgrad_mfma_thin_ci", "conv_wgrad_mfma_thin_co"   # "@31" / "@30": the row-MFMA kernels, else modes 10..12 / 20..22
WD = "conv_wgrad_direct"

# (B, H, W, Cin, Cout, k, stride, forward route, data-gradient route, filter-gradient route)
CASES = [
    # ---- gather-GEMM.  128x32 tile for N <= 32, else 64x64; K step 16 for 32 / 64 channels per tap, 32 from 128 on
    (2, 8, 8, 32, 32, 3, 2, IGF, IGD, WG),                    # 128x32 both ways, BK 16; filter gradient mode 5
    (3, 8, 8, 32, 64, 3, 1, IGF, IGD, WG),                    # 64x64 / 128x32, BK 16; mode 4
    (2, 16, 16, 64, 128, 3, 2, IGF, IGD, WG),                 # fwd BK 16 (64 ch), dgrad BK 32 (128 ch), 64x64; mode 2
    (2, 4, 4, 128, 256, 3, 2, IGF + SPLIT, IGD, WG),          # BK 32; small M: forward split-K (36 steps); mode 1
    (5, 2, 2, 256, 512, 3, 2, IGF + SPLIT, IGD, WG),          # M = 5: split-K 4; the dgrad's 1-tap phase has 16 steps: unsplit
    (130, 4, 4, 128, 256, 3, 2, IGF + SPLIT, IGD, WG),        # ragged M (520 rows), split-K 2
    (5, 2, 2, 256, 512, 3, 1, IGF + SPLIT, IGD + SPLIT, WG),  # stride 1: nine taps both ways, both split
    (5, 2, 2, 1024, 64, 1, 1, IGF + SPLIT, IGD, WG),          # k = 1: ONE tap of 1024 channels is 32 K steps: split-K 2
    (3, 7, 7, 32, 48, 3, 2, IGF, IGD, WG),                    # ragged M and ragged N (48 of 64); odd map: phases of different extents
    (2, 7, 9, 32, 64, 3, 1, IGF, IGD, WG),
    (3, 9, 7, 48, 24, 3, 2, IGF, "conv_direct_dgrad", WG),    # N = 24 of 32; dy has 24 channels (not 16 | 24): direct; mode 3
    (128, 4, 4, 64, 64, 3, 1, IGF, IGD, WG),                  # position-major tiles (B = 2 x 64, 16 positions): padding taps skipped;
    (128, 8, 8, 32, 64, 3, 2, IGF, IGD, WG),                  # ... filter gradient position-major with the tap-sorted order (9 taps)
    (128, 4, 4, 64, 64, 1, 1, IGF, IGD, WG),                  # ... and with 1 tap
    (128, 8, 8, 32, 64, 1, 2, IGF, IGD, WG),                  # k = 1, stride 2: position-major data gradient with three empty phases
    (1024, 16, 16, 16, 32, 3, 2, IGF, IGD, WG),               # position-major AND phases merged two by two (9+1 and 2+2 taps ... 4/2/2/1 here)
    (1024, 16, 16, 16, 32, 1, 2, IGF, IGD, WG),               # ... at k = 1 the merged pair (1, 2) has NO tap at all
    (520, 16, 16, 16, 32, 1, 2, IGF, IGD, WG),                # merged pairs on image-major tiles, ragged M
    (3, 6, 6, 128, 128, 1, 1, IGF, IGD, WG),                  # k = 1 filter gradient mode 1
    (3, 6, 6, 64, 32, 1, 2, IGF, IGD, WG),                    # ... mode 3; 64x64 data gradient with empty phases
    # ---- thin-channel row kernels at k = 3: thin side 1 / 3 / 4 / 5, wide side 16 / 32 / 64, rows of 16 / 32 / 64 / 128 pixels, ragged strips
    (5, 40, 16, 16, 5, 3, 1, RF, GD, WD),                     # 5 thin channels (15 of 16 MFMA columns); 4 images per workgroup, B = 5; strips 32 + 8
    (3, 20, 32, 32, 3, 3, 1, RF, GD, WTO + "@30"),            # filter gradient: row blocks 16 + 4
    (2, 36, 64, 64, 4, 3, 1, RF, GD, WTO),                    # 64 channels: thin-Co row kernel declines (Ci 16 / 32 only): mode 21
    (2, 20, 128, 16, 1, 3, 1, RF, GD, WTO + "@30"),           # 128-pixel rows (8 waves)
    (5, 32, 32, 3, 32, 3, 2, GF, RD, WTI + "@31"),            # stride 2: dy rows of 16 pixels, 4 images per workgroup
    (3, 40, 64, 5, 16, 3, 2, GF, RD, WD),                     # 5 thin channels; dx strips 16 + 16 + 8, forward strips 8 + 8 + 4
    (2, 44, 128, 4, 64, 3, 2, GF, RD, WTI + "@31"),           # 4 channels (thin_ci's own limit), 64 wide
    (2, 18, 16, 1, 16, 3, 1, GF, RD, WTI + "@31"),            # stride-1 scatter; forward strips 16 + 2
    (2, 24, 256, 3, 16, 3, 2, GF, RD, WTI + "@31"),           # 128-pixel dy rows
    (3, 31, 31, 3, 32, 3, 2, GF, RD, WTI + "@31"),            # odd image: 93 floats per row (scalar staging), dx one pixel short of 2 x 16
    (2, 33, 32, 3, 64, 3, 1, GF, RD, WTI + "@31"),            # strips 32 + 1 / 16 + 16 + 1
    (2, 20, 24, 2, 32, 3, 1, "conv_thin_k_mfma_fwd", "conv_thin_n_patch_dgrad", WTI + "@31"),   # 24-pixel rows: only the filter gradient has a row kernel
    (2, 24, 20, 32, 4, 3, 1, "conv_thin_n_mfma_fwd", "conv_thin_k_mfma_dgrad", WTO + "@30"),
    # ---- the families behind the row kernels
    (2, 12, 20, 16, 5, 3, 1, "conv_thin_n_mfma_fwd", "conv_direct_dgrad", WD),       # N = 5 at k = 3: 15 MFMA columns
    (2, 9, 11, 48, 3, 3, 1, "conv_thin_n_mfma_fwd", "conv_thin_k_mfma_dgrad", WTO),   # 48 channels in three chunks; dgrad 3 -> 48: NT = 2; mode 20
    (2, 9, 11, 20, 12, 1, 1, "conv_thin_n_mfma_fwd", "conv_direct_dgrad", WD),        # k = 1: N = 12 columns, 20 channels (ragged chunk)
    (2, 8, 8, 24, 16, 1, 1, "conv_thin_n_mfma_fwd", IGD, WG),                         # k = 1: all 16 columns
    (2, 8, 8, 3, 16, 1, 1, "conv_thin_k_mfma_fwd", "conv_thin_n_mfma_dgrad", WTI),    # a 1x1 stride-1 data gradient IS a forward rectangle; mode 10
    (3, 14, 14, 1, 64, 3, 2, "conv_thin_k_mfma_fwd", "conv_thin_n_patch_all_dgrad", WTI),     # NT = 2; all four phases from one patch
    (3, 14, 14, 4, 32, 1, 2, "conv_thin_k_mfma_fwd", "conv_thin_n_patch_all_dgrad", WTI),     # ... three of them empty
    (2, 10, 14, 4, 32, 3, 2, "conv_thin_k_mfma_fwd", "conv_thin_n_patch_all_dgrad", WTI),     # 36 rows of taps x channels: mode 11
    (2, 14, 14, 16, 1, 3, 2, "conv_thin_n_patch_fwd", "conv_thin_k_mfma_dgrad", WD),   # stride-2 patch of 33 x 33 x (16 + 4) floats: 87 KB
    (2, 14, 14, 64, 1, 3, 2, "conv_thin_n_fwd", "conv_thin_k_mfma_dgrad", WD),         # ... x (64 + 4): 296 KB, past the 150 KB the patch kernel may take
    (2, 10, 12, 2, 32, 3, 1, "conv_thin_k_mfma_fwd", "conv_thin_n_patch_dgrad", WTI + "@31"),
    (2, 6, 6, 8, 4, 3, 2, "conv_thin_n_fwd", "conv_thin_k_mfma_dgrad", WD),
    (2, 9, 7, 128, 3, 3, 2, "conv_thin_n_fwd", "conv_thin_k_dgrad", WD),              # 128 output channels of a thin contraction: scalar thin-K
    (2, 9, 7, 3, 96, 3, 2, "conv_thin_k_fwd", "conv_thin_n_dgrad", WTI),
    (2, 12, 12, 3, 24, 3, 2, "conv_thin_k_mfma_fwd", "conv_thin_n_dgrad", WTI),       # NT = 1
    (2, 9, 7, 20, 12, 3, 2, "conv_direct_fwd", "conv_direct_dgrad", WD),
    (2, 9, 7, 20, 12, 1, 2, "conv_direct_fwd", "conv_direct_dgrad", WD),
    # ---- shapes of the 5x5-only fast paths at k = 3: the generic kernels must take them
    (3, 64, 64, 16, 32, 3, 2, IGF, IGD, WG),                  # row-staged 16-channel kernels (conv_c16_* / conv_wgrad_c16)
    (2, 128, 128, 16, 32, 3, 2, IGF, IGD, WG),
    (3, 16, 16, 32, 64, 3, 2, IGF, IGD, WG),                  # strip-resident filter gradient: Wo = 8
    (2, 32, 32, 64, 128, 3, 2, IGF, IGD, WG),                 # ... 16
    (2, 64, 64, 32, 64, 3, 2, IGF, IGD, WG),                  # ... 32
    (128, 32, 32, 16, 16, 3, 1, IGF, IGD, WG),                # tap-grouped filter gradient: Ci <= 64, M = 131072
]

# Rows too wide for the row-MFMA filter gradients' 64 KB of LDS (thin-Ci: > 287 pixels of RGB at 5x5 stride 2, > 227 of 4 channels at
# 3x3 stride 1; thin-Co: > 300 of 32 -> 3): the plan must fall back to the generic thin kernels instead of failing at the launch.
WIDE_CASES = [
    (1, 16, 320, 3, 32, 5, 2, "conv_thin_k_mfma_fwd", "conv_thin_n_patch_all_dgrad", WTI),
    (1, 8, 512, 3, 16, 5, 2, "conv_thin_k_mfma_fwd", "conv_thin_n_patch_all_dgrad", WTI),
    (1, 8, 320, 32, 3, 5, 1, "conv_thin_n_mfma_fwd", GD, WTO),
    (1, 8, 256, 4, 32, 3, 1, GF, "conv_thin_n_patch_dgrad", WTI),
]


def _data(B, H, W, Ci, Co, k, s, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(B, H, W, Ci))
    w = rng.uniform(-1, 1, size=(k, k, Ci, Co)) / np.sqrt(k * k * Ci)
    Ho, Wo = -(-H // s), -(-W // s)
    dy = rng.uniform(-1, 1, size=(B, Ho, Wo, Co))
    return x, w, dy


def _kernels(fn):
    from blurred_gan_amd import ops
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.prof_records()]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    return out, names


def _poisoned(shape):
    return torch.full(tuple(shape), float("nan"), device="cuda")


def _splitk_ws(bwd, B, H, W, Ci, Co, k, s):
    from blurred_gan_amd import ops
    nb = ops.conv2d_splitk_workspace_bytes(bwd, B, H, W, Ci, Co, k, s)
    return nb, (torch.empty(nb // 4 + 4, device="cuda") if nb else None)


def _gather_route(route, names, nb):
    if route.endswith(SPLIT):
        assert nb > 0, "the split-K plan asks for no workspace"
        assert names == [route[:-len(SPLIT)], "conv_igemm_splitk_reduce"], names
    else:
        assert names == [route], names


def _wgrad_route(route, names, nb, B, H, W, Ci, Co, k, s):
    name, _, mode = route.partition("@")
    assert names == [name] + (["conv_wgrad_reduce"] if nb else []), names
    nout = k * k * Ci * Co
    assert nb % (4 * nout) == 0
    if mode == "31":                 # one slab per workgroup, a workgroup per block of 8 (stride 2) / 16 output rows
        assert nb // (4 * nout) == max(2, min(B * -(-(-(-H // s)) // (8 if s == 2 else 16)), 1024)), nb // (4 * nout)
    elif mode == "30":               # ... per block of 16 image rows
        assert nb // (4 * nout) == max(2, min(B * -(-H // 16), 1024)), nb // (4 * nout)


def _check_fwd(B, H, W, Ci, Co, k, s, route, seed=0):
    from blurred_gan_amd import ops
    x, w, dy = _data(B, H, W, Ci, Co, k, s, seed)
    ref = O.conv2d_fwd(x, w, s)
    wT = dev(np.transpose(w, (0, 1, 3, 2)))
    nb, ws = _splitk_ws(False, B, H, W, Ci, Co, k, s)
    epi = ops.epilogue(ws=ws) if ws is not None else None
    xd = dev(x)
    y, names = _kernels(lambda: ops.conv2d_fwd(xd, wT, _poisoned(ref.shape), k, s, epi))
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(k * k * Ci, np.abs(ref).max()))
    if route is not None:
        _gather_route(route, names, nb)


def _check_bwd_data(B, H, W, Ci, Co, k, s, route, seed=1):
    from blurred_gan_amd import ops
    x, w, dy = _data(B, H, W, Ci, Co, k, s, seed)
    ref = O.conv2d_bwd_data(dy, w, s, (H, W))
    nb, ws = _splitk_ws(True, B, H, W, Ci, Co, k, s)
    epi = ops.epilogue(ws=ws) if ws is not None else None
    dyd, wd = dev(dy), dev(w)
    dx, names = _kernels(lambda: ops.conv2d_bwd_data(dyd, wd, _poisoned(x.shape), k, s, epi))
    np.testing.assert_allclose(dx.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(k * k * Co, np.abs(ref).max()))
    if route is not None:
        _gather_route(route, names, nb)


def _check_bwd_filter(B, H, W, Ci, Co, k, s, route, seed=2):
    from blurred_gan_amd import ops
    x, w, dy = _data(B, H, W, Ci, Co, k, s, seed)
    ref = O.conv2d_bwd_filter(x, dy, s, k)
    nb = ops.conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, k, s)
    ws = torch.empty(nb // 4 + 4, device="cuda") if nb else None
    dw = _poisoned(w.shape)                                     # beta = 0 must overwrite
    xd, dyd = dev(x), dev(dy)
    _, names = _kernels(lambda: ops.conv2d_bwd_filter(xd, dyd, dw, k, s, 0.0, 1.0, ws))
    K = dy.shape[0] * dy.shape[1] * dy.shape[2]
    tol = conv_tol(K, np.abs(ref).max())
    np.testing.assert_allclose(dw.cpu().numpy(), ref, rtol=1e-4, atol=tol)
    if route is not None:
        _wgrad_route(route, names, nb, B, H, W, Ci, Co, k, s)
    ops.conv2d_bwd_filter(xd, dyd, dw, k, s, 0.5, 2.0, ws)     # accumulate form: dw = 0.5*dw + 2*grad
    torch.cuda.synchronize()
    np.testing.assert_allclose(dw.cpu().numpy(), 2.5 * ref, rtol=1e-4, atol=2.5 * tol)


@pytest.mark.parametrize("B,H,W,Ci,Co,k,s,rf,rd,rw", CASES + WIDE_CASES)
def test_conv_fwd(B, H, W, Ci, Co, k, s, rf, rd, rw):
    _check_fwd(B, H, W, Ci, Co, k, s, rf)


@pytest.mark.parametrize("B,H,W,Ci,Co,k,s,rf,rd,rw", CASES + WIDE_CASES)
def test_conv_bwd_data(B, H, W, Ci, Co, k, s, rf, rd, rw):
    _check_bwd_data(B, H, W, Ci, Co, k, s, rd)


@pytest.mark.parametrize("B,H,W,Ci,Co,k,s,rf,rd,rw", CASES + WIDE_CASES)
def test_conv_bwd_filter(B, H, W, Ci, Co, k, s, rf, rd, rw):
    _check_bwd_filter(B, H, W, Ci, Co, k, s, rw)


def test_the_table_reaches_every_family():
    """The route column names every family of the dispatchers that a k != 5 call can reach (host-side bookkeeping of the table)."""
    fwd = {c[7].replace(SPLIT, "") for c in CASES}
    bwd = {c[8].replace(SPLIT, "") for c in CASES} | {r for (*_, r) in EMPTY_PHASE_CASES}
    flt = {c[9] for c in CASES}
    assert fwd == {IGF, RF, GF, "conv_thin_n_mfma_fwd", "conv_thin_n_patch_fwd", "conv_thin_n_fwd", "conv_thin_k_mfma_fwd", "conv_thin_k_fwd",
                   "conv_direct_fwd"}
    assert bwd == {IGD, RD, GD, "conv_thin_n_mfma_dgrad", "conv_thin_n_patch_all_dgrad", "conv_thin_n_patch_dgrad", "conv_thin_n_dgrad",
                   "conv_thin_k_mfma_dgrad", "conv_thin_k_dgrad", "conv_direct_dgrad"}
    assert flt == {WG, WTI, WTI + "@31", WTO, WTO + "@30", WD}
    assert any(c[7].endswith(SPLIT) for c in CASES) and any(c[8].endswith(SPLIT) for c in CASES)
    assert {c[5] for c in CASES} == {1, 3}


# ------------------------------------------------------------------------------------------------------------------------------------
# k = 1, stride 2: the data gradient (= forward of a 1x1 stride-2 Conv2DTranspose) has ONE tap, in phase (0, 0); the other three
# phases have none and their outputs are exactly epilogue(0 + bias)
# ------------------------------------------------------------------------------------------------------------------------------------
EMPTY_PHASE_CASES = [
    (3, 8, 8, 32, 64, IGD), (3, 7, 9, 32, 64, IGD),                      # 128x32 tile, even / odd map
    (3, 8, 8, 64, 32, IGD), (2, 7, 9, 128, 128, IGD),                    # 64x64 tile, BK 16 / 32
    (128, 8, 8, 32, 64, IGD),                                            # position-major
    (520, 16, 16, 16, 32, IGD),                                          # phases merged in pairs: the pair (1, 2) has no tap at all
    (3, 8, 8, 3, 32, "conv_thin_n_patch_all_dgrad"), (3, 7, 9, 3, 32, "conv_thin_n_patch_all_dgrad"),
    (3, 8, 8, 32, 3, "conv_thin_k_mfma_dgrad"), (3, 7, 9, 32, 3, "conv_thin_k_mfma_dgrad"),
    (2, 9, 7, 3, 8, "conv_thin_n_dgrad"), (2, 9, 7, 128, 3, "conv_thin_k_dgrad"), (2, 9, 7, 20, 12, "conv_direct_dgrad"),
]


@pytest.mark.parametrize("B,H,W,Ci,Co,route", EMPTY_PHASE_CASES)
def test_stride2_1x1_data_gradient_writes_its_empty_phases(B, H, W, Ci, Co, route):
    from blurred_gan_amd import ops
    from blurred_gan_amd._lib import EPI_BIAS_LRELU, EPI_MUL_GRAD, EPI_TANH, EPI_NONE
    k, s = 1, 2
    x, w, dy = _data(B, H, W, Ci, Co, k, s, seed=11)
    rng = np.random.default_rng(12)
    bias = rng.normal(size=Ci)
    b32 = bias.astype(np.float32)
    ref = O.conv2d_bwd_data(dy, w, s, (H, W))
    tol = conv_tol(k * k * Co, np.abs(ref).max())
    empty = np.ones((H, W), bool)
    empty[0::2, 0::2] = False                                   # SAME pads of a 1x1 kernel are 0: the tap lands on even rows / columns
    assert not ref[:, empty].any()
    dyd, wd = dev(dy), dev(w)

    def run(epi):
        dx, names = _kernels(lambda: ops.conv2d_bwd_data(dyd, wd, _poisoned(x.shape), k, s, epi))
        assert names == [route], names
        return dx.cpu().numpy()

    # no epilogue: exact zeros
    got = run(None)
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=tol)
    assert (got[:, empty] == 0).all()
    # bias only
    got = run(ops.epilogue(EPI_NONE, bias=dev(bias)))
    np.testing.assert_allclose(got, ref + bias, rtol=1e-4, atol=tol)
    assert (got[:, empty] == b32).all()
    # bias + LeakyReLU + dropout mask on all samples but the last
    keep = (rng.uniform(size=x.shape) >= 0.3).astype(np.uint8)
    nk = (B - 1) * x[0].size
    got = run(ops.epilogue(EPI_BIAS_LRELU, bias=dev(bias), keep=dev(keep, torch.uint8), alpha=0.3, scale=1 / 0.7, keep_elems=nk))
    exp = O.lrelu_fwd(ref + bias)
    exp[:B - 1] = exp[:B - 1] * keep[:B - 1] / 0.7
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=2 * tol)
    lr32 = np.where(b32 > 0, b32, np.float32(0.3) * b32).astype(np.float32)       # the epilogue's float32 arithmetic on acc = 0
    exact = np.broadcast_to(lr32, x.shape).copy()
    exact[:B - 1] = np.where(keep[:B - 1] != 0, exact[:B - 1] * np.float32(1 / 0.7), np.float32(0))
    assert (got[:, empty] == exact[:, empty]).all()
    # LeakyReLU' x mask of a reference activation: 0 * factor
    ref_act = rng.normal(size=x.shape)
    got = run(ops.epilogue(EPI_MUL_GRAD, ref=dev(ref_act), keep=dev(keep, torch.uint8), alpha=0.3, scale=1 / 0.7, keep_elems=nk))
    exp = ref * O.lrelu_mask(ref_act)
    exp[:B - 1] *= keep[:B - 1] / 0.7
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=2 * tol)
    assert (got[:, empty] == 0).all()
    # tanh: tanh(0) = 0 exactly; with a bias every empty element of a channel is the SAME float, tanh(bias) to rounding
    got = run(ops.epilogue(EPI_TANH))
    np.testing.assert_allclose(got, np.tanh(ref), rtol=1e-4, atol=tol)
    assert (got[:, empty] == 0).all()
    got = run(ops.epilogue(EPI_TANH, bias=dev(bias)))
    np.testing.assert_allclose(got, np.tanh(ref + bias), rtol=1e-4, atol=tol)
    e = got[:, empty]                                            # [B, positions, Ci]
    assert (e == e[0, 0]).all()
    np.testing.assert_allclose(e[0, 0], np.tanh(b32.astype(np.float64)), rtol=2e-6)


# ------------------------------------------------------------------------------------------------------------------------------------
# epilogues
# ------------------------------------------------------------------------------------------------------------------------------------
def test_epilogues():
    """The gather-GEMM's float4 epilogues at k = 3 (tests/test_conv_gpu.py test_epilogues at 5x5)."""
    from blurred_gan_amd import ops
    from blurred_gan_amd._lib import EPI_BIAS_LRELU, EPI_MUL_GRAD, EPI_TANH, EPI_NONE
    B, H, W, Ci, Co, k, s = 2, 8, 8, 32, 32, 3, 2
    x, w, dy = _data(B, H, W, Ci, Co, k, s, seed=3)
    rng = np.random.default_rng(4)
    bias = rng.normal(size=Co)
    keep = (rng.uniform(size=dy.shape) >= 0.3).astype(np.uint8)
    z = O.conv2d_fwd(x, w, s) + bias
    wT = dev(np.transpose(w, (0, 1, 3, 2)))
    xd = dev(x)
    tol = conv_tol(k * k * Ci, np.abs(z).max())

    def fwd(epi):
        y, names = _kernels(lambda: ops.conv2d_fwd(xd, wT, _poisoned(z.shape), k, s, epi))
        assert names == [IGF], names
        return y.cpu().numpy()

    y = fwd(ops.epilogue(EPI_BIAS_LRELU, bias=dev(bias), keep=dev(keep, torch.uint8), alpha=0.3, scale=1 / 0.7))
    np.testing.assert_allclose(y, O.dropout_fwd(O.lrelu_fwd(z), keep, 0.3), rtol=1e-4, atol=2 * tol)
    np.testing.assert_allclose(fwd(ops.epilogue(EPI_BIAS_LRELU, bias=dev(bias), alpha=0.3)), O.lrelu_fwd(z), rtol=1e-4, atol=2 * tol)
    np.testing.assert_allclose(fwd(ops.epilogue(EPI_TANH, bias=dev(bias))), np.tanh(z), rtol=1e-4, atol=2 * tol)
    np.testing.assert_allclose(fwd(ops.epilogue(EPI_NONE, bias=dev(bias))), z, rtol=1e-4, atol=2 * tol)
    ref_act = rng.normal(size=x.shape)
    keep_x = (rng.uniform(size=x.shape) >= 0.3).astype(np.uint8)
    dxr = O.conv2d_bwd_data(dy, w, s, (H, W))
    dyd, wd = dev(dy), dev(w)
    dx, names = _kernels(lambda: ops.conv2d_bwd_data(dyd, wd, _poisoned(x.shape), k, s,
                                                     ops.epilogue(EPI_MUL_GRAD, ref=dev(ref_act), keep=dev(keep_x, torch.uint8), alpha=0.3, scale=1 / 0.7)))
    assert names == [IGD], names
    exp = dxr * O.lrelu_mask(ref_act) * keep_x / 0.7
    np.testing.assert_allclose(dx.cpu().numpy(), exp, rtol=1e-4, atol=2 * conv_tol(k * k * Co, np.abs(dxr).max()))


# (B, H, W, thin, wide): H x W is the map of the WIDE side at stride 1 and of the stride-2 conv's output; thin 1 / 3 / 4 / 5 channels,
# wide 16 / 32 / 64, rows of 16 / 32 / 64 / 128 pixels, ragged strips, a last workgroup with fewer images than it holds (B = 5, 3)
@pytest.mark.parametrize("B,H,W,thin,wide", [(5, 16, 16, 5, 16), (3, 40, 32, 3, 32), (2, 36, 64, 4, 64), (2, 12, 128, 1, 16),
                                             (5, 20, 16, 4, 32), (3, 33, 32, 5, 64)])
def test_thin_row_kernel_epilogues(B, H, W, thin, wide):
    """The four row kernels at k = 3 with the epilogue variants of test_thin_n_row_kernel_epilogues: conv_rows_scatter_kernel's three
    (bias only, bias + branch-free tanh, generic with per-element loads) forward and as a data gradient, conv_rows_gather_kernel's
    two (generic, and the batched-mask variant of bias + LeakyReLU + dropout) forward and as a data gradient; masks on the leading
    samples only."""
    from blurred_gan_amd import ops
    from blurred_gan_amd._lib import EPI_BIAS_LRELU, EPI_MUL_GRAD, EPI_TANH, EPI_NONE, EPI_AFFINE_LRELU
    k = 3
    rng = np.random.default_rng(100 + W + thin)

    def fwd_variants(x, w, s, route):
        Bn, Co = x.shape[0], w.shape[-1]
        bias = rng.normal(size=Co)
        z0 = O.conv2d_fwd(x, w, s)
        z = z0 + bias
        wT, xd = dev(np.transpose(w, (0, 1, 3, 2))), dev(x)
        tol = conv_tol(k * k * x.shape[-1], np.abs(z).max())

        def run(epi):
            y, names = _kernels(lambda: ops.conv2d_fwd(xd, wT, _poisoned(z.shape), k, s, epi))
            assert names == [route], names
            return y.cpu().numpy()

        np.testing.assert_allclose(run(None), z0, rtol=1e-4, atol=tol)
        np.testing.assert_allclose(run(ops.epilogue(EPI_NONE, bias=dev(bias))), z, rtol=1e-4, atol=2 * tol)
        np.testing.assert_allclose(run(ops.epilogue(EPI_TANH, bias=dev(bias))), np.tanh(z), rtol=1e-4, atol=2 * tol)
        keep = (rng.uniform(size=z.shape) >= 0.3).astype(np.uint8)
        nk = (Bn - 1) * z[0].size                               # the mask covers all samples but the last
        y = run(ops.epilogue(EPI_BIAS_LRELU, bias=dev(bias), keep=dev(keep, torch.uint8), alpha=0.3, scale=1 / 0.7, keep_elems=nk))
        exp = O.lrelu_fwd(z)
        exp[:Bn - 1] = exp[:Bn - 1] * keep[:Bn - 1] / 0.7
        np.testing.assert_allclose(y, exp, rtol=1e-4, atol=2 * tol)
        mul = rng.uniform(0.5, 1.5, size=Co)
        y = run(ops.epilogue(EPI_AFFINE_LRELU, bias=dev(bias), ref=dev(mul), alpha=0.3))
        np.testing.assert_allclose(y, O.lrelu_fwd(z0 * mul + bias), rtol=1e-4, atol=2 * tol)

    def dgrad_variants(dy, w, s, hw, route):
        Bn, Ci = dy.shape[0], w.shape[2]
        dxr = O.conv2d_bwd_data(dy, w, s, hw)
        told = conv_tol(k * k * dy.shape[-1], np.abs(dxr).max())
        dyd, wd = dev(dy), dev(w)

        def run(epi):
            dx, names = _kernels(lambda: ops.conv2d_bwd_data(dyd, wd, _poisoned(dxr.shape), k, s, epi))
            assert names == [route], names
            return dx.cpu().numpy()

        np.testing.assert_allclose(run(None), dxr, rtol=1e-4, atol=told)
        bias = rng.normal(size=Ci)
        np.testing.assert_allclose(run(ops.epilogue(EPI_BIAS_LRELU, bias=dev(bias), alpha=0.3)), O.lrelu_fwd(dxr + bias), rtol=1e-4, atol=2 * told)
        ref_act = rng.normal(size=dxr.shape)
        keep_x = (rng.uniform(size=dxr.shape) >= 0.3).astype(np.uint8)
        dx = run(ops.epilogue(EPI_MUL_GRAD, ref=dev(ref_act), keep=dev(keep_x, torch.uint8), alpha=0.3, scale=1 / 0.7,
                              keep_elems=(Bn - 1) * dxr[0].size))
        expd = dxr * O.lrelu_mask(ref_act)
        expd[:Bn - 1] *= keep_x[:Bn - 1] / 0.7
        np.testing.assert_allclose(dx, expd, rtol=1e-4, atol=2 * told)

    # wide -> thin, stride 1 (the generator's last conv): scatter-form forward, gather-form data gradient
    x, w, dy = _data(B, H, W, wide, thin, k, 1, seed=W + thin)
    fwd_variants(x, w, 1, RF)
    dgrad_variants(dy, w, 1, (H, W), GD)
    # thin -> wide, stride 2 (the critic's first conv) on a 2H x 2W image: gather-form forward, scatter-form data gradient
    x, w, dy = _data(B, 2 * H, 2 * W, thin, wide, k, 2, seed=W + thin + 1)
    fwd_variants(x, w, 2, GF)
    dgrad_variants(dy, w, 2, (2 * H, 2 * W), RD)


@pytest.mark.parametrize("B,H,W,Ci,Co,k,s,bwd", [
    (8, 32, 32, 64, 128, 3, 2, True), (8, 64, 64, 32, 64, 3, 2, True),   # data gradients: 64x64 and 128x32 tiles, 4 phases
    (130, 8, 8, 128, 256, 3, 2, True),                                     # ragged last M tile
    (1024, 16, 16, 16, 32, 3, 2, True),                                    # position-major, phases merged
    (8, 16, 16, 32, 64, 1, 2, True), (1024, 16, 16, 16, 32, 1, 2, True),   # k = 1: empty phases, one per workgroup / a whole merged pair
    (3, 16, 16, 64, 128, 3, 1, False), (5, 9, 7, 32, 64, 3, 2, False), (4, 8, 8, 64, 64, 1, 1, False),
])
def test_conv_epilogue_leaves_batchnorm_statistics(B, H, W, Ci, Co, k, s, bwd):
    """bg_epilogue.stats at k = 3 and 1: the partial rows the gather-GEMM leaves sum to the statistics of the tensor it stored (same
    assertions as the 5x5 test in tests/test_conv_gpu.py)."""
    from blurred_gan_amd import ops
    x, w, dy = _data(B, H, W, Ci, Co, k, s, seed=3)
    if bwd:
        src, wd = dev(dy), dev(w).reshape(k * k, Ci, Co)
        out = _poisoned((B, H, W, Ci))
        N = Ci
    else:
        wd = dev(np.transpose(w, (0, 1, 3, 2)))
        src = dev(x)
        out = _poisoned((B, -(-H // s), -(-W // s), Co))
        N = Co
    stats = torch.full(((out.numel() // N // 32 + 64) * 2 * N,), float("nan"), device="cuda")
    epi = ops.epilogue(stats=stats)
    if bwd:
        _, names = _kernels(lambda: ops.conv2d_bwd_data(src, wd, out, k, s, epi))
    else:
        _, names = _kernels(lambda: ops.conv2d_fwd(src, wd, out, k, s, epi))
    assert names == [IGD if bwd else IGF], names
    rows = ops.conv2d_stats_rows(epi)
    assert rows > 0, "this geometry is expected on the MFMA gather kernel without split-K"
    part = stats[:rows * 2 * N].view(rows, 2, N).double().cpu().numpy()
    assert np.isfinite(part).all(), "every partial row must have been written"
    flat = out.view(-1, N).double().cpu().numpy()
    scale = np.abs(flat).max()
    np.testing.assert_allclose(part[:, 0].sum(0), flat.sum(0), rtol=1e-5, atol=2e-5 * scale * np.sqrt(flat.shape[0]))
    np.testing.assert_allclose(part[:, 1].sum(0), (flat ** 2).sum(0), rtol=1e-5, atol=1e-6)
    ref = O.conv2d_bwd_data(dy, w, s, (H, W)) if bwd else O.conv2d_fwd(x, w, s)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(k * k * (Co if bwd else Ci), np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------------------------------------------
# bf16x6, Conv2DTranspose roles, adjointness, random sweep, rejected sizes
# ------------------------------------------------------------------------------------------------------------------------------------
def test_bf16x6_declines_other_kernel_sizes():
    """The split-bf16 table holds 5x5 layers only: at k = 1 / 3 the C2 layer shapes are not taken, and a math="bf16x6" call is the
    fp32 call, bit for bit."""
    from blurred_gan_amd import ops
    from test_conv_math_gpu import C2_LAYERS, C2_B
    for k in (1, 3):
        for (H, W, Ci, Co) in C2_LAYERS:
            for bwd in (0, 1):
                assert ops.conv2d_math_taken(bwd, C2_B, H, W, Ci, Co, k, 2, "bf16x6") == 0, (k, H, W, Ci, Co, bwd)
    for (B, H, W, Ci, Co) in ((8, 16, 16, 64, 128), (4, 32, 32, 32, 64)):
        k, s = 3, 2
        x, w, dy = _data(B, H, W, Ci, Co, k, s, seed=5)
        wT, xd, dyd, wd = dev(np.transpose(w, (0, 1, 3, 2))), dev(x), dev(dy), dev(w)
        y32, n32 = _kernels(lambda: ops.conv2d_fwd(xd, wT, _poisoned(dy.shape), k, s))
        y6, n6 = _kernels(lambda: ops.conv2d_fwd(xd, wT, _poisoned(dy.shape), k, s, math="bf16x6"))
        assert n32 == n6 == [IGF] and torch.equal(y32, y6)
        d32, n32 = _kernels(lambda: ops.conv2d_bwd_data(dyd, wd, _poisoned(x.shape), k, s))
        d6, n6 = _kernels(lambda: ops.conv2d_bwd_data(dyd, wd, _poisoned(x.shape), k, s, math="bf16x6"))
        assert n32 == n6 == [IGD] and torch.equal(d32, d6)
        ref = O.conv2d_fwd(x, w, s)
        np.testing.assert_allclose(y6.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(k * k * Ci, np.abs(ref).max()))


@pytest.mark.parametrize("k", [3, 1])
def test_conv_transpose_roles(k):
    """Conv2DTranspose forward = bwd_data with the kernel array as is; its filter gradient swaps x and dy."""
    from blurred_gan_amd import ops
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, size=(2, 4, 4, 32))
    w = rng.uniform(-1, 1, size=(k, k, 16, 32)) / np.sqrt(k * k * 32)           # [k,k,c_out,c_in]
    ref = O.conv2d_transpose_fwd(x, w, 2)
    y = ops.conv2d_bwd_data(dev(x), dev(w), _poisoned(ref.shape), k, 2)
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(k * k * 32, np.abs(ref).max()))
    dyt = rng.uniform(-1, 1, size=ref.shape)
    dwr = O.conv2d_transpose_bwd_filter(x, dyt, 2, k)
    nb = ops.conv2d_bwd_filter_workspace_bytes(2, 8, 8, 16, 32, k, 2)
    ws = torch.empty(nb // 4 + 4, device="cuda") if nb else None
    dw = ops.conv2d_bwd_filter(dev(dyt), dev(x), _poisoned(w.shape), k, 2, 0.0, 1.0, ws)
    np.testing.assert_allclose(dw.cpu().numpy(), dwr, rtol=1e-4, atol=conv_tol(32, np.abs(dwr).max()))


@pytest.mark.parametrize("B,H,W,Ci,Co,s", [(256, 32, 32, 32, 64, 2), (256, 64, 64, 3, 32, 2), (256, 4, 4, 256, 512, 2)])
def test_adjointness_full_size(B, H, W, Ci, Co, s):
    """<conv(x), dy> == <x, conv^T(dy)> == <w, wgrad(x, dy)> at C2 layer sizes with 3x3 kernels (no oracle needed)."""
    from blurred_gan_amd import ops
    k = 3
    torch.manual_seed(0)
    x = torch.rand(B, H, W, Ci, device="cuda") * 2 - 1
    w = (torch.rand(k, k, Ci, Co, device="cuda") * 2 - 1) / (k * k * Ci) ** 0.5
    Ho, Wo = -(-H // s), -(-W // s)
    dy = torch.rand(B, Ho, Wo, Co, device="cuda") * 2 - 1
    wT = ops.transpose_last2(w, torch.empty_like(w).view(-1), k * k, Ci, Co)
    nbf, wsf = _splitk_ws(False, B, H, W, Ci, Co, k, s)
    nbd, wsd = _splitk_ws(True, B, H, W, Ci, Co, k, s)
    y = ops.conv2d_fwd(x, wT, _poisoned((B, Ho, Wo, Co)), k, s, ops.epilogue(ws=wsf) if nbf else None)
    dx = ops.conv2d_bwd_data(dy, w, _poisoned(x.shape), k, s, ops.epilogue(ws=wsd) if nbd else None)
    nb = ops.conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, k, s)
    ws = torch.empty(nb // 4 + 4, device="cuda") if nb else None
    dw = ops.conv2d_bwd_filter(x, dy, _poisoned(w.shape), k, s, 0.0, 1.0, ws)
    a = (y.double() * dy.double()).sum().item()
    b = (x.double() * dx.double()).sum().item()
    c = (w.double() * dw.double()).sum().item()
    scale = max(1.0, abs(a))
    assert abs(a - b) < 2e-4 * scale and abs(a - c) < 2e-4 * scale, (a, b, c)


def _random_cases(n, seed):
    rng = np.random.default_rng(seed)
    chans = [1, 2, 3, 4, 5, 8, 12, 16, 20, 32, 48, 64, 96, 128]
    out = []
    while len(out) < n:
        B = int(rng.integers(1, 6))
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if rng.uniform() < 0.3:                                   # the row kernels want widths that are multiples of 16
            W = int(rng.choice([16, 32, 64]))
        Ci, Co = int(rng.choice(chans)), int(rng.choice(chans))
        k, s = int(rng.choice([1, 3])), int(rng.choice([1, 2]))
        if B * H * W * max(Ci, Co) > 400_000:
            continue
        out.append((B, H, W, Ci, Co, k, s))
    return out


@pytest.mark.parametrize("B,H,W,Ci,Co,k,s", _random_cases(48, 20261017))
def test_conv_random_shapes(B, H, W, Ci, Co, k, s):
    """Seeded random geometries with k drawn from {1, 3} across the dispatch boundaries (maps from 1x1 on): the three operators
    against the float64 oracle, whichever kernels take them."""
    seed = B * 1000 + H * 31 + W
    _check_fwd(B, H, W, Ci, Co, k, s, None, seed)
    _check_bwd_data(B, H, W, Ci, Co, k, s, None, seed)
    _check_bwd_filter(B, H, W, Ci, Co, k, s, None, seed)


@pytest.mark.parametrize("k", [2, 4, 7])
def test_rejected_kernel_sizes(k):
    """Even sizes and k*k > 25 are refused by all three entry points, before anything is launched."""
    from blurred_gan_amd import ops
    x = torch.zeros(1, 8, 8, 32, device="cuda")
    w = torch.zeros(k * k * 32 * 32, device="cuda")
    y = torch.zeros(1, 8, 8, 32, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")
    with pytest.raises(ValueError):
        ops.conv2d_fwd(x, w, y, k, 1)
    with pytest.raises(ValueError):
        ops.conv2d_bwd_data(y, w, x, k, 1)
    with pytest.raises(ValueError):
        ops.conv2d_bwd_filter(x, y, w.view(k, k, 32, 32), k, 1, 0.0, 1.0, ws)
