"""The native SWD metric on the GPU (csrc/swd.hip, swd_native.py, SWDMetric(native=True)): every kernel against the host
functions of sliced_wasserstein.py -- exactly where the contract is exact (ingest, pyramid, gather, sort, integer abs-diff), within
derived bounds where it rounds (standardise, real-valued abs-diff) -- then the reference's goldens, the whole metric against a
float64 restatement, and the callback inside a real fit()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EQ = np.testing.assert_array_equal


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return t.cpu().numpy()


def u8_images(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- ingest
@pytest.mark.parametrize("scale,shift,kind", [(1.0, 0.0, "u8"), (127.5, 127.5, "u8"), (127.5, 127.5, "unit")])
@pytest.mark.parametrize("nhwc", [True, False])
@pytest.mark.parametrize("B,H,W,C", [(1, 16, 16, 1), (3, 18, 30, 3), (2, 28, 28, 1)])
def test_ingest_exact(B, H, W, C, nhwc, scale, shift, kind):
    from blurred_gan_amd import swd_native as sn
    planar = u8_images((B, C, H, W), 1)
    if kind == "unit":
        planar = (planar - np.float32(127.5)) / np.float32(127.5)          # what model.images hold
    src = np.transpose(planar, (0, 2, 3, 1)) if nhwc else planar
    got = host(sn.ingest(dev(src), "NHWC" if nhwc else "NCHW", scale, shift))
    want = planar * np.float32(scale) + np.float32(shift)
    want = np.repeat(want, 3, axis=1) if C == 1 else want
    assert got.shape == (B, 3, H, W) and got.dtype == np.float32
    EQ(got, want)


# ---------------------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("planes,H,W", [(1, 3, 3), (3, 16, 16), (6, 17, 19), (3, 28, 28), (2, 64, 64), (1, 5, 130)])
def test_pyr_down_exact(planes, H, W):
    from blurred_gan_amd import swd_native as sn, sliced_wasserstein as sw
    x = u8_images((1, planes, H, W), 2)
    got = host(sn.pyr_down(dev(x)))
    EQ(got, sw.pyr_down(x))
    frac = x + np.random.RandomState(3).rand(*x.shape).astype(np.float32)       # values that round in every product
    EQ(host(sn.pyr_down(dev(frac))), sw.pyr_down(frac))


@pytest.mark.parametrize("planes,h,w", [(1, 2, 2), (3, 8, 8), (6, 9, 10), (3, 14, 14), (2, 32, 32), (1, 3, 65)])
def test_pyr_up_exact_plain_fused_and_in_place(planes, h, w):
    from blurred_gan_amd import ops, swd_native as sn, sliced_wasserstein as sw
    for low in (u8_images((1, planes, h, w), 4), u8_images((1, planes, h, w), 5) + np.random.RandomState(6).rand(1, planes, h, w).astype(np.float32)):
        up = sw.pyr_up(low)
        EQ(host(sn.pyr_up(dev(low))), up)
        x = u8_images((1, planes, 2 * h, 2 * w), 7)
        low_d, x_d = dev(low), dev(x)
        out = torch.empty_like(x_d)
        EQ(host(ops.pyr_up(low_d, out, minuend=x_d)), x - up)
        EQ(host(x_d), x)                                                         # the minuend is read only
        EQ(host(ops.pyr_up(low_d, x_d, minuend=x_d)), x - up)                    # in place


@pytest.mark.parametrize("size,levels", [(64, 3), (28, 1)])
def test_laplacian_pyramid_exact(size, levels):
    from blurred_gan_amd import swd_native as sn, sliced_wasserstein as sw
    x = u8_images((2, 3, size, size), 8)
    x_d = dev(x)
    got = sn.generate_laplacian_pyramid(x_d, levels)
    want = sw.generate_laplacian_pyramid(x, levels)
    assert len(got) == len(want) == levels
    for g, w in zip(got, want):
        EQ(host(g), w)
    EQ(host(x_d), x)                                                             # the input is left alone


# ---------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("shape,per_image", [((1, 3, 7, 7), 1), ((3, 3, 16, 16), 5), ((2, 3, 16, 24), 128)])
def test_gather_exact(shape, per_image):
    from blurred_gan_amd import swd_native as sn, sliced_wasserstein as sw
    level = u8_images(shape, 9)
    level_d = dev(level)
    got = host(sn.get_descriptors_for_minibatch(level_d, 7, per_image, np.random.RandomState(77)))
    EQ(got, sw.get_descriptors_for_minibatch(level, 7, per_image, np.random.RandomState(77)))
    # centres forced to the four extreme legal corners (and drawn ones between them)
    n, _, H, W = shape
    total = n * per_image
    rng = np.random.RandomState(78)
    cx, cy = rng.randint(3, W - 3, size=total), rng.randint(3, H - 3, size=total)
    corners = [(3, 3), (W - 4, 3), (3, H - 4), (W - 4, H - 4)]
    for k in range(total):
        if k % 2 == 0 or total < 4:
            cx[k], cy[k] = corners[(k // 2) % 4]
    cx[-1], cy[-1] = corners[3]
    cx[0], cy[0] = corners[0]
    got = host(sn.gather_descriptors(level_d, cx, cy, 7, per_image))
    img = (np.arange(total) // per_image).reshape(total, 1, 1, 1)
    ch = np.arange(3).reshape(1, 3, 1, 1)
    dy = np.arange(-3, 4).reshape(1, 1, 1, 7)
    dx = np.arange(-3, 4).reshape(1, 1, 7, 1)
    EQ(got, level[img, ch, cy.reshape(-1, 1, 1, 1) + dy, cx.reshape(-1, 1, 1, 1) + dx])
    with pytest.raises(ValueError):
        sn.gather_descriptors(level_d, cx + W, cy, 7, per_image)                 # the range check is the host's


# ---------------------------------------------------------------------------------------------------- sort
def _sort_inputs(rows, n, seed):
    rng = np.random.RandomState(seed)
    normal = rng.randn(rows, n).astype(np.float32)
    special = normal.copy()
    special.reshape(-1)[::3] = np.resize(np.array([0.0, -0.0, np.inf, -np.inf, 1.0], np.float32), special.reshape(-1)[::3].shape)
    return {"normal": normal, "duplicates": rng.randint(0, 8, size=(rows, n)).astype(np.float32), "sorted": np.sort(normal, axis=1),
            "reversed": np.sort(normal, axis=1)[:, ::-1].copy(), "equal": np.full((rows, n), 2.5, np.float32), "special": special}


def _check_sort(x):
    from blurred_gan_amd import ops
    rows, n = x.shape
    got = host(ops.sort_rows(dev(x), rows, n))
    EQ(got, np.sort(x, axis=1))


# 4095 / 4097: one below / above the kernel's LDS chunk of 4096
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 9856, 16385, 32767, 32769, 65537])
def test_sort_rows_exact(n):
    for rows in (1, 3):
        for kind, x in _sort_inputs(rows, n, 100 + n).items():
            _check_sort(x)


@pytest.mark.parametrize("rows,n", [(512, 2048), (8, 128_000)])
def test_sort_rows_exact_at_the_metric_sizes(rows, n):
    for kind, x in _sort_inputs(rows, n, 11).items():
        _check_sort(x)


def test_sort_rows_with_nans_returns():
    from blurred_gan_amd import ops
    x = np.random.RandomState(12).randn(2, 5000).astype(np.float32)
    x[:, ::7] = np.nan
    got = host(ops.sort_rows(dev(x), 2, 5000))
    assert got.shape == x.shape                                                 # where the NaNs end up is unspecified


# ---------------------------------------------------------------------------------------------------- mean |a - b|
def _abs_diff(a, b, seg, nseg):
    from blurred_gan_amd import ops
    out = torch.empty(nseg, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(ops.abs_diff_mean_workspace_bytes(seg, nseg), 8), dtype=torch.uint8, device="cuda")
    return host(ops.abs_diff_mean(dev(a), dev(b), seg, nseg, out, ws))


@pytest.mark.parametrize("nseg", [1, 4])
@pytest.mark.parametrize("seg", [1, 7, 4096, 128 * 2048])
def test_abs_diff_mean_exact_on_integers(seg, nseg):
    rng = np.random.RandomState(13)
    a = rng.randint(0, 256, size=seg * nseg).astype(np.float32)
    b = rng.randint(0, 256, size=seg * nseg).astype(np.float32)
    want = np.abs(a - b).astype(np.float64).reshape(nseg, seg).sum(axis=1) / seg        # sums below 2^53: exact in any order
    EQ(_abs_diff(a, b, seg, nseg), want)


@pytest.mark.parametrize("seg,nseg", [(7, 4), (4099, 3), (128 * 2048, 4)])
def test_abs_diff_mean_real_valued_within_the_float64_sum_bound(seg, nseg):
    rng = np.random.RandomState(14)
    a, b = rng.randn(seg * nseg).astype(np.float32), rng.randn(seg * nseg).astype(np.float32)
    want = np.abs(a - b).astype(np.float64).reshape(nseg, seg).mean(axis=1)             # the fp32 difference, summed in float64
    got = _abs_diff(a, b, seg, nseg)
    rel = np.abs(got - want) / want
    print("abs-diff rel err", rel.max(), "bound", seg * 2.0 ** -53)
    assert (rel <= seg * 2.0 ** -53).all(), (rel, seg * 2.0 ** -53)


# ---------------------------------------------------------------------------------------------------- standardise
@pytest.mark.parametrize("rows", [1, 5, 640, 128 * 250])
def test_standardize_within_the_derived_bound(rows):
    """|got - want| <= 4 * 2^-24 * ((|x| + |mu|) / sigma + |want|): the fp32 roundings of mu, of x - mu, of sigma and of the
    quotient, with a factor-4 margin -- it holds only if the statistics themselves are as accurate as float64 ones."""
    from blurred_gan_amd import ops
    rng = np.random.RandomState(15)
    x = np.empty((rows, 3, 7, 7), np.float32)
    x[:, 0] = rng.randint(120, 136, size=(rows, 7, 7))                           # low contrast
    x[:, 1] = rng.randint(0, 256, size=(rows, 7, 7))                             # full range
    x[:, 2] = rng.randn(rows, 7, 7) * 40 + 90
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=(0, 2, 3), keepdims=True)
    sd = x64.std(axis=(0, 2, 3), keepdims=True)
    want = (x64 - mu) / sd
    x_d = dev(x)
    stats = torch.empty(6, dtype=torch.float64, device="cuda")
    ws = torch.empty(ops.swd_standardize_workspace_bytes(rows, 7), dtype=torch.uint8, device="cuda")
    got = host(ops.swd_standardize(x_d, rows, 7, ws, stats)).astype(np.float64)
    bound = 4 * 2.0 ** -24 * ((np.abs(x64) + np.abs(mu)) / sd + np.abs(want))
    err = np.abs(got - want)
    print("standardise worst err / bound", (err / bound).max())
    assert (err <= bound).all(), (err / bound).max()
    st = host(stats).reshape(3, 2)
    np.testing.assert_allclose(st[:, 0], mu.reshape(3), rtol=1e-12, atol=0)
    np.testing.assert_allclose(st[:, 1], sd.reshape(3), rtol=1e-12, atol=0)
    # without stats_out, through the module: the same numbers, the inputs untouched
    from blurred_gan_amd import swd_native as sn
    pieces = [dev(x[: rows // 2]), dev(x[rows // 2:])] if rows > 1 else dev(x)
    fin = host(sn.finalize_descriptors(pieces))
    assert fin.shape == (rows, 147)
    EQ(fin, got.astype(np.float32).reshape(rows, 147))


# ---------------------------------------------------------------------------------------------------- the reference's goldens
def test_native_path_matches_the_reference_goldens():
    """The tolerances of tests/test_metrics_gpu.py's device-path test, on the native path."""
    import test_metrics_cpu as cpu
    from blurred_gan_amd import swd_native as sn, sliced_wasserstein as sw
    G = cpu.G
    np.testing.assert_allclose(host(sn.pyr_up(dev(G["small"]))), G["small_up"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(sn.pyr_down(dev(G["down_in"]))), G["small_down"], rtol=1e-5, atol=1e-6)
    pyr = sn.generate_laplacian_pyramid(dev(G["batch"]), 2)
    assert all(p.is_cuda for p in pyr)
    np.testing.assert_allclose(host(pyr[0]), G["pyr0"], rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(host(pyr[1]), G["pyr1"], rtol=1e-5, atol=1e-3)
    desc = sn.get_descriptors_for_minibatch(dev(G["level"]), 7, 5, np.random.RandomState(4321))
    assert desc.is_cuda
    EQ(host(desc), G["desc"].astype(np.float32))
    np.testing.assert_allclose(host(sn.finalize_descriptors(desc)), G["desc_final"], rtol=1e-5, atol=2e-6)
    got = sn.sliced_wasserstein(dev(G["A"]), dev(G["B"]), 3, 16, np.random.RandomState(999))
    assert abs(got - float(G["swd"])) < 1e-5 * max(1.0, abs(float(G["swd"])))
    assert sn.sliced_wasserstein(dev(G["A"]), dev(G["A"]), 2, 8, np.random.RandomState(1)) == 0.0
    api = sw.API((4, 32, 32, 3), seed=2024, native=True)
    api.begin("reals"); api.feed("reals", dev(G["api_reals"])); api.end("reals")
    api.begin("fakes"); api.feed("fakes", dev(G["api_fakes"])); res = api.end("fakes")
    np.testing.assert_allclose(res, G["api_result"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------------- end to end
def _sets(n, size, seed):
    rng = np.random.RandomState(seed)
    real = rng.randint(0, 256, size=(n, 3, size, size)).astype(np.float32)
    ramp = np.linspace(0, 255, size)[None, None, None, :] + np.linspace(0, 255, size)[None, None, :, None]
    fake = np.clip(np.round(ramp / 2 + rng.normal(scale=20, size=(n, 3, size, size))), 0, 255).astype(np.float32)   # smooth: another distribution
    return real, fake


def _restated_in_float64(real, fake, seed, halves):
    """The metric with the package's own fp32 pyramid and gather (exact on every path), then finalize, projection with the
    float32-cast directions, sort and mean in float64 -- the draws in the metric's order."""
    from blurred_gan_amd import sliced_wasserstein as sw
    rng = np.random.RandomState(seed)
    res, r = [], real.shape[2]
    while r >= 16:
        res.append(r)
        r //= 2
    dr, df = [[] for _ in res], [[] for _ in res]
    for sl in halves:
        for store, x in ((dr, real[sl]), (df, fake[sl])):
            for lod, level in enumerate(sw.generate_laplacian_pyramid(x, len(res))):
                store[lod].append(sw.get_descriptors_for_minibatch(level, 7, 128, rng))

    def fin(lst):
        d = np.concatenate(lst, axis=0).astype(np.float64)
        d = (d - d.mean(axis=(0, 2, 3), keepdims=True)) / d.std(axis=(0, 2, 3), keepdims=True)
        return d.reshape(d.shape[0], -1)

    dist = []
    for a, b in zip(dr, df):
        A, B = fin(a), fin(b)
        per = []
        for _ in range(4):
            dirs = rng.randn(A.shape[1], 128)
            dirs = (dirs / np.sqrt((dirs ** 2).sum(axis=0, keepdims=True))).astype(np.float32).astype(np.float64)
            per.append(np.abs(np.sort(A @ dirs, axis=0) - np.sort(B @ dirs, axis=0)).mean())
        dist.append(float(np.mean(per)) * 1e3)
    return dist + [float(np.mean(dist))]


@pytest.mark.parametrize("n,size", [(16, 64), (8, 32), (4, 16)])
def test_metric_end_to_end_against_a_float64_restatement(n, size):
    from blurred_gan_amd import metrics, swd_native as sn
    real, fake = _sets(n, size, 20 + size)
    halves = (slice(0, n // 2), slice(n // 2, n))
    want = _restated_in_float64(real, fake, 31, halves)
    m = metrics.SWDMetric(native=True, seed=31)
    for sl in halves:
        m.update_state(dev(real[sl]), dev(fake[sl]))
    assert all(d.is_cuda for lst in m.real_descriptors + m.fake_descriptors for d in lst)
    got = m.results()
    assert list(got) == m.get_metric_names() and len(got) == len(want)
    for (k, g), w in zip(got.items(), want):
        print(k, g, w, abs(g - w))
        assert abs(g - w) <= 1e-4 * max(1.0, abs(w)), (k, g, w)
    # NHWC in, the same numbers: the ingest is the only thing that sees the layout
    mh = metrics.SWDMetric(native=True, seed=31, data_format="NHWC")
    for sl in halves:
        mh.update_state(dev(np.transpose(real[sl], (0, 2, 3, 1))), dev(np.transpose(fake[sl], (0, 2, 3, 1))))
    assert mh.results() == got
    # identical descriptor sets are at distance exactly 0.0 on every level (two patch DRAWS of one image set are not identical,
    # on any path: the draws differ)
    fin = [sn.finalize_descriptors(d) for d in m.real_descriptors]
    again = [sn.finalize_descriptors(d) for d in m.real_descriptors]
    assert sn.level_distances(fin, again, 4, 128, np.random.RandomState(1)) == [0.0] * len(fin)
    # real = fake through the metric: two patch draws of one set, sampling noise only -- far below real against fake
    same = metrics.SWDMetric(native=True, seed=31)
    for sl in halves:
        same.update_state(dev(real[sl]), dev(real[sl]))
    rs = same.results()
    print("real = fake", rs)
    assert all(np.isfinite(v) and v >= 0 for v in rs.values()) and rs["SWDx1e3_avg"] < 0.7 * got["SWDx1e3_avg"]
    # the reference's bug switch keeps its meaning: fakes sampled from the REAL minibatch
    b = metrics.SWDMetric(native=True, seed=31, reproduce_reference_bug=True)
    for sl in halves:
        b.update_state(dev(real[sl]), dev(fake[sl]))
    assert b.result() < 0.7 * got["SWDx1e3_avg"]
    m.reset_states()
    assert all(len(l) == 0 for l in m.real_descriptors + m.fake_descriptors)


# ---------------------------------------------------------------------------------------------------- in a real fit()
def _fit(tmp_path, tag, make_callbacks, profile=False):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models, ops
    bg.set_seed(3)
    B, nb = 8, 4
    gen, disc = models.DCGANGenerator(arch="mnist"), models.DCGANDiscriminator(arch="mnist")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=1.0, global_batch_size=B, batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir=str(tmp_path / tag)))
    g = torch.Generator().manual_seed(2)
    data = [torch.rand(B, 28, 28, 1, generator=g) * 2 - 1 for _ in range(nb)]
    cbs = make_callbacks(B)
    records = []
    if profile:
        ops.prof_reset()
        ops.prof_enable(True)
    try:
        gan.fit(data, epochs=1, callbacks=cbs)
        if profile:
            records = ops.prof_records()
    finally:
        if profile:
            ops.prof_enable(False)
            ops.prof_reset()
    return gan, cbs, records


def test_native_callback_in_a_real_fit(tmp_path):
    """SWDMetricCallback(None, native=True) takes model.images as they are, beside the host callback fed through the demo's
    preprocessing: same seeds, same numbers to rounding; its kernels show in the profile, and the step programs replay as they do
    without it."""
    import test_metrics_gpu as mg
    from blurred_gan_amd import callbacks

    def both(B):
        return [callbacks.SWDMetricCallback(mg._preprocess, num_samples=2 * B, every_n_examples=2 * B, seed=5),
                callbacks.SWDMetricCallback(None, num_samples=2 * B, every_n_examples=2 * B, seed=5, native=True)]

    gan, (host_cb, native_cb), records = _fit(tmp_path, "with", both, profile=True)
    assert len(host_cb.results) == len(native_cb.results) >= 1
    for rh, rn in zip(host_cb.results, native_cb.results):
        assert rh.keys() == rn.keys()
        for k in rh:
            print(k, rh[k], rn[k])
            assert abs(rh[k] - rn[k]) <= 1e-4 * max(1.0, abs(rh[k])), (k, rh[k], rn[k])
    names = {r[0] for r in records}
    assert {"swd_ingest", "swd_gather", "swd_standardize", "sort_rows_chunk", "abs_diff_mean"} <= names, sorted(names)
    plain, _, _ = _fit(tmp_path, "without", lambda B: [])
    assert gan._programs.stats["replayed"] == plain._programs.stats["replayed"] > 0
