"""GPU tests of generator weight averaging (WGAN(generator_ema=...), include/bgan.h bg_ema_f32): the kernel bit for bit against
the float32 numpy statement of its rule, whole recorded-and-replayed steps against the float32 recursion over the live
generator's weights, the untouched off path, sampling from the averages, checkpoints and two data-parallel ranks.

The contract everywhere is BIT equality: the update is ``avg = avg - w * (avg - theta)`` in fp32 without contraction, which the
numpy line ``a = a - w * (a - t)`` on float32 operands reproduces exactly."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models, ops
from blurred_gan_amd.ema import GeneratorEMA

pytestmark = pytest.mark.gpu

ARCH, B = "tiny", 8
SHAPE = models.IMAGE_SHAPE[ARCH]


# ------------------------------------------------------------------ kernel
FULL_SWEEP = 2048 * 256 * 4          # floats one sweep of the largest grid covers


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, FULL_SWEEP + 4 + 1])
def test_kernel_parity_bit_for_bit(n):
    rng = np.random.default_rng(n)
    draw = lambda size: np.float32(rng.normal(size=size) * 10.0 ** rng.integers(-3, 2, size=size))
    thetas, thetas2 = [draw(n) for _ in range(5)], [draw(6) for _ in range(5)]
    a0, b0 = draw(n), draw(6)
    guard = 4                                    # floats behind each segment that no update may touch
    t_d, t2_d = torch.empty(n, device="cuda"), torch.empty(8, device="cuda")
    for n2 in (0, 1, 6):
        for w in (np.float32(0.0), np.float32(1e-4), np.float32(0.1), np.float32(0.9)):
            a, b = a0.copy(), b0[:n2].copy()
            a_d = torch.full((n + guard,), 777.0, device="cuda")
            b_d = torch.full((8 + guard,), 777.0, device="cuda")
            a_d[:n].copy_(torch.from_numpy(a))
            b_d[:n2].copy_(torch.from_numpy(b))
            for t, t2 in zip(thetas, thetas2):
                t_d.copy_(torch.from_numpy(t))
                t2_d[:6].copy_(torch.from_numpy(t2))
                ops.ema(a_d[:n], t_d, b_d[:n2] if n2 else None, t2_d[:n2] if n2 else None, float(w))
                a = a - w * (a - t)
                b = b - w * (b - t2[:n2])
            assert a.dtype == np.float32 and b.dtype == np.float32
            got_a, got_b = a_d.cpu().numpy(), b_d.cpu().numpy()
            np.testing.assert_array_equal(got_a[:n], a, err_msg=f"n={n} n2={n2} w={w}")
            np.testing.assert_array_equal(got_b[:n2], b, err_msg=f"n={n} n2={n2} w={w} (second segment)")
            assert (got_a[n:] == 777.0).all() and (got_b[n2:] == 777.0).all(), (n, n2, float(w))
            if w == 0:
                np.testing.assert_array_equal(got_a[:n], a0)
                np.testing.assert_array_equal(got_b[:n2], b0[:n2])


def test_misaligned_pointers_and_bad_w_are_errors_and_launch_nothing():
    a, t = torch.ones(72, device="cuda"), torch.zeros(72, device="cuda")
    for call in (lambda: ops.ema(a[1:65], t[:64], None, None, 0.5), lambda: ops.ema(a[:64], t[2:66], None, None, 0.5),
                 lambda: ops.ema(a[:64], t[:64], a[65:69], t[64:68], 0.5), lambda: ops.ema(a[:64], t[:64], a[64:68], t[67:71], 0.5)):
        with pytest.raises(ValueError, match="aligned"):
            call()
    with pytest.raises(ValueError, match="outside"):
        ops.ema(a[:64], t[:64], None, None, 1.5)
    torch.cuda.synchronize()
    assert float(a.min()) == 1.0


# ------------------------------------------------------------------ whole steps
def _hand_built_generator():
    """The "tiny" generator minus one stage, put together by hand with a nested Sequential: not a DCGANGenerator."""
    stem = layers.Sequential([layers.Dense(2 * 2 * 32, use_bias=False, input_shape=(10,)), layers.BatchNormalization(), layers.LeakyReLU(),
                              layers.Reshape((2, 2, 32))])
    return layers.Sequential([stem, layers.Conv2DTranspose(16, (5, 5), strides=(2, 2), padding="same", use_bias=False),
                              layers.BatchNormalization(), layers.LeakyReLU(),
                              layers.Conv2DTranspose(16, (5, 5), strides=(2, 2), padding="same", use_bias=False),
                              layers.BatchNormalization(), layers.LeakyReLU(),
                              layers.Conv2D(3, (5, 5), padding="same", use_bias=False, activation="tanh")])


def _gan(ema, replay=True, seed=21, d_steps=1, batch=B, make_gen=None, world=1):
    bg.set_seed(seed)
    gen = make_gen() if make_gen else models.DCGANGenerator(arch=ARCH)
    disc = models.DCGANDiscriminator(arch=ARCH)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=batch * world, batch_size=batch, d_steps_per_g_step=d_steps)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_ema_logs"), step_replay=replay, generator_ema=ema)


def _batches(n, batch=B, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(batch, *SHAPE, generator=g) * 2 - 1).cuda() for _ in range(n)]


def _recursion(avg, thetas, ws):
    """The float32 statement of the rule over a sequence of live weights (lists of float32 arrays)."""
    for theta, w in zip(thetas, ws):
        w = np.float32(w)
        avg = [a - w * (a - t) for a, t in zip(avg, theta)]
    assert all(a.dtype == np.float32 for a in avg)
    return avg


def _same(got, want, what=""):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what} variable {i}")


WARM = dict(decay=0.9, warmup=True)


@functools.lru_cache(maxsize=None)
def _six_steps(with_ema, replay):
    """Six train_on_batch calls on the same batches; the live generator's variables after every step."""
    gan = _gan(GeneratorEMA(**WARM) if with_ema else None, replay=replay)
    start = gan.generator.get_weights()
    live = []
    for reals in _batches(6):
        gan.train_on_batch(reals)
        live.append(gan.generator.get_weights())
    torch.cuda.synchronize()
    return {"start": start, "live": live, "g_theta": gan.generator.store.theta.cpu().numpy(), "g_state": gan.generator.store.state.cpu().numpy(),
            "d_theta": gan.discriminator.store.theta.cpu().numpy(), "stats": dict(gan._programs.stats),
            "avg": gan.generator_ema.get_weights() if with_ema else None, "updates": gan.generator_ema_updates,
            "avg_theta": gan.generator_ema.store.theta.cpu().numpy() if with_ema else None,
            "avg_state": gan.generator_ema.store.state.cpu().numpy() if with_ema else None}


def test_recorded_and_replayed_steps_follow_the_float32_recursion():
    run = _six_steps(True, True)
    sched = GeneratorEMA(**WARM)
    ws = [sched.w_at(k, B, 1, 1) for k in range(6)]
    assert len({np.float32(w) for w in ws}) == 6            # warm-up: another w at every step, so a stale binding cannot pass
    want = _recursion(run["start"], run["live"], ws)
    names = [spec[0] for l, shape in models.DCGANGenerator(arch=ARCH).flat_layers() for spec in l.var_specs(shape)]
    assert "moving_mean" in names and "kernel" in names and len(names) == len(want)       # trainable and BatchNorm statistics alike
    _same(run["avg"], want, "averaged")
    assert any(not np.array_equal(a, b) for a, b in zip(run["avg"], run["live"][-1]))     # and it is an average, not a copy
    assert run["updates"] == 6
    assert run["stats"]["replayed"] > 0, run["stats"]


def test_eager_steps_give_the_same_averages_bit_for_bit():
    a, b = _six_steps(True, True), _six_steps(True, False)
    assert b["stats"]["replayed"] == 0 and b["updates"] == 6
    np.testing.assert_array_equal(a["avg_theta"], b["avg_theta"])
    np.testing.assert_array_equal(a["avg_state"], b["avg_state"])


def test_the_feature_does_not_perturb_training():
    on, off = _six_steps(True, True), _six_steps(False, True)
    assert off["avg"] is None and off["updates"] == 0
    for name in ("g_theta", "g_state", "d_theta"):
        np.testing.assert_array_equal(on[name], off[name], err_msg=name)


def _launch_names(fn):
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in ops.prof_records()]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


@pytest.mark.parametrize("with_ema", [False, True], ids=["off", "on"])
def test_launch_list_one_ema_per_generator_step_none_elsewhere(with_ema):
    """d_steps_per_g_step = 2: a batch with an even index runs the critic and the generator step, an odd one the critic step only."""
    gan = _gan(0.9 if with_ema else None, d_steps=2)
    per_batch = []
    for reals in _batches(8):
        per_batch.append(_launch_names(lambda: gan.train_on_batch(reals)))
    assert gan._programs.last_was_replay and gan._programs.stats["replayed"] >= 4, gan._programs.stats
    counts = [names.count("ema") for names in per_batch]
    assert counts == ([1, 0] * 4 if with_ema else [0] * 8), counts          # eager, recorded and replayed steps alike
    assert all("adam" in names for names in per_batch)
    if with_ema:
        # eager, outside train_on_batch: the critic step has none, the generator step exactly one, right after its optimizer
        assert "ema" not in _launch_names(lambda: gan.discriminator_step(_batches(1)[0]))
        names = _launch_names(gan.generator_step)
        assert names.count("ema") == 1 and names[names.index("ema") - 1] == "adam", names


def test_d_steps_per_g_step_two_counts_generator_updates_and_scales_the_halflife():
    sched = GeneratorEMA(halflife_images=40)
    gan = _gan(sched, d_steps=2)
    start, live = gan.generator.get_weights(), []
    for i, reals in enumerate(_batches(6)):
        gan.train_on_batch(reals)
        if i % 2 == 0:
            live.append(gan.generator.get_weights())
    assert gan.generator_ema_updates == 3 and gan._programs.stats["replayed"] > 0
    w = sched.w_at(0, B, 1, 2)
    assert w == 1.0 - 0.5 ** (B * 2 / 40.0)
    _same(gan.generator_ema.get_weights(), _recursion(start, live, [w] * 3), "averaged")
    wrong = _recursion(start, live, [sched.w_at(0, B, 1, 1)] * 3)
    assert any(not np.array_equal(a, b) for a, b in zip(gan.generator_ema.get_weights(), wrong))


# ------------------------------------------------------------------ sampling
@pytest.mark.parametrize("make_gen", [None, _hand_built_generator], ids=["dcgan", "hand_built"])
def test_sampling_uses_the_current_averages(make_gen):
    gan = _gan(GeneratorEMA(decay=0.5), make_gen=make_gen)
    z = torch.rand(5, 10, generator=torch.Generator().manual_seed(1)).cuda()
    batches = _batches(5)

    def check():
        got = gan.generate_samples(z, ema=True).clone()
        assert torch.equal(got, gan.generator_ema(z))
        bg.set_seed(99)
        fresh = make_gen() if make_gen else models.DCGANGenerator(arch=ARCH)
        fresh.build()
        fresh.set_weights(gan.generator_ema.get_weights())
        assert torch.equal(got, fresh(z))
        assert not torch.equal(got, gan.generate_samples(z).clone())            # the live generator is elsewhere
        return got

    for reals in batches[:4]:
        gan.train_on_batch(reals)
    first = check()
    gan.train_on_batch(batches[4])                                                # a replay: the averages move, the transposed copies are stale
    assert gan._programs.last_was_replay and gan.generator_ema.store.tr_dirty
    second = check()
    assert not torch.equal(first, second) and not gan.generator_ema.store.tr_dirty
    assert gan.generator_ema_updates == 5


def test_sampling_without_the_feature_is_an_error():
    gan = _gan(None)
    with pytest.raises(ValueError, match="generator_ema"):
        gan.generate_samples(torch.rand(2, 10), ema=True)
    with pytest.raises(ValueError, match="inference"):
        _gan(0.9).generate_samples(torch.rand(2, 10), training=True, ema=True)


def test_building_the_average_draws_nothing_from_the_init_rng():
    out = []
    for ema in (None, GeneratorEMA(decay=0.9)):
        _gan(ema, seed=11)
        out.append(models.DCGANGenerator(arch=ARCH).build().get_weights())
    _same(out[0], out[1])
    gan = _gan(0.9)
    st = gan.generator_ema.store
    assert st.grad is None and st.m is None and st.v is None and st.s3 is None
    assert torch.equal(st.theta, gan.generator.store.theta) and torch.equal(st.state, gan.generator.store.state)


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_resume_is_bit_identical_for_averages_and_count(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    sched = lambda: GeneratorEMA(halflife_images=64, warmup=True)
    batches = _batches(6)
    ref = _gan(sched())
    for reals in batches[:3]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path)).save(3)
    for reals in batches[3:]:
        ref.train_on_batch(reals)
    resumed = _gan(sched(), seed=5)
    CheckpointManager(resumed, str(tmp_path)).restore(path)
    assert resumed.generator_ema_updates == 3 and resumed.generator_ema.store.tr_dirty
    for reals in batches[3:]:
        resumed.train_on_batch(reals)
    assert resumed.generator_ema_updates == ref.generator_ema_updates == 6
    for a, b in ((ref.generator_ema, resumed.generator_ema), (ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
    assert not torch.equal(ref.generator_ema.store.theta, ref.generator.store.theta)


def test_checkpoints_cross_between_models_with_and_without_the_feature(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    batches = _batches(2)
    plain, avg = _gan(None), _gan(0.9)
    for gan in (plain, avg):
        for reals in batches:
            gan.train_on_batch(reals)
    p_plain = CheckpointManager(plain, str(tmp_path / "plain")).save(2)
    p_avg = CheckpointManager(avg, str(tmp_path / "avg")).save(2)
    # written without the feature -> a model with it: averages == restored live weights, count 0, a warning
    into = _gan(0.9, seed=6)
    into.generator_ema_updates = 4
    with pytest.warns(RuntimeWarning, match="averaged generator"):
        CheckpointManager(into, str(tmp_path / "plain")).restore(p_plain)
    assert into.generator_ema_updates == 0
    for name in ("theta", "state"):
        assert torch.equal(getattr(into.generator_ema.store, name), getattr(plain.generator.store, name))
        assert torch.equal(getattr(into.generator.store, name), getattr(plain.generator.store, name))
    # written with the feature -> a model without it
    bare = _gan(None, seed=7)
    CheckpointManager(bare, str(tmp_path / "avg")).restore(p_avg)
    assert bare.generator_ema is None and torch.equal(bare.generator.store.theta, avg.generator.store.theta)
    bare.train_on_batch(batches[0])


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from blurred_gan_amd import dist
    torch.cuda.set_device(0)
    torch.distributed.init_process_group(backend="gloo")
    assert dist.world_size() == world
    b_local = 4
    sched = GeneratorEMA(halflife_images=32)
    gan = _gan(sched, batch=b_local, world=world, seed=17)
    start, live = gan.generator.get_weights(), []
    for reals in _batches(3, batch=b_local, seed=40 + rank):           # every rank its own shard
        gan.train_on_batch(reals)
        live.append(gan.generator.get_weights())
    torch.cuda.synchronize()
    assert gan.generator_ema_updates == 3
    w = sched.w_at(0, b_local, world, 1)
    assert w == 1.0 - 0.5 ** (b_local * world / 32.0)
    _same(gan.generator_ema.get_weights(), _recursion(start, live, [w] * 3), f"rank {rank}")
    wrong = _recursion(start, live, [sched.w_at(0, b_local, 1, 1)] * 3)
    assert any(not np.array_equal(a, b) for a, b in zip(gan.generator_ema.get_weights(), wrong))
    st = gan.generator_ema.store
    np.save(os.path.join(out_dir, f"avg_theta_{rank}.npy"), st.theta.cpu().numpy())
    np.save(os.path.join(out_dir, f"avg_state_{rank}.npy"), st.state.cpu().numpy())
    np.save(os.path.join(out_dir, f"g_theta_{rank}.npy"), gan.generator.store.theta.cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_end_with_bit_identical_averages(tmp_path):
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for name in ("avg_theta", "avg_state", "g_theta"):
        np.testing.assert_array_equal(np.load(tmp_path / f"{name}_0.npy"), np.load(tmp_path / f"{name}_1.npy"), err_msg=name)
    assert not np.array_equal(np.load(tmp_path / "avg_theta_0.npy"), np.load(tmp_path / "g_theta_0.npy"))
