"""Writes tests/golden/engine_trace.json: the ORDER and the arguments of everything engine.Net and the wgan step enqueue, traced
on the CPU with no device.

Every launch the engine makes is a call of a function in ``ops``, every collective a call into ``dist``.  Here the public
functions of ``ops`` are replaced by recorders that append one line per call and return what the real function returns (its
output tensor, or None), so a whole forward / backward / gradient-penalty pass -- or a whole ``train_on_batch`` -- runs on CPU
tensors and leaves its call list behind.  A line reads ``name(param=value, ...)`` with the arguments bound to the real
function's signature (defaults included, so positional and keyword spellings of one launch give one line).

* A tensor is written ``T<label>+<storage offset>:<shape>:<dtype>``; labels number the storages in order of first appearance
  within a configuration.  Aliasing, slicing and buffer reuse are therefore part of the trace, addresses are not.
* ``ops.epilogue`` returns a plain dict of its fields; it is written inside the conv launch that consumes it, not as a call.
* ``ops.uniform`` / ``ops.keep_mask`` advance their host counter as the real ones do and show the offset they drew at.
* ``dist.collectives_active`` / ``world_size`` answer what the configuration says; ``all_reduce_sum_``,
  ``all_reduce_sum_async`` and the ``wait()`` of its handle are recorded, as are ``ready(lo, hi)`` / ``finish()`` of a reducer.
* Pure host queries are answered and NOT traced, so a later change may cache or reorder them: ``*_workspace_bytes``,
  ``blur_policy`` and ``gauss_kernel_1d`` by the real library, ``conv2d_stats_rows`` and ``blur3_lerp_supported`` by the
  constants a configuration sets (their real answers depend on a launch that never ran).
* Not traced: the ``capture_branches`` test instrumentation of ``gp_second_order_merged``, and torch-side host plumbing (the
  pinned upload of the blur taps, injected masks copied into the mask buffer, the read of the metric buffer).

``python tests/golden/make_engine_trace.py [--root DIR] [--out FILE]`` traces the package importable from DIR (default: this
repository) -- the committed file comes from the engine before a refactor and must be reproduced byte for byte after it.
``--coverage`` also lists the lines of Net.forward / backward / gp_second_order / gp_second_order_merged and of the private
helpers of Net that no configuration executed (tests/test_engine_trace_cpu.py asserts there are none)."""
import argparse
import contextlib
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "engine_trace.json")

# the parameter whose tensor each recorder hands back, as the real function does (None: returns nothing)
RETURNS = {"blur_nhwc": "y", "blur3_lerp": "y3", "conv2d_fwd": "y", "conv2d_bwd_data": "dx", "conv2d_bwd_filter": "dw",
           "transpose_last2": "dst", "transpose_last2_batched": "dst_base", "gemm": "Cm", "colsum": "out", "bn_train_fwd": "y",
           "bn_train_fwd_partials": "y", "bn_sums_from_partials": "sums", "bn_infer_fwd": "y", "bn_train_bwd": "dx",
           "bn_fold": None, "bn_fold_many": None, "bn_stats": "sums", "bn_finalize": None, "bn_apply": "y",
           "bn_finalize_apply": "y", "bn_bwd_stats": "sums", "bn_bwd_apply": "dx", "bn_param_grads": None, "lerp": "out",
           "row_norm": "out_b", "gp_seed": "out", "mul_grad": "out", "tanh_bwd": "out", "fill": "x", "scale_": "x", "copy_": "dst",
           "upsample2x": "y", "pool2x_sum": "y", "wgangp_d_loss": None, "wgan_g_loss": None, "adam": None, "sgd": None,
           "rmsprop": None, "adam_amsgrad": None, "ema": None, "uniform": "out", "keep_mask": "out"}
FUNCTIONS = ("forward", "backward", "gp_second_order", "gp_second_order_merged")


class Trace:
    def __init__(self):
        self.calls, self._labels, self._held = [], {}, []

    def enc(self, v):
        if isinstance(v, torch.Tensor):
            st = v.untyped_storage()
            key = st.data_ptr()
            if key not in self._labels:
                self._labels[key] = len(self._labels)
                self._held.append(st)               # a freed storage's address could come back under another label
            s = f"T{self._labels[key]}+{v.storage_offset()}:{'x'.join(map(str, v.shape))}:{str(v.dtype)[6:]}"
            return s if v.is_contiguous() else s + f":strides{tuple(v.stride())}"
        if isinstance(v, dict):
            return "{" + ", ".join(f"{k}={self.enc(x)}" for k, x in v.items()) + "}"
        if isinstance(v, (list, tuple)):
            return "[" + ", ".join(self.enc(x) for x in v) + "]"
        if isinstance(v, (bool, np.bool_)):
            return str(bool(v))
        if isinstance(v, (int, np.integer)):
            return str(int(v))
        if isinstance(v, (float, np.floating)):
            return repr(float(v))
        if v is None or isinstance(v, str):
            return repr(v)
        raise TypeError(f"cannot trace an argument of type {type(v).__name__}")

    def add(self, name, bound):
        self.calls.append(f"{name}(" + ", ".join(f"{k}={self.enc(v)}" for k, v in bound.items()) + ")")


class _Work:
    def __init__(self, tr, n):
        self._tr, self._n = tr, n

    def wait(self):
        self._tr.calls.append(f"wait(all_reduce_sum_async#{self._n})")


class Reducer:
    """Stands in for dist.GradReducer: records what the engine hands over and when."""

    def __init__(self, tr, *a, **k):
        self._tr = tr

    def ready(self, lo, hi):
        self._tr.calls.append(f"reducer.ready({int(lo)}, {int(hi)})")

    def finish(self):
        self._tr.calls.append("reducer.finish()")


@contextlib.contextmanager
def tracing(bg, tr, collectives=False, world=1, stats_rows=0, blur3=True, env=()):
    """Patches ``ops`` and ``dist`` of the package ``bg`` for the duration of one configuration."""
    ops, dist = bg.ops, bg.dist
    saved = []

    def patch(mod, name, fn):
        saved.append((mod, name, getattr(mod, name)))
        setattr(mod, name, fn)

    def recorder(name, real):
        sig = inspect.signature(real)

        def rec(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            if "counter" in args:                   # the draw's offset is the launch's argument; the counter advances as in ops
                args["offset"] = ops._draw_offset(args["out"], args["offset"], args.pop("counter"))
            tr.add(name, args)
            return args[RETURNS[name]] if RETURNS[name] else None
        return rec

    def epilogue(*a, **k):
        b = inspect.signature(saved_epilogue).bind(*a, **k)
        b.apply_defaults()
        return dict(b.arguments)

    for name, real in list(vars(ops).items()):
        if name in RETURNS:
            patch(ops, name, recorder(name, real))
        elif (inspect.isfunction(real) and real.__module__ == ops.__name__ and not name.startswith("_")
              and not name.endswith("_workspace_bytes") and name not in _UNTRACED):
            raise RuntimeError(f"ops.{name} is neither traced nor listed as a host query")
    saved_epilogue = ops.epilogue
    patch(ops, "epilogue", epilogue)
    patch(ops, "trace_range", lambda name: contextlib.nullcontext())
    patch(ops, "conv2d_stats_rows", lambda epi: stats_rows if epi is not None and epi["stats"] is not None else 0)
    patch(ops, "blur3_lerp_supported", lambda *a: bool(blur3))
    n_async = [0]

    def all_reduce_sum_(flat):
        tr.add("all_reduce_sum_", {"flat": flat})
        return flat

    def all_reduce_sum_async(flat):
        n_async[0] += 1
        tr.add(f"all_reduce_sum_async#{n_async[0]}", {"flat": flat})
        return _Work(tr, n_async[0])

    patch(dist, "collectives_active", lambda: bool(collectives))
    patch(dist, "world_size", lambda: int(world))
    patch(dist, "all_reduce_sum_", all_reduce_sum_)
    patch(dist, "all_reduce_sum_async", all_reduce_sum_async)
    patch(dist, "GradReducer", lambda *a, **k: Reducer(tr, *a, **k))
    patch(bg.layers, "default_device", lambda: torch.device("cpu"))      # also where a GPU is present: nothing is launched
    old_env = {k: os.environ.get(k) for k in ("BGAN_NO_FUSED_BLUR3", "BGAN_NO_FUSED_BN_STATS", "BGAN_NO_STEP_REPLAY")}
    for k in old_env:
        os.environ.pop(k, None)
    os.environ.update(dict(env))
    try:
        yield
    finally:
        for mod, name, fn in reversed(saved):
            setattr(mod, name, fn)
        for k, v in old_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# public functions of ops that launch nothing a training step uses, or answer a host question
_UNTRACED = {"same_out", "epilogue", "blur_policy", "gauss_kernel_1d", "blur3_lerp_supported", "conv_math_code", "conv2d_math_taken",
             "conv2d_stats_rows", "outer", "u8_normalize_resize", "u8_gather_normalize_resize", "swd_ingest", "pyr_down", "pyr_up",
             "swd_gather", "swd_standardize", "sort_rows", "abs_diff_mean", "prof_enable", "prof_reset", "conv2d_useful_flops",
             "prof_records", "check"}


# ---------------------------------------------------------------------------------------------------- stacks
def _f(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def _net(bg, ls, blur=None):
    L = bg.layers
    m = L.Sequential(ls)
    if blur is not None:
        m = L.Sequential([bg.gaussian_blur.GaussianBlur2D(initial_std=blur, input_shape=m.input_shape[1:]), m])
    m.build("cpu")
    return m.net()


def _critic(bg, blur=0.9, rates=(0.3, 0.3), pool=False, hw=8):
    """conv + LeakyReLU + Dropout (+ AveragePooling2D) x len(rates) -> Flatten -> Dense(1)."""
    L = bg.layers
    ls = []
    for i, r in enumerate(rates):
        kw = dict(input_shape=(hw, hw, 3)) if i == 0 else {}
        ls += [L.Conv2D(4 * (i + 1), 3, strides=1 if pool else 2, padding="same", **kw), L.LeakyReLU(), L.Dropout(r)]
        if pool:
            ls.append(L.AveragePooling2D())
    return _net(bg, ls + [L.Flatten(), L.Dense(1)], blur)


def _generator(bg, n_bn=1, bias=False, resize=False):
    """Dense + BN + LeakyReLU -> Reshape -> [ConvT | UpSampling2D + Conv] + BN + LeakyReLU x n_bn -> ConvT + tanh."""
    L = bg.layers
    ls = [L.Dense(2 * 2 * 8, use_bias=False, input_shape=(5,)), L.BatchNormalization(), L.LeakyReLU(), L.Reshape((2, 2, 8))]
    for j in range(n_bn):
        if resize:
            ls += [L.UpSampling2D(), L.Conv2D(4, 3, padding="same", use_bias=bias)]
        else:
            ls.append(L.Conv2DTranspose(4, 3, strides=2 if j == 0 else 1, padding="same", use_bias=bias))
        ls += [L.BatchNormalization(), L.LeakyReLU()]
    ls.append(L.Conv2DTranspose(3, 3, strides=2, padding="same", use_bias=False, activation="tanh"))
    return _net(bg, ls)


def _red(bg):
    return bg.dist.GradReducer(None, 0)


# ---------------------------------------------------------------------------------------------------- configurations
def _merged(bg, net, B, defer, masks=None, seed=11):
    """The merged 3B critic pass as wgan.discriminator_step drives it."""
    shp = net.in_shape
    c3 = net.context(3 * B, "fr3", drop_rows=2 * B)
    net.forward(c3, [_f(B, *shp), _f(B, *shp)], training=True, masks=masks, seed=seed, lerp_alpha=_f(B), lerp_out=_f(B, *shp))
    g = net.backward(c3, _f(3 * B, 1), need_dx=True, need_dw=True, dw_rows=2 * B, dx_rows=(2 * B, 3 * B), defer_conv_dw=defer)
    if defer:
        net.gp_second_order_merged(c3, 2 * B, 3 * B, reducer=_red(bg))
    else:
        net.gp_second_order(c3.rows(2 * B, 3 * B), _f(*g.shape), reducer=_red(bg))


def _unmerged(bg, net, B, masks=None):
    """The reference's order: [fakes; reals] pass, x-hat pass without weight gradients, then the second order."""
    shp = net.in_shape
    cfr, chat = net.context(2 * B, "fr"), net.context(B, "hat")
    net.forward(cfr, [_f(B, *shp), _f(B, *shp)], training=True, masks=masks, seed=11)
    net.forward(chat, _f(B, *shp), training=False)
    g = net.backward(chat, _f(B, 1), need_dx=True, need_dw=False)
    net.backward(cfr, _f(2 * B, 1), need_dx=False, need_dw=True)
    net.gp_second_order(chat, _f(*g.shape), reducer=_red(bg))


def _masks(net, rows):
    return [torch.ones((rows,) + st.out_shape, dtype=torch.uint8) for st in net.stages if st.drop]


def _g_step(bg, net, B, reducer=True, need_dw=True, need_dx=None, training=True):
    ctx = net.context(B, "g")
    out = net.forward(ctx, _f(B, *net.in_shape), training=training)
    if training:
        net.backward(ctx, _f(*out.shape), need_dx=not need_dw if need_dx is None else need_dx, need_dw=need_dw,
                     reducer=_red(bg) if reducer else None)


def _refused(bg, tr):
    """Both second-order passes on a network that is not the reference critic shape."""
    net = _generator(bg)
    ctx = net.context(2)
    for call in (lambda: net.gp_second_order(ctx, _f(2, *net.in_shape)), lambda: net.gp_second_order_merged(ctx, 0, 2)):
        try:
            call()
        except NotImplementedError as e:
            tr.calls.append(f"NotImplementedError({e})")


def _unfused_pool(bg, B=2):
    """A pooling stage behind a conv WITHOUT LeakyReLU (plain upsample backward, EPI_NONE conv) and one behind conv + LeakyReLU
    without Dropout (fused backward, no mask)."""
    L = bg.layers
    net = _net(bg, [L.Conv2D(4, 3, padding="same", input_shape=(4, 4, 3)), L.AveragePooling2D(),
                    L.Conv2D(4, 3, padding="same"), L.LeakyReLU(), L.AveragePooling2D(), L.Flatten(), L.Dense(1)])
    ctx = net.context(B)
    net.forward(ctx, _f(B, 4, 4, 3), training=True)
    net.backward(ctx, _f(B, 1), need_dx=True)


def _gan(bg, cls, blur=True, gbs=2, **kw):
    bg.layers.set_seed(3)
    gen, disc = bg.models.DCGANGenerator(arch="tiny"), bg.models.DCGANDiscriminator(arch="tiny")
    hp = cls.HyperParameters(batch_size=2, global_batch_size=gbs, **({"initial_blur_std": 0.9} if blur else {}))
    for m in (gen, disc):
        m.build("cpu")
    return cls(gen, disc, hp, bg.TrainingConfig(log_dir=os.devnull), step_replay=False, **kw)


def _train(gan, steps=1, randomness=None):
    for _ in range(steps):
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32), randomness=randomness)


def _randomness(bg):
    m = [np.ones((2, 4, 4, 16), np.uint8), np.ones((2, 2, 2, 32), np.uint8)]
    return dict(z_d=np.zeros((2, 10), np.float32), z_g=np.zeros((2, 10), np.float32), alpha=np.zeros(2, np.float32), mask_fake=m, mask_real=m)


def _gp_fn(bg):
    bg.layers.set_seed(3)
    disc = bg.models.DCGANDiscriminator(arch="tiny")
    disc.build("cpu")
    bg.wgan.gradient_penalty(disc, _f(2, 8, 8, 3), _f(2, 8, 8, 3), alpha=_f(2))


DP = dict(collectives=True, world=2)
# name -> (the branches it is there for, keywords of tracing(), run(bg))
CONFIGS = {
    "critic_merged_blur3_deferred": ("forward: lerp_alpha on the three-source blur, one mask draw for all stages, LRELU epilogue with keep_elems; "
                                     "backward: dw_rows / dx_rows, defer_conv_dw, MUL_GRAD epilogue with mask tail, mul_grad split into "
                                     "masked rows + tail, blur^T into a0 rows; gp_second_order_merged: conv, dense",
                                     {}, lambda bg: _merged(bg, _critic(bg), 2, True)),
    "critic_merged_lerp_two_wgrads": ("forward: lerp_alpha through bg_lerp_f32 + per-slice blur; backward: conv filter gradients taken here; "
                                      "gp_second_order on ctx.rows(2B, 3B): conv, dense", dict(blur3=False),
                                      lambda bg: _merged(bg, _critic(bg), 2, False)),
    "critic_merged_blur3_switched_off": ("forward: BGAN_NO_FUSED_BLUR3 forces the bg_lerp_f32 route", dict(env={"BGAN_NO_FUSED_BLUR3": "1"}),
                                         lambda bg: _merged(bg, _critic(bg), 3, True)),
    "critic_unmerged": ("forward: list input through per-slice blur, single input, training=False; backward: need_dw=False, "
                        "need_dx=False early return, full-batch masks; gp_second_order on a whole context", {},
                        lambda bg: _unmerged(bg, _critic(bg), 2)),
    "critic_injected_masks": ("forward: masks copied in instead of drawn", {},
                              lambda bg: (lambda n: _merged(bg, n, 2, True, masks=_masks(n, 4)))(_critic(bg))),
    "critic_no_blur_list_input": ("forward: copy path of a list input without blur, lerp_alpha without blur; backward: no blur^T; "
                                  "second order without blur", {}, lambda bg: (_merged(bg, _critic(bg, blur=None), 2, True),
                                                                              _unmerged(bg, _critic(bg, blur=None), 2))),
    "critic_rates_differ": ("forward: keep_rate None, masks drawn per stage; injected masks per stage", {},
                            lambda bg: (_merged(bg, _critic(bg, rates=(0.3, 0.5)), 2, True),
                                        (lambda n: _unmerged(bg, n, 2, masks=_masks(n, 4)))(_critic(bg, rates=(0.3, 0.5))))),
    "pool_critic_merged_mask_tail": ("forward: resampling stage; backward: fused pooling backward split into masked rows + tail; "
                                     "gp_second_order_merged and gp_second_order: resampling stage", {},
                                     lambda bg: (_merged(bg, _critic(bg, pool=True), 2, True), _merged(bg, _critic(bg, pool=True), 2, False))),
    "pool_critic_unmerged": ("backward: fused pooling backward with a full-batch mask and (training=False) without one", {},
                             lambda bg: _unmerged(bg, _critic(bg, pool=True, hw=4), 3)),
    "pool_unfused": ("forward: EPI_NONE conv (no activation, no BatchNorm); backward: plain pooling backward, fused one without Dropout",
                     {}, _unfused_pool),
    "generator_train": ("forward: Dense + BatchNorm, bn_train_fwd, tanh epilogue, ConvT as data gradient; backward: tanh_bwd, "
                        "bn_train_bwd, ConvT filter / input gradients, Dense gradients, reducer.ready at once", {},
                        lambda bg: _g_step(bg, _generator(bg), 3)),
    "generator_train_fused_stats": ("forward: fuse_bn_stats, statistics partials from the conv epilogue (bn_train_fwd_partials)",
                                    dict(stats_rows=3), lambda bg: (lambda n: (setattr(n, "fuse_bn_stats", True), _g_step(bg, n, 2)))(_generator(bg))),
    "generator_train_no_dw": ("backward: BatchNorm gradients into scratch (need_dw=False), input gradient returned", {},
                              lambda bg: _g_step(bg, _generator(bg), 2, need_dw=False)),
    "generator_infer_one_fold": ("forward: inference, one BatchNorm conv -> bn_fold + AFFINE_LRELU epilogue; Dense BatchNorm -> bn_infer_fwd",
                                 {}, lambda bg: _g_step(bg, _generator(bg), 2, training=False)),
    "generator_infer_fold_many": ("forward: inference, two BatchNorm convs -> one bn_fold_many", {},
                                  lambda bg: _g_step(bg, _generator(bg, n_bn=2), 2, training=False)),
    "generator_bias_conv": ("forward: BatchNorm conv WITH bias: bn_infer_fwd in inference, no statistics epilogue in training; "
                            "backward: bias column sums", dict(stats_rows=3),
                            lambda bg: (lambda n: (setattr(n, "fuse_bn_stats", True), _g_step(bg, n, 2, training=False), _g_step(bg, n, 2)))
                            (_generator(bg, bias=True))),
    "generator_resize_train": ("forward / backward: UpSampling2D stage and a Conv2D with BatchNorm in a generator", {},
                               lambda bg: _g_step(bg, _generator(bg, n_bn=2, resize=True), 2)),
    "dp_generator_epilogue_stats": ("forward: SyncBN statistics out of the conv epilogue (bn_sums_from_partials) and, for Dense, bn_stats; "
                                    "backward: overlap order, deferred_ready released behind the exchange", dict(DP, stats_rows=3),
                                    lambda bg: _g_step(bg, _generator(bg, n_bn=2), 2)),
    "dp_generator_separate_stats": ("forward: SyncBN statistics by the separate pass (the conv took a kernel without the epilogue)",
                                    dict(DP, stats_rows=0), lambda bg: _g_step(bg, _generator(bg, n_bn=2), 2)),
    "dp_generator_stats_switched_off": ("forward: BGAN_NO_FUSED_BN_STATS under SyncBN", dict(DP, stats_rows=3, env={"BGAN_NO_FUSED_BN_STATS": "1"}),
                                        lambda bg: _g_step(bg, _generator(bg), 2)),
    "dp_generator_no_reducer": ("backward: SyncBN overlap without a reducer; need_dw=False under SyncBN (statistics per stage)", DP,
                                lambda bg: (_g_step(bg, _generator(bg, n_bn=2), 2, reducer=False), _g_step(bg, _generator(bg), 2, need_dw=False))),
    "dp_generator_sync_bn_off": ("forward / backward: sync_bn=False with collectives active: per-replica statistics", DP,
                                 lambda bg: (lambda n: (setattr(n, "sync_bn", False), _g_step(bg, n, 2)))(_generator(bg))),
    "dp_resize_generator": ("backward: overlap across an UpSampling2D stage (no filter gradient, no overlap step of its own)", dict(DP, stats_rows=3),
                            lambda bg: (_g_step(bg, _generator(bg, n_bn=2, resize=True), 2),
                                        _g_step(bg, _generator(bg, n_bn=2, resize=True), 2, reducer=False))),
    "dp_generator_input_gradient": ("backward: need_dx with a reducer under the overlap: the last deferred slices go out after the loop", DP,
                                    lambda bg: _g_step(bg, _generator(bg), 2, need_dx=True)),
    "dp_critic_merged": ("backward / gp_second_order_merged: reducer with collectives active on the critic", DP,
                         lambda bg: (_merged(bg, _critic(bg), 2, True), _unmerged(bg, _critic(bg), 2))),
    "step_blurred_wgangp_merged": ("wgan: two whole train_on_batch calls, merged critic pass with the filter gradients merged too", {},
                                   lambda bg: _train(_gan(bg, bg.BlurredWGANGP), steps=2)),
    "step_blurred_wgangp_merged_two_wgrads": ("wgan: merged pass, second order through gp_second_order; injected randomness", {},
                                              lambda bg: _train(_gan(bg, bg.BlurredWGANGP, merge_gp_filter_gradients=False),
                                                                randomness=_randomness(bg))),
    "step_wgangp_merged_no_blur": ("wgan: merged pass without blur (the seed written straight into the x-hat rows), zero-norm guard", {},
                                   lambda bg: _train(_gan(bg, bg.WGANGP, blur=False, gp_zero_norm_guard=True))),
    "step_blurred_wgangp_unmerged": ("wgan: merge_critic_passes=False, _gp_first_order", {},
                                     lambda bg: _train(_gan(bg, bg.BlurredWGANGP, merge_critic_passes=False))),
    "step_wgangp_unmerged_no_blur": ("wgan: unmerged without blur; injected randomness", {},
                                     lambda bg: _train(_gan(bg, bg.WGANGP, blur=False, merge_critic_passes=False), randomness=_randomness(bg))),
    "step_wgan": ("wgan: plain WGAN, the reducer handed to the critic's only backward", {}, lambda bg: _train(_gan(bg, bg.WGAN, blur=False))),
    "step_dp_blurred_wgangp": ("wgan: a whole step with collectives active (SyncBN in the G-step, reducers in both steps)", dict(DP, stats_rows=2),
                               lambda bg: _train(_gan(bg, bg.BlurredWGANGP, gbs=4))),
    "gradient_penalty_function": ("wgan.gradient_penalty (value only)", {}, _gp_fn),
    "second_order_refused": ("gp_second_order / gp_second_order_merged: a network of another shape is refused", {}, _refused),
}


def load_package(root):
    """The package importable from ``root`` (with the HIP library built: the host queries are its own)."""
    root = os.path.abspath(root)
    for k in [k for k in sys.modules if k == "blurred_gan_amd" or k.startswith("blurred_gan_amd.")]:
        del sys.modules[k]
    sys.path.insert(0, root)
    try:
        import blurred_gan_amd as bg
        from blurred_gan_amd import dist, engine, gaussian_blur, layers, models, ops, wgan  # noqa: F401
    finally:
        sys.path.remove(root)
    return bg


def run_config(bg, name):
    _, kw, run = CONFIGS[name]
    tr = Trace()
    torch.manual_seed(0)
    bg.layers.set_seed(3)
    with tracing(bg, tr, **kw):
        run(bg, tr) if run is _refused else run(bg)
    return tr.calls


def make(bg):
    return {name: run_config(bg, name) for name in CONFIGS}


def dumps(traces):
    return json.dumps(traces, indent=0, sort_keys=True) + "\n"


def missed_lines(bg):
    """Lines of Net.forward / backward / gp_second_order(_merged) and of what they delegate to (Net's private helpers, the
    backward's per-pass object, the Dropout helpers of Context) that no configuration executed, as {function: [line, ...]}.  The body of the ``capture_branches`` instrumentation does not count."""
    import dis
    Net = bg.engine.Net
    src = inspect.getsourcelines(bg.engine)[0]
    owner = {}                  # code object (lambdas and closures included) -> the method it belongs to

    def claim(code, fn):
        owner[code] = fn
        for k in code.co_consts:
            if inspect.iscode(k):
                claim(k, fn)

    for cls, wanted in ((Net, lambda n: n in FUNCTIONS or (n.startswith("_") and not n.startswith("__"))),
                        (getattr(bg.engine, "_BackwardPass", None), lambda n: True),
                        (bg.engine.Context, lambda n: n in ("dropout", "masked_then_tail"))):
        for n, f in vars(cls).items() if cls is not None else ():
            if inspect.isfunction(f) and wanted(n):
                claim(f.__code__, f.__qualname__)
    want = {(fn, ln) for code, fn in owner.items() for _, ln in dis.findlinestarts(code)
            if ln is not None and ln != code.co_firstlineno and "capture_branches.append" not in src[ln - 1]}
    seen = set()

    def tracer(frame, event, arg):
        fn = owner.get(frame.f_code)
        if fn is None:
            return None
        if event == "line":
            seen.add((fn, frame.f_lineno))
        return tracer

    sys.settrace(tracer)
    try:
        make(bg)
    finally:
        sys.settrace(None)
    missed = {}
    for fn, ln in sorted(want - seen):
        missed.setdefault(fn, []).append(ln)
    return missed


def ensure_library(root):
    """The host queries are the real library's: build it (incrementally) where the package of ``root`` looks for it."""
    if os.environ.get("BGAN_HIP_LIB"):
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("bgan_build", os.path.join(root, "blurred-gan_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build_lib(verbose=False)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--coverage", action="store_true")
    a = ap.parse_args()
    ensure_library(a.root)
    pkg = load_package(a.root)
    text = dumps(make(pkg))
    with open(a.out, "w") as fh:
        fh.write(text)
    print(f"{a.out}: {len(CONFIGS)} configurations, {text.count(chr(10)) - len(CONFIGS) - 2} calls, {len(text)} bytes")
    if a.coverage:
        missed = missed_lines(pkg)
        print("lines never executed:", missed or "none")
        sys.exit(1 if missed else 0)
