#!/usr/bin/env python
"""Optimiser updates at the C2 parameter counts (celeba64 generator / critic flat trainable buffers, store.n_train): us per launch
and algorithmic GB/s of every bg_sgd_f32 / bg_rmsprop_f32 / bg_adam_amsgrad_f32 variant, of bg_adam_f32 and of the weight average
bg_ema_f32 (12 B per element; the network's state buffer rides along as its second segment) in the same run, then C2 images/s
(celeba64, B 256, sigma 5) with the default Adam, RMSprop() and SGD(momentum=0.9), built and driven as tools/bench_step_math.py
does, and the default step with generator_ema=GeneratorEMA(halflife_images=10_000) against the same step without it
(--ema-repeats alternating pairs: one 30-step run each is inside the run-to-run noise).  One JSON line per measurement.
Usage: python tools/bench_optim.py [--iters 200] [--steps 30] [--warmup 10] [--no-step] [--ema-repeats 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

# variant -> (bytes per element, optimizer factory)
VARIANTS = {
    "adam": (28, lambda O: O.Adam()),
    "sgd": (12, lambda O: O.SGD()),
    "sgd_momentum": (20, lambda O: O.SGD(momentum=0.9)),
    "sgd_nesterov": (20, lambda O: O.SGD(momentum=0.9, nesterov=True)),
    "rmsprop": (20, lambda O: O.RMSprop()),
    "rmsprop_momentum": (28, lambda O: O.RMSprop(momentum=0.9)),
    "rmsprop_centered": (28, lambda O: O.RMSprop(centered=True)),
    "rmsprop_centered_momentum": (36, lambda O: O.RMSprop(momentum=0.9, centered=True)),
    "adam_amsgrad": (36, lambda O: O.Adam(amsgrad=True)),
}


def c2_sizes():
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    out = {}
    for tag, m in (("G", models.DCGANGenerator(arch="celeba64")), ("D", models.DCGANDiscriminator(arch="celeba64"))):
        m.build()
        out[tag] = (m.store.n_train, m.store.n_state)
    return out


def _time_us(launch, iters):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_rates(n, iters, n_state=0):
    from blurred_gan_amd import ops
    from blurred_gan_amd import optimizers as O
    bufs = [torch.randn(n, device="cuda") * 1e-2 for _ in range(5)]       # theta, m, v, s3, g
    th, m, v, s3, g = bufs
    rows = []
    for name, (bpe, make) in VARIANTS.items():
        opt = make(O)
        us = _time_us(lambda: opt._launch(th, m, v, s3, g, 1e-9), iters)
        rows.append({"variant": name, "n": n, "bytes_per_elem": bpe, "us": round(us, 2), "GBps": round(bpe * n / us * 1e-3, 1)})
    # the weight average: avg (m's buffer) towards theta, the state buffer's average as the second segment of the same launch
    avg2, th2 = (torch.zeros(n_state, device="cuda"), torch.ones(n_state, device="cuda")) if n_state else (None, None)
    us = _time_us(lambda: ops.ema(m, th, avg2, th2, 1e-3), iters)
    rows.append({"variant": "ema", "n": n, "n2": n_state, "bytes_per_elem": 12, "us": round(us, 2), "GBps": round(12 * (n + n_state) / us * 1e-3, 1)})
    by = {r["variant"]: r["GBps"] for r in rows}
    for r in rows:
        r["vs_adam"] = round(r["GBps"] / by["adam"], 3)
        r["vs_sgd"] = round(r["GBps"] / by["sgd"], 3)
    return rows


def step_rate(make_opt, steps, warmup, arch="celeba64", B=256, sigma=5.0, generator_ema=None):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models, callbacks
    from blurred_gan_amd.models import IMAGE_SHAPE
    bg.set_seed(123123)
    gen, disc = models.DCGANGenerator(arch=arch), models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"), generator_ema=generator_ema)
    gan._rng_seed = 123123
    if make_opt is not None:
        gan.generator.optimizer, gan.discriminator.optimizer = make_opt(), make_opt()
    H, W, C = IMAGE_SHAPE[arch]
    g = torch.Generator(device="cuda").manual_seed(123123)
    reals = torch.rand(B, H, W, C, device="cuda", generator=g) * 2 - 1
    ctl = callbacks.BlurDecayController(total_n_training_examples=202599 * 10, max_value=sigma)
    ctl.set_model(gan)

    def step():
        ctl.on_batch_begin(0, {})
        return gan.train_on_batch(reals)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"images_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 4), "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--ema-repeats", type=int, default=5, help="alternating (off, on) pairs of the C2 step without / with the weight average")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sizes = c2_sizes()
    for tag, (n, n_state) in sizes.items():
        for r in kernel_rates(n, a.iters, n_state):
            print(json.dumps({"what": "kernel", "net": tag, **r}), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    from blurred_gan_amd import optimizers as O
    base = None
    for name, make in (("default_adam", None), ("RMSprop()", lambda: O.RMSprop()), ("SGD(momentum=0.9)", lambda: O.SGD(momentum=0.9))):
        r = {"what": "step", "config": "C2", "optimizer": name, **step_rate(make, a.steps, a.warmup)}
        base = base or r["images_per_s"]
        r["vs_default"] = round(r["images_per_s"] / base, 4)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    import statistics
    import blurred_gan_amd as bg
    runs = {"off": [], "on": []}
    for i in range(a.ema_repeats):
        for tag in ("off", "on"):
            ema = bg.GeneratorEMA(halflife_images=10_000) if tag == "on" else None
            r = step_rate(None, a.steps, a.warmup, generator_ema=ema)
            runs[tag].append(r["images_per_s"])
            print(json.dumps({"what": "step", "config": "C2", "optimizer": "default_adam", "generator_ema": None if ema is None else ema.get_config(),
                              "pair": i, **r}), flush=True)
            torch.cuda.empty_cache()
    if a.ema_repeats:
        med = {k: statistics.median(v) for k, v in runs.items()}
        print(json.dumps({"what": "step_ema_summary", "config": "C2", "pairs": a.ema_repeats, "steps": a.steps,
                          "median_images_per_s": med, "min_max": {k: [min(v), max(v)] for k, v in runs.items()},
                          "on_vs_off": round(med["on"] / med["off"], 4)}), flush=True)


if __name__ == "__main__":
    main()
