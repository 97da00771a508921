#!/usr/bin/env python
"""The noise kernels at the five noise maps of the celeba64 generator (normalization="pixel", noise=True) at batch 256 (4096 x 512 ...
1 M x 32): us per launch and GB/s of algorithmic bytes of bg_noise_add_f32 (in place, as the engine runs it), of the two launches of
bg_noise_grad_f32 and of bg_normal_f32 over the pass's one noise buffer (256 x 5456 floats), each beside bg_adam_f32 -- the project's
own streaming yardstick -- moving the same total bytes (reads + writes) in the same process, the two alternating over --repeats
rounds (median and min..max of the rounds).  Then ms per step of timed train_on_batch calls of celeba64 at batch 256 with
noise=False and noise=True (both normalization="pixel"), in alternating rounds, and the medians with the spread.
Timing: device events around --iters launches after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_noise.py [--iters 100] [--repeats 5] [--steps 10] [--warmup 5] [--rounds 3] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B = 256
# (rows per sample, channels) of the celeba64 generator's noise maps
SHAPES = {"4x4x512": (16, 512), "8x8x256": (64, 256), "16x16x128": (256, 128), "32x32x64": (1024, 64), "64x64x32": (4096, 32)}
P = sum(r for r, _ in SHAPES.values())          # 5456 noise values per sample


def _time_us(launch, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _alternate(launches, iters, repeats):
    """{name: [us per launch, one entry per round]}; every round times each candidate once, in turn."""
    for f in launches.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in launches}
    for _ in range(repeats):
        for k, f in launches.items():
            out[k].append(_time_us(f, iters))
    return out


def _row(what, shape, nbytes, us):
    rates = [nbytes / u * 1e-3 for u in us]
    return {"what": what, "shape": list(shape), "bytes": int(nbytes), "us_median": round(statistics.median(us), 2),
            "GBps_median": round(statistics.median(rates), 1), "GBps_min_max": [round(min(rates), 1), round(max(rates), 1)]}


def _adam_of(ops, nbytes):
    """bg_adam_f32 moving nbytes in all: 28 bytes per element."""
    m = max(int(nbytes) // 28 // 4 * 4, 4)
    th, m1, m2, gr = (torch.rand(m, device="cuda") for _ in range(4))
    return lambda: ops.adam(th, m1, m2, gr, 1e-3)


def _beside_adam(ops, cases, shape, iters, repeats, **extra):
    out = []
    for what, (nbytes, launch) in cases.items():
        t = _alternate({what: launch, "adam": _adam_of(ops, nbytes)}, iters, repeats)
        row, ad = _row(what, shape, nbytes, t[what]), _row("adam_same_bytes", shape, nbytes, t["adam"])
        row.update(extra)
        row["vs_adam"] = round(row["GBps_median"] / ad["GBps_median"], 3)
        row["adam_us_median"], row["adam_GBps_median"], row["adam_GBps_min_max"] = ad["us_median"], ad["GBps_median"], ad["GBps_min_max"]
        out.append(row)
    return out


def kernel_rates(name, iters, repeats):
    from blurred_gan_amd import ops
    rows_per_sample, C = SHAPES[name]
    R = B * rows_per_sample
    n = R * C
    x, dz = torch.rand(R, C, device="cuda") - 0.5, torch.rand(R, C, device="cuda") - 0.5
    nz = ops.rng.normal(torch.empty(R, device="cuda"), 1)
    s, ds = torch.full((1,), 1e-3, device="cuda"), torch.zeros(1, device="cuda")
    ws = torch.empty(max(ops.noise.workspace_bytes(R, C) // 4, 1), device="cuda")
    # algorithmic bytes: the add reads x and the noise and writes y (in place: |strength| is small, the values stay finite over the
    # repeats); the gradient reads dz and the noise
    cases = {"noise_add": (4 * (2 * n + R), lambda: ops.noise.add(x, nz, s, x, R, C, lrelu_alpha=0.3)),
             "noise_grad": (4 * (n + R), lambda: ops.noise.grad(dz, nz, ds, R, C, ws))}
    return _beside_adam(ops, cases, (R, C), iters, repeats, map=name, route=ops.noise.route(C))


def draw_rate(iters, repeats):
    from blurred_gan_amd import ops
    out = torch.empty(B * P, device="cuda")
    return _beside_adam(ops, {"normal_draw": (4 * B * P, lambda: ops.rng.normal(out, 1))}, (B, P), iters, repeats)


def make_gan(noise, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch, normalization="pixel", noise=noise)
    disc = models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"))


def timed_steps(gan, reals, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for name in SHAPES:
        for r in kernel_rates(name, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    for r in draw_rate(a.iters, a.repeats):
        print(json.dumps(r), flush=True)
    if a.no_step:
        return
    from blurred_gan_amd import models
    H, W, C = models.IMAGE_SHAPE["celeba64"]
    reals = torch.rand(B, H, W, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(123123)) * 2 - 1
    gans = {k: make_gan(k == "noise") for k in ("plain", "noise")}
    for gan in gans.values():
        for _ in range(a.warmup):
            gan.train_on_batch(reals)
    ms = {k: [] for k in gans}
    for rnd in range(a.rounds):                  # alternating rounds: the spread beside the difference
        for k, gan in gans.items():
            ms[k].append(timed_steps(gan, reals, a.steps))
            print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "generator": k, "round": rnd, "ms_per_step": round(ms[k][-1], 3)}), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"what": "step_medians", "ms_per_step": {k: round(v, 3) for k, v in med.items()},
                      "images_per_s": {k: round(B / v * 1e3, 1) for k, v in med.items()},
                      "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                      "noise_over_plain_ms": round(med["noise"] / med["plain"], 3)}), flush=True)


if __name__ == "__main__":
    main()
