#!/usr/bin/env python
"""The DiffAugment kernels on both routes: us per launch and GB/s of algorithmic bytes (one read and one write of the batch) of
bg_diffaug_f32 and bg_diffaug_adjoint_f32, for the full policy and for the policy without ``color`` (no mean: a gather), each
beside bg_adam_f32 -- the project's own streaming yardstick -- moving the same total bytes in the same process, the two alternating
over --repeats rounds (median and min..max of the rounds).  Shapes: the celeba64 critic's input at the D-step's 3 x 256 and the
G-step's 256 samples (the sample-resident route) and 128 x 128 x 3 images at 3 x 64 and 16 samples (the two-sweep route; the small
batch is what the cut along the sample is for).  Then ms per step of a few timed train_on_batch calls of celeba64 at batch 256 with
augment=None and with the full policy, twice each in turn, same build, same process.
Timing: device events around --iters launches after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_diffaug.py [--iters 50] [--repeats 5] [--steps 20] [--warmup 5] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B = 256
SHAPES = [(3 * B, 64, 64, 3), (B, 64, 64, 3), (3 * 64, 128, 128, 3), (16, 128, 128, 3)]
POLICIES = ["color,translation,cutout", "translation,cutout"]


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


def kernel_rates(shape, policy, iters, repeats):
    import blurred_gan_amd as bg
    from blurred_gan_amd import ops
    cfg = bg.DiffAugment(policy)
    n, H, W, C = shape
    x, g = torch.rand(*shape, device="cuda") - 0.5, torch.rand(*shape, device="cuda") - 0.5
    y, dx = torch.empty_like(x), torch.empty_like(x)
    params = torch.rand(n, 8, device="cuda").clamp_(max=1 - 2.0 ** -24)
    nbytes = 8 * x.numel() + 32 * n                              # algorithmic: the batch read once and written once, the params

    def adam_of(nbytes):                                        # bg_adam_f32 moving nbytes in all: 28 bytes per element
        m = int(nbytes) // 28 // 4 * 4
        th, m1, m2, gr = (torch.rand(m, device="cuda") for _ in range(4))
        return lambda: ops.adam(th, m1, m2, gr, 1e-3)

    cases = {"diffaug_fwd": lambda: ops.diffaug.fwd(x, y, params, **cfg.kernel_args()),
             "diffaug_adjoint": lambda: ops.diffaug.adjoint(g, dx, params, **cfg.kernel_args())}
    rows = []
    for name, launch in cases.items():
        t = _alternate({name: launch, "adam": adam_of(nbytes)}, iters, repeats)
        row, ad = _row(name, shape, nbytes, t[name]), _row("adam_same_bytes", shape, nbytes, t["adam"])
        row["policy"] = cfg.policy
        row["route"] = "resident" if ops.diffaug.route(H, W, C)["resident"] else "two_sweep"
        row["vs_adam"] = round(row["GBps_median"] / ad["GBps_median"], 3)
        row["adam_us_median"], row["adam_GBps_median"], row["adam_GBps_min_max"] = ad["us_median"], ad["GBps_median"], ad["GBps_min_max"]
        rows.append(row)
    return rows


def step_rate(augment, steps, warmup, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch)
    disc = models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"), augment=augment)
    H, W, C = models.IMAGE_SHAPE[arch]
    g = torch.Generator(device="cuda").manual_seed(123123)
    reals = torch.rand(B, H, W, C, device="cuda", generator=g) * 2 - 1
    for _ in range(warmup):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    launches = {k: int(v) for k, v in gan._programs.stats.items()} if hasattr(gan._programs, "stats") else {}
    return {"images_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup,
            "programs": launches}


def step_launch_times(augment, arch="celeba64", sigma=5.0):
    """us per launch of the augmentation's own launches inside one eager step (the library's event pairs, bg_prof_*)."""
    import blurred_gan_amd as bg
    from blurred_gan_amd import models, ops
    bg.set_seed(123123)
    gan = bg.BlurredWGANGP(models.DCGANGenerator(arch=arch), models.DCGANDiscriminator(arch=arch),
                           bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B),
                           bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"), augment=augment, step_replay=False)
    reals = torch.rand(B, *models.IMAGE_SHAPE[arch], device="cuda") * 2 - 1
    for _ in range(3):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_reset()
    for _ in range(5):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    per, total = {}, 0.0
    for rec in ops.prof_records():
        total += rec[1] * 1e3
        if rec[0].startswith("diffaug") or rec[0] == "uniform":
            per.setdefault(rec[0], []).append(rec[1] * 1e3)
    ops.prof_enable(False)
    ops.prof_reset()
    return {"us_per_step_all_launches": round(total / 5, 1), "launches_per_step": {k: len(v) // 5 for k, v in per.items()},
            "us_per_step": {k: round(sum(v) / 5, 2) for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_diffaug.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for shape in SHAPES:
        for policy in POLICIES:
            for r in kernel_rates(shape, policy, a.iters, a.repeats):
                print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    full = POLICIES[0]
    rates = {}
    for aug in (None, full, None, full):                        # twice each, in turn: the spread beside the difference
        r = step_rate(aug, a.steps, a.warmup)
        rates.setdefault(aug, []).append(r["ms_per_step"])
        print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "augment": aug, **r}), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps({"what": "step_ratio", "augmented_over_plain_ms_per_step": round(statistics.mean(rates[full]) / statistics.mean(rates[None]), 4),
                      "plain_ms": rates[None], "augmented_ms": rates[full]}), flush=True)
    print(json.dumps({"what": "step_launches", "augment": full, **step_launch_times(full)}), flush=True)


if __name__ == "__main__":
    main()
