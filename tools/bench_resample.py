#!/usr/bin/env python
"""The resampling kernels at the workload's shapes: us per launch and GB/s of algorithmic bytes of bg_upsample2x_nhwc_f32,
bg_pool2x_sum_nhwc_f32 and the fused pooling backward (the upsample with ref + keep), each beside bg_copy_f32 moving the same
total bytes (reads + writes) in the same process, the two alternating over --repeats rounds (median and min..max of the rounds);
the fused backward also beside its two-launch form (upsample, then bg_mul_grad_f32 in place).  Then images/s of a few timed
train_on_batch calls of celeba64 at batch 256 with the default stacks, the resize generator, and resize + pool.
Timing: device events around --iters launches after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_resample.py [--iters 50] [--repeats 5] [--steps 10] [--warmup 5] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

# low-resolution (B, H, W, C): celeba64's two largest resized stages at batch 256, celeba128's largest at batch 128
SHAPES = [(256, 32, 32, 64), (256, 16, 16, 128), (128, 64, 64, 32)]


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


def kernel_rates(shape, iters, repeats):
    from blurred_gan_amd import ops
    B, H, W, C = shape
    n = B * H * W * C                                           # low-resolution elements; the other side holds 4 n
    lo = torch.rand(shape, device="cuda") - 0.5
    hi = torch.rand(B, 2 * H, 2 * W, C, device="cuda") - 0.5
    ref = torch.rand_like(hi) - 0.5
    keep = (torch.rand_like(hi) >= 0.3).to(torch.uint8)
    out_hi, out_lo = torch.empty_like(hi), torch.empty_like(lo)
    rows = []

    def copy_of(nbytes):                                        # bg_copy_f32 moving nbytes in all: nbytes / 8 floats
        m = int(nbytes) // 8
        src, dst = torch.rand(m, device="cuda"), torch.empty(m, device="cuda")
        return lambda: ops.copy_(dst, src)

    cases = {"upsample2x": (20 * n, lambda: ops.upsample2x(lo, out_hi, 0.25)),
             "pool2x_sum": (20 * n, lambda: ops.pool2x_sum(hi, out_lo, 0.25)),
             "upsample2x_mul_grad": (40 * n, lambda: ops.upsample2x(lo, out_hi, 0.25, ref=ref, keep=keep, alpha=0.3, grad_scale=1 / 0.7))}
    for name, (nbytes, f) in cases.items():
        t = _alternate({name: f, "copy": copy_of(nbytes)}, iters, repeats)
        r, c = _row(name, shape, nbytes, t[name]), _row("copy_same_bytes", shape, nbytes, t["copy"])
        r["vs_copy"] = round(r["GBps_median"] / c["GBps_median"], 3)
        r["copy_GBps_median"], r["copy_GBps_min_max"] = c["GBps_median"], c["GBps_min_max"]
        rows.append(r)

    def two_launches():
        ops.upsample2x(lo, out_hi, 0.25)
        ops.mul_grad(out_hi, ref, out_hi, keep=keep, alpha=0.3, scale=1 / 0.7)

    t = _alternate({"fused": cases["upsample2x_mul_grad"][1], "two": two_launches}, iters, repeats)
    f_us, t_us = statistics.median(t["fused"]), statistics.median(t["two"])
    rows.append({"what": "pool_backward_fused_vs_two_launches", "shape": list(shape), "fused_us_median": round(f_us, 2),
                 "fused_us_min_max": [round(min(t["fused"]), 2), round(max(t["fused"]), 2)], "two_launch_us_median": round(t_us, 2),
                 "two_launch_us_min_max": [round(min(t["two"]), 2), round(max(t["two"]), 2)], "saved_us": round(t_us - f_us, 2),
                 "two_over_fused": round(t_us / f_us, 3)})
    return rows


def step_rate(upsampling, downsampling, steps, warmup, arch="celeba64", B=256, sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch, upsampling=upsampling)
    disc = models.DCGANDiscriminator(arch=arch, downsampling=downsampling)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"))
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
    return {"images_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for shape in SHAPES:
        for r in kernel_rates(shape, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    for up, down in (("transpose", "stride"), ("resize", "stride"), ("resize", "pool")):
        r = step_rate(up, down, a.steps, a.warmup)
        print(json.dumps({"what": "step", "arch": "celeba64", "B": 256, "upsampling": up, "downsampling": down, **r}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
