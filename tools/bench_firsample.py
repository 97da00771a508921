#!/usr/bin/env python
"""The FIR-filtered resampling kernels at the workload's shapes: us per launch and GB/s of algorithmic bytes of
bg_fir_upsample2x_nhwc_f32, bg_fir_downsample2x_nhwc_f32 and the fused down-sampling backward (the upsample with ref + keep), each
beside its nearest twin (bg_upsample2x_nhwc_f32 / bg_pool2x_sum_nhwc_f32, which move the same algorithmic bytes) and beside
bg_adam_f32 moving the same total bytes, the three alternating in one process over --repeats rounds (median and min..max of the
rounds).  The shapes are the maps of celeba64's filtered stages: the generator's at batch 256, the critic's at the 768 rows of its
merged D-step pass.  Then images/s of timed train_on_batch calls of celeba64 at batch 256 with the filtered pair and with the
resize + pool pair, alternating.
Timing: device events around --iters launches after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_firsample.py [--kernel 1,3,3,1] [--iters 20] [--repeats 5] [--steps 10] [--warmup 5] [--rounds 3] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def workload_shapes(kernel, arch="celeba64", B=256):
    """[(side, (rows, H, W, C) of the low-resolution map)] of every filtered stage of the arch's pair."""
    from blurred_gan_amd import models
    gen = models.DCGANGenerator(arch=arch, upsampling="filtered", resample_kernel=kernel)
    disc = models.DCGANDiscriminator(arch=arch, downsampling="filtered", resample_kernel=kernel)
    out = [("generator", (B,) + tuple(s)) for l, s in gen.flat_layers() if l.kind == "firup"]
    out += [("critic", (3 * B,) + tuple(l.out_shape(s))) for l, s in disc.flat_layers() if l.kind == "firdown"]
    return out


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


def _stats(nbytes, us):
    rates = [nbytes / u * 1e-3 for u in us]
    return {"us_median": round(statistics.median(us), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)],
            "GBps_median": round(statistics.median(rates), 1)}


def kernel_rates(side, shape, taps, iters, repeats):
    from blurred_gan_amd import ops
    B, H, W, C = shape
    n = B * H * W * C                                           # low-resolution elements; the other side holds 4 n
    lo = torch.rand(shape, device="cuda") - 0.5
    hi = torch.rand(B, 2 * H, 2 * W, C, device="cuda") - 0.5
    ref = torch.rand_like(hi) - 0.5
    keep = (torch.rand_like(hi) >= 0.3).to(torch.uint8)
    out_hi, out_lo = torch.empty_like(hi), torch.empty_like(lo)

    def adam_of(nbytes):                                        # bg_adam_f32 moving nbytes in all: 28 bytes per element
        m = max(int(nbytes) // 28 // 4 * 4, 4)
        th, m1, m2, gr = (torch.rand(m, device="cuda") for _ in range(4))
        return lambda: ops.adam(th, m1, m2, gr, 1e-3)

    fused = dict(ref=ref, keep=keep, alpha=0.3, grad_scale=1 / 0.7)
    cases = {"fir_upsample2x": (20 * n, lambda: ops.fir_upsample2x(lo, out_hi, taps, 4.0), lambda: ops.upsample2x(lo, out_hi, 1.0)),
             "fir_downsample2x": (20 * n, lambda: ops.fir_downsample2x(hi, out_lo, taps, 1.0), lambda: ops.pool2x_sum(hi, out_lo, 0.25)),
             "fir_upsample2x_mul_grad": (40 * n, lambda: ops.fir_upsample2x(lo, out_hi, taps, 1.0, **fused),
                                         lambda: ops.upsample2x(lo, out_hi, 0.25, **fused))}
    rows = []
    for name, (nbytes, fir, twin) in cases.items():
        t = _alternate({"fir": fir, "twin": twin, "adam": adam_of(nbytes)}, iters, repeats)
        f, w, a = (_stats(nbytes, t[k]) for k in ("fir", "twin", "adam"))
        rows.append({"what": name, "side": side, "shape": list(shape), "n_taps": len(taps), "bytes": int(nbytes), **f,
                     "twin_us_median": w["us_median"], "twin_us_min_max": w["us_min_max"], "twin_GBps_median": w["GBps_median"],
                     "fir_over_twin": round(f["us_median"] / w["us_median"], 3), "adam_GBps_median": a["GBps_median"],
                     "vs_adam": round(f["GBps_median"] / a["GBps_median"], 3)})
    return rows


def make_gan(upsampling, downsampling, kernel, arch="celeba64", B=256, sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch, upsampling=upsampling, resample_kernel=kernel)
    disc = models.DCGANDiscriminator(arch=arch, downsampling=downsampling, resample_kernel=kernel)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"))


def step_rates(kernel, steps, warmup, rounds, arch="celeba64", B=256):
    """The two pairs in one process, alternating: ``rounds`` timed windows of ``steps`` calls each."""
    from blurred_gan_amd import models
    pairs = {"filtered": make_gan("filtered", "filtered", kernel), "nearest": make_gan("resize", "pool", kernel)}
    H, W, C = models.IMAGE_SHAPE[arch]
    g = torch.Generator(device="cuda").manual_seed(123123)
    reals = torch.rand(B, H, W, C, device="cuda", generator=g) * 2 - 1
    for gan in pairs.values():
        for _ in range(warmup):
            gan.train_on_batch(reals)
    torch.cuda.synchronize()
    ms = {k: [] for k in pairs}
    for _ in range(rounds):
        for k, gan in pairs.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                gan.train_on_batch(reals)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    return [{"what": "step", "arch": arch, "B": B, "pair": k, "ms_per_step_median": round(statistics.median(v), 3),
             "ms_per_step_min_max": [round(min(v), 3), round(max(v), 3)], "images_per_s_median": round(B / statistics.median(v) * 1e3, 1),
             "steps": steps, "warmup": warmup, "rounds": rounds} for k, v in ms.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="1,3,3,1")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_firsample.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    from blurred_gan_amd import layers
    kernel = tuple(float(v) for v in a.kernel.split(","))
    taps = layers.resample_taps(kernel)
    for side, shape in workload_shapes(kernel):
        for r in kernel_rates(side, shape, taps, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    for r in step_rates(kernel, a.steps, a.warmup, a.rounds):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
