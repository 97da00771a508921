#!/usr/bin/env python
"""Whole-step throughput in both conv math modes: BlurredWGANGP.train_on_batch at C2 (celeba64, B 256, sigma 5) and C4
(celeba128, B 128, sigma 5), built and driven as bench.py builds and drives its flagship run (same seed, same blur-decay
callback, warm-up steps, then a timed region of back-to-back steps with per-step HIP events).  One JSON line per (config, mode).
Usage: python tools/bench_step_math.py [--steps 50] [--warmup 10] [--configs C2,C4]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

CONFIGS = {"C2": ("celeba64", 256), "C4": ("celeba128", 128)}


def measure(arch, B, math, steps, warmup, sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models, callbacks
    from blurred_gan_amd.models import IMAGE_SHAPE
    bg.set_seed(123123)
    gen, disc = models.DCGANGenerator(arch=arch), models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"), conv_math=math)
    gan._rng_seed = 123123
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
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(steps):
        step()
        marks[i + 1].record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    return {"config": None, "arch": arch, "batch": B, "conv_math": math, "images_per_s": round(B * steps / dt, 1),
            "ms_per_step": round(dt / steps * 1e3, 4), "p50_ms": round(per[steps // 2], 4), "p90_ms": round(per[(9 * steps) // 10], 4),
            "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--configs", default="C2,C4")
    a = ap.parse_args()
    for name in a.configs.split(","):
        arch, B = CONFIGS[name]
        base = None
        for math in ("fp32", "bf16x6"):
            r = measure(arch, B, math, a.steps, a.warmup)
            r["config"] = name
            if base is None:
                base = r["images_per_s"]
            else:
                r["vs_fp32"] = round(r["images_per_s"] / base, 4)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
