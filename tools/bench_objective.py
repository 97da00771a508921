#!/usr/bin/env python
"""What the objective costs and what lazy regularisation saves: ms per train_on_batch of celeba64 at batch 256 for the default
objective (the reference's: Wasserstein loss, two-sided penalty on interpolates every step -- the launch list of the commit before
``objective=`` existed, which is the baseline of every ratio below) and for the non-saturating loss with R1 at penalty_interval
k = 1, 4 and 16, --repeats times each in turn, same build, same process (median and min..max of the rounds).  A timed stretch is
a whole number of intervals and starts on a penalty step; the warm-up is long enough for both kinds of critic step to have been
recorded and to replay (a key is recorded at its second use, and a model's first step has a key of its own: 3 k + 1 steps).
Then us per launch of the three kernels of the objective beside the launches they stand in for, at the step's shapes.
Timing: wall clock around the synchronised stretch for steps, device events around --iters launches for kernels.  One JSON line
per measurement.
Usage: python tools/bench_objective.py [--steps 48] [--warmup 8] [--repeats 3] [--iters 200] [--no-kernels]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B = 256
INTERVALS = (1, 4, 16)


def _objectives():
    import blurred_gan_amd as bg
    out = {"default": None}
    for k in INTERVALS:
        out[f"nonsaturating_r1_k{k}"] = bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals", penalty_interval=k)
    return out


def step_rate(objective, steps, warmup, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch)
    disc = models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"), objective=objective)
    k = gan.objective.penalty_interval
    warmup = -(-max(warmup, 3 * k + 1) // k) * k             # both step kinds replay, and the timed stretch starts on a penalty step
    steps = -(-steps // k) * k
    H, W, C = models.IMAGE_SHAPE[arch]
    g = torch.Generator(device="cuda").manual_seed(123123)
    reals = torch.rand(B, H, W, C, device="cuda", generator=g) * 2 - 1
    for _ in range(warmup):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    before = dict(gan._programs.stats)
    t0 = time.perf_counter()
    for _ in range(steps):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    during = {n: int(v - before[n]) for n, v in gan._programs.stats.items()}
    return {"images_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup,
            "penalty_steps": steps // k, "programs_during_timing": during}


def _time_us(launch, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        launch()
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_times(iters, repeats):
    """us per launch, launches back to back on one stream (so a small kernel's figure is the launch rate, not its latency)."""
    from blurred_gan_amd import ops
    fs, rs = torch.randn(B, device="cuda"), torch.randn(B, device="cuda")
    norms = torch.rand(B, device="cuda") + 0.5
    dfs, drs, met = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(8, device="cuda")
    g = torch.randn(B, 64 * 64 * 3, device="cuda")
    out = torch.empty_like(g)
    L = ops.objective.LOSS
    cases = {"wgangp_d_loss": lambda: ops.wgangp_d_loss(fs, rs, norms, 1 / B, 10.0, 1e-4, float(B), dfs, drs, met),
             "wgan_g_loss": lambda: ops.wgan_g_loss(fs, 1 / B, dfs, met),
             "gp_seed": lambda: ops.gp_seed(g, norms, 0.7, out)}
    for name, code in L.items():
        cases[f"gan_d_loss[{name}]"] = lambda code=code: ops.objective.d_loss(fs, rs, norms, code, 1 / B, 10.0, 0.0, 1e-4, float(B), dfs, drs, met)
    cases["gan_g_loss[nonsaturating]"] = lambda: ops.objective.g_loss(fs, L["nonsaturating"], 1 / B, dfs, met)
    for t in (0.0, 1.0):
        cases[f"gp_seed_target[t={t:g}]"] = lambda t=t: ops.objective.gp_seed(g, norms, 0.7, t, out)
    rows = []
    for name, launch in cases.items():
        us = [_time_us(launch, iters) for _ in range(repeats)]
        row = {"what": "kernel", "name": name, "B": B, "us_median": round(statistics.median(us), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)]}
        if name.startswith("gp_seed"):
            row["GBps_median"] = round(8 * g.numel() / statistics.median(us) * 1e-3, 1)          # one read and one write of the gradient
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objective.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    objectives = _objectives()
    ms = {name: [] for name in objectives}
    for _ in range(a.repeats):                                  # each in turn: the spread stands beside the differences
        for name, obj in objectives.items():
            r = step_rate(obj, a.steps, a.warmup)
            ms[name].append(r["ms_per_step"])
            print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "objective": name, **r}), flush=True)
            torch.cuda.empty_cache()
    base = statistics.median(ms["default"])
    for name, v in ms.items():
        print(json.dumps({"what": "step_summary", "objective": name, "ms_median": round(statistics.median(v), 3), "ms_min_max": [min(v), max(v)],
                          "over_default": round(statistics.median(v) / base, 4)}), flush=True)
    if not a.no_kernels:
        for row in kernel_times(a.iters, a.repeats):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
