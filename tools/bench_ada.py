#!/usr/bin/env python
"""Adaptive augmentation beside its yardsticks, modelled on tools/bench_diffaug.py.

Kernels, at the D-step's 768 x 64 x 64 x 3 of celeba64 at batch 256: bg_diffaug_gated_f32 / bg_diffaug_gated_adjoint_f32 at p = 1 (the
same work plus three compares per sample) against their ungated twins, the two alternating over --repeats rounds (median and
min..max of the rounds: the twins' own run-to-run spread stands beside the difference); the gated kernels at p = 0.5 and p = 0 for
what a gate that does not fire saves; and the two controller kernels on 256 scores (us per launch: they are latency, not bandwidth).
Steps, celeba64 at batch 256 with loss="nonsaturating": DiffAugment (full policy), AdaptiveAugment(p=0.5, target=None) and
AdaptiveAugment(target=0.6), in alternating rounds, medians of the rounds' ms per step.
Timing: device events around --iters launches after a warm-up; wall clock around --steps train_on_batch calls.  One JSON line each.
Usage: python tools/bench_ada.py [--iters 50] [--repeats 5] [--steps 20] [--warmup 5] [--rounds 3] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_diffaug import _alternate  # noqa: E402

B = 256
SHAPE = (3 * B, 64, 64, 3)
FULL = "color,translation,cutout"


def _stat(us):
    return {"us_median": round(statistics.median(us), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)]}


def kernel_rows(iters, repeats):
    import blurred_gan_amd as bg
    from blurred_gan_amd import ops
    cfg = bg.DiffAugment(FULL)
    n = SHAPE[0]
    x, g = torch.rand(*SHAPE, device="cuda") - 0.5, torch.rand(*SHAPE, device="cuda") - 0.5
    y, dx = torch.empty_like(x), torch.empty_like(x)
    params = torch.rand(n, 12, device="cuda").clamp_(max=1 - 2.0 ** -24)
    p8 = params[:, :8].contiguous()
    p = torch.ones(1, device="cuda")
    twins = {"fwd": (lambda: ops.diffaug.fwd(x, y, p8, **cfg.kernel_args()), lambda: ops.diffaug.fwd_gated(x, y, params, p, **cfg.kernel_args())),
             "adjoint": (lambda: ops.diffaug.adjoint(g, dx, p8, **cfg.kernel_args()),
                         lambda: ops.diffaug.adjoint_gated(g, dx, params, p, **cfg.kernel_args()))}
    rows = []
    for name, (plain, gated) in twins.items():
        for value in (1.0, 0.5, 0.0):
            p.fill_(value)
            t = _alternate({"ungated": plain, "gated": gated}, iters, repeats)
            rows.append({"what": f"diffaug_gated_{name}", "shape": list(SHAPE), "p": value, "gated": _stat(t["gated"]), "ungated_twin": _stat(t["ungated"]),
                         "gated_over_ungated": round(statistics.median(t["gated"]) / statistics.median(t["ungated"]), 4)})
    scores = torch.randn(B, device="cuda")
    stats, state, met = torch.zeros(4, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(2, device="cuda")
    t = _alternate({"ada_stats": lambda: ops.ada.stats(scores, stats), "ada_update": lambda: ops.ada.update(stats, state, met, 0.6, 4, 1.0 / 500_000)},
                   iters, repeats)
    rows += [{"what": k, "n": B, **_stat(v)} for k, v in t.items()]
    return rows


def step_rate(augment, steps, warmup, arch="celeba64", sigma=5.0):
    """bench_diffaug.step_rate under the non-saturating loss; also what p ended at."""
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    gan = bg.BlurredWGANGP(models.DCGANGenerator(arch=arch), models.DCGANDiscriminator(arch=arch), hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"),
                           augment=augment, objective="nonsaturating")
    g = torch.Generator(device="cuda").manual_seed(123123)
    reals = torch.rand(B, *models.IMAGE_SHAPE[arch], device="cuda", generator=g) * 2 - 1
    for _ in range(warmup):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"images_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup,
            "programs": {k: int(v) for k, v in gan._programs.stats.items()}, "augment_p": gan.augment_p}


def step_rows(steps, warmup, rounds):
    import blurred_gan_amd as bg
    cases = {"diffaugment": bg.DiffAugment(FULL), "adaptive_fixed_p_0.5": bg.AdaptiveAugment(FULL, p=0.5, target=None),
             "adaptive_target_0.6": bg.AdaptiveAugment(FULL, target=0.6)}
    ms, rows = {k: [] for k in cases}, []
    for r in range(rounds):
        for name, aug in cases.items():
            out = step_rate(aug, steps, warmup)
            ms[name].append(out["ms_per_step"])
            rows.append({"what": "step", "arch": "celeba64", "B": B, "loss": "nonsaturating", "augment": name, "round": r, **out})
            torch.cuda.empty_cache()
    med = {k: statistics.median(v) for k, v in ms.items()}
    rows.append({"what": "step_medians", "ms_per_step": {k: round(v, 3) for k, v in med.items()},
                 "ms_min_max": {k: [min(v), max(v)] for k, v in ms.items()},
                 "over_diffaugment": {k: round(v / med["diffaugment"], 4) for k, v in med.items()}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ada.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for r in kernel_rows(a.iters, a.repeats):
        print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    if not a.no_step:
        for r in step_rows(a.steps, a.warmup, a.rounds):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
