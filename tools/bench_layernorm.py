#!/usr/bin/env python
"""The layer normalisation kernels at the celeba64 critic's five stage shapes, batch 256: us per launch and GB/s of algorithmic
bytes of bg_ln_fwd_f32 (with a Dropout mask), bg_ln_bwd_f32 (with mask and gamma / beta sums; and the generator step's form
without either), bg_ln_tangent_f32 and bg_ln_gp_source_f32, each beside bg_adam_f32 -- the project's own streaming yardstick --
moving the same total bytes (reads + writes) in the same process, the two alternating over --repeats rounds (median and min..max
of the rounds); the two calls that take column sums also split into their launches (bg_prof_* event pairs).  Then images/s of a
few timed train_on_batch calls of celeba64 at batch 256 with normalization=None and "layer", twice each in turn.
Timing: device events around --iters launches after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_layernorm.py [--iters 50] [--repeats 5] [--steps 10] [--warmup 5] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B = 256
# (rows R = B * H * W, channels C) of the celeba64 critic's conv outputs: 64x64x3 -> 32x32x32 -> 16x16x64 -> 8x8x128 -> 4x4x256 -> 2x2x512
SHAPES = [(B * 32 * 32, 32), (B * 16 * 16, 64), (B * 8 * 8, 128), (B * 4 * 4, 256), (B * 2 * 2, 512)]


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
    ln = ops.layernorm
    R, C = shape
    n = R * C
    f = lambda *s: torch.rand(*s, device="cuda") - 0.5
    z, g, zdot, u = f(R, C), f(R, C), f(R, C), f(R, C)
    a, dz, v, s = (torch.empty(R, C, device="cuda") for _ in range(4))
    keep = (torch.rand(R, C, device="cuda") >= 0.3).to(torch.uint8)
    gamma, beta = 1 + 0.2 * torch.rand(C, device="cuda"), 0.1 * f(C)
    mu, r = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    ws = torch.empty(max(ln.workspace_bytes(R, C) // 4, 4), device="cuda")
    ln.fwd(z, a, R, C, gamma, beta, mu, r, keep=keep, scale=1 / 0.7)

    def adam_of(nbytes):                                        # bg_adam_f32 moving nbytes in all: 28 bytes per element
        m = int(nbytes) // 28 // 4 * 4
        th, m1, m2, gr = (torch.rand(m, device="cuda") for _ in range(4))
        return lambda: ops.adam(th, m1, m2, gr, 1e-3)

    # algorithmic bytes: every [R, C] tensor once (4 n; the mask n), the rows' statistics 8 R; the sums' partials are not counted
    cases = {"ln_fwd_keep": (9 * n + 8 * R, lambda: ln.fwd(z, a, R, C, gamma, beta, mu, r, keep=keep, scale=1 / 0.7)),
             "ln_bwd_keep_sums": (13 * n + 8 * R, lambda: ln.bwd(g, z, dz, R, C, gamma, beta, mu, r, keep=keep, scale=1 / 0.7, dgamma=dg,
                                                                dbeta=db, ws=ws)),
             "ln_bwd_no_sums": (12 * n + 8 * R, lambda: ln.bwd(g, z, dz, R, C, gamma, beta, mu, r)),
             "ln_tangent": (12 * n + 8 * R, lambda: ln.tangent(zdot, z, v, R, C, gamma, beta, mu, r)),
             "ln_gp_source": (16 * n + 8 * R, lambda: ln.gp_source(u, zdot, z, s, R, C, gamma, mu, r, dg, ws))}
    rows = []
    for name, (nbytes, launch) in cases.items():
        t = _alternate({name: launch, "adam": adam_of(nbytes)}, iters, repeats)
        row, ad = _row(name, shape, nbytes, t[name]), _row("adam_same_bytes", shape, nbytes, t["adam"])
        row["route"] = ln.route(C)
        row["vs_adam"] = round(row["GBps_median"] / ad["GBps_median"], 3)
        row["adam_us_median"], row["adam_GBps_median"], row["adam_GBps_min_max"] = ad["us_median"], ad["GBps_median"], ad["GBps_min_max"]
        rows.append(row)
    # the two launches of a call that takes column sums, timed apart by the library's own event pairs (bg_prof_*)
    for name in ("ln_bwd_keep_sums", "ln_gp_source"):
        ops.prof_enable(True)
        ops.prof_reset()
        for _ in range(20):
            cases[name][1]()
        torch.cuda.synchronize()
        per = {}
        for rec in ops.prof_records():
            per.setdefault(rec[0], []).append(rec[1] * 1e3)
        ops.prof_enable(False)
        ops.prof_reset()
        rows.append({"what": name + "_split", "shape": list(shape), "us_median_per_launch": {k: round(statistics.median(v), 2) for k, v in per.items()},
                     "partial_bytes": int(ln.workspace_bytes(R, C)), "workgroups": int(ln.workspace_bytes(R, C)) // (8 * C)})
    return rows


def step_rate(normalization, steps, warmup, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch)
    disc = models.DCGANDiscriminator(arch=arch, normalization=normalization)
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
    launches = {k: int(v) for k, v in gan._programs.stats.items()} if hasattr(gan._programs, "stats") else {}
    return {"images_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup,
            "programs": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layernorm.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for shape in SHAPES:
        for r in kernel_rates(shape, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    rates = {}
    for norm in (None, "layer", None, "layer"):                 # twice each, in turn: the spread beside the difference
        r = step_rate(norm, a.steps, a.warmup)
        rates.setdefault(norm, []).append(r["images_per_s"])
        print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "normalization": norm, **r}), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps({"what": "step_ratio", "layer_over_none_images_per_s": round(statistics.mean(rates["layer"]) / statistics.mean(rates[None]), 3),
                      "none": rates[None], "layer": rates["layer"]}), flush=True)


if __name__ == "__main__":
    main()
