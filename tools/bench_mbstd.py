#!/usr/bin/env python
"""The minibatch standard deviation kernels at the tops of the stock critics, at the D-step's 768 rows (3 x batch 256), groups of 4:
us per launch and GB/s of algorithmic bytes of bg_mbstd_fwd_f32, bg_mbstd_bwd_f32 and bg_mbstd_gp_f32, each beside bg_adam_f32 --
the project's own streaming yardstick -- moving the same total bytes (reads + writes) in the same process, the two alternating
over --repeats rounds (median and min..max of the rounds).  Then ms per step of timed train_on_batch calls of celeba64 at batch 256
with minibatch_stddev=None and 4, in alternating rounds, and the medians.
Timing: device events around --iters launches after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_mbstd.py [--iters 200] [--repeats 5] [--steps 10] [--warmup 5] [--rounds 3] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B, G = 256, 4
ROWS = 3 * B
# (pixels P, channels C) of the map in front of the critic's Flatten: celeba64 / celeba128 2x2x512, mnist 7x7x128
SHAPES = {"celeba": (4, 512), "mnist": (49, 128)}


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


def kernel_rates(name, iters, repeats, N=ROWS):
    from blurred_gan_amd import ops
    mb = ops.mbstd
    P, C = SHAPES[name]
    n, n1, ng = N * P * C, N * P * (C + 1), (N // G) * P * C
    f = lambda *s: torch.rand(*s, device="cuda") - 0.5
    x, d, u = f(N, P, C), f(N, P, C), f(N, P, C + 1)
    y, vout = torch.empty(N, P, C + 1, device="cuda"), torch.empty(N, P, C + 1, device="cuda")
    dx, src = torch.empty(N, P, C, device="cuda"), torch.empty(N, P, C, device="cuda")
    mu, rs = torch.empty(ng, device="cuda"), torch.empty(ng, device="cuda")
    fg, q, fdot = (torch.empty(N // G, device="cuda") for _ in range(3))
    nb = mb.workspace_bytes(N, G, P, C)
    ws = torch.empty(nb // 4, device="cuda") if nb else None
    mb.fwd(x, y, mu, rs, fg, G, ws=ws)
    mb.bwd(u, x, mu, rs, dx, q, G)

    def adam_of(nbytes):                                        # bg_adam_f32 moving nbytes in all: 28 bytes per element
        m = int(nbytes) // 28 // 4 * 4
        th, m1, m2, gr = (torch.rand(m, device="cuda") for _ in range(4))
        return lambda: ops.adam(th, m1, m2, gr, 1e-3)

    # algorithmic bytes: every tensor once, the groups' statistics (mu, 1 / s) once
    cases = {"mbstd_fwd": (4 * (n + n1 + 2 * ng), lambda: mb.fwd(x, y, mu, rs, fg, G, ws=ws)),
             "mbstd_bwd": (4 * (n1 + 2 * n + 2 * ng), lambda: mb.bwd(u, x, mu, rs, dx, q, G)),
             "mbstd_gp": (4 * (3 * n + n1 + 2 * ng), lambda: mb.gp(d, x, mu, rs, q, vout, src, fdot, G, ws=ws))}
    rows = []
    for what, (nbytes, launch) in cases.items():
        t = _alternate({what: launch, "adam": adam_of(nbytes)}, iters, repeats)
        row, ad = _row(what, (N, P, C), nbytes, t[what]), _row("adam_same_bytes", (N, P, C), nbytes, t["adam"])
        row["top"], row["G"] = name, G
        row["plan"] = mb.plan(N, G, P, C, what.split("_")[1])
        row["vs_adam"] = round(row["GBps_median"] / ad["GBps_median"], 3)
        row["adam_us_median"], row["adam_GBps_median"], row["adam_GBps_min_max"] = ad["us_median"], ad["GBps_median"], ad["GBps_min_max"]
        rows.append(row)
    return rows


def make_gan(minibatch_stddev, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch)
    disc = models.DCGANDiscriminator(arch=arch, minibatch_stddev=minibatch_stddev)
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mbstd.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for name in SHAPES:
        for r in kernel_rates(name, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    from blurred_gan_amd import models
    H, W, C = models.IMAGE_SHAPE["celeba64"]
    reals = torch.rand(B, H, W, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(123123)) * 2 - 1
    gans = {None: make_gan(None), G: make_gan(G)}
    for gan in gans.values():
        for _ in range(a.warmup):
            gan.train_on_batch(reals)
    ms = {k: [] for k in gans}
    for rnd in range(a.rounds):                  # alternating rounds: the spread beside the difference
        for k, gan in gans.items():
            ms[k].append(timed_steps(gan, reals, a.steps))
            print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "minibatch_stddev": k, "round": rnd, "ms_per_step": round(ms[k][-1], 3)}), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"what": "step_medians", "ms_per_step": {str(k): round(v, 3) for k, v in med.items()},
                      "images_per_s": {str(k): round(B / v * 1e3, 1) for k, v in med.items()},
                      "mbstd_over_none_ms": round(med[G] / med[None], 3)}), flush=True)


if __name__ == "__main__":
    main()
