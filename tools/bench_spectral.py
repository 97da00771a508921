#!/usr/bin/env python
"""The spectral normalisation entry points over all wrapped matrices of the celeba64 critic and of the celeba64 generator (one
batched call each, as the step makes it): us per call and GB/s of algorithmic bytes of bg_spectral_power_f32 (a round, and the
sigma-only form), bg_spectral_scale_f32 and bg_spectral_grad_f32, each beside bg_adam_f32 -- the project's streaming yardstick --
moving the same total bytes in the same process, the two alternating over --repeats rounds (median and min..max of the rounds); the
two-launch calls also split into their launches (bg_prof_* event pairs).  Then images/s of a few timed train_on_batch calls of
celeba64 at batch 256: plain, spectral_norm on the critic, and on both models, twice each in turn.
Timing: device events around --iters calls after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_spectral.py [--iters 50] [--repeats 5] [--steps 10] [--warmup 5] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B = 256


def _time_us(launch, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _alternate(launches, iters, repeats):
    for f in launches.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in launches}
    for _ in range(repeats):
        for k, f in launches.items():
            out[k].append(_time_us(f, iters))
    return out


def _row(what, model, nbytes, us):
    rates = [nbytes / u * 1e-3 for u in us]
    return {"what": what, "model": model, "bytes": int(nbytes), "us_median": round(statistics.median(us), 2),
            "GBps_median": round(statistics.median(rates), 1), "GBps_min_max": [round(min(rates), 1), round(max(rates), 1)]}


def kernel_rates(which, iters, repeats):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models, ops
    bg.set_seed(1)
    model = (models.DCGANDiscriminator if which == "critic" else models.DCGANGenerator)(arch="celeba64", spectral_norm=True)
    net = model.net()
    st = model.store
    st.ensure_opt_state()
    table = st.spectral_table(net.spectral_layers)
    st.grad.copy_(torch.rand_like(st.grad) - 0.5)
    sp = ops.spectral
    shapes = [[int(r[6]), int(r[7])] for r in table.host]
    elems = sum(k * n for k, n in shapes)
    tr = sum(k * n for (k, n), r in zip(shapes, table.host) if r[5] >= 0)
    sp.power(st.theta, st.state, table)
    sp.scale(st.theta, st.state, st.eff, table)

    def adam_of(nbytes):                                        # bg_adam_f32 moving nbytes in all: 28 bytes per element
        m = int(nbytes) // 28 // 4 * 4
        th, m1, m2, gr = (torch.rand(m, device="cuda") for _ in range(4))
        return lambda: ops.adam(th, m1, m2, gr, 1e-3)

    # algorithmic bytes: W once for a round or for sigma; W in, W-bar (and the transposed copy) out for the scale; g and W-bar for
    # the dot, g in and out for the apply.  The partials and the vectors are not counted
    cases = {"power_round": (4 * elems, lambda: sp.power(st.theta, st.state, table)),
             "power_sigma_only": (4 * elems, lambda: sp.power(st.theta, st.state, table, sigma_only=True)),
             "scale": (8 * elems + 4 * tr, lambda: sp.scale(st.theta, st.state, st.eff, table)),
             "grad": (16 * elems, lambda: sp.grad(st.grad, st.eff, st.state, table))}
    rows = []
    for name, (nbytes, launch) in cases.items():
        t = _alternate({name: launch, "adam": adam_of(nbytes)}, iters, repeats)
        row, ad = _row(name, which, nbytes, t[name]), _row("adam_same_bytes", which, nbytes, t["adam"])
        row["vs_adam"] = round(row["GBps_median"] / ad["GBps_median"], 3)
        row["adam_us_median"], row["adam_GBps_median"], row["adam_GBps_min_max"] = ad["us_median"], ad["GBps_median"], ad["GBps_min_max"]
        row["matrices"] = shapes
        rows.append(row)
    for name in ("power_round", "grad"):
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
        rows.append({"what": name + "_split", "model": which, "us_median_per_launch": {k: round(statistics.median(v), 2) for k, v in per.items()},
                     "workspace_bytes": int(table.ws_bytes)})
    return rows


def step_rate(critic_sn, generator_sn, steps, warmup, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch, spectral_norm=generator_sn)
    disc = models.DCGANDiscriminator(arch=arch, spectral_norm=critic_sn)
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
    return {"images_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup,
            "programs": {k: int(v) for k, v in gan._programs.stats.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectral.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for which in ("critic", "generator"):
        for r in kernel_rates(which, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    rates = {}
    configs = {"plain": (False, False), "critic": (True, False), "both": (True, True)}
    for name in list(configs) * 2:                              # twice each, in turn: the spread beside the difference
        r = step_rate(*configs[name], a.steps, a.warmup)
        rates.setdefault(name, []).append(r["images_per_s"])
        print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "spectral_norm": name, **r}), flush=True)
        torch.cuda.empty_cache()
    mean = {k: statistics.mean(v) for k, v in rates.items()}
    print(json.dumps({"what": "step_ratio", "critic_over_plain": round(mean["critic"] / mean["plain"], 3),
                      "both_over_plain": round(mean["both"] / mean["plain"], 3), **rates}), flush=True)


if __name__ == "__main__":
    main()
