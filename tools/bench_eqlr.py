#!/usr/bin/env python
"""The equalised-learning-rate kernels at the tables of the stock celeba64 generator and critic: us per launch and GB/s of
algorithmic bytes of bg_eqlr_scale_f32 (W in, c * W out, and the transposed copy of every conv kernel out) and bg_eqlr_grad_f32 (the
wrapped gradients in and out), each beside bg_adam_f32 -- the project's own streaming yardstick -- moving the same total bytes
(reads + writes) in the same process, the two alternating over --repeats rounds (median and min..max of the rounds).  Then ms per
step of timed train_on_batch calls of celeba64 at batch 256 with ``equalized_lr`` False and True on both models, in alternating
rounds, and the medians.  Timing: device events around --iters launches after a warm-up.  One JSON line per measurement.
Usage: python tools/bench_eqlr.py [--iters 100] [--repeats 5] [--steps 10] [--warmup 5] [--rounds 3] [--no-step]"""
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


def _row(what, nbytes, us):
    rates = [nbytes / u * 1e-3 for u in us]
    return {"what": what, "bytes": int(nbytes), "us_median": round(statistics.median(us), 2),
            "GBps_median": round(statistics.median(rates), 1), "GBps_min_max": [round(min(rates), 1), round(max(rates), 1)]}


def kernel_rates(which, iters, repeats):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models, ops
    bg.set_seed(123123)
    cls = {"generator": models.DCGANGenerator, "critic": models.DCGANDiscriminator}[which]
    model = cls(arch="celeba64", equalized_lr=True)
    net, st = model.net(), model.store
    st.ensure_opt_state()
    table = st.eqlr_table(net.eqlr_layers)
    elems = sum(int(l.vars["kernel"].numel()) for l in net.eqlr_layers)
    tr = sum(int(l.vars["kernel"].numel()) for l in net.eqlr_layers if l.kind != "dense")
    st.grad.uniform_(-1.0, 1.0)

    def adam_of(nbytes):                                        # bg_adam_f32 moving nbytes in all: 28 bytes per element
        m = max(int(nbytes) // 28 // 4 * 4, 4)
        th, m1, m2, gr = (torch.rand(m, device="cuda") for _ in range(4))
        return lambda: ops.adam(th, m1, m2, gr, 1e-3)

    # repeated in place the gradients shrink by c per launch and end at zero; the bytes moved are the same
    cases = {"eqlr_scale": (8 * elems + 4 * tr, lambda: ops.eqlr.scale(st.theta, st.eff, table)),
             "eqlr_grad": (8 * elems, lambda: ops.eqlr.grad(st.grad, table))}
    out = []
    for what, (nbytes, launch) in cases.items():
        t = _alternate({what: launch, "adam": adam_of(nbytes)}, iters, repeats)
        row, ad = _row(what, nbytes, t[what]), _row("adam_same_bytes", nbytes, t["adam"])
        row["model"], row["layers"], row["parameters"] = which, table.n, elems
        row["vs_adam"] = round(row["GBps_median"] / ad["GBps_median"], 3)
        row["adam_us_median"], row["adam_GBps_median"], row["adam_GBps_min_max"] = ad["us_median"], ad["GBps_median"], ad["GBps_min_max"]
        out.append(row)
    return out


def make_gan(equalized_lr, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch, equalized_lr=equalized_lr)
    disc = models.DCGANDiscriminator(arch=arch, equalized_lr=equalized_lr)
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
        raise SystemExit("bench_eqlr.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for which in ("generator", "critic"):
        for r in kernel_rates(which, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    from blurred_gan_amd import models
    H, W, C = models.IMAGE_SHAPE["celeba64"]
    reals = torch.rand(B, H, W, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(123123)) * 2 - 1
    gans = {k: make_gan(v) for k, v in (("plain", False), ("equalized_lr", True))}
    for gan in gans.values():
        for _ in range(a.warmup):
            gan.train_on_batch(reals)
    ms = {k: [] for k in gans}
    for rnd in range(a.rounds):                  # alternating rounds: the spread beside the difference
        for k, gan in gans.items():
            ms[k].append(timed_steps(gan, reals, a.steps))
            print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "models": k, "round": rnd, "ms_per_step": round(ms[k][-1], 3)}), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"what": "step_medians", "ms_per_step": {k: round(v, 3) for k, v in med.items()},
                      "images_per_s": {k: round(B / v * 1e3, 1) for k, v in med.items()},
                      "equalized_lr_over_plain_ms": round(med["equalized_lr"] / med["plain"], 3)}), flush=True)


if __name__ == "__main__":
    main()
