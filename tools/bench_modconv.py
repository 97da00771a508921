#!/usr/bin/env python
"""The StyleModulation kernels at the five demodulated layers of the celeba64 generator (normalization="style") at batch 256: us per
launch and GB/s of algorithmic bytes of bg_mod_scale_f32 (y = d * z + bias -> LeakyReLU on the layer's output map), bg_mod_dot_f32
(dd on the same map), bg_mod_wsq_f32, bg_mod_demod_f32, bg_mod_demod_bwd_f32 and bg_mod_wsq_grad_f32, each beside bg_adam_f32 -- the
project's own streaming yardstick -- moving the same total bytes in the same process, the two alternating over --repeats rounds
(tools/bench_noise.py's harness).  Then ms per step of timed train_on_batch calls of celeba64 at batch 256 with
normalization="pixel" and "style" (both noise=True), in alternating rounds, medians with the spread, and under bg_prof the share of
the step each new kernel takes.
Usage: python tools/bench_modconv.py [--iters 100] [--repeats 5] [--steps 10] [--warmup 5] [--rounds 3] [--no-step]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_noise import B, _beside_adam, timed_steps  # noqa: E402

TAPS = 25
# (pixels in, channels in, pixels out, channels out, transposed kernel) of the celeba64 generator's demodulated layers
LAYERS = {"4x4x512": (16, 512, 16, 512, True), "8x8x256": (16, 512, 64, 256, True), "16x16x128": (64, 256, 256, 128, True),
          "32x32x64": (256, 128, 1024, 64, True), "64x64x32": (1024, 64, 4096, 32, True)}


def kernel_rates(name, iters, repeats):
    from blurred_gan_amd import ops
    Pi, I, Po, O, tr = LAYERS[name]
    r = lambda *s: torch.rand(*s, device="cuda") - 0.5
    z, dy, y = r(B, Po, O), r(B, Po, O), torch.empty(B, Po, O, device="cuda")
    d, s, bias = r(B, O) + 1.0, r(B, I) + 1.0, r(O)
    w, dw, Q, dQ = r(TAPS, O, I), torch.zeros(TAPS, O, I, device="cuda"), torch.empty(I, O, device="cuda"), r(I, O) * 1e-3
    dd, dq, ds = torch.empty(B, O, device="cuda"), torch.empty(B, O, device="cuda"), torch.zeros(B, I, device="cuda")
    nb = ops.modconv.dot_workspace_bytes(B, Po, O)
    ws = torch.empty(nb // 4 + 4, device="cuda") if nb else None
    ops.modconv.wsq(w, Q, TAPS, I, O, transposed=tr)
    n = B * Po * O
    cases = {
        "mod_scale": (4 * (2 * n + B * O + O), lambda: ops.modconv.scale(z, d, y, B, Po, O, bias=bias, lrelu_alpha=0.3)),
        "mod_dot": (4 * (2 * n + B * O), lambda: ops.modconv.dot(dy, z, dd, B, Po, O, ws)),
        "mod_wsq": (4 * (TAPS + 1) * I * O, lambda: ops.modconv.wsq(w, Q, TAPS, I, O, transposed=tr)),
        "mod_demod": (4 * (B * I + I * O + B * O), lambda: ops.modconv.demod(s, Q, d, B, I, O)),
        "mod_demod_bwd": (4 * (3 * B * O + I * O + 3 * B * I), lambda: ops.modconv.demod_bwd(d, dd, s, Q, dq, ds, B, I, O)),
        "mod_wsq_grad": (4 * (3 * TAPS + 1) * I * O, lambda: ops.modconv.wsq_grad(w, dQ, dw, TAPS, I, O, transposed=tr, scale=1e-3)),
    }
    return _beside_adam(ops, cases, (B, Po, O, I), iters, repeats, layer=name, dot_plan=ops.modconv.dot_plan(B, Po, O))


def make_gan(normalization, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch, normalization=normalization, noise=True)
    disc = models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"))


def kernel_shares(gan, reals, steps):
    """ms per step by launch name under the library's profiling hooks, for the names the new kernels carry."""
    from blurred_gan_amd import ops
    ops.prof_enable(True)
    ops.prof_reset()
    for _ in range(steps):
        gan.train_on_batch(reals)
    torch.cuda.synchronize()
    tot, per = 0.0, {}
    for name, ms, _, _ in ops.prof_records():
        tot += ms
        if name.startswith("mod_"):
            per[name] = per.get(name, 0.0) + ms
    ops.prof_enable(False)
    return {"what": "step_shares", "generator": "style", "kernel_ms_per_step": round(tot / steps, 3),
            "ms_per_step": {k: round(v / steps, 4) for k, v in sorted(per.items())},
            "share": {k: round(v / tot, 4) for k, v in sorted(per.items())}}


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
        raise SystemExit("bench_modconv.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for name in LAYERS:
        for r in kernel_rates(name, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.no_step:
        return
    from blurred_gan_amd import models
    H, W, C = models.IMAGE_SHAPE["celeba64"]
    reals = torch.rand(B, H, W, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(123123)) * 2 - 1
    gans = {k: make_gan(k) for k in ("pixel", "style")}
    for gan in gans.values():
        for _ in range(a.warmup):
            gan.train_on_batch(reals)
    ms = {k: [] for k in gans}
    for rnd in range(a.rounds):                  # alternating rounds: the spread beside the difference
        for k, gan in gans.items():
            ms[k].append(timed_steps(gan, reals, a.steps))
            print(json.dumps({"what": "step", "arch": "celeba64", "B": B, "generator": k, "round": rnd, "ms_per_step": round(ms[k][-1], 3)}), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"what": "step_medians", "ms_per_step": {k: round(v, 3) for k, v in med.items()},
                      "images_per_s": {k: round(B / v * 1e3, 1) for k, v in med.items()},
                      "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                      "style_over_pixel_ms": round(med["style"] / med["pixel"], 3)}), flush=True)
    print(json.dumps(kernel_shares(gans["style"], reals, a.steps)), flush=True)


if __name__ == "__main__":
    main()
