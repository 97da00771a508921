#!/usr/bin/env python
"""The mapping-network kernels at the workload's shapes, batch 256: us per call of bg_dense_lrelu_f32 at (M, N, K) = (256, 512, 512) and
(256, 100, 100) beside the two launches that computed the same thing before it existed -- bg_gemm_f32 with bias, then the in-place
LeakyReLU launch (bg_mod_scale_f32 with v = 1) on the same buffers -- and of bg_lrelu_bias_bwd_f32 at (256, 512) and (256, 100) beside
bg_mul_grad_f32 + bg_colsum_f32, the candidates alternating over --repeats rounds (tools/bench_noise.py's harness), medians with the
spread, and the workgroups of the fused kernel.  Then ms per step of timed train_on_batch calls of celeba64 at batch 256 with
normalization="style", noise=True and mapping_layers = 0, 8 (units 100) and 8 (units 512), in alternating rounds.
Usage: python tools/bench_mapping.py [--iters 200] [--repeats 7] [--steps 10] [--warmup 5] [--rounds 3] [--no-step]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_noise import B, _alternate, timed_steps  # noqa: E402

SHAPES = [(B, 512, 512), (B, 100, 100)]


def _row(what, shape, t, **extra):
    r = {"what": what, "shape": list(shape), "us_median": round(statistics.median(t), 3), "us_min_max": [round(min(t), 3), round(max(t), 3)]}
    r.update(extra)
    return r


def kernel_rates(shape, iters, repeats):
    from blurred_gan_amd import ops
    M, N, K = shape
    r = lambda *s: torch.rand(*s, device="cuda") - 0.5
    x, W, bias, y = r(M, K), r(K, N), r(N), torch.empty(M, N, device="cuda")
    ones = torch.ones(1, N, device="cuda")
    c, m, alpha = 0.0625, 0.01, 0.2

    def pair():         # what the parent computes the layer with: Dense with bias, then LeakyReLU in place on the same buffer
        ops.gemm(x, W, y, M, N, K, bias=bias, scale=c)
        ops.modconv.scale(y, ones, y, 1, M, N, lrelu_alpha=alpha)

    t = _alternate({"fused": lambda: ops.mapping.dense_lrelu(x, W, bias, y, M, N, K, c=c, bias_mul=m, alpha=alpha), "pair": pair}, iters, repeats)
    fwd = _row("dense_lrelu", shape, t["fused"], plan=ops.mapping.plan(M, N, K), pair_us_median=round(statistics.median(t["pair"]), 3),
               pair_us_min_max=[round(min(t["pair"]), 3), round(max(t["pair"]), 3)])
    fwd["fused_over_pair"] = round(fwd["us_median"] / fwd["pair_us_median"], 3)
    g, gp, db = r(M, N), torch.empty(M, N, device="cuda"), torch.zeros(N, device="cuda")
    ws = torch.empty(ops.mapping.workspace_bytes(M, N) // 4 + 4, device="cuda")
    cws = torch.empty(ops.colsum_workspace_bytes(M, N) // 4 + 4, device="cuda")

    def pair_bwd():
        ops.mul_grad(g, y, gp, alpha=alpha)
        ops.colsum(gp, db, M, N, cws, scale=m)

    t = _alternate({"fused": lambda: ops.mapping.lrelu_bias_bwd(g, y, gp, db, M, N, ws, alpha=alpha, scale=m), "pair": pair_bwd}, iters, repeats)
    bwd = _row("lrelu_bias_bwd", (M, N), t["fused"], pair_us_median=round(statistics.median(t["pair"]), 3),
               pair_us_min_max=[round(min(t["pair"]), 3), round(max(t["pair"]), 3)])
    bwd["fused_over_pair"] = round(bwd["us_median"] / bwd["pair_us_median"], 3)
    return [fwd, bwd]


def make_gan(mapping_layers, units, arch="celeba64", sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    bg.set_seed(123123)
    gen = models.DCGANGenerator(arch=arch, normalization="style", noise=True, equalized_lr=True, mapping_layers=mapping_layers, mapping_units=units)
    disc = models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_bench_logs"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mapping.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for shape in SHAPES:
        for r in kernel_rates(shape, a.iters, a.repeats):
            print(json.dumps(r), flush=True)
    if a.no_step:
        return
    from blurred_gan_amd import models
    H, W, C = models.IMAGE_SHAPE["celeba64"]
    reals = torch.rand(B, H, W, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(123123)) * 2 - 1
    gans = {"mapping_0": make_gan(0, None), "mapping_8x100": make_gan(8, None), "mapping_8x512": make_gan(8, 512)}
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
                      "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                      "cost_ms": {k: round(med[k] - med["mapping_0"], 3) for k in med if k != "mapping_0"}}), flush=True)


if __name__ == "__main__":
    main()
