#!/usr/bin/env python
"""The input launch of a device-resident dataset, measured.

Kernel cases (one JSON line each): bg_u8_gather_normalize_resize_f32 (gather + normalise + resize from a dataset of --images uint8
images, a different random index vector every launch) against the dense bg_u8_normalize_resize_f32 on already gathered batches of
the same shape (as many distinct batches as index vectors, so neither side re-reads a cache-resident input), timed in the same run
in alternating windows of --iters launches between device events: us per launch (median / min / max over --rounds windows), GB/s of
the algorithmic bytes B*Hs*Ws*C + 4*B*Hd*Wd*C, and new / dense with each side's own spread.
  C4: B 128, 218x178x3 -> 128x128    C2: B 256, 218x178x3 -> 64x64    C1: B 64, 28x28x1 identity

End to end at C2 (celeba64, B 256, default constructor): images/s of train_on_batch fed by (a) a DeviceDataset over --images
synthetic uint8 218x178x3 images, (b) one fixed device batch (what bench.py times), (c) the demos' host path (fancy-index gather on a
float32 memmap + torch.from_numpy + the step's own upload), the three alternating --repeats times on ONE model.
Usage: python tools/bench_input.py [--iters 400] [--rounds 7] [--steps 60] [--warmup 10] [--repeats 5] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = [("C4", 128, (218, 178, 3), (128, 128)), ("C2", 256, (218, 178, 3), (64, 64)), ("C1", 64, (28, 28, 1), (28, 28))]
N_SETS = 16          # distinct index vectors / pre-gathered batches a window cycles through


def _window_us(launch, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        launch(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _summary(us, nbytes):
    med = statistics.median(us)
    return {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "spread": round((max(us) - min(us)) / med, 4),
            "GBps": round(nbytes / med * 1e-3, 1)}


def kernel_case(tag, B, src_shape, dst_hw, n_images, iters, rounds):
    from blurred_gan_amd import ops
    Hs, Ws, C = src_shape
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(0, 256, (n_images, Hs, Ws, C), dtype=torch.uint8, device="cuda", generator=g)
    idx = [torch.randint(0, n_images, (B,), dtype=torch.int32, device="cuda", generator=g) for _ in range(N_SETS)]
    dense = [data[i.long()].contiguous() for i in idx]
    flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.empty(B, *dst_hw, C, device="cuda")
    nbytes = B * Hs * Ws * C + 4 * dst.numel()
    sides = {"gather": lambda i: ops.u8_gather_normalize_resize(data, idx[i % N_SETS], dst),
             "gather_flip": lambda i: ops.u8_gather_normalize_resize(data, idx[i % N_SETS], dst, flip),
             "dense": lambda i: ops.u8_normalize_resize(dense[i % N_SETS], dst)}
    us = {k: [] for k in sides}
    for f in sides.values():                                   # warm-up: code objects, every input touched once
        _window_us(f, 2 * N_SETS)
    for _ in range(rounds):
        for k, f in sides.items():
            us[k].append(_window_us(f, iters))
    out = {k: _summary(v, nbytes) for k, v in us.items()}
    return {"what": "kernel", "case": tag, "B": B, "src": list(src_shape), "dst": list(dst_hw), "dataset_images": n_images,
            "algorithmic_bytes": nbytes, "iters": iters, "rounds": rounds, **out,
            "gather_vs_dense": round(out["gather"]["us"] / out["dense"]["us"], 4)}


def end_to_end(n_images, steps, warmup, repeats, arch="celeba64", B=256, sigma=5.0):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models, callbacks
    from blurred_gan_amd.models import IMAGE_SHAPE
    bg.set_seed(123123)
    gen, disc = models.DCGANGenerator(arch=arch), models.DCGANDiscriminator(arch=arch)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=sigma, batch_size=B, global_batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir=os.path.join(tempfile.gettempdir(), "bg_bench_logs")))
    H, W, C = IMAGE_SHAPE[arch]
    g = torch.Generator(device="cuda").manual_seed(2)
    ds = bg.DeviceDataset(torch.randint(0, 256, (n_images, 218, 178, 3), dtype=torch.uint8, device="cuda", generator=g), image_size=(H, W),
                          batch_size=B, drop_remainder=True)
    fixed = torch.rand(B, H, W, C, device="cuda", generator=g) * 2 - 1
    tmp = tempfile.NamedTemporaryFile(suffix=".npy", delete=False)
    tmp.close()
    np.save(tmp.name, np.random.default_rng(3).uniform(-1, 1, size=(n_images, H, W, C)).astype(np.float32))
    host = np.load(tmp.name, mmap_mode="r")
    rng = np.random.default_rng(4)

    def feed_dataset():
        while True:
            yield from ds

    def feed_fixed():
        while True:
            yield fixed

    def feed_host():                                           # demo_celeba.make_dataset's per-batch work
        while True:
            perm = rng.permutation(n_images)
            for i in range(n_images // B):
                yield torch.from_numpy(np.ascontiguousarray(host[np.sort(perm[i * B:(i + 1) * B])]))

    feeds = {"device_dataset": feed_dataset(), "fixed_device_batch": feed_fixed(), "host_memmap_gather": feed_host()}
    ctl = callbacks.BlurDecayController(total_n_training_examples=202599 * 10, max_value=sigma)
    ctl.set_model(gan)

    def run(feed, n):
        for _ in range(n):
            ctl.on_batch_begin(0, {})
            gan.train_on_batch(next(feed))
        torch.cuda.synchronize()

    rates = {k: [] for k in feeds}
    try:
        for k, f in feeds.items():
            run(f, warmup)
        for _ in range(repeats):
            for k, f in feeds.items():
                run(f, 3)
                t0 = time.perf_counter()
                run(f, steps)
                rates[k].append(B * steps / (time.perf_counter() - t0))
    finally:
        os.unlink(tmp.name)
    med = {k: statistics.median(v) for k, v in rates.items()}
    return {"what": "end_to_end", "config": "C2", "arch": arch, "B": B, "dataset_images": n_images, "steps": steps, "repeats": repeats,
            "images_per_s": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1),
                                 "spread": round((max(v) - min(v)) / med[k], 4)} for k, v in rates.items()},
            "dataset_vs_fixed": round(med["device_dataset"] / med["fixed_device_batch"], 4),
            "host_vs_fixed": round(med["host_memmap_gather"] / med["fixed_device_batch"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for tag, B, src_shape, dst_hw in CASES:
        print(json.dumps(kernel_case(tag, B, src_shape, dst_hw, a.images, a.iters, a.rounds)), flush=True)
        torch.cuda.empty_cache()
    if not a.no_step:
        print(json.dumps(end_to_end(a.images, a.steps, a.warmup, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
