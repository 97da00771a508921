#!/usr/bin/env python
"""One SWD evaluation, measured on the three paths of metrics.SWDMetric.

The evaluation is the reference's (SWDMetricCallback(num_samples=1000), demo_celeba.py at 64x64): --samples images of --size x --size x 3
per set in --batches minibatches, `update_state` per minibatch plus one `results()`, host clock around work that ends in the
metric's read-back (a device synchronise precedes the start).  Paths, alternating inside every repetition so that they share the
machine's state: `native` (SWDMetric(native=True): the library's kernels), `on_device` (SWDMetric(on_device=True): torch device ops
with host-built index arrays) and `host` (SWDMetric(): numpy).  One warm-up evaluation per path, then --repeats timed ones.

A separate, profiled evaluation of the native path (bg_prof_enable: an event pair per launch, so it is not timed end to end) gives the
per-kernel times from ops.prof_records().  With --c2-images-per-s R the native evaluation is also put against the training it
measures: evaluation time / time of --cadence images at R images/s.

Writes JSON lines to --out (default: a new profiles/swd_eval_<date>_<time>.jsonl; an existing file is never overwritten) and prints them.
Usage: python tools/bench_swd.py [--repeats 5] [--paths native,on_device,host] [--c2-images-per-s 32372]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_sets(samples, size, seed=0):
    """uint8-valued NCHW sets: noisy reals, smooth fakes (another distribution, as an untrained generator's)."""
    rng = np.random.RandomState(seed)
    real = rng.randint(0, 256, size=(samples, 3, size, size)).astype(np.float32)
    ramp = np.linspace(0, 255, size)[None, None, None, :] + np.linspace(0, 255, size)[None, None, :, None]
    fake = np.clip(np.round(ramp / 2 + rng.normal(scale=20, size=real.shape)), 0, 255).astype(np.float32)
    return real, fake


def evaluate(path, batches, seed):
    from blurred_gan_amd import metrics
    m = metrics.SWDMetric(seed=seed, native=path == "native", on_device=path == "on_device")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for real, fake in batches:
        m.update_state(real, fake)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = m.results()                      # ends in the read-back of the distances
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"update_state_s": t1 - t0, "results_s": t2 - t1, "total_s": t2 - t0}, res


def summary(v):
    med = statistics.median(v)
    return {"median_s": round(med, 5), "min_s": round(min(v), 5), "max_s": round(max(v), 5), "spread_s": round(max(v) - min(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", default="native,on_device,host")
    ap.add_argument("--c2-images-per-s", dest="c2_rate", type=float, default=None, help="measured C2 training rate (bench.py) for the share")
    ap.add_argument("--cadence", type=int, default=50_000, help="training images between two evaluations (the reference's 50 000)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", time.strftime("swd_eval_%Y%m%d_%H%M%S.jsonl")))
    a = ap.parse_args()
    if os.path.exists(a.out):
        raise SystemExit(f"{a.out} exists: records are not overwritten, choose another --out")
    if not torch.cuda.is_available():
        raise SystemExit("bench_swd.py measures on the GPU; no device found")
    torch.cuda.set_device(0)
    from blurred_gan_amd import ops
    paths = [p for p in a.paths.split(",") if p]
    assert set(paths) <= {"native", "on_device", "host"} and a.samples % a.batches == 0
    real, fake = make_sets(a.samples, a.size)
    per = a.samples // a.batches
    host_batches = [(real[i * per:(i + 1) * per], fake[i * per:(i + 1) * per]) for i in range(a.batches)]
    dev_batches = [(torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda()) for r, f in host_batches]
    feed = {"native": dev_batches, "on_device": dev_batches, "host": host_batches}
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    times = {p: {"update_state_s": [], "results_s": [], "total_s": []} for p in paths}
    values = {}
    for p in paths:                                            # warm-up: code objects, allocator pools
        _, values[p] = evaluate(p, feed[p], seed=1)
    for rep in range(a.repeats):
        for p in paths:
            t, res = evaluate(p, feed[p], seed=1)
            for k, v in t.items():
                times[p][k].append(v)
            assert res.keys() == values[p].keys()
        print(f"repetition {rep + 1} / {a.repeats} done", file=sys.stderr, flush=True)
    cfg = {"samples": a.samples, "size": a.size, "batches": a.batches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    for p in paths:
        emit({"what": "evaluation", "path": p, **cfg, **{k: summary(v) for k, v in times[p].items()}, "result": values[p]})
    if "native" in paths:
        ref = values.get("host") or values.get("on_device")
        if ref:
            emit({"what": "agreement", "native_vs": "host" if "host" in values else "on_device",
                  "max_abs_diff": max(abs(values["native"][k] - ref[k]) for k in ref)})
        nat = times["native"]["total_s"]
        if "on_device" in paths:
            dv = times["on_device"]["total_s"]
            emit({"what": "native_vs_on_device", "speedup_of_medians": round(statistics.median(dv) / statistics.median(nat), 2),
                  "slowest_native_s": round(max(nat), 5), "fastest_on_device_s": round(min(dv), 5),
                  "faster_beyond_spread": max(nat) < min(dv)})
        if a.c2_rate:
            interval = a.cadence / a.c2_rate
            emit({"what": "share_of_training_interval", "cadence_images": a.cadence, "c2_images_per_s": a.c2_rate,
                  "interval_s": round(interval, 4), "native_evaluation_s": round(statistics.median(nat), 5),
                  "share": round(statistics.median(nat) / interval, 4)})
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            evaluate("native", feed["native"], seed=1)
            recs = ops.prof_records()
        finally:
            ops.prof_enable(False)
            ops.prof_reset()
        agg = {}
        for name, ms, _, nbytes in recs:
            e = agg.setdefault(name, {"launches": 0, "ms": 0.0, "bytes": 0.0})
            e["launches"] += 1
            e["ms"] += ms
            e["bytes"] += nbytes
        total = sum(e["ms"] for e in agg.values())
        kernels = {k: {"launches": e["launches"], "ms": round(e["ms"], 4), "share": round(e["ms"] / total, 4),
                       "algorithmic_GBps": round(e["bytes"] / e["ms"] * 1e-6, 1) if e["bytes"] and e["ms"] else None}
                   for k, e in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])}
        sort_ms = sum(e["ms"] for k, e in agg.items() if k.startswith("sort_rows"))
        emit({"what": "native_kernels", "kernel_ms_total": round(total, 4), "sort_share": round(sort_ms / total, 4), "kernels": kernels})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
