#!/usr/bin/env python
"""TV denoiser (TVDenoiser prior, dpx_tv_denoise) at 8 x 3 x 1024^2 in 3-D mode and with dims = (2, 3), and at 1 x 31 x 512 x 512 in
3-D mode (that cube's working set, ~230 MB with its dual buffers, sits inside the 256 MiB Infinity Cache: its rate is not an HBM rate);
lam = 0.1, iters 5 and 100.

Prints ONE JSON line: per shape and iteration count the ms per call (hip events around `calls` back-to-back calls, `warmup` calls
excluded; `rounds` windows per setting, the two settings alternating; the median and the min .. max spread are reported) with knob
tv_steps = 0 (the plan's steps per launch on one LDS tile) and = 1 (one step per launch), the plan of each, the bytes each schedule
really moves -- every launch reads y and, behind the first, the k dual fields over its tiles' haloed boxes clipped to the volume, and
writes the k dual fields or, last, x over the cores -- and the fraction of the 6.29 TB/s measured copy rate that is; and, as the
baseline, the same arithmetic as torch ops on the device (fp32: per step the cat / slice / clamp chain of the formula), timed the same way.

    python tools/bench_tv.py [--calls 20] [--warmup 3] [--rounds 3] [--baseline-calls 2] [--no-baseline]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd")]

import torch  # noqa: E402

from dprox import _backend as be  # noqa: E402
from dprox import _ops as ops  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, the chip's measured copy rate
CASES = [((8, 3, 1024, 1024), (1, 2, 3)), ((8, 3, 1024, 1024), (2, 3)), ((1, 31, 512, 512), (1, 2, 3))]


def tv_torch(y, lam, iters, dims):
    """the reference's op chain for any axis set: per axis y - D^T z as cat([-z[:1], z[:-1] - z[1:], z[-1:]]), the mean, clamp(z + D x / 5)"""
    theta = (lam / 2).view(-1, 1, 1, 1)
    z = {d: torch.zeros_like(y.narrow(d, 0, y.shape[d] - 1)) for d in dims}
    for t in range(iters):
        x = None
        for d in dims:
            n = z[d].shape[d]
            dtz = (torch.cat([-z[d].narrow(d, 0, 1), z[d].narrow(d, 0, n - 1) - z[d].narrow(d, 1, n - 1), z[d].narrow(d, n - 1, 1)], d)
                   if n > 0 else torch.zeros_like(y))
            term = y - dtz
            x = term if x is None else x + term
        x = x / len(dims)
        if t + 1 < iters:
            for d in dims:
                n = y.shape[d]
                z[d] = torch.maximum(torch.minimum(z[d] + 0.2 * (x.narrow(d, 1, n - 1) - x.narrow(d, 0, n - 1)), theta), -theta)
    return x


def schedule_bytes(shape, dims, iters):
    """bytes dpx_tv_denoise moves at the current tv_steps: (bytes, plan)"""
    N, D = shape[0], shape[1:]
    p = ops.tv_plan(shape, iters, dims)
    S, L, t, k = p["steps"], p["launches"], p["tile"], len(dims)
    haloed = core = 1
    for a in range(3):
        h = S if (a + 1) in dims and t[a] < D[a] else 0
        haloed *= sum(min(D[a], c + t[a] + h) - max(0, c - h) for c in range(0, D[a], t[a]))
        core *= D[a]
    reads = L * haloed + (L - 1) * k * haloed
    writes = (L - 1) * k * core + core
    return 4 * N * (reads + writes), p


def time_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def tune_set(value):
    be.lib().call("dpx_tune_set", b"tv_steps", int(value))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"metric": "tv_denoise", "lam": 0.1, "device": torch.cuda.get_device_name(dev), "copy_rate_TBps": COPY_RATE / 1e12,
           "timing": f"median of {a.rounds} windows of {a.calls} calls, settings alternating; (min, max) alongside", "cases": {}}
    for shape, dims in CASES:
        g = torch.Generator(device=dev).manual_seed(shape[1])
        v = torch.rand(*shape, device=dev, generator=g)
        lam = torch.full((shape[0],), 0.1, device=dev)
        for iters in (5, 100):
            calls = a.calls if iters == 5 else max(a.calls // 5, 2)
            row, ms = {}, {0: [], 1: []}
            for r in range(a.rounds):
                for steps in (0, 1):
                    tune_set(steps)
                    ms[steps].append(time_ms(lambda: ops.tv_denoise(v, lam, iters, dims), calls, a.warmup if r == 0 else 1))
            outs = {}
            for steps in (0, 1):
                tune_set(steps)
                nbytes, p = schedule_bytes(shape, dims, iters)
                med = statistics.median(ms[steps])
                outs[steps] = ops.tv_denoise(v, lam, iters, dims)
                row[f"tv_steps_{steps}"] = {"ms": round(med, 4), "ms_min_max": [round(min(ms[steps]), 4), round(max(ms[steps]), 4)],
                                            "plan": p, "bytes_per_voxel": round(nbytes / v.numel(), 1),
                                            "copy_rate_fraction": round(nbytes / (med * 1e-3) / COPY_RATE, 3)}
            tune_set(0)
            row["bit_identical"] = bool(torch.equal(outs[0], outs[1]))
            row["blocked_speedup_vs_one_step"] = round(row["tv_steps_1"]["ms"] / row["tv_steps_0"]["ms"], 3)
            if not a.no_baseline:
                with torch.no_grad():
                    base = time_ms(lambda: tv_torch(v, lam, iters, dims), a.baseline_calls if iters == 5 else 1, 1)
                    diff = (tv_torch(v, lam, iters, dims) - outs[0]).abs().max().item()
                row.update(torch_ms=round(base, 3), speedup_vs_torch=round(base / row["tv_steps_0"]["ms"], 1), max_abs_diff_vs_torch=float(f"{diff:.3g}"))
            res["cases"][f"{'x'.join(map(str, shape))} dims {dims} iters {iters}"] = row
            del outs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
