#!/usr/bin/env python
"""The TV denoiser's gradient (dpx_tv_denoise_rec + dpx_tv_backward) at 8 x 3 x 1024^2 with dims = (2, 3) and in 3-D mode, and at
1 x 31 x 512 x 512 in 3-D mode (that cube's working set sits inside the 256 MiB Infinity Cache: its rate is not an HBM rate); lam = 0.1,
iters 5 (TVDenoiser's default) and 13 (a chain of launches everywhere).

Writes ONE JSON document (--out, default profiles/tv_bwd_bench.json) and prints it: per shape and iteration count the ms per call (hip
events around `calls` back-to-back calls, `warmup` calls excluded; `rounds` windows, the three kernels alternating; the median and the
min .. max spread) of the plain forward, the recording forward and the backward (gradient of lam included), the two ratios against the
plain forward, the plan, the bytes each really moves -- the recording forward: the plain forward's (tools/bench_tv.py:schedule_bytes)
plus one state byte per voxel and step; the backward: every launch reads p and, behind the first, gy and the k fields q over its tiles'
haloed boxes clipped to the volume, one state byte per cell of every step's shrinking box, and writes gy and, unless last, p and the k
fields q over the cores -- and the fraction of the 6.29 TB/s measured copy rate that is; and, as the baseline, forward + backward of
the same arithmetic as torch ops on the device under torch autograd (fp32), timed the same way.

    python tools/bench_tv_bwd.py [--calls 20] [--warmup 3] [--rounds 3] [--baseline-calls 2] [--no-baseline] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from dprox import _ops as ops  # noqa: E402
from bench_tv import CASES, COPY_RATE, schedule_bytes, time_ms, tv_torch  # noqa: E402


def backward_bytes(shape, dims, iters):
    """bytes dpx_tv_backward moves: (bytes, plan)"""
    N, D = shape[0], shape[1:]
    p = ops.tv_bwd_plan(shape, iters, dims)
    S, L, t, k = p["steps"], p["launches"], p["tile"], len(dims)
    tiled = [(a + 1) in dims and t[a] < D[a] for a in range(3)]

    def cells(shrink_lo, shrink_hi):
        n = 1
        for a in range(3):
            h = S if tiled[a] else 0
            lo, hi = (shrink_lo, shrink_hi) if tiled[a] else (0, 0)
            n *= sum(max(0, min(D[a], c + t[a] + h - hi) - max(0, c - h + lo)) for c in range(0, D[a], t[a]))
        return n

    haloed, core = cells(0, 0), D[0] * D[1] * D[2]
    floats = codes = 0
    for l in range(L):
        steps = min((l + 1) * S, iters) - l * S
        first, last = l == L - 1, l == 0
        floats += haloed + (0 if first else (1 + k) * haloed) + core + (0 if last else (1 + k) * core)
        codes += sum(cells(s - 1, s) for s in range(1, steps + 1) if min((l + 1) * S, iters) - s + 1 > 1)
    return N * (4 * floats + codes), p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv_bwd_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"metric": "tv_denoise forward + backward", "lam": 0.1, "device": torch.cuda.get_device_name(dev), "copy_rate_TBps": COPY_RATE / 1e12,
           "timing": f"median of {a.rounds} windows of {a.calls} calls, kernels alternating; (min, max) alongside", "cases": {}}
    for shape, dims in [CASES[1], CASES[0], CASES[2]]:
        gen = torch.Generator(device=dev).manual_seed(shape[1])
        v = torch.rand(*shape, device=dev, generator=gen)
        g = torch.randn(*shape, device=dev, generator=gen)
        lam = torch.full((shape[0],), 0.1, device=dev)
        mask = ops._tv_axes_mask(dims)
        for iters in (5, 13):
            out, codes = ops.tv_denoise_rec(v, lam, iters, mask)
            fns = {"forward": lambda: ops.tv_denoise(v, lam, iters, dims), "recording_forward": lambda: ops.tv_denoise_rec(v, lam, iters, mask),
                   "backward": lambda: ops.tv_backward(g, codes, iters, mask)}
            ms = {name: [] for name in fns}
            for r in range(a.rounds):
                for name, fn in fns.items():
                    ms[name].append(time_ms(fn, a.calls, a.warmup if r == 0 else 1))
            fwd_bytes, plan = schedule_bytes(shape, dims, iters)
            bwd_bytes, bplan = backward_bytes(shape, dims, iters)
            nbytes = {"forward": fwd_bytes, "recording_forward": fwd_bytes + (iters - 1) * v.numel(), "backward": bwd_bytes}
            row = {"plan": bplan, "state_bytes_per_voxel": iters - 1}
            for name in fns:
                med = statistics.median(ms[name])
                row[name] = {"ms": round(med, 4), "ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                             "bytes_per_voxel": round(nbytes[name] / v.numel(), 1), "copy_rate_fraction": round(nbytes[name] / (med * 1e-3) / COPY_RATE, 3)}
            row["recording_forward_vs_forward"] = round(row["recording_forward"]["ms"] / row["forward"]["ms"], 3)
            row["backward_vs_forward"] = round(row["backward"]["ms"] / row["forward"]["ms"], 3)
            row["recording_forward_bit_identical"] = bool(torch.equal(out, ops.tv_denoise(v, lam, iters, dims)))
            gy, glam = ops.tv_backward(g, codes, iters, mask)
            if not a.no_baseline:
                def torch_step():
                    vt, lt = v.clone().requires_grad_(True), lam.clone().requires_grad_(True)
                    tv_torch(vt, lt, iters, dims).backward(g)
                    return vt.grad, lt.grad
                base = time_ms(torch_step, a.baseline_calls if iters == 5 else 1, 1)
                tgy, tgl = torch_step()
                ours = row["recording_forward"]["ms"] + row["backward"]["ms"]
                row.update(torch_autograd_ms=round(base, 3), speedup_vs_torch_autograd=round(base / ours, 1),
                           gy_rel_l2_vs_torch=float(f"{((gy - tgy).norm() / tgy.norm()).item():.3g}"),
                           glam_max_rel_diff_vs_torch=float(f"{((glam - tgl).abs() / tgl.abs()).max().item():.3g}"))
                del tgy, tgl
            res["cases"][f"{'x'.join(map(str, shape))} dims {dims} iters {iters}"] = row
            del out, codes, gy
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
