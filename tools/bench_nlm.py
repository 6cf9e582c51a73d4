#!/usr/bin/env python
"""Non-local means (patch_nlm prior, dpx_nlm) at 8 x 3 x 1024^2 and 1 x 3 x 1024^2, the reference's windows (11, 5), sigma = 0.05.

Prints ONE JSON line: per shape the kernel's ms per call (hip events around `iters` back-to-back calls, `warmup` calls excluded),
pixel-shifts per second (B H W x 121), and the fraction of the VALU-issue model reached:

    model: 60 SIMD cycles per 64 pixel-shifts (~11 VALU at 4 cycles + v_sqrt_f32, v_exp_f32 at 8) on 256 CUs x 4 SIMDs at 2.4 GHz

and, as the baseline, the same math as torch ops on the device (fp32, the roll loop of the formula: per shift one roll of the
luminance, d^2, a 25-roll box sum, sqrt / exp, three rolled colour planes accumulated), timed the same way.

    python tools/bench_nlm.py [--iters 20] [--warmup 3] [--baseline-iters 2] [--no-baseline]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd")]

import torch  # noqa: E402

from dprox import _ops as ops  # noqa: E402

MODEL_CYC_PER_64 = 60.0
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9


def nlm_torch(v, sigma, search=11, patch=5):
    y = 0.299 * v[:, :1] + 0.587 * v[:, 1:2] + 0.114 * v[:, 2:]
    rs, rp = search // 2, patch // 2
    h = (torch.relu(2 * sigma) + 1e-6).view(-1, 1, 1, 1)
    num, den = torch.zeros_like(v), torch.zeros_like(y)
    for dx in range(-rs, rs + 1):
        for dy in range(-rs, rs + 1):
            d2 = (y - torch.roll(y, (dy, dx), (2, 3))) ** 2
            D = torch.zeros_like(d2)
            for oy in range(-rp, rp + 1):
                for ox in range(-rp, rp + 1):
                    D += torch.roll(d2, (oy, ox), (2, 3))
            w = torch.exp(-torch.sqrt(D) / h)
            num += w * torch.roll(v, (dy, dx), (2, 3))
            den += w
    return torch.clamp(num / den, 0, 1)


def time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-iters", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"metric": "nlm", "windows": [11, 5], "sigma": 0.05, "device": torch.cuda.get_device_name(dev),
           "model": f"{MODEL_CYC_PER_64:g} SIMD cycles / 64 pixel-shifts, {SIMDS} SIMDs, {CLOCK_HZ / 1e9:g} GHz", "shapes": {}}
    for B in (8, 1):
        g = torch.Generator(device=dev).manual_seed(B)
        v = torch.rand(B, 3, 1024, 1024, device=dev, generator=g)
        sigma = torch.full((B,), 0.05, device=dev)
        ms = time_ms(lambda: ops.nlm(v, sigma), a.iters, a.warmup)
        ps = B * 1024 * 1024 * 121
        model_ms = ps / 64 * MODEL_CYC_PER_64 / SIMDS / CLOCK_HZ * 1e3
        row = {"ms": round(ms, 4), "pixel_shifts_per_s": float(f"{ps / ms * 1e3:.4g}"), "model_ms": round(model_ms, 4),
               "model_fraction": round(model_ms / ms, 3)}
        if not a.no_baseline:
            with torch.no_grad():
                base = time_ms(lambda: nlm_torch(v, sigma), a.baseline_iters, 1)
                diff = (nlm_torch(v, sigma) - ops.nlm(v, sigma)).abs().max().item()
            row.update(torch_ms=round(base, 2), speedup_vs_torch=round(base / ms, 1), max_abs_diff_vs_torch=float(f"{diff:.3g}"))
        res["shapes"][f"{B}x3x1024x1024"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
