#!/usr/bin/env python
"""compress_sensing's x-update (ops.cs_xupdate, dpx_cs_xupdate) with one and with two right-hand sides, and its gradient (dpx_cs_backward,
all four gradients), at 1 x 31 x 512 x 512 -- the cube of the reference's hyperspectral example; its operands, 130 .. 200 MB, sit inside
the 256 MiB Infinity Cache: its rate is not an HBM rate -- and at 8 x 31 x 512 x 512, which does not fit.  A mask and a y per image, so
that the algorithmic traffic is exact: per pixel nb C + C + 1 floats read and C written by the x-update; 3 C + 1 read and 2 C + 1
written by the gradient.  At the larger shape the gradient is also timed with ONE mask and y for the batch (`shared`: the thread loops
over the images and adds their mask gradients in registers; the mask and its gradient then count once).

Prints ONE JSON line: per shape and setting the ms per call of the C entry point on prepared arguments (hip events around `calls`
back-to-back calls, `warmup` calls excluded; the median and the min .. max of `rounds` windows; `ops_ms`: the same through
ops.cs_xupdate, whose checks and allocation cost the host more than the small shape's kernel runs), the algorithmic bytes and the
fraction of the 6.29 TB/s measured copy rate they amount to; and, as the baseline, the same arithmetic as torch ops on the device -- the reference's `_prox` expression behind the sum of
the right-hand sides, phi precomputed as its `_reload` does, and torch autograd's backward of it -- timed the same way.

    python tools/bench_cs.py [--calls 20] [--warmup 3] [--rounds 3] [--baseline-calls 5] [--no-baseline]
"""
import argparse
import ctypes
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
SHAPES = [(1, 31, 512, 512), (8, 31, 512, 512)]
LAM = 0.05


def prox_torch(bs, y, mask, phi, lam, I):
    """the reference's expression (proxfn/fast/cs.py:21-27) behind ext_sum_squares.solve's sum"""
    v = bs[0]
    for b in bs[1:]:
        v = v + b
    rhs = mask * ((I * y - torch.sum(v * mask, dim=1, keepdim=True)) / (phi + I * lam))
    return (v + rhs) / I


def raw_xupdate(bs, y3, mask, lam, I):
    """the C entry point on prepared arguments (the launch alone: ops.cs_xupdate's checks and allocation cost the host 30 .. 40 us a call)"""
    L, ptr = be.lib(), be.ptr
    x = torch.empty_like(bs[0])
    pb = (ctypes.c_void_p * len(bs))(*[t.data_ptr() for t in bs])
    N, C, H, W = bs[0].shape
    return lambda: L.call("dpx_cs_xupdate", pb, len(bs), ptr(y3), ptr(mask), ptr(lam), I, ptr(x), N, C, H, W, mask.shape[0], y3.shape[0], be.stream())


def raw_backward(g, v, y3, mask, lam, I):
    L, ptr = be.lib(), be.ptr
    N, C, H, W = g.shape
    gv, gy, glam, gmask = torch.empty_like(g), torch.empty_like(y3), torch.empty(N, device=g.device), torch.empty_like(mask)
    ws = ops.workspace("cs_bwd", L.query("dpx_cs_bwd_ws_bytes", N, C, H, W), g.device)
    return lambda: L.call("dpx_cs_backward", ptr(g), ptr(v), ptr(y3), ptr(mask), ptr(lam), I, ptr(gv), ptr(gy), ptr(glam), ptr(gmask), N, C, H, W,
                          mask.shape[0], y3.shape[0], ptr(ws), be.stream())


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


def windows(fn, calls, warmup, rounds):
    ms = [time_ms(fn, calls, warmup if r == 0 else 1) for r in range(rounds)]
    return statistics.median(ms), [round(min(ms), 4), round(max(ms), 4)]


def entry(ms, spread, floats):
    return {"ms": round(ms, 4), "ms_min_max": spread, "algorithmic_MB": round(4 * floats / 1e6, 1),
            "copy_rate_fraction": round(4 * floats / (ms * 1e-3) / COPY_RATE, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-calls", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"metric": "cs_xupdate", "lam": LAM, "device": torch.cuda.get_device_name(dev), "copy_rate_TBps": COPY_RATE / 1e12,
           "timing": f"median of {a.rounds} windows of {a.calls} back-to-back calls; (min, max) alongside", "cases": {}}
    for shape in SHAPES:
        N, C, H, W = shape
        px = N * H * W
        gen = torch.Generator(device=dev).manual_seed(N)
        b1, b2, g = (torch.randn(*shape, device=dev, generator=gen) for _ in range(3))
        mask = (torch.rand(*shape, device=dev, generator=gen) < 0.5).float()
        y = torch.randn(N, 1, H, W, device=dev, generator=gen)
        lam = torch.full((N,), LAM, device=dev)
        row = {"in_infinity_cache": N == 1,
               "note": "operands fit the 256 MiB Infinity Cache: not an HBM rate" if N == 1 else "operands exceed the Infinity Cache: an HBM rate"}
        settings = {"xupdate_nb1": ([b1], 1), "xupdate_nb2": ([b1, b2], 2)}
        y3 = y.reshape(N, H, W)
        for key, (bs, I) in settings.items():
            ms, spread = windows(raw_xupdate(bs, y3, mask, lam, I), a.calls, a.warmup, a.rounds)
            row[key] = entry(ms, spread, px * (len(bs) * C + C + 1 + C))
            ms, spread = windows(lambda: ops.cs_xupdate(bs, y, mask, lam, I), a.calls, a.warmup, a.rounds)
            row[key].update(ops_ms=round(ms, 4), ops_ms_min_max=spread)
        ms, spread = windows(raw_backward(g, b1, y3, mask, lam, 1), a.calls, a.warmup, a.rounds)
        row["backward_all_four"] = entry(ms, spread, px * (3 * C + 1 + 2 * C + 1) + N)
        if N > 1:
            ms, spread = windows(raw_backward(g, b1, y3[:1].contiguous(), mask[:1].contiguous(), lam, 1), a.calls, a.warmup, a.rounds)
            row["backward_all_four_shared"] = entry(ms, spread, px * 3 * C + H * W * (2 * C + 2) + N)
        if not a.no_baseline:
            lam4 = lam.view(N, 1, 1, 1)
            with torch.no_grad():
                phi = torch.sum(mask ** 2, dim=1, keepdim=True)
                for key, (bs, I) in settings.items():
                    ms, spread = windows(lambda: prox_torch(bs, y, mask, phi, lam4, I), a.baseline_calls, 1, a.rounds)
                    diff = (prox_torch(bs, y, mask, phi, lam4, I) - ops.cs_xupdate(bs, y, mask, lam, I)).abs().max().item()
                    row[key].update(torch_ms=round(ms, 4), torch_ms_min_max=spread, speedup_vs_torch=round(ms / row[key]["ms"], 2),
                                    max_abs_diff_vs_torch=float(f"{diff:.3g}"))
            leaves = [t.clone().requires_grad_(True) for t in (b1, y, lam4, mask)]
            x = prox_torch([leaves[0]], leaves[1], leaves[3], torch.sum(leaves[3] ** 2, dim=1, keepdim=True), leaves[2], 1)
            ms, spread = windows(lambda: torch.autograd.grad(x, leaves, g, retain_graph=True), a.baseline_calls, 1, a.rounds)
            ours = ops.cs_backward(g, b1, y3, mask, lam, 1)
            theirs = torch.autograd.grad(x, leaves, g)
            diff = max((o.reshape(t.shape) - t).abs().max().item() / max(t.abs().max().item(), 1e-30) for o, t in zip((ours[0], ours[1], ours[2], ours[3]), theirs))
            row["backward_all_four"].update(torch_autograd_ms=round(ms, 4), torch_autograd_ms_min_max=spread,
                                            speedup_vs_torch=round(ms / row["backward_all_four"]["ms"], 2), max_rel_diff_vs_torch=float(f"{diff:.3g}"))
            del x, leaves, theirs, ours
        res["cases"]["x".join(map(str, shape))] = row
        del b1, b2, g, mask, y
    print(json.dumps(res))


if __name__ == "__main__":
    main()
