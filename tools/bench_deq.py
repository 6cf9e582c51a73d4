#!/usr/bin/env python
"""Times the Anderson step of the DEQ specialization and a whole DEQSolver.solve on one GPU.

  step      one Anderson step without f at n = m = 6 on the packed state of a B x C x H x W problem with two split terms (5 pieces):
            dpx_anderson_mix + dpx_anderson_gram_row, each timed alone with device events, against the same arithmetic composed from
            torch ops on the device (G = F - X, the bordered system through bmm / linalg.solve, the alpha products, the two norms
            with their host reads).  Bytes per launch from DESIGN.md's count: mix reads n vectors and writes 1, gram_row reads n + 1
            and writes 1; the fraction is of the 6.29 TB/s copy rate the project measured.
  unaligned the two kernels at a piece length that is no multiple of 4 (4-byte accesses), same count
  solve     DEQSolver.solve with f_thres = 40 (eps = 0: all 38 steps) against 40 plain ADMM iterations of the same solver

    python tools/bench_deq.py [--shape 8 3 1024 1024] [--reps 20] [--out profiles/deq_bench.json] [--only step|solve]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dprox as dp  # noqa: E402
from dprox import _ops as ops  # noqa: E402

COPY_RATE = 6.29e12
M, P = 6, 5


def timed(fn, reps, warmup=3):
    """median / min / max of ``reps`` device-event timings of fn(), in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "reps": reps}


def with_rate(t, vectors, vec_bytes):
    t["bytes"] = vectors * vec_bytes
    t["TBps"] = t["bytes"] / (t["median_us"] * 1e-6) / 1e12
    t["frac_of_copy"] = t["TBps"] * 1e12 / COPY_RATE
    return t


def filled_history(shape, dev):
    B = shape[0]
    hist = ops.AndersonHistory(M, P, B, shape[1:], dev)
    for k in range(M):
        hist.X.normal_()
        hist.F[k].copy_(hist.X).add_(torch.randn_like(hist.X), alpha=0.1 + 0.05 * k)
        hist.gram_row(k, k + 1)
    return hist


def torch_step(F, X, lam=1e-4):
    """the same step from torch ops: F, X [B, m, N] packed histories; returns the new point and the two stop-rule scalars"""
    B, n, _ = F.shape
    G = F - X
    H = torch.zeros(B, n + 1, n + 1, dtype=F.dtype, device=F.device)
    H[:, 0, 1:] = H[:, 1:, 0] = 1
    y = torch.zeros(B, n + 1, 1, dtype=F.dtype, device=F.device)
    y[:, 0] = 1
    H[:, 1:, 1:] = torch.bmm(G, G.transpose(1, 2)) + lam * torch.eye(n, dtype=F.dtype, device=F.device)[None]
    alpha = torch.linalg.solve(H, y)[:, 1:n + 1, 0]
    Xn = (alpha[:, None] @ F)[:, 0]
    g = F[:, 0] - X[:, 0]
    return Xn, g.norm().item(), g.norm().item() / (1e-5 + F[:, 0].norm().item())


def bench_step(shape, reps, dev):
    hist = filled_history(shape, dev)
    vec = hist.X.numel() * 4
    out = {"shape": list(shape), "pieces": P, "m": M, "vector_bytes": vec}
    out["mix"] = with_rate(timed(lambda: hist.mix(M, 1.0, 1e-4), reps), M + 1, vec)
    out["gram_row"] = with_rate(timed(lambda: hist.gram_row(M - 1, M), reps), M + 2, vec)
    out["step"] = timed(lambda: (hist.mix(M, 1.0, 1e-4), hist.gram_row(M - 1, M)), reps)
    return out, hist


def bench(args):
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12}
    B, C, H, W = args.shape
    if args.only in (None, "step"):
        res["aligned"], hist = bench_step((B, C, H, W), args.reps, dev)
        N = hist.X.numel() // B
        F = hist.F.permute(2, 0, 1, 3, 4, 5).reshape(B, M, N).contiguous()      # the reference's packed [B, m, N] layout
        del hist
        X = F - 0.1 * torch.randn_like(F)
        res["aligned"]["torch_step"] = timed(lambda: torch_step(F, X), max(args.reps // 4, 3), warmup=2)
        res["aligned"]["speedup_vs_torch"] = res["aligned"]["torch_step"]["median_us"] / res["aligned"]["step"]["median_us"]
        del F, X
        torch.cuda.empty_cache()
        res["unaligned"], hist = bench_step((B, C, H - 1, W - 1), args.reps, dev)
        del hist
        torch.cuda.empty_cache()
    if args.only in (None, "solve"):
        rng = np.random.RandomState(0)
        b = torch.from_numpy(rng.rand(B, C, H, W).astype(np.float32)).to(dev)
        g = np.exp(-0.5 * (np.arange(-7, 8) / 2.0) ** 2)
        psf = (np.outer(g, g) / np.outer(g, g).sum()).astype(np.float32)
        x = dp.Variable()
        fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
        solver = dp.compile(fns, method="admm", device=dev)
        model = dp.specialize(solver, method="deq", device=dev).eval()
        model.eps = 0.0

        def deq_solve():
            with torch.no_grad():
                model.solve(x0=b, rhos=0.3, lams=0.02, f_thres=40)

        def admm40():
            with torch.no_grad():
                solver.solve(x0=b, rhos=0.3, lams=0.02, max_iter=40)
        r = max(args.reps // 4, 3)
        res["solve"] = {"deq_f_thres_40": timed(deq_solve, r, warmup=2), "admm_40_iterations": timed(admm40, r, warmup=2)}
        res["solve"]["final_rel_residual"] = model.last_forward["rel_trace"][-1]
        res["solve"]["deq_over_admm"] = res["solve"]["deq_f_thres_40"]["median_us"] / res["solve"]["admm_40_iterations"]["median_us"]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 3, 1024, 1024])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deq_bench.json"))
    ap.add_argument("--only", choices=["step", "solve"], default=None)
    args = ap.parse_args()
    res = bench(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
