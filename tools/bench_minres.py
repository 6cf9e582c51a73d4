#!/usr/bin/env python
"""Times the MINRES step and a whole ``minres`` solve on one GPU, float32, one shift, identity preconditioner.

  step    the three launches of a step without the operator (dpx_minres_alpha, dpx_minres_lanczos, dpx_minres_update), each timed
          alone and all three together, against the same arithmetic written as torch ops on the device (``torch_step``: the
          reference's step, solver_minres.py:150-213 and 258-290, restated; no host read).  A timed window is ``--chain`` steps
          long so that it is not a few microseconds.  Bytes from DESIGN.md's count at one shift: alpha reads 2 vectors, lanczos
          reads 3 and writes 1, update reads 5 and writes 3 -- 14 vector passes; the rate is given as a fraction of the 8.0 TB/s
          HBM peak and of the 6.29 TB/s copy rate the project measured.
  solve   ``dprox.linalg.solve.minres`` against the reference's loop restated in torch ops on the device (``torch_minres``), both on
          a matrix-free symmetric tridiagonal operator written in torch ops, rtol = 0 and max_iters = 30: all 32 steps and the three
          stop tests with their host reads.

Sizes [G][N][K]: [1][2^20][1], [8][3 * 256^2][1], [1][65536][8].

    python tools/bench_minres.py [--reps 20] [--chain 20] [--out profiles/minres_bench.json] [--only step|solve]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd")]

import torch  # noqa: E402

from dprox import _ops as ops  # noqa: E402
from dprox.linalg.solve import minres  # noqa: E402

HBM_PEAK, COPY_RATE = 8.0e12, 6.29e12
SIZES = [(1, 1 << 20, 1), (8, 3 * 256 * 256, 1), (1, 65536, 8)]
PASSES = {"alpha": 2, "lanczos": 4, "update": 8}


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


def per_step(t, chain, passes, vec_bytes):
    t = {k: (v / chain if k.endswith("_us") else v) for k, v in t.items()}
    t["bytes"] = passes * vec_bytes
    t["TBps"] = t["bytes"] / (t["median_us"] * 1e-6) / 1e12
    t["frac_of_hbm_peak"] = t["TBps"] * 1e12 / HBM_PEAK
    t["frac_of_copy_rate"] = t["TBps"] * 1e12 / COPY_RATE
    return t


def torch_state(b):
    """the state of the reference's loop for a scaled right-hand side b [G, N, K], one shift"""
    sc = lambda v: torch.full((1,) + b.shape[:-2] + (1, b.shape[-1]), v, dtype=b.dtype, device=b.device)
    beta = (b * b).sum(-2, keepdim=True).sqrt()
    z1 = b / beta
    return dict(z2=torch.zeros_like(b), z1=z1, q=z1.clone(), beta_prev=beta, cos2=sc(1.0), sin2=sc(0.0), cos1=sc(1.0), sin1=sc(0.0),
                s2=torch.zeros((1,) + b.shape, dtype=b.dtype, device=b.device), s1=torch.zeros((1,) + b.shape, dtype=b.dtype, device=b.device),
                scale=beta[None].clone(), x=torch.zeros((1,) + b.shape, dtype=b.dtype, device=b.device), eps=torch.tensor(1e-25, device=b.device))


def torch_step(st, prod):
    """one step of the reference's loop from its product ``prod = A(q)`` on, op for op (out-of-place where it used out=)"""
    alpha = (prod * st["q"]).sum(-2, keepdim=True)
    z = prod.addcmul_(alpha, st["z1"], value=-1).addcmul_(st["beta_prev"], st["z2"], value=-1)
    q = z.clone()
    beta = (z * q).sum(-2, keepdim=True).sqrt_().clamp_min_(st["eps"])
    z.div_(beta)
    q.div_(beta)
    subsub = st["sin2"] * st["beta_prev"]
    sub = st["cos2"] * st["beta_prev"]
    diag = (alpha * st["cos1"]).addcmul_(st["sin1"], sub, value=-1)
    sub = sub.mul_(st["cos1"]).addcmul_(st["sin1"], alpha)
    radius = (diag * diag).addcmul_(beta, beta).sqrt_()
    cos, sin = diag / radius, beta / radius
    diag = diag.mul_(cos).addcmul_(sin, beta)
    scale_next = (st["scale"] * sin).mul_(-1)
    st["scale"].mul_(cos)
    search = torch.addcmul(st["q"], sub, st["s1"], value=-1).addcmul_(subsub, st["s2"], value=-1).div_(diag)
    st["x"].add_(search * st["scale"])
    st.update(z2=st["z1"], z1=z, q=q, beta_prev=beta, cos2=st["cos1"], sin2=st["sin1"], cos1=cos, sin1=sin, s2=st["s1"], s1=search,
              scale=scale_next)


def torch_minres(A, b, rtol, max_iters):
    """the reference's minres restated in torch ops on b's device (identity preconditioner, one shift, no value)"""
    norm = b.norm(2, dim=-2, keepdim=True)
    zero = norm.lt(1e-10)
    norm = norm.masked_fill(zero, 1)
    b = b / norm
    st = torch_state(b)
    bnorm = torch.linalg.vector_norm(b)
    for i in range(min(max_iters, b.size(-2) + 1) + 2):
        torch_step(st, A(st["q"]))
        if (i + 1) % 10 == 0 and torch.linalg.vector_norm(A(st["x"][0]) - b) <= rtol * bnorm:
            break
    return st["x"].masked_fill_(zero, 0).squeeze(0).mul_(norm)


def tridiag(N, dev):
    d = 2.0 + torch.rand(N, device=dev)
    e = 0.5 * torch.rand(N - 1, device=dev) - 0.25

    def A(x):
        y = d[:, None] * x
        y[..., 1:, :] += e[:, None] * x[..., :-1, :]
        y[..., :-1, :] += e[:, None] * x[..., 1:, :]
        return y
    return A


def bench(args):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12, "copy_rate_TBps": COPY_RATE / 1e12, "chain": args.chain,
           "sizes": {}}
    for G, N, K in SIZES:
        b = torch.randn(G, N, K, device=dev)
        vec = b.numel() * 4
        out = {"vector_bytes": vec}
        if args.only in (None, "step"):
            ctl = ops.MinresControl(b, torch.zeros(1), None, 1e-25)
            ctl.alpha(b, b, value=1.0)
            ctl.init(0)
            ctl.alpha(b, b, value=1.0)
            ctl.init(1)
            ctl.zring[1].copy_(b)
            prod = torch.randn_like(b)
            chain = args.chain
            launches = {"alpha": lambda: ctl.alpha(prod), "lanczos": lambda: ctl.lanczos(prod), "update": ctl.update}
            for name, fn in launches.items():
                out[name] = per_step(timed(lambda: [fn() for _ in range(chain)], args.reps), chain, PASSES[name], vec)
            out["step"] = per_step(timed(lambda: [(ctl.alpha(prod), ctl.lanczos(prod), ctl.update()) for _ in range(chain)], args.reps), chain,
                                   sum(PASSES.values()), vec)
            st = torch_state(b / b.norm(2, dim=-2, keepdim=True))
            out["torch_step"] = per_step(timed(lambda: [torch_step(st, prod.clone()) for _ in range(chain)], max(args.reps // 2, 3)), chain,
                                         sum(PASSES.values()), vec)
            out["torch_over_kernels"] = out["torch_step"]["median_us"] / out["step"]["median_us"]
            del ctl, st, prod
        if args.only in (None, "solve"):
            A = tridiag(N, dev)
            r = max(args.reps // 4, 3)
            with torch.no_grad():
                mine = minres(A, b, rtol=0.0, max_iters=30)
                theirs = torch_minres(A, b, 0.0, 30)
                out["solve_rel_l2_vs_torch"] = float((mine - theirs).norm() / theirs.norm())
                out["solve_minres"] = timed(lambda: minres(A, b, rtol=0.0, max_iters=30), r, warmup=2)
                out["solve_torch"] = timed(lambda: torch_minres(A, b, 0.0, 30), r, warmup=2)
            out["solve_torch_over_minres"] = out["solve_torch"]["median_us"] / out["solve_minres"]["median_us"]
        res["sizes"][f"{G}x{N}x{K}"] = out
        del b
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minres_bench.json"))
    ap.add_argument("--only", choices=["step", "solve"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_minres.py needs a HIP device")
    res = bench(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
