#!/usr/bin/env python
"""Times the LP solver's inner and outer iteration on one GPU (float64, sparse).

The LP is synthetic, built as tests/golden/make_golden_lp.py builds its cases (a primal-dual pair: feasible and bounded), restated
here with NumPy: n unknowns, n / 2 inequality and n / 8 equality rows of 8 entries each (multiples of 1 / 4), so [A_ub; A_eq; I] has
about 4 entries per row and its transpose about 6.  Sizes n = 2^10, 2^14, 2^17.

  inner   one PCG iteration (dpx_lp_pcg_iters with a tolerance of 0, so it never stops), ``--chain`` iterations per timed window,
          in both forms of the direction update: folded into the product's gather (3 launches) and as a launch of its own (4)
  outer   ``LPSolverADMM.solve`` for ``--outer`` outer iterations, wall clock with a final synchronisation: us per outer iteration
          and the inner iterations it took (host pacing, pinned read-backs and the evaluations included)
  spmv    the plain row product (dpx_lp_spmv_chain: ``--chain`` launches from one host call) with A and with its transpose: bytes 12 nnz + 8 (rows + gathered vector) per second,
          against the copy rate of a 256 MiB float64 ``copy_`` measured in the same run
  torch   the same inner iteration written with torch ops on the device (no host read).  Sparse CSR ``@`` in float64 if this torch
          build runs it on the device; otherwise dense matrices, for n <= 2^12 only -- the result says which.

Kernel times (profiles/lp_kernel_stats.csv) come from a kernel trace of this tool at one size, in a run of its own:
``rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_lp.py --sizes 131072 --reps 5 --out DIR/bench.json``.

    python tools/bench_lp.py [--reps 20] [--chain 20] [--outer 50] [--sizes N ...] [--out profiles/lp_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dprox import _backend as be  # noqa: E402
from dprox.algo import lp  # noqa: E402

SIZES = [1 << 10, 1 << 14, 1 << 17]
PER_ROW = 8


def rows_of(rng, rows, n):
    """CSR of a rows x n matrix with PER_ROW distinct columns per row, entries non-zero multiples of 1/4 in [-2, 2]"""
    start = rng.randint(n, size=(rows, 1))
    cols = np.sort((start + np.cumsum(rng.randint(1, max(n // (2 * PER_ROW), 2), size=(rows, PER_ROW)), axis=1)) % n, axis=1)
    vals = rng.randint(1, 9, size=(rows, PER_ROW)) / 4.0 * np.where(rng.rand(rows, PER_ROW) < 0.5, -1.0, 1.0)
    return (np.arange(rows + 1) * PER_ROW, cols.ravel(), vals.ravel(), (rows, n))


def matvec(csr, v, transpose=False):
    indptr, indices, data, (rows, n) = csr
    r = np.repeat(np.arange(rows), np.diff(indptr))
    return np.bincount(indices, weights=data * v[r], minlength=n) if transpose else np.bincount(r, weights=data * v[indices], minlength=rows)


def synthetic_lp(n, seed=7):
    rng = np.random.RandomState(seed)
    m_ub, m_eq = n // 2, n // 8
    A_ub, A_eq = rows_of(rng, m_ub, n), rows_of(rng, m_eq, n)
    zero = rng.rand(n) < 0.4
    xstar = np.where(zero, 0.0, rng.randint(1, 17, n) / 4.0)
    tight = rng.rand(m_ub) < 0.5
    b_ub = matvec(A_ub, xstar) + np.where(tight, 0.0, rng.randint(1, 17, m_ub) / 4.0)
    b_eq = matvec(A_eq, xstar)
    y_u, y_e = np.where(tight, rng.randint(1, 9, m_ub) / 4.0, 0.0), rng.randint(-8, 9, m_eq) / 4.0
    c = -matvec(A_ub, y_u, True) - matvec(A_eq, y_e, True) + np.where(zero, rng.randint(1, 9, n) / 4.0, 0.0)
    return c, A_ub, b_ub, A_eq, b_eq


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


def per(t, chain):
    return {k: (v / chain if k.endswith("_us") else v) for k, v in t.items()}


def copy_rate(dev, reps):
    a = torch.empty(32 << 20, dtype=torch.float64, device=dev)
    b = torch.empty_like(a)
    t = timed(lambda: b.copy_(a), reps)
    return 2 * a.numel() * 8 / (t["median_us"] * 1e-6)


def torch_iteration(p, dev, rho, sigma):
    """the inner iteration in torch ops: (a function that runs one, "sparse_csr" or "dense"), or (None, why)"""
    n, m, nnz = p.n, p.m, len(p.A[2])
    try:
        mk = lambda csr, shape: torch.sparse_csr_tensor(torch.from_numpy(csr[0]), torch.from_numpy(csr[1]), torch.from_numpy(csr[2]), size=shape).to(dev)
        A, AT = mk(p.A, (m, n)), mk(p.AT, (n, m))
        (AT @ (A @ torch.ones(n, 1, dtype=torch.float64, device=dev))).sum().item()
        kind = "sparse_csr"
    except Exception as why:                                            # this build does not run float64 CSR @ on the device
        if n > 1 << 12:
            return None, f"no sparse CSR @ in float64 on this build ({type(why).__name__}); dense only for n <= 2^12"
        D = torch.zeros(m, n, dtype=torch.float64)
        D[np.repeat(np.arange(m), np.diff(p.A[0])), p.A[1]] = torch.from_numpy(p.A[2])
        A, AT, kind = D.to(dev), D.T.contiguous().to(dev), "dense"
    g = torch.Generator(device="cpu").manual_seed(0)
    st = {k: torch.randn(n, 1, dtype=torch.float64, generator=g).to(dev) for k in ("x", "r", "p")}
    M = sigma + rho * torch.from_numpy(p.Acnorm).to(dev).unsqueeze(1) ** 2
    st["y"] = st["r"] / M

    def step():
        x, r, y, pv = st["x"], st["r"], st["y"], st["p"]
        Ap = AT @ (rho * (A @ pv)) + sigma * pv
        ry = r.ravel() @ y.ravel()
        a = ry / (pv.ravel() @ Ap.ravel())
        x = x + a * pv
        r = r + a * Ap
        y = r / M
        beta = (r.ravel() @ y.ravel()) / ry
        pv = -y + beta * pv
        st["rnorm"] = torch.linalg.vector_norm(r.ravel(), ord=float("inf"))
        st.update(x=x, r=r, y=y, p=pv)
    return step, kind


def bench(args):
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "chain": args.chain, "copy_rate_TBps": copy_rate(dev, args.reps) / 1e12, "sizes": {}}
    rho, sigma = 0.1, 1e-6
    for n in args.sizes or SIZES:
        t0 = time.perf_counter()
        p = lp.LPProblem(*synthetic_lp(n), device=dev)
        nnz = len(p.A[2])
        out = {"n": n, "m": p.m, "nnz": nnz, "preprocess_s": time.perf_counter() - t0}
        solver = lp.LPSolverADMM(rho=rho, abstol=1e-3, reltol=1e-6, max_iters=args.outer, verbose=False).eval()
        ctl, _, _ = solver.control(p, dev)
        out["lanes_A_AT"] = list(ctl.lanes())
        g = torch.Generator(device="cpu").manual_seed(0)
        for t, length in ((ctl.x, n), (ctl.xt, n), (ctl.z, p.m), (ctl.y, p.m)):
            t.copy_(torch.randn(length, dtype=torch.float64, generator=g))
        ctl.t.copy_(ctl.spmv("a", ctl.xt))
        for form, knob in (("folded", 0), ("split", 1)):
            with be.tuned(lp_split_direction=knob):
                ctl.pcg_start(rho, sigma, 0.0)
                before = ctl.launches
                t = per(timed(lambda: ctl.pcg_iters(rho, sigma, args.chain), args.reps), args.chain)
                t["launches_per_iteration"] = (ctl.launches - before) // ((args.reps + 3) * args.chain)
                out[f"inner_{form}"] = t
        out["folded_over_split"] = out["inner_folded"]["median_us"] / out["inner_split"]["median_us"]
        for which, rows, cols in (("a", p.m, n), ("at", n, p.m)):
            v = ctl.xt if which == "a" else ctl.y
            t = per(timed(lambda: ctl.spmv(which, v, reps=args.chain), args.reps), args.chain)     # one host call: the kernels' rate
            t["bytes"] = 12 * nnz + 8 * (rows + cols)
            t["TBps"] = t["bytes"] / (t["median_us"] * 1e-6) / 1e12
            t["frac_of_copy_rate"] = t["TBps"] / res["copy_rate_TBps"]
            out[f"spmv_{which}"] = t
        step, kind = torch_iteration(p, dev, rho, sigma)
        out["torch_baseline"] = kind
        if step is not None:
            out["inner_torch"] = per(timed(lambda: [step() for _ in range(args.chain)], max(args.reps // 2, 3)), args.chain)
            out["torch_over_kernels"] = out["inner_torch"]["median_us"] / out["inner_folded"]["median_us"]
        del ctl
        solver.solve(p, residual_balance=True, max_iters=3)                     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.solve(p, residual_balance=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        s = solver.last_stats
        inner = s["operator_applications"] / s["outer_iterations"] - 1
        out["outer"] = {"outer_iterations": s["outer_iterations"], "us_per_outer_iteration": wall * 1e6 / s["outer_iterations"],
                        "inner_iterations_per_outer": inner, "us_per_inner_iteration_in_the_solve": wall * 1e6 / s["operator_applications"],
                        "launches": s["launches"]}
        res["sizes"][str(n)] = out
        print(json.dumps({str(n): out}), flush=True)
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--outer", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", help="unknowns (default 2^10 2^14 2^17); one size for a kernel trace's per-kernel statistics")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lp.py needs a HIP device")
    res = bench(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
