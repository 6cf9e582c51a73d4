#!/usr/bin/env python
"""Golden vectors of the DEQ specialization -- runs ONLY in the build container (needs the reference checkout).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt) and runs the reference's
DEQSolver (specialization/deq/solver.py) on the CPU, at fp32 and, inside reference_in_float64, at float64.  Two generator-side
patches, both in this process only: ``torch.cuda.synchronize`` is a no-op (the reference's backward hook calls it), and the solver's
``anderson`` is wrapped so that it runs with eps = 1e-12 (never reached: every run takes threshold - 2 steps) and its returned
dicts (traces, nstep) are recorded.

  g41_deq_tv      TV deconvolution 2 x 1 x 32 x 48, threshold 12: inputs, z* = x of the forward solve, rel / abs traces, nstep
                  (fp32 and float64), and in training mode with learned_params the gradients of sum(w * x) w.r.t. r, l and the
                  observation (fp32 and float64), and the float64 run's packed z*
  g41_deq_tv256   TV deconvolution 1 x 3 x 256 x 256, threshold 12: the observation's seed (the test rebuilds the inputs from
                  synthetic.deconv_case), x of the fp32 run, traces, nstep
  g41_deq_tv256_f64   x of the float64 run, stored rounded to fp32 (6e-8 relative: far inside the 1e-5 slack of the criterion that
                  reads it; the float64 array alone would exceed the size limit of a committed file)

    python tests/golden/make_golden_deq.py [fixture names; default: all]
"""
import os
import runpy
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp, synthetic = G["np"], G["torch"], G["dp"], G["synthetic"]
T, T64, save, reference_in_float64 = G["T"], G["T64"], G["save"], G["reference_in_float64"]
from dprox.algo.specialization.deq.solver import DEQSolver  # noqa: E402   (the REFERENCE's)
from dprox.algo.specialization.deq.utils.solvers import anderson  # noqa: E402

assert dp.__file__.startswith(G["REF"]), dp.__file__
torch.cuda.synchronize = lambda *a, **k: None

THRES, EPS = 12, 1e-12
RHO, LAM = 0.3, 0.02


def run(b, psf, f64, train, w=None):
    """the reference's DEQSolver on sum_squares(conv(x, psf) - b) + norm1(grad_H x) + norm1(grad_W x); returns x, the recorded
    anderson dicts and (train) the gradients of sum(w x)"""
    b_ = (T64(b) if f64 else T(b)).clone().requires_grad_(train)
    psf_ = T64(psf) if f64 else psf
    x = dp.Variable()
    fns = dp.sum_squares(dp.conv(x, psf_) - b_) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
    solver = dp.compile(fns, method="admm", device="cpu")
    deq = DEQSolver(solver, learned_params=train)
    if f64:
        deq = deq.double()
    calls = []

    def recorded(f, x0, **kw):
        out = anderson(f, x0, eps=EPS, **kw)
        calls.append(out)
        return out
    deq.solver.solver = recorded
    deq.solver.f_thres = deq.solver.b_thres = THRES
    deq.train(train)
    rho = torch.tensor(RHO, dtype=b_.dtype)
    lam = torch.tensor(LAM, dtype=b_.dtype)
    if not train:
        with torch.no_grad():
            out = deq.solve(x0=b_.detach().clone(), rhos=rho, lams=lam)
        return out, calls, None
    out = deq.solve(x0=b_.detach().clone(), rhos=rho, lams=lam)
    ((T64(w) if f64 else T(w)) * out).sum().backward()
    return out, calls, (deq.r.grad, deq.l.grad, b_.grad)


def both(b, psf, train, w=None):
    o32 = run(b, psf, False, train, w)
    with reference_in_float64():
        o64 = run(b, psf, True, train, w)
    assert o32[0].dtype == torch.float32 and o64[0].dtype == torch.float64
    for a, c in zip(o32[1], o64[1]):
        assert a["nstep"] == c["nstep"], (a["nstep"], c["nstep"])         # the fp32 and float64 runs choose the same iterate
        assert len(a["rel_trace"]) == THRES - 2
    rel = float((o32[0].double() - o64[0]).norm() / o64[0].norm())
    print(f"   train={train}: nstep {[c['nstep'] for c in o32[1]]}, the reference's fp32 vs float64 x: rel-L2 {rel:.2e}, final rel "
          f"{o32[1][0]['rel_trace'][-1]:.2e}")
    return o32, o64


def traces(out, tag, o32, o64):
    for suf, o in (("", o32), ("_f64", o64)):
        out[f"{tag}_x{suf}"] = o[0].detach()
        out[f"{tag}_rel_trace{suf}"] = np.array(o[1][0]["rel_trace"], np.float64)
        out[f"{tag}_abs_trace{suf}"] = np.array(o[1][0]["abs_trace"], np.float64)
        out[f"{tag}_nstep{suf}"] = np.int64(o[1][0]["nstep"])


def g41_deq_tv():
    out = {"thres": np.int64(THRES), "eps": np.float64(EPS), "rho": np.float32(RHO), "lam": np.float32(LAM), "seed": np.int64(410)}
    gt, b, psf = synthetic.deconv_case(2, 1, 32, 48, seed=410)
    out["b"], out["psf"] = b, psf
    traces(out, "fwd", *both(b, psf, False))
    w = np.random.RandomState(411).randn(*b.shape).astype(np.float32)
    out["w"] = w
    o32, o64 = both(b, psf, True, w)
    traces(out, "train", o32, o64)
    out["train_z_f64"] = o64[1][0]["result"].detach()      # the packed z* (x, v_1, v_2, u_1, u_2) the float64 run differentiates at
    for suf, o in (("", o32), ("_f64", o64)):
        out[f"g_r{suf}"], out[f"g_l{suf}"], out[f"g_b{suf}"] = o[2]
        out[f"bwd_nstep{suf}"] = np.int64(o[1][1]["nstep"])
        out[f"bwd_rel_trace{suf}"] = np.array(o[1][1]["rel_trace"], np.float64)
    for k in ("g_r", "g_l", "g_b"):
        a, c = out[k].double(), out[k + "_f64"]
        print(f"   {k}: fp32 {a.norm():.4e} vs float64: rel {float((a - c).norm() / c.norm()):.2e}")
    save("g41_deq_tv", **out)


def g41_deq_tv256():
    out = {"thres": np.int64(THRES), "eps": np.float64(EPS), "rho": np.float32(RHO), "lam": np.float32(LAM), "seed": np.int64(412)}
    gt, b, psf = synthetic.deconv_case(1, 3, 256, 256, seed=412)
    out["b_checksum"] = np.float64(np.asarray(b, np.float64).sum())
    o32, o64 = both(b, psf, False)
    x64 = o64[0]
    traces(out, "fwd", o32, o64)
    del out["fwd_x_f64"]
    save("g41_deq_tv256", **out)
    save("g41_deq_tv256_f64", fwd_x_f64_rounded=x64.float())


if __name__ == "__main__":
    for name in sys.argv[1:] or ["g41_deq_tv", "g41_deq_tv256"]:
        {"g41_deq_tv": g41_deq_tv, "g41_deq_tv256": g41_deq_tv256}[name]()
