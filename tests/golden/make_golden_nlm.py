#!/usr/bin/env python
"""Golden vectors of the patch_nlm prior -- runs ONLY in the build container (needs the reference checkout).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt) and stores the
reference's own outputs:

  op_*     NonLocalMeansFast (proxfn/nlm/nlm.py) on a noisy 2 x 3 x 33 x 47 batch with a per-image sigma, fp32 and float64 runs
  wrap_*   the same on 1 x 3 x 7 x 9 (every index wraps more than once), at sigma > 0 and sigma = 0
  admm_*   sum_squares(conv(x, psf) - b) + patch_nlm(x), the reference's ADMM for 5 iterations: x, v, u (+ the float64 run's x)
  nn_*     the same data term + 0.5 * patch_nlm(x) + nonneg(x)

    python tests/golden/make_golden_nlm.py          # writes tests/golden/g40_patch_nlm.npz
"""
import os
import runpy

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp, synthetic = G["np"], G["torch"], G["dp"], G["synthetic"]
T, T64, save, reference_in_float64 = G["T"], G["T64"], G["save"], G["reference_in_float64"]
from dprox.proxfn.nlm.nlm import NonLocalMeansFast  # noqa: E402   (the REFERENCE's)

assert dp.__file__.startswith(G["REF"]), dp.__file__


def noisy(B, C, H, W, seed, noise=0.05):
    rng = np.random.RandomState(seed)
    gt = synthetic.synth(rng, B, C, H, W)
    return (gt + noise * rng.randn(B, C, H, W)).astype(np.float32)


def run_nlm(v, sigma):
    """the reference's operator at fp32 and (same numbers, promoted) float64; sigma [B]"""
    B = v.shape[0]
    with torch.no_grad():
        out = NonLocalMeansFast()(T(v), T(sigma).view(B, 1, 1, 1))
        out64 = NonLocalMeansFast()(T64(v), T64(sigma).view(B, 1, 1, 1))
    assert out.dtype == torch.float32 and out64.dtype == torch.float64
    return out, out64


def admm(b, psf, rhos, lams, nonneg, f64):
    """the reference's ADMM on sum_squares(conv(x, psf) - b) + alpha * patch_nlm(x) [+ nonneg(x)] (alpha = 0.5 with nonneg)"""
    b_, psf_ = (T64(b), T64(psf)) if f64 else (T(b), psf)
    x = dp.Variable()
    prior = dp.patch_nlm(x)
    if nonneg:
        prior = 0.5 * prior
    fns = dp.sum_squares(dp.conv(x, psf_) - b_) + prior
    lam_arg = {prior: lams}
    if nonneg:
        nn = dp.nonneg(x)
        fns = fns + nn
        lam_arg[nn] = 0.0
    with torch.no_grad():
        st = dp.Problem(fns).solve(method="admm", device="cpu", x0=b_.clone(), rhos=rhos, lams=lam_arg, max_iter=5, return_full_states=True)
    assert st[0].dtype == (torch.float64 if f64 else torch.float32)
    return st


def g40_patch_nlm():
    out = {}
    v = noisy(2, 3, 33, 47, seed=400)
    sig = np.array([0.04, 0.09], np.float32)
    out["op_v"], out["op_sigma"] = v, sig
    out["op_out"], out["op_out_f64"] = run_nlm(v, sig)
    w = noisy(1, 3, 7, 9, seed=401)
    out["wrap_v"], out["wrap_sigma"] = w, np.array([0.1], np.float32)
    out["wrap_out"], out["wrap_out_f64"] = run_nlm(w, out["wrap_sigma"])
    out["wrap0_out"], out["wrap0_out_f64"] = run_nlm(w, np.zeros(1, np.float32))
    gt, b, psf = synthetic.deconv_case(2, 3, 32, 40, seed=402)
    rhos = torch.tensor([0.2, 0.15, 0.1, 0.08, 0.06])
    lams = torch.tensor([0.004, 0.003, 0.0025, 0.002, 0.0015])          # sigma = sqrt(alpha lam): 0.063 .. 0.039
    out["b"], out["psf"], out["rhos"], out["lams"] = b, psf, rhos, lams
    for tag, nonneg in (("admm", False), ("nn", True)):
        st = admm(b, psf, rhos, lams, nonneg, False)
        with reference_in_float64():
            st64 = admm(b, psf, rhos, lams, nonneg, True)
        out[f"{tag}_x"], out[f"{tag}_v0"], out[f"{tag}_u0"] = st[0], st[1][0], st[2][0]
        out[f"{tag}_x_f64"] = st64[0]
        rel = float((st[0].double() - st64[0]).norm() / st64[0].norm())
        out[f"{tag}_ref_f32_vs_f64"] = np.float64(rel)
        print(f"   {tag}: the reference's fp32 vs float64 iterate: rel-L2 {rel:.2e}")
    for k in ("op", "wrap", "wrap0"):
        a, b64 = out[f"{k}_out"], out[f"{k}_out_f64"]
        print(f"   {k}: the reference's fp32 vs float64 operator: rel-L2 {float((a.double() - b64).norm() / b64.norm()):.2e}")
    save("g40_patch_nlm", **out)


if __name__ == "__main__":
    g40_patch_nlm()
