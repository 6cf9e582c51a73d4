#!/usr/bin/env python
"""Golden vectors of the TV denoiser prior -- runs ONLY in the build container (needs the reference checkout).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt) and stores the
reference's own outputs:

  fn2_* / fn3_*     TV_denoising / TV_denoising3d (proxfn/pnp/denoisers/models/TV_denoising.py) on a noisy 3 x 33 x 47 volume (`a`)
                    and a noisy 31 x 17 x 19 volume (`b`), iteration in {1, 5, 13}, lamda in {0.05, 0.3}: fp32 and float64 runs
  den2_* / den3_*   TVDenoiser(5, use_3dtv).denoise (denoisers/wrapper.py:8-22) on [1, 3, 33, 47] with a 0-d sigma
  admm2_* / admm3_* sum_squares(conv(x, psf) - b) + deep_prior(x, denoiser=TVDenoiser(5, use_3dtv)), the reference's ADMM for 5
                    iterations at 1 x 3 x 32 x 40: x, v, u (+ the float64 run's x and the reference's own fp32-vs-float64 distance)

Three files, each below the 1 MiB a committed file may have: g43_tv_denoiser.npz (den*, admm*), g43_tv_fn2.npz and g43_tv_fn3.npz.
The float64 outputs are incompressible and fill the fn files on their own, so those store an fp32 output `<key>` losslessly as
`<key>_bits`, the int32 difference between its bit pattern and that of its float64 twin rounded to fp32 (a few units, compressed to
nothing); tests/tv_cases.py:fn_fixture adds it back.

    python tests/golden/make_golden_tv.py          # writes tests/golden/g43_tv_{denoiser,fn2,fn3}.npz
"""
import os
import runpy

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp, synthetic = G["np"], G["torch"], G["dp"], G["synthetic"]
T, T64, save, reference_in_float64 = G["T"], G["T64"], G["save"], G["reference_in_float64"]
from dprox.proxfn.pnp.denoisers.models.TV_denoising import TV_denoising, TV_denoising3d  # noqa: E402   (the REFERENCE's)
from dprox.proxfn.pnp.denoisers.wrapper import TVDenoiser  # noqa: E402

assert dp.__file__.startswith(G["REF"]), dp.__file__

ITERS, LAMS = (1, 5, 13), (0.05, 0.3)
SIGMA = 0.1


def noisy(shape, seed, noise=0.05):
    rng = np.random.RandomState(seed)
    gt = synthetic.synth(rng, 1, *shape)[0]
    return (gt + noise * rng.randn(*shape)).astype(np.float32)


def admm(b, psf, rhos, lams, use_3dtv, f64):
    b_, psf_ = (T64(b), T64(psf)) if f64 else (T(b), psf)
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=TVDenoiser(5, use_3dtv))
    fns = dp.sum_squares(dp.conv(x, psf_) - b_) + prior
    with torch.no_grad():
        st = dp.Problem(fns).solve(method="admm", device="cpu", x0=b_.clone(), rhos=rhos, lams={prior: lams}, max_iter=5, return_full_states=True)
    assert st[0].dtype == (torch.float64 if f64 else torch.float32)
    return st


def g43_tv_denoiser():
    vols = {"a": noisy((3, 33, 47), seed=430), "b": noisy((31, 17, 19), seed=431)}
    gaps = []
    for tag, fn in (("fn2", TV_denoising), ("fn3", TV_denoising3d)):
        out = {"iters": np.array(ITERS), "lams": np.array(LAMS)}
        for vk, v in vols.items():
            out[f"{vk}_v"] = v
            for it in ITERS:
                for li, lam in enumerate(LAMS):
                    with torch.no_grad():
                        r32 = fn(T(v), lam, it)
                        r64 = fn(T64(v), lam, it)
                    assert r32.dtype == torch.float32 and r64.dtype == torch.float64
                    key = f"{vk}_i{it}_l{li}"
                    out[key + "_f64"] = r64
                    out[key + "_bits"] = r32.numpy().view(np.int32) - r64.numpy().astype(np.float32).view(np.int32)
                    gaps.append(float((r32.double() - r64).norm() / r64.norm()))
        save(f"g43_tv_{tag}", **out)
    print(f"   fn2 / fn3: the reference's fp32 vs float64 operator: rel-L2 {min(gaps):.2e} .. {max(gaps):.2e}")
    out = {}
    v4 = vols["a"][None]
    out["den_v"], out["den_sigma"] = v4, np.float32(SIGMA)
    for tag, use_3dtv in (("den2", False), ("den3", True)):
        with torch.no_grad():
            out[f"{tag}_out"] = TVDenoiser(5, use_3dtv).denoise(T(v4), torch.tensor(SIGMA))
            out[f"{tag}_out_f64"] = TVDenoiser(5, use_3dtv).denoise(T64(v4), torch.tensor(SIGMA).double())      # (the same number, promoted)
        assert tuple(out[f"{tag}_out"].shape) == v4.shape and out[f"{tag}_out_f64"].dtype == torch.float64
    gt, b, psf = synthetic.deconv_case(1, 3, 32, 40, seed=432)
    rhos = torch.tensor([0.2, 0.15, 0.1, 0.08, 0.06])
    lams = torch.tensor([0.05, 0.04, 0.03, 0.025, 0.02])
    out["b"], out["psf"], out["rhos"], out["prior_lams"] = b, psf, rhos, lams
    for tag, use_3dtv in (("admm2", False), ("admm3", True)):
        st = admm(b, psf, rhos, lams, use_3dtv, False)
        with reference_in_float64():
            st64 = admm(b, psf, rhos, lams, use_3dtv, True)
        out[f"{tag}_x"], out[f"{tag}_v0"], out[f"{tag}_u0"] = st[0], st[1][0], st[2][0]
        out[f"{tag}_x_f64"] = st64[0]
        rel = float((st[0].double() - st64[0]).norm() / st64[0].norm())
        out[f"{tag}_ref_f32_vs_f64"] = np.float64(rel)
        print(f"   {tag}: the reference's fp32 vs float64 iterate: rel-L2 {rel:.2e}")
    save("g43_tv_denoiser", **out)


if __name__ == "__main__":
    g43_tv_denoiser()
