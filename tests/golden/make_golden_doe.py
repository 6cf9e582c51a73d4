#!/usr/bin/env python
"""Golden vectors of the DOE wave-optics model -- runs ONLY in the build container (needs the reference checkout).

The reference's ``dprox/contrib/optic/__init__.py`` imports packages that are not installed; its ``common.py`` and ``doe_model.py``
import only torch and numpy, so they are loaded by file path under a synthetic package name.  Every number below comes out of the
reference's own ``RGBCollimator`` / ``HeightMap`` / ``FresnelPropagator`` / ``img_psf_conv``, run twice on identical parameter values:
as shipped (float32) and built under ``torch.set_default_dtype(torch.float64)`` with the configuration's tensors widened (float64,
the yardstick).  All other configuration values are the reference's defaults.

g48_doe.npz, per case R -> P in (20 -> 20, 30 -> 10, 32 -> 16, 88 -> 44, 136 -> 68) and state in (init = the Fresnel initialisation,
pert = init * (1 + 0.2 rand), seeded):
  <case>_<state>_s                         height_map_sqrt [1,1,R,R] float32
  <case>_<state>_psf64 / _psfbits          get_psf()
  <case>_<state>_w                         a seeded cotangent [1,3,P,P]
  <case>_<state>_grad64 / _gradbits        d sum(w psf) / d height_map_sqrt
  <case>_<state>_d_psf / _d_grad           the reference's own float32-vs-float64 relative l2 distances
32 -> 16 also: phase32 / phase64 (get_phase_profile() at init), base32 / base64 (build_baseline_profile), basepsf32 / basepsf64
(get_psf of it), field (a seeded complex64 [1,3,32,32]), prop32 / prop64 (the propagator's output for it).
cfg_*: the reference's DOEModelConfig defaults.  The exact integer aperture rule is asserted against the reference's float32 one for
every size stored (and 1496).  Float64 outputs are incompressible and the 136 -> 68 case alone holds most of a file's 1 MiB, so it has a
file of its own, g48_doe_r136.npz, and a float32 result is stored losslessly as `<key>bits`: the integer difference between its bit
pattern and that of its float64 twin rounded to float32 (tests/doe_cases.py:golden adds it back as `<key>32`).

g48_doe_e2e.npz: the 32 -> 16 model at init in front of a solver -- a seeded 2 x 3 x 16 x 16 scene, y = img_psf_conv(scene, psf) +
noise (stored), conv_doe data term + the two TV terms and unrolled ADMM of g25_doe_psf_grad, 3 iterations, rhos = 0.2, lam = 0.01, MSE
loss: loss and the gradients to height_map_sqrt and rhos, float32 and float64, with the PSF handed to the Placeholder and used inside y
as the example's step does.  The reference's conv_doe wraps a Placeholder's value in an nn.Parameter of its own, so its gradient to
height_map_sqrt runs through y (and x0 = y) alone, and the gradient to the data term's kernel stops in that parameter's .grad: stored
as g_psf_term32 / g_psf_term64.

    python tests/golden/make_golden_doe.py
"""
import importlib.util
import os
import runpy
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp = G["np"], G["torch"], G["dp"]
T, T64, save, reference_in_float64, REF = G["T"], G["T64"], G["save"], G["reference_in_float64"], G["REF"]
assert dp.__file__.startswith(REF), dp.__file__

CASES = ((20, 20), (30, 10), (32, 16), (88, 44), (136, 68))


def load_optic():
    """the reference's common.py and doe_model.py as modules of a synthetic package (doe_model does `from .common import *`)"""
    pkg = types.ModuleType("ref_optic")
    pkg.__path__ = [os.path.join(REF, "dprox", "contrib", "optic")]
    sys.modules["ref_optic"] = pkg
    mods = {}
    for name in ("common", "doe_model"):
        spec = importlib.util.spec_from_file_location(f"ref_optic.{name}", os.path.join(pkg.__path__[0], name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["common"], mods["doe_model"]


common, doe_model = load_optic()
CFG = doe_model.DOEModelConfig()


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a.astype(b.dtype) - b).ravel()) / np.linalg.norm(b.ravel()))


def bits(a32, a64):
    """a float32 result, stored losslessly as the int32 difference between its bit pattern and that of its float64 twin rounded to float32"""
    a32, near = a32.numpy(), a64.numpy().astype(np.float32)
    return a32.view(np.int32).astype(np.int64) - near.view(np.int32).astype(np.int64)


def build(R, P, f64):
    if not f64:
        return doe_model.RGBCollimator(CFG.sensor_distance, CFG.refractive_idcs, CFG.wave_lengths, P, CFG.sample_interval, (R, R))
    torch.set_default_dtype(torch.float64)
    try:
        return doe_model.RGBCollimator(CFG.sensor_distance, CFG.refractive_idcs.double(), CFG.wave_lengths.double(), P, CFG.sample_interval, (R, R))
    finally:
        torch.set_default_dtype(torch.float32)


def integer_aperture(R):
    a = 2 * np.arange(R, dtype=np.int64) - (R - 1)
    return (a[:, None] ** 2 + a[None, :] ** 2) < (R - 1) ** 2


def psf_and_grad(model, s, w):
    with torch.no_grad():
        model.height_map.height_map_sqrt.copy_(s)
    model.height_map.height_map_sqrt.grad = None
    psf = model.get_psf()
    (psf * w).sum().backward()
    return psf.detach(), model.height_map.height_map_sqrt.grad.clone()


def g48_doe():
    out = {"cfg_refractive_idcs": CFG.refractive_idcs.numpy(), "cfg_wave_lengths": CFG.wave_lengths.numpy(),
           "cfg_scalars": np.array([CFG.aperture_diameter, CFG.sensor_distance, CFG.sample_interval], np.float64),
           "cfg_ints": np.array([CFG.num_steps, CFG.patch_size, CFG.wave_resolution[0], CFG.wave_resolution[1], int(CFG.circular)], np.int64),
           "cases": np.array(CASES, np.int64)}
    m = build(1496, 748, False)
    assert np.array_equal(m.aperture[0, 0].numpy() != 0, integer_aperture(1496)), "aperture rule at 1496"
    del m
    rng = np.random.RandomState(480)
    big = {}
    for R, P in CASES:
        m32, m64 = build(R, P, False), build(R, P, True)
        assert m64.height_map.height_map_sqrt.dtype == torch.float64 and m64.propagator.H.dtype == torch.complex128
        assert np.array_equal(m32.aperture[0, 0].numpy() != 0, integer_aperture(R)), f"aperture rule at {R}"
        s0 = m32.height_map.height_map_sqrt.detach().clone()
        for state in ("init", "pert"):
            s = s0 if state == "init" else (s0 * T((1 + 0.2 * rng.rand(*s0.shape)).astype("float32"))).float()
            w = T(rng.randn(1, 3, P, P).astype("float32"))
            p32, g32 = psf_and_grad(m32, s, w)
            with reference_in_float64():
                p64, g64 = psf_and_grad(m64, s.double(), w.double())
            assert p32.dtype == torch.float32 and p64.dtype == torch.float64 and g64.dtype == torch.float64
            k = f"r{R}_{state}_"
            dst = big if R == 136 else out
            dst.update({k + "s": s, k + "psfbits": bits(p32, p64), k + "psf64": p64, k + "w": w, k + "gradbits": bits(g32, g64), k + "grad64": g64,
                        k + "d_psf": np.float64(rel(p32, p64)), k + "d_grad": np.float64(rel(g32, g64))})
            print(f"g48 {R}->{P} {state}: psf32 vs psf64 {rel(p32, p64):.2e}, grad {rel(g32, g64):.2e}, sum psf32 - 1 = {float(p32.double().sum()) - 1:.2e}")
        if R == 32:
            with torch.no_grad():
                m32.height_map.height_map_sqrt.copy_(s0)
                m64.height_map.height_map_sqrt.copy_(s0.double())
                field = T((rng.randn(1, 3, R, R) + 1j * rng.randn(1, 3, R, R)).astype("complex64"))
                out.update(phase32=m32.height_map.get_phase_profile(), phase64=m64.height_map.get_phase_profile(), field=field,
                           prop32=m32.propagator(field), prop64=m64.propagator(field.to(torch.complex128)))
                b32, b64 = doe_model.build_baseline_profile(m32), doe_model.build_baseline_profile(m64)
                with reference_in_float64():
                    bp64 = m64.get_psf(b64)
                out.update(base32=b32, base64=b64, basepsf32=m32.get_psf(b32), basepsf64=bp64)
                assert out["phase64"].dtype == torch.complex128 and bp64.dtype == torch.float64
    save("g48_doe", **out)
    save("g48_doe_r136", **big)


def e2e_run(model, gt, noise, K, f64):
    from dprox.linop.conv import conv_doe
    cast = (lambda t: t.double()) if f64 else (lambda t: t)
    xv = dp.Variable()
    P, Y = dp.Placeholder(), dp.Placeholder()
    op = conv_doe(xv, P, circular=True)
    n0, n1 = dp.norm1(dp.grad(xv, dim=0)), dp.norm1(dp.grad(xv, dim=1))
    solver = dp.compile(dp.sum_squares(op, Y) + n0 + n1, method="admm", device="cpu")
    solver = dp.specialize(solver, method="unroll", device="cpu", max_iter=K)
    rhos = cast(torch.full((K,), 0.2)).requires_grad_(True)
    lam = cast(torch.full((K,), 0.01))
    model.height_map.height_map_sqrt.grad = None
    psf = model.get_psf()
    y = common.img_psf_conv(cast(gt), psf, circular=True) + cast(noise)
    Y.value, P.value = y, psf
    xo = solver.solve(x0=y, rhos=rhos, lams={n0: lam, n1: lam})
    loss = ((xo - cast(gt)) ** 2).mean()
    loss.backward()
    assert op.psf is not psf and op.psf.grad is not None
    return loss.detach().double(), model.height_map.height_map_sqrt.grad.clone(), rhos.grad.clone(), y.detach(), xo.detach(), op.psf.grad.clone()


def g48_doe_e2e():
    R, P, K = 32, 16, 3
    rng = np.random.RandomState(481)
    m32, m64 = build(R, P, False), build(R, P, True)
    with torch.no_grad():
        m64.height_map.height_map_sqrt.copy_(m32.height_map.height_map_sqrt.double())
    gt = T(rng.rand(2, 3, P, P).astype("float32"))
    noise = T((rng.randn(2, 3, P, P) * 0.01).astype("float32"))
    l32, gs32, gr32, y32, x32, gp32 = e2e_run(m32, gt, noise, K, False)
    with reference_in_float64():
        l64, gs64, gr64, y64, x64, gp64 = e2e_run(m64, gt, noise, K, True)
    assert gs64.dtype == torch.float64 and gr64.dtype == torch.float64 and x64.dtype == torch.float64
    print(f"g48 e2e: loss {float(l32):.6e} / {float(l64):.6e}, g_s {rel(gs32, gs64):.2e}, g_rhos {rel(gr32, gr64):.2e}, x {rel(x32, x64):.2e}")
    save("g48_doe_e2e", s=m32.height_map.height_map_sqrt.detach(), gt=gt, noise=noise, K=K, loss32=l32, loss64=l64, g_s32=gs32, g_s64=gs64,
         g_rhos32=gr32, g_rhos64=gr64, y32=y32, y64=y64, x32=x32, x64=x64, d_g_s=np.float64(rel(gs32, gs64)), d_g_rhos=np.float64(rel(gr32, gr64)),
         d_x=np.float64(rel(x32, x64)), g_psf_term32=gp32, g_psf_term64=gp64, d_g_psf_term=np.float64(rel(gp32, gp64)))


if __name__ == "__main__":
    g48_doe()
    g48_doe_e2e()
