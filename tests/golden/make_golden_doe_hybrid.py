#!/usr/bin/env python
"""Golden vectors of the hybrid DOE model and of the gradients to explicit arguments -- runs ONLY in the build container (needs the
reference checkout).

As in make_golden_doe.py the reference's ``common.py``, ``doe_model.py`` and ``doe_model_hybrid.py`` are loaded by file path under a
synthetic package name -- twice: as shipped (float32), and under ``torch.set_default_dtype(torch.float64)``, where the module-level
``wvls`` / ``RI`` and with them ``DOEModelConfig`` come out in float64 (the yardstick).  Every case runs in both on identical parameter
values.  A float32 result is stored as `<key>bits` (the integer difference between its bit pattern and that of its float64 twin
rounded to float32; complex results as [..., 2] real views), tests/doe_hybrid_cases.py:golden adds it back as `<key>32`.

g49_doe_hybrid.npz / g49_doe_hybrid_r88.npz, per case R -> P in (20 -> 20, 30 -> 10, 32 -> 16, 33 -> 11, 88 -> 44), aperture kind in
(half = 'half_circular', circ = 'circular') and state in (init = the Fresnel initialisation, pert = init * (1 + 0.2 rand), seeded):
  r<R>_<kind>_<state>_s / _psf64 / _psfbits / _w / _grad64 / _gradbits / _d_psf / _d_grad     as in g48_doe.npz
The integer aperture rules -- (2 i - (R-1))^2 + (2 j - (R-1))^2 < (R-1)^2, and 2 j - (R-1) > 0 on top for the half -- are asserted
against the reference's float32 AND float64 apertures at every size stored and at 1536.
wide_<state>_*: 32 -> 16, half-circular, sample_interval = 2.7e-4 (the lens phase is thousands of radians; the reference's float32
`% 2 pi` of it is 7e-4 rad off), with a third run `r64`: float64 arithmetic on the float32-rounded s and refractive_len, stored as
_d_psf_r64 / _d_grad_r64 -- the bound of that case.  r32_reflen64, wide_reflen64, r32_init64, wide_init64: the float64 model's
refractive_len and Fresnel initialisation (what the host tables are checked against).
Explicit arguments at 32 -> 16 (x_*): a seeded complex phase profile through get_psf of the base model (x_base_*) and of the hybrid,
half-circular (x_hyb_*): prof, w, psf, gprof (the base model is built as make_golden_doe.py builds it: its float64 twin takes the
configuration's float32 tensors widened);  get_phase_profile(height_map) of the base HeightMap (x_phb_*) and of the hybrid one
with its refractive_len (x_phh_*): hm, wr, wi, out, ghm for L = sum(wr Re + wi Im);  the propagator on a seeded field (x_prop_*):
field, wr, wi, out, gfield.

    python tests/golden/make_golden_doe_hybrid.py
"""
import importlib.util
import os
import runpy
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch = G["np"], G["torch"]
T, save, reference_in_float64, REF = G["T"], G["save"], G["reference_in_float64"], G["REF"]

CASES = ((20, 20), (30, 10), (32, 16), (33, 11), (88, 44))
KINDS = (("half", "half_circular"), ("circ", "circular"))
WIDE_INTERVAL = 2.7e-4


def load_optic(pkg_name):
    pkg = types.ModuleType(pkg_name)
    pkg.__path__ = [os.path.join(REF, "dprox", "contrib", "optic")]
    sys.modules[pkg_name] = pkg
    mods = {}
    for name in ("common", "doe_model", "doe_model_hybrid"):
        spec = importlib.util.spec_from_file_location(f"{pkg_name}.{name}", os.path.join(pkg.__path__[0], name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods


M32 = load_optic("ref_optic")
torch.set_default_dtype(torch.float64)
try:
    M64 = load_optic("ref_optic64")
finally:
    torch.set_default_dtype(torch.float32)
CFG32, CFG64 = M32["doe_model_hybrid"].DOEModelConfig(), M64["doe_model_hybrid"].DOEModelConfig()
assert CFG32.wave_lengths.dtype == torch.float32 and CFG64.wave_lengths.dtype == torch.float64 and CFG64.refractive_idcs.dtype == torch.float64
BASE32 = M32["doe_model"].DOEModelConfig()


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a.astype(b.dtype) - b).ravel()) / np.linalg.norm(b.ravel()))


def real_view(t):
    t = t.detach()
    return torch.view_as_real(t).numpy() if t.is_complex() else t.numpy()


def bits(a32, a64):
    a32, near = real_view(a32), real_view(a64).astype(np.float32)
    return a32.view(np.int32).astype(np.int64) - near.view(np.int32).astype(np.int64)


def pair(out, key, a32, a64):
    """one result <case>_<what> in both precisions: <key>64, <key>bits and the reference's own distance <case>_d_<what>"""
    case, what = key.rsplit("_", 1)
    out[key + "64"], out[key + "bits"] = real_view(a64), bits(a32, a64)
    out[f"{case}_d_{what}"] = np.float64(rel(real_view(a32), real_view(a64)))


def build(R, P, kind, f64, interval=None):
    cfg, mod = (CFG64, M64) if f64 else (CFG32, M32)
    if f64:
        torch.set_default_dtype(torch.float64)
    try:
        return mod["doe_model_hybrid"].RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs, cfg.wave_lengths, P, interval or cfg.sample_interval, (R, R),
                                                     aperture_type=kind)
    finally:
        torch.set_default_dtype(torch.float32)


def build_base(R, P, f64):
    """the base model as make_golden_doe.py builds it: in float64 with the configuration's float32 tensors widened"""
    cfg, mod = BASE32, (M64 if f64 else M32)
    if f64:
        torch.set_default_dtype(torch.float64)
    try:
        return mod["doe_model"].RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs.to(torch.get_default_dtype()),
                                              cfg.wave_lengths.to(torch.get_default_dtype()), P, cfg.sample_interval, (R, R))
    finally:
        torch.set_default_dtype(torch.float32)


def integer_aperture(R, half):
    a = 2 * np.arange(R, dtype=np.int64) - (R - 1)
    disc = (a[:, None] ** 2 + a[None, :] ** 2) < (R - 1) ** 2
    return disc & (a[None, :] > 0) if half else disc


def assert_apertures(R, interval=None):
    for short, kind in KINDS:
        for f64 in (False, True):
            m = build(R, R, kind, f64, interval)
            assert np.array_equal(m.aperture[0, 0].numpy() != 0, integer_aperture(R, short == "half")), f"aperture rule at {R}, {kind}, f64={f64}"


def psf_and_grad(model, s, w):
    with torch.no_grad():
        model.height_map.height_map_sqrt.copy_(s)
    model.height_map.height_map_sqrt.grad = None
    psf = model.get_psf()
    (psf * w).sum().backward()
    return psf.detach(), model.height_map.height_map_sqrt.grad.clone()


def run_states(out, prefix, m32, m64, rng, P, r64=False):
    s0 = m32.height_map.height_map_sqrt.detach().clone()
    for state in ("init", "pert"):
        s = s0 if state == "init" else (s0 * T((1 + 0.2 * rng.rand(*s0.shape)).astype("float32"))).float()
        w = T(rng.randn(1, 3, P, P).astype("float32"))
        p32, g32 = psf_and_grad(m32, s, w)
        with reference_in_float64():
            p64, g64 = psf_and_grad(m64, s.double(), w.double())
        assert p32.dtype == torch.float32 and p64.dtype == torch.float64 and g64.dtype == torch.float64
        k = f"{prefix}_{state}_"
        out.update({k + "s": s, k + "w": w})
        pair(out, k + "psf", p32, p64)
        pair(out, k + "grad", g32, g64)
        msg = f"g49 {k}: psf32 vs psf64 {rel(p32, p64):.2e}, grad {rel(g32, g64):.2e}"
        if r64:
            keep = m64.refractive_len
            m64.refractive_len = keep.float().double()
            with reference_in_float64():
                pr, gr = psf_and_grad(m64, s.double(), w.double())
            m64.refractive_len = keep
            out[k + "d_psf_r64"], out[k + "d_grad_r64"] = np.float64(rel(pr, p64)), np.float64(rel(gr, g64))
            msg += f"; r64: psf {rel(pr, p64):.2e}, grad {rel(gr, g64):.2e}; refractive_len32 off by {float((m32.refractive_len.double() - keep).abs().max()):.1e} rad"
        print(msg)


def seeded_complex(rng, *shape):
    return T((rng.randn(*shape) + 1j * rng.randn(*shape)).astype("complex64"))


def explicit(out, rng):
    R, P = 32, 16
    # get_psf(phase_profile): a complex leaf through the base model and the hybrid (half-circular, one sum per channel)
    for key, m32, m64 in (("x_base", build_base(R, P, False), build_base(R, P, True)),
                          ("x_hyb", build(R, P, "half_circular", False), build(R, P, "half_circular", True))):
        prof, w = seeded_complex(rng, 1, 3, R, R), T(rng.randn(1, 3, P, P).astype("float32"))
        res = []
        for m, p, ww in ((m32, prof.clone(), w), (m64, prof.to(torch.complex128), w.double())):
            p.requires_grad_(True)
            with reference_in_float64():
                psf = m.get_psf(p)
                (psf * ww).sum().backward()
            res.append((psf.detach(), p.grad.clone()))
        assert res[1][0].dtype == torch.float64 and res[1][1].dtype == torch.complex128
        out.update({key + "_prof": real_view(prof), key + "_w": w})
        pair(out, key + "_psf", res[0][0], res[1][0])
        pair(out, key + "_gprof", res[0][1], res[1][1])
        print(f"g49 {key}: psf {out[key + '_d_psf']:.2e}, gprof {out[key + '_d_gprof']:.2e}")
    # get_phase_profile(height_map): the gradient to an explicit height map, without and with the lens term
    for key, m32, m64, lens in (("x_phb", build_base(R, P, False), build_base(R, P, True), False),
                                ("x_phh", build(R, P, "half_circular", False), build(R, P, "half_circular", True), True)):
        hm = T((1.2e-6 * rng.rand(1, 1, R, R)).astype("float32"))
        wr, wi = T(rng.randn(1, 3, R, R).astype("float32")), T(rng.randn(1, 3, R, R).astype("float32"))
        res = []
        for m, h, cast in ((m32, hm.clone(), lambda t: t), (m64, hm.double(), lambda t: t.double())):
            h.requires_grad_(True)
            o = m.height_map.get_phase_profile(h, m.refractive_len) if lens else m.height_map.get_phase_profile(h)
            (cast(wr) * o.real + cast(wi) * o.imag).sum().backward()
            res.append((o.detach(), h.grad.clone()))
        assert res[1][0].dtype == torch.complex128 and res[1][1].dtype == torch.float64
        out.update({key + "_hm": hm, key + "_wr": wr, key + "_wi": wi})
        pair(out, key + "_out", res[0][0], res[1][0])
        pair(out, key + "_ghm", res[0][1], res[1][1])
        print(f"g49 {key}: out {out[key + '_d_out']:.2e}, ghm {out[key + '_d_ghm']:.2e}")
    # the propagator on a seeded field
    m32, m64 = build(R, P, "half_circular", False), build(R, P, "half_circular", True)
    field = seeded_complex(rng, 1, 3, R, R)
    wr, wi = T(rng.randn(1, 3, R, R).astype("float32")), T(rng.randn(1, 3, R, R).astype("float32"))
    res = []
    for m, f, cast in ((m32, field.clone(), lambda t: t), (m64, field.to(torch.complex128), lambda t: t.double())):
        f.requires_grad_(True)
        o = m.propagator(f)
        (cast(wr) * o.real + cast(wi) * o.imag).sum().backward()
        res.append((o.detach(), f.grad.clone()))
    assert res[1][0].dtype == torch.complex128 and res[1][1].dtype == torch.complex128
    out.update(x_prop_field=real_view(field), x_prop_wr=wr, x_prop_wi=wi)
    pair(out, "x_prop_out", res[0][0], res[1][0])
    pair(out, "x_prop_gfield", res[0][1], res[1][1])
    print(f"g49 x_prop: out {out['x_prop_d_out']:.2e}, gfield {out['x_prop_d_gfield']:.2e}")


def g49():
    out = {"cfg_refractive_idcs": CFG64.refractive_idcs.numpy(), "cfg_wave_lengths": CFG64.wave_lengths.numpy(),
           "cfg_refractive_idcs32": CFG32.refractive_idcs.numpy(), "cfg_wave_lengths32": CFG32.wave_lengths.numpy(),
           "cfg_scalars": np.array([CFG32.aperture_diameter, CFG32.sensor_distance, CFG32.sample_interval, WIDE_INTERVAL], np.float64),
           "cfg_ints": np.array([CFG32.num_steps, CFG32.patch_size, CFG32.wave_resolution[0], CFG32.wave_resolution[1], int(CFG32.circular)], np.int64),
           "cfg_aperture_type": np.array(CFG32.aperture_type), "cases": np.array(CASES, np.int64),
           "base_refractive_idcs": BASE32.refractive_idcs.numpy(), "base_wave_lengths": BASE32.wave_lengths.numpy(),
           "base_scalars": np.array([BASE32.sensor_distance, BASE32.sample_interval], np.float64)}
    assert_apertures(1536)
    rng = np.random.RandomState(490)
    big = {}
    for R, P in CASES:
        assert_apertures(R)
        for short, kind in KINDS:
            m32, m64 = build(R, P, kind, False), build(R, P, kind, True)
            assert m64.height_map.height_map_sqrt.dtype == torch.float64 and m64.propagator.H.dtype == torch.complex128
            assert m64.refractive_len.dtype == torch.float64
            run_states(big if R == 88 else out, f"r{R}_{short}", m32, m64, rng, P)
            if R == 32 and short == "half":
                out.update(r32_reflen64=m64.refractive_len, r32_init64=build(R, P, kind, True).height_map.height_map_sqrt.detach())
    assert_apertures(32, WIDE_INTERVAL)
    m32, m64 = build(32, 16, "half_circular", False, WIDE_INTERVAL), build(32, 16, "half_circular", True, WIDE_INTERVAL)
    out.update(wide_reflen64=m64.refractive_len, wide_init64=m64.height_map.height_map_sqrt.detach().clone())
    run_states(out, "wide", m32, m64, rng, 16, r64=True)
    explicit(out, rng)
    save("g49_doe_hybrid", **out)
    save("g49_doe_hybrid_r88", **big)


if __name__ == "__main__":
    g49()
