"""TEST INFRASTRUCTURE: the shared cases of the hybrid DOE model (dprox.contrib.optic.doe_hybrid) and of the gradients to explicit
phase profiles, height maps and fields, run by tests/test_doe_hybrid_emul.py (SIMT emulator), tests/test_gpu_doe_hybrid.py (MI355X),
the guarded runs, and, for the parts that need no kernel, tests/test_doe_hybrid_host.py.  Fixtures: tests/golden/g49_doe_hybrid*.npz
(tests/golden/make_golden_doe_hybrid.py: the reference's own models in float32 and float64).

Criteria (the project's own, as tests/doe_cases.py):
  * this backend's float32 result is at most as far (relative l2) from the reference's float64 result as the reference's own float32
    result is (the fixture's stored distance), plus 1e-5 (SLACK);
  * on the wide case (sample_interval = 2.7e-4: a lens phase of thousands of radians, where the reference's float32 `% 2 pi` is 7e-4 rad
    off and so a poor yardstick) the bound is the distance of the fixture's `r64` run -- float64 arithmetic on the float32-rounded
    height_map_sqrt and refractive_len -- from float64, plus 1e-5;
  * each colour of a PSF normalised per channel sums to 1 within 4 float32 ulps of 1;
  * dark samples (outside the aperture) get a gradient of exactly 0;
  * two backward calls give identical bits.
Achieved distances go to the JSON file DPX_DOE_HYBRID_PARITY_OUT names (write_achieved), which is how
profiles/doe_hybrid_parity_achieved.json is produced from a GPU run."""
import json
import os

import numpy as np
import torch

from conftest import load_golden, record, rel_l2
from dprox import _ops as ops
from dprox.contrib import optic
from dprox.contrib.optic import doe_hybrid as hyb

SLACK = 1e-5
ULPS_OF_ONE = 4 * float(np.finfo(np.float32).eps)
CASES = {20: 20, 30: 10, 32: 16, 33: 11, 88: 44}        # R -> P
KINDS = {"half": "half_circular", "circ": "circular"}
STATES = ("init", "pert")
ACHIEVED = {}

_golden = {}


def golden():
    """the fixture files as one dict; a float32 result stored as `<key>bits` comes back as `<key>32` (make_golden_doe_hybrid.py)"""
    if not _golden:
        for f in ("g49_doe_hybrid", "g49_doe_hybrid_r88"):
            _golden.update(load_golden(f))
        for k in [k for k in _golden if k.endswith("bits")]:
            r64 = _golden[k[:-4] + "64"]
            _golden[k[:-4] + "32"] = (r64.astype(np.float32).view(np.int32) + _golden[k].astype(np.int32)).view(np.float32)
    return _golden


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def TC(a, device):
    """a complex tensor from its stored [..., 2] real view"""
    return torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(a))).to(device)


def as_real(t):
    t = t.detach().cpu()
    return (torch.view_as_real(t) if t.is_complex() else t).numpy()


def note(case, what, dist, bound):
    ACHIEVED.setdefault(case, {})[what] = {"rel_l2": float(dist), "bound": float(bound)}
    record(f"doe hybrid {case} {what}", dist, bound)


def aperture(R, half):
    a = 2 * np.arange(R, dtype=np.int64) - (R - 1)
    disc = (a[:, None] ** 2 + a[None, :] ** 2) < (R - 1) ** 2
    return disc & (a[None, :] > 0) if half else disc


def build(R, P, kind, device, s=None, interval=None):
    """the hybrid model of a fixture case: the configuration of the reference's float64 run (the module's own defaults are checked against
    it in tests/test_doe_hybrid_host.py), the case's sizes"""
    g = golden()
    _, d, default_interval, _ = (float(v) for v in g["cfg_scalars"])
    m = hyb.RGBCollimator(d, torch.from_numpy(g["cfg_refractive_idcs"]), torch.from_numpy(g["cfg_wave_lengths"]), P, interval or default_interval, (R, R),
                          aperture_type=KINDS[kind]).to(device)
    if s is not None:
        with torch.no_grad():
            m.height_map.height_map_sqrt.copy_(T(s, device))
    return m


def build_base(R, P, device):
    g = golden()
    d, interval = (float(v) for v in g["base_scalars"])
    return optic.RGBCollimator(d, torch.from_numpy(g["base_refractive_idcs"]), torch.from_numpy(g["base_wave_lengths"]), P, interval, (R, R)).to(device)


def psf_and_grad(m, w):
    m.height_map.height_map_sqrt.grad = None
    psf = m.get_psf()
    (psf * w).sum().backward()
    return psf.detach(), m.height_map.height_map_sqrt.grad.detach().clone()


def check(case, what, ours, ref64, own):
    r = rel_l2(as_real(ours), ref64)
    print(f"doe hybrid {case} {what}: rel l2 {r:.3e}, bound {own + SLACK:.3e} (own {own:.3e})")
    note(case, what, r, own + SLACK)
    assert r <= own + SLACK, (case, what, r, own)


def channel_sums_are_one(psf):
    for c in range(3):
        total = float(psf[0, c].double().sum())
        assert abs(total - 1.0) <= ULPS_OF_ONE, (c, total - 1.0)


def run_parity(device, prefix, label, R, P, kind, state, interval=None, suffix=""):
    g = golden()
    k = f"{prefix}_{state}_"
    m = build(R, P, kind, device, g[k + "s"], interval)
    psf, grad = psf_and_grad(m, T(g[k + "w"], device))
    assert psf.shape == (1, 3, P, P) and psf.dtype == torch.float32 and grad.shape == (1, 1, R, R) and grad.dtype == torch.float32
    assert bool((psf >= 0).all()) and bool(torch.isfinite(grad).all())
    channel_sums_are_one(psf)
    dark = ~torch.from_numpy(aperture(R, kind == "half"))
    assert bool((grad[0, 0].cpu()[dark] == 0).all()) and float(grad.abs().max()) > 0
    assert np.array_equal(m.aperture[0, 0].cpu().numpy() != 0, ~dark.numpy())
    check(label, "psf", psf, g[k + "psf64"], float(g[k + "d_psf" + suffix]))
    check(label, "grad", grad, g[k + "grad64"], float(g[k + "d_grad" + suffix]))
    return m


def case_parity(device, R, kind, state):
    """forward and backward of one fixture case against the reference's float64 run, within the reference's own float32 distance + 1e-5"""
    run_parity(device, f"r{R}_{kind}", f"{R}->{CASES[R]} {kind} {state}", R, CASES[R], kind, state)


def case_wide(device, state):
    """the wide case against the reference's float64 run, within the r64 run's distance + 1e-5"""
    interval = float(golden()["cfg_scalars"][3])
    run_parity(device, "wide", f"wide 32->16 half {state}", 32, 16, "half", state, interval=interval, suffix="_r64")


def case_explicit_profile(device):
    """get_psf(phase_profile) with a complex leaf, base model and hybrid: the psf and the complex gradient; dark samples get exactly 0"""
    g = golden()
    for key, m, half in (("x_base", build_base(32, 16, device), None), ("x_hyb", build(32, 16, "half", device), True)):
        prof = TC(g[key + "_prof"], device).requires_grad_(True)
        psf = m.get_psf(prof)
        (psf * T(g[key + "_w"], device)).sum().backward()
        assert prof.grad.dtype == torch.complex64 and prof.grad.shape == (1, 3, 32, 32)
        dark = ~torch.from_numpy(aperture(32, bool(half)))
        assert bool((prof.grad.cpu()[0][:, dark] == 0).all())
        if half:
            channel_sums_are_one(psf.detach())
        check(f"32->16 explicit profile ({key})", "psf", psf, g[key + "_psf64"], float(g[key + "_d_psf"]))
        check(f"32->16 explicit profile ({key})", "grad", prof.grad, g[key + "_gprof64"], float(g[key + "_d_gprof"]))
        first = prof.grad.clone()
        prof.grad = None
        (m.get_psf(prof) * T(g[key + "_w"], device)).sum().backward()
        assert torch.equal(torch.view_as_real(first), torch.view_as_real(prof.grad))


def case_explicit_height_map(device):
    """the phase profile of a leaf height map: ops.doe_phase with the base model's constants (its HeightMap.get_phase_profile stays forward
    only for an explicit argument), and the hybrid HeightMap.get_phase_profile with its refractive_len"""
    g = golden()
    for key, m, lens in (("x_phb", build_base(32, 16, device), False), ("x_phh", build(32, 16, "half", device), True)):
        hm = T(g[key + "_hm"], device).requires_grad_(True)
        out = m.height_map.get_phase_profile(hm, m.refractive_len) if lens else ops.doe_phase(hm, False, m.wave_lengths, m.refractive_idcs)
        (T(g[key + "_wr"], device) * out.real + T(g[key + "_wi"], device) * out.imag).sum().backward()
        assert out.dtype == torch.complex64 and hm.grad.shape == hm.shape
        check(f"32->16 explicit height map ({key})", "profile", out, g[key + "_out64"], float(g[key + "_d_out"]))
        check(f"32->16 explicit height map ({key})", "grad", hm.grad, g[key + "_ghm64"], float(g[key + "_d_ghm"]))


def case_explicit_field(device):
    """FresnelPropagator on a complex leaf, L = sum(wr Re + wi Im): the output and the gradient to the field"""
    g = golden()
    m = build(32, 16, "half", device)
    field = TC(g["x_prop_field"], device).requires_grad_(True)
    out = m.propagator(field)
    (T(g["x_prop_wr"], device) * out.real + T(g["x_prop_wi"], device) * out.imag).sum().backward()
    check("32->16 explicit field", "propagated", out, g["x_prop_out64"], float(g["x_prop_d_out"]))
    check("32->16 explicit field", "grad", field.grad, g["x_prop_gfield64"], float(g["x_prop_d_gfield"]))


def case_chain(device):
    """the pieces composed as a user with a parametrisation of their own composes them -- get_psf(get_phase_profile(height_map,
    refractive_len)) from a leaf height map -- give the fused path's gradient: d/dh = d/ds / (2 (s + eps)) on the aperture, within the
    sum of the two float32 distances the fixture shows for this case plus 1e-5"""
    g = golden()
    k = "r32_half_pert_"
    m = build(32, 16, "half", device, g[k + "s"])
    w = T(g[k + "w"], device)
    _, gs = psf_and_grad(m, w)
    sv = m.height_map.height_map_sqrt.detach() + torch.tensor(hyb.EPS, dtype=torch.float32, device=device)
    h = (sv * sv).requires_grad_(True)
    (m.get_psf(m.height_map.get_phase_profile(h, m.refractive_len)) * w).sum().backward()
    live = torch.from_numpy(aperture(32, True)).to(device)
    want = (gs[0, 0].double() / (2 * sv[0, 0].double()))[live]
    r = float((h.grad[0, 0].double()[live] - want).norm() / want.norm())
    bound = 2 * float(g[k + "d_grad"]) + SLACK
    note("32->16 half pert", "grad through get_phase_profile + get_psf(profile) vs the fused path", r, bound)
    assert r <= bound, (r, bound)
    assert bool((h.grad[0, 0][~live] == 0).all())


def case_deterministic(device, R=88):
    g, P = golden(), CASES[R]
    k = f"r{R}_half_pert_"
    m, w = build(R, P, "half", device, g[k + "s"]), T(g[k + "w"], device)
    a, b = psf_and_grad(m, w), psf_and_grad(m, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[1].abs().max()) > 0


def case_baseline_and_no_grad(device):
    """build_baseline_profile (explicit height map, no lens term) through get_psf: every channel sums to 1; a call that needs no gradient
    keeps no field"""
    m = build(32, 16, "half", device)
    ctx = m._context()
    with torch.no_grad():
        base = hyb.build_baseline_profile(m)
        psf = m.get_psf(base)
        assert ctx.last_ws_bytes == ctx.ws_bytes(False)
        psf2 = m.get_psf()
    assert base.dtype == torch.complex64 and base.shape == (1, 3, 32, 32) and psf.grad_fn is None and psf2.grad_fn is None
    channel_sums_are_one(psf)
    channel_sums_are_one(psf2)
    assert m.get_psf().grad_fn is not None and ctx.last_ws_bytes == ctx.ws_bytes(True)


def case_argument_errors(device):
    """the new entry points' argument checks: DPX_ERR_ARG surfaces as DpxError naming the argument, nothing is launched"""
    import ctypes
    from dprox import _backend as be
    L, p = be.lib(), be.ptr
    m = build(32, 16, "half", device)
    ctx = m._context()
    s = m.height_map.height_map_sqrt.detach()
    psf, gs = torch.empty(1, 3, 16, 16, device=device), torch.empty_like(s)
    ws = torch.zeros(ctx.ws_bytes(True), dtype=torch.uint8, device=device)
    prof = torch.zeros(1, 3, 32, 32, dtype=torch.complex64, device=device)
    gprof = torch.empty_like(prof)
    phi = m.refractive_len

    def opts(eps=1e-7, kind=1, norm=1, phi_=phi, gs_=None, gf=None):
        return ctypes.byref(be.DoeOpts(eps, kind, norm, 0, None if phi_ is None else phi_.data_ptr(), None if gs_ is None else gs_.data_ptr(),
                                       None if gf is None else gf.data_ptr()))
    neg = (ctypes.c_double * 3)(4.6e-7, -1.0, 6.4e-7)
    fwd = [p(s), None, ctx.wl, ctx.ri, p(psf), p(ctx.H), p(ctx.table), 32, 16, 1, 0, opts(), p(ws), be.stream()]
    bwd = [p(psf), p(psf), p(s), ctx.wl, ctx.ri, p(ctx.H), p(ctx.table), 32, 16, 0, opts(gs_=gs), p(ws), be.stream()]
    pbw = [p(prof), p(gprof), p(ctx.H), p(ctx.table), 32, 0, p(ws), be.stream()]
    phx = [p(s), 1, ctypes.c_float(1e-7), p(phi), ctx.wl, ctx.ri, p(prof), 32 * 32, be.stream()]
    phb = [p(prof), p(s), 1, ctypes.c_float(1e-7), p(phi), ctx.wl, ctx.ri, p(gs), 32 * 32, be.stream()]
    for name, good, cases in (
            ("dpx_doe_psf_ex", fwd, ((0, None, "null"), (4, None, "null"), (12, None, "null"), (11, opts(kind=2), "aperture_kind"), (11, opts(norm=3), "norm_mode"),
                                     (11, opts(eps=-1.0), "eps"), (8, 5, "P=5"), (7, 2, "R=2"), (10, 99, "cols_per_wg"), (2, neg, "wave length"))),
            ("dpx_doe_psf_backward_ex", bwd, ((0, None, "null"), (1, None, "null"), (2, None, "null"), (10, None, "null"), (11, None, "null"),
                                              (10, opts(), "null"), (10, opts(gs_=gs, gf=gprof), "both"), (10, opts(gs_=s), "in-place"),
                                              (10, opts(kind=-1, gs_=gs), "aperture_kind"), (8, 7, "P=7"), (9, 99, "cols_per_wg"), (3, None, "null"))),
            ("dpx_doe_propagate_backward", pbw, ((0, None, "null"), (1, None, "null"), (6, None, "null"), (1, p(prof), "in-place"), (4, 3, "R=3"),
                                                 (5, 99, "cols_per_wg"))),
            ("dpx_doe_phase_ex", phx, ((0, None, "null"), (6, None, "null"), (7, 0, "n=0"), (2, ctypes.c_float(-1.0), "eps"), (4, neg, "wave length"))),
            ("dpx_doe_phase_backward", phb, ((0, None, "null"), (1, None, "null"), (7, None, "null"), (7, p(s), "in-place"), (8, 0, "n=0"),
                                             (3, ctypes.c_float(-1.0), "eps"), (5, neg, "wave length")))):
        for idx, bad, msg in cases:
            args = list(good)
            args[idx] = bad
            try:
                L.call(name, *args)
            except be.DpxError as e:
                assert "(-1)" in str(e) and msg in str(e), (name, idx, msg, str(e))
            else:
                raise AssertionError(f"{name} accepted argument {idx} = {bad}")
        L.call(name, *good)              # ... and the unchanged argument list runs
    # a NULL options block is the base model: the same bits as dpx_doe_psf
    a, b = torch.empty_like(psf), torch.empty_like(psf)
    L.call("dpx_doe_psf", p(s), None, ctx.wl, ctx.ri, p(a), p(ctx.H), p(ctx.table), 32, 16, 0, 0, p(ws), be.stream())
    L.call("dpx_doe_psf_ex", p(s), None, ctx.wl, ctx.ri, p(b), p(ctx.H), p(ctx.table), 32, 16, 0, 0, None, p(ws), be.stream())
    assert torch.equal(a, b)


def write_achieved():
    """the measured distances of the cases run so far -> the JSON file the environment variable DPX_DOE_HYBRID_PARITY_OUT names; without
    the variable nothing is written"""
    path = os.environ.get("DPX_DOE_HYBRID_PARITY_OUT")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ACHIEVED, f, indent=1, sort_keys=True)


# the runs of tests/test_gpu_guard_doe_hybrid.py on guarded workspaces: case, arguments, the size queries whose buffers they use
GUARDED_RUNS = {
    "doe_hybrid_parity_30_half_pert": (case_parity, (30, "half", "pert"), ("dpx_doe_ws_bytes", "dpx_doe_propagator_bytes", "dpx_fft_table_bytes")),
    "doe_hybrid_parity_33_circ_pert": (case_parity, (33, "circ", "pert"), ("dpx_doe_ws_bytes", "dpx_doe_propagator_bytes", "dpx_fft_table_bytes")),
    "doe_hybrid_explicit_profile": (case_explicit_profile, (), ("dpx_doe_ws_bytes", "dpx_doe_propagator_bytes")),
    "doe_hybrid_explicit_field": (case_explicit_field, (), ("dpx_doe_ws_bytes", "dpx_doe_propagator_bytes")),
    "doe_hybrid_baseline_and_no_grad": (case_baseline_and_no_grad, (), ("dpx_doe_ws_bytes",)),
}
