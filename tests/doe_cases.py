"""TEST INFRASTRUCTURE: the shared cases of the DOE wave-optics model (dprox.contrib.optic; csrc/dpx_doe.hip + the dpx_doe_* kernels of
csrc/dpx_fft.hip), run by tests/test_doe_emul.py (SIMT emulator), tests/test_gpu_doe.py (MI355X) and, for the parts that need no kernel,
tests/test_doe_host.py.  Fixtures: tests/golden/g48_doe*.npz (tests/golden/make_golden_doe.py: the reference's own model in float32 and
float64).

Criteria (the project's own: README "parity", tests/minres_cases.py):
  * `restate` -- a float64 restatement of the model's equations in this file -- is pinned to the reference's float64 outputs at
    <= 1e-12 relative l2 (RESTATE_TOL);
  * this backend's float32 result is at most as far from the reference's float64 result as the reference's own float32 result is
    (the fixture's stored distance), plus 1e-5 (SLACK): PSFs, gradients and the end-to-end gradients alike.
Achieved distances go to the JSON file DPX_DOE_PARITY_OUT names (write_achieved), which is how profiles/doe_parity_achieved.json is
produced from a GPU run."""
import json
import os

import numpy as np
import torch

import dprox as dp
from conftest import load_golden, record, rel_l2
from dprox import _ops as ops
from dprox.contrib import optic

SLACK = 1e-5
RESTATE_TOL = 1e-12
CASES = {20: 20, 30: 10, 32: 16, 88: 44, 136: 68}        # R -> P
STATES = ("init", "pert")
ACHIEVED = {}

_golden = {}


def golden():
    """the fixture files as one dict; a float32 result stored as `<key>bits` comes back as `<key>32` (make_golden_doe.py)"""
    if not _golden:
        for f in ("g48_doe", "g48_doe_r136"):
            _golden.update(load_golden(f))
        for k in [k for k in _golden if k.endswith("bits")]:
            r64 = _golden[k[:-4] + "64"]
            _golden[k[:-4] + "32"] = (r64.astype(np.float32).view(np.int32) + _golden[k].astype(np.int32)).view(np.float32)
    return _golden


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def note(case, what, dist, bound):
    ACHIEVED.setdefault(case, {})[what] = {"rel_l2": float(dist), "bound": float(bound)}
    record(f"doe {case} {what}", dist, bound)


def config():
    """(wave lengths, refractive indices) as float64 arrays widened exactly from the fixture's float32 values, sensor distance, interval"""
    g = golden()
    _, d, interval = (float(v) for v in g["cfg_scalars"])
    return g["cfg_wave_lengths"].astype(np.float64), g["cfg_refractive_idcs"].astype(np.float64), d, interval


# ---- the float64 restatement of the model (section "The computation" of the design): torch, any device, differentiable ------------
def aperture(R):
    a = 2 * np.arange(R, dtype=np.int64) - (R - 1)
    return (a[:, None] ** 2 + a[None, :] ** 2) < (R - 1) ** 2


def transfer_function(R, device="cpu"):
    """H [3, M, M] complex128, WITHOUT the 1 / M^2 of the inverse transform"""
    wl, _, d, interval = config()
    M = R + 2 * (R // 4)
    fx = np.fft.ifftshift((np.arange(M) - (M - 1) / 2) / (interval * M))
    ss = fx[:, None] ** 2 + fx[None, :] ** 2
    return torch.from_numpy(np.exp(-1j * np.pi * d * wl[:, None, None] * ss[None])).to(device)


def restate_field(u, R, device="cpu"):
    p = R // 4
    U = torch.nn.functional.pad(u, [p, p, p, p])
    return torch.fft.ifft2(torch.fft.fft2(U) * transfer_function(R, device))[..., p:p + R, p:p + R]


def restate_psf_of_field(u, R, P, device="cpu"):
    f = R // P
    w = restate_field(u, R, device)
    q = (w.real ** 2 + w.imag ** 2).reshape(3, P, f, P, f).mean(dim=(2, 4))
    return (q / q.sum())[None]


def restate(s, R, P, device="cpu"):
    """psf [1, 3, P, P] float64 from s = height_map_sqrt (a float64 tensor [1, 1, R, R] on `device`, may require a gradient)"""
    wl, ri, _, _ = config()
    k = torch.from_numpy(2 * np.pi / wl * (ri - 1)).to(device)[:, None, None]
    phi = k * s[0] ** 2
    u = torch.from_numpy(aperture(R)).to(device) * torch.exp(1j * phi)
    return restate_psf_of_field(u, R, P, device)


def restate_with_grad(s_np, w_np, R, P, device="cpu"):
    s = T(np.asarray(s_np, np.float64), device).requires_grad_(True)
    psf = restate(s, R, P, device)
    (psf * T(np.asarray(w_np, np.float64), device)).sum().backward()
    return psf.detach(), s.grad.detach()


def case_restatement(R, state):
    g, P = golden(), CASES[R]
    k = f"r{R}_{state}_"
    psf, grad = restate_with_grad(g[k + "s"], g[k + "w"], R, P)
    for what, ours, ref in (("psf", psf, g[k + "psf64"]), ("grad", grad, g[k + "grad64"])):
        r = rel_l2(ours.numpy(), ref)
        assert r <= RESTATE_TOL, (R, state, what, r)


def case_restatement_extras():
    g = golden()
    wl, ri, _, _ = config()
    s = T(g["r32_init_s"].astype(np.float64), "cpu")
    phase = torch.exp(1j * torch.from_numpy(2 * np.pi / wl * (ri - 1))[:, None, None] * s[0] ** 2)[None]
    assert rel_l2(phase.numpy(), g["phase64"]) <= RESTATE_TOL
    assert rel_l2(restate_field(T(g["field"], "cpu")[0].to(torch.complex128), 32).numpy(), g["prop64"][0]) <= RESTATE_TOL
    bp = restate_psf_of_field(torch.from_numpy(aperture(32)) * T(g["base64"], "cpu")[0], 32, 16)
    assert rel_l2(bp.numpy(), g["basepsf64"]) <= RESTATE_TOL


# ---- this backend ---------------------------------------------------------------------------------------------------------------
def build(R, P, device, s=None):
    g = golden()
    _, d, interval = (float(v) for v in g["cfg_scalars"])
    m = optic.RGBCollimator(d, torch.from_numpy(g["cfg_refractive_idcs"]), torch.from_numpy(g["cfg_wave_lengths"]), P, interval, (R, R)).to(device)
    if s is not None:
        with torch.no_grad():
            m.height_map.height_map_sqrt.copy_(T(s, device))
    return m


def psf_and_grad(m, w):
    m.height_map.height_map_sqrt.grad = None
    psf = m.get_psf()
    (psf * w).sum().backward()
    return psf.detach(), m.height_map.height_map_sqrt.grad.detach().clone()


def case_parity(device, R, state):
    """forward and backward of one fixture case against the reference's float64 run, within the reference's own float32 distance + 1e-5;
    psf >= 0, sum psf = 1 within the reference float32 run's own deviation + 1e-6"""
    g, P = golden(), CASES[R]
    k = f"r{R}_{state}_"
    m = build(R, P, device, g[k + "s"])
    psf, grad = psf_and_grad(m, T(g[k + "w"], device))
    assert psf.shape == (1, 3, P, P) and psf.dtype == torch.float32 and grad.shape == (1, 1, R, R)
    assert bool((psf >= 0).all()) and bool(torch.isfinite(grad).all())
    dev_ref = abs(float(g[k + "psf32"].astype(np.float64).sum()) - 1.0)
    assert abs(float(psf.double().sum()) - 1.0) <= dev_ref + 1e-6
    for what, ours, ref, own in (("psf", psf, g[k + "psf64"], float(g[k + "d_psf"])), ("grad", grad, g[k + "grad64"], float(g[k + "d_grad"]))):
        r = rel_l2(ours.cpu().numpy(), ref)
        note(f"{R}->{P} {state}", what, r, own + SLACK)
        assert r <= own + SLACK, (R, state, what, r, own)


def case_phase_baseline_propagator(device):
    """get_phase_profile, build_baseline_profile and the psf it gives (the explicit-phase_profile form), the propagator on a field"""
    g = golden()
    m = build(32, 16, device, g["r32_init_s"])
    with torch.no_grad():
        phase, base = m.height_map.get_phase_profile(), optic.build_baseline_profile(m)
        prop = m.propagator(T(g["field"], device))
        bpsf = m.get_psf(base)
        bpsf_ref_profile = m.get_psf(T(g["base32"], device))
    assert phase.dtype == torch.complex64 and phase.shape == (1, 3, 32, 32) and m.propagator.H.shape == (1, 3, 48, 48)
    assert m.propagator.Mpad == 8 and m.propagator.Npad == 8
    for what, ours, r32, r64 in (("phase", phase, "phase32", "phase64"), ("baseline", base, "base32", "base64"), ("propagator", prop, "prop32", "prop64"),
                                 ("baseline psf", bpsf, "basepsf32", "basepsf64"), ("baseline psf (fixture profile)", bpsf_ref_profile, "basepsf32", "basepsf64")):
        own = rel_l2(g[r32], g[r64])
        r = rel_l2(ours.cpu().numpy(), g[r64])
        note("32->16 extras", what, r, own + SLACK)
        assert r <= own + SLACK, (what, r, own)
    # the propagator's table: H with the inverse transform's 1 / M^2 folded in, evaluated in float64
    H = m.propagator.H.cpu().numpy()[0].astype(np.complex128) * 48 ** 2
    assert rel_l2(H, transfer_function(32).numpy()) <= 2e-7


def case_deterministic(device, R=136):
    g, P = golden(), CASES[R]
    k = f"r{R}_pert_"
    m, w = build(R, P, device, g[k + "s"]), T(g[k + "w"], device)
    a, b = psf_and_grad(m, w), psf_and_grad(m, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[1].abs().max()) > 0


def case_no_grad_stores_no_field(device):
    g = golden()
    m = build(32, 16, device, g["r32_init_s"])
    ctx = m._context()
    small, big = ctx.ws_bytes(False), ctx.ws_bytes(True)
    assert big - small == 3 * 32 * 32 * 8
    with torch.no_grad():
        psf = m.get_psf()
    assert psf.grad_fn is None and ctx.last_ws_bytes == small
    psf = m.get_psf()
    assert psf.grad_fn is not None and ctx.last_ws_bytes == big
    m.height_map.height_map_sqrt.requires_grad_(False)
    assert m.get_psf().grad_fn is None and ctx.last_ws_bytes == small


def case_argument_errors(device):
    """the C ABI's own argument checks: DPX_ERR_ARG surfaces as DpxError naming the argument, the size queries answer 0"""
    import ctypes
    from dprox import _backend as be
    L, p = be.lib(), be.ptr
    g = golden()
    m = build(32, 16, device, g["r32_init_s"])
    ctx = m._context()
    assert L.query("dpx_doe_ws_bytes", 32, 5, 0) == 0 and L.query("dpx_doe_ws_bytes", 2, 1, 0) == 0 and L.query("dpx_doe_propagator_bytes", 3) == 0
    assert L.query("dpx_doe_ws_bytes", 20000, 20000, 0) == 0                       # a row beyond the LDS-resident transforms
    assert L.query("dpx_doe_propagator_bytes", 32) == 3 * 48 * 48 * 8
    widest = L.query("dpx_doe_cols_per_wg", 32, 1)
    assert 1 <= L.query("dpx_doe_cols_per_wg", 32, 0) <= widest <= 16
    s = m.height_map.height_map_sqrt.detach()
    psf, gs = torch.empty(1, 3, 16, 16, device=device), torch.empty_like(s)
    ws = torch.zeros(ctx.ws_bytes(True), dtype=torch.uint8, device=device)
    prof = torch.zeros(1, 3, 32, 32, dtype=torch.complex64, device=device)
    neg = (ctypes.c_double * 3)(4.6e-7, -1.0, 6.4e-7)
    fwd = [p(s), None, ctx.wl, ctx.ri, p(psf), p(ctx.H), p(ctx.table), 32, 16, 1, 0, p(ws), be.stream()]
    bwd = [p(psf), p(psf), p(s), ctx.wl, ctx.ri, p(gs), p(ctx.H), p(ctx.table), 32, 16, 0, p(ws), be.stream()]
    prop = [p(prof), p(prof.clone()), p(ctx.H), p(ctx.table), 32, 0, p(ws), be.stream()]
    phase = [p(s), 1, ctx.wl, ctx.ri, p(prof), 32 * 32, be.stream()]
    init = [p(torch.empty_like(ctx.H)), 32, ctypes.c_double(0.015), ctypes.c_double(2e-6), ctx.wl, be.stream()]
    for name, good, cases in (
            ("dpx_doe_psf", fwd, ((0, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"), (11, None, "null"), (1, p(prof), "keep_field"),
                                  (8, 5, "P=5"), (7, 2, "R=2"), (10, widest + 1, "cols_per_wg"), (10, -1, "cols_per_wg"), (2, None, "null"), (2, neg, "wave length"))),
            ("dpx_doe_psf_backward", bwd, ((0, None, "null"), (1, None, "null"), (2, None, "null"), (5, None, "null"), (11, None, "null"), (5, p(s), "in-place"),
                                           (9, 7, "P=7"), (10, 99, "cols_per_wg"), (3, None, "null"))),
            ("dpx_doe_propagate", prop, ((0, None, "null"), (1, None, "null"), (6, None, "null"), (4, 3, "R=3"), (5, 99, "cols_per_wg"))),
            ("dpx_doe_phase", phase, ((0, None, "null"), (4, None, "null"), (5, 0, "n=0"), (2, neg, "wave length"))),
            ("dpx_doe_propagator_init", init, ((0, None, "null"), (1, 3, "R=3"), (3, ctypes.c_double(0.0), "sample interval"), (4, None, "null")))):
        for idx, bad, msg in cases:
            args = list(good)
            args[idx] = bad
            try:
                L.call(name, *args)
            except be.DpxError as e:
                assert "(-1)" in str(e) and msg in str(e), (name, idx, msg, str(e))
            else:
                raise AssertionError(f"{name} accepted argument {idx} = {bad}")
    try:                                 # the host layer names a wavefront whose padded row no workgroup can hold
        ops.doe_context(20000, 20000, 0.015, 2e-6, g["cfg_wave_lengths"], g["cfg_refractive_idcs"], device)
    except NotImplementedError as e:
        assert "LDS-resident" in str(e), str(e)
    else:
        raise AssertionError("a 30000-sample padded row was accepted")
    L.call("dpx_doe_psf", *fwd)          # ... and the unchanged argument lists run
    L.call("dpx_doe_psf_backward", *bwd)


def e2e_run(device, m, gt, noise, K, detach_kernel):
    """one step of the example: psf = model.get_psf(), y = img_psf_conv(scene, psf) + noise, unrolled ADMM on conv_doe + TV, MSE loss,
    backward.  detach_kernel: the data term's Placeholder gets a detached leaf copy of the psf -- what the reference's conv_doe does with
    a Placeholder's value (it wraps it in an nn.Parameter of its own), so that height_map_sqrt's gradient runs through y and x0 alone and
    the gradient to the data term's kernel lands in the copy's .grad"""
    xv = dp.Variable()
    Pp, Y = dp.Placeholder(), dp.Placeholder()
    n0, n1 = dp.norm1(dp.grad(xv, dim=0)), dp.norm1(dp.grad(xv, dim=1))
    fns = dp.sum_squares(dp.conv_doe(xv, Pp, circular=True), Y) + n0 + n1
    solver = dp.compile(fns, method="admm", device=device)
    solver = dp.specialize(solver, method="unroll", device=device, max_iter=K)
    rhos = torch.full((K,), 0.2, requires_grad=True, device=device)
    lam = torch.full((K,), 0.01, device=device)
    m.height_map.height_map_sqrt.grad = None
    psf = m.get_psf()
    kernel = psf.detach().clone().requires_grad_(True) if detach_kernel else psf
    y = optic.img_psf_conv(gt, psf, circular=True) + noise
    Y.value, Pp.value = y, kernel
    xo = solver.solve(x0=y, rhos=rhos, lams={n0: lam, n1: lam})
    loss = ((xo - gt) ** 2).mean()
    loss.backward()
    gs = m.height_map.height_map_sqrt.grad
    return dict(loss=loss.detach(), g_s=None if gs is None else gs.detach().clone(), g_rhos=rhos.grad, y=y.detach(), x=xo.detach(), psf=psf,
                g_kernel=kernel.grad if detach_kernel else None)


def case_e2e(device):
    """the model in front of conv_doe and the unrolled solver.  With the data term's kernel detached as the reference has it: loss, y, x
    and the gradients to height_map_sqrt, rhos and the kernel against the reference's float64 chain, within the reference's own float32
    distance + 1e-5.  With the psf handed over as it is (what a user of this backend writes): loss.backward() fills height_map_sqrt.grad
    through both paths -- the first run's gradient plus the model's own vector-Jacobian product of the kernel's gradient."""
    g = load_golden("g48_doe_e2e")
    m = build(32, 16, device, g["s"])
    gt, noise, K = T(g["gt"], device), T(g["noise"], device), int(g["K"])
    a = e2e_run(device, m, gt, noise, K, True)
    assert a["g_s"] is not None and a["g_rhos"] is not None and a["g_kernel"] is not None
    assert abs(float(a["loss"]) - float(g["loss64"])) <= abs(float(g["loss32"]) - float(g["loss64"])) + SLACK * abs(float(g["loss64"]))
    for what, key, ref, own in (("y", "y", g["y64"], rel_l2(g["y32"], g["y64"])), ("x", "x", g["x64"], float(g["d_x"])),
                                ("g_height_map_sqrt", "g_s", g["g_s64"], float(g["d_g_s"])), ("g_rhos", "g_rhos", g["g_rhos64"], float(g["d_g_rhos"])),
                                ("g_psf of the data term", "g_kernel", g["g_psf_term64"], float(g["d_g_psf_term"]))):
        r = rel_l2(a[key].detach().cpu().numpy(), ref)
        note("e2e 32->16", what, r, own + SLACK)
        assert r <= own + SLACK, (what, r, own)
    (vjp,) = torch.autograd.grad(m.get_psf(), m.height_map.height_map_sqrt, a["g_kernel"])
    b = e2e_run(device, m, gt, noise, K, False)
    assert b["g_s"] is not None and torch.equal(b["x"], a["x"])
    r = rel_l2(b["g_s"].cpu().numpy(), (a["g_s"] + vjp).cpu().numpy())
    note("e2e 32->16", "g_height_map_sqrt through both paths vs the sum of the two", r, SLACK)
    assert r <= SLACK, r


def write_achieved():
    """the measured distances of the cases run so far -> the JSON file the environment variable DPX_DOE_PARITY_OUT names (how
    profiles/doe_parity_achieved.json is produced from a GPU run); without the variable nothing is written"""
    path = os.environ.get("DPX_DOE_PARITY_OUT")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ACHIEVED, f, indent=1, sort_keys=True)


# the runs of tests/test_gpu_guard_doe.py and tests/test_guard_doe_emul.py on guarded workspaces: case, arguments, the size queries
# whose buffers they use (a forward + backward keeps the field in its workspace; the small entry points run on the one without it)
GUARDED_RUNS = {
    "doe_parity_30_pert": (case_parity, (30, "pert"), ("dpx_doe_ws_bytes", "dpx_doe_propagator_bytes", "dpx_fft_table_bytes")),
    "doe_phase_baseline_propagator": (case_phase_baseline_propagator, (), ("dpx_doe_ws_bytes", "dpx_doe_propagator_bytes")),
    "doe_no_grad_stores_no_field": (case_no_grad_stores_no_field, (), ("dpx_doe_ws_bytes",)),
}
