"""Cases of the TV denoiser's gradient shared by the GPU tests (-m gpu, real MI355X) and the emulated-kernel tests (CPU, the same kernel
source under the SIMT emulator).  Every case differentiates the drop-in API (ops.tv_denoise(..., differentiable=True) /
TVDenoiser(..., differentiable=True)) on `device` and compares with the reference's own autograd (tests/golden/g44_tv_bwd_*.npz,
make_golden_tv_bwd.py) or with torch autograd over `tv_torch64`, tv_cases.tv_f64 restated as float64 torch ops.

Bounds (the project's rule, not tuned to the kernel): the gradient to the input within rel-L2 1e-5 of the reference's float32 gradient
(of the float64 one where there is no reference run; the reference's own fp32-vs-float64 distance is 1e-7 .. 2e-7 on the fixtures); the
gradient to sigma at least as close to the reference's float64 value as the reference's float32 value is, plus 1e-5 relative, and no
further from the float32 value than that plus the two references' distance (`check_glam`).  TV is piecewise linear, so a comparison is
meaningful only where no dual update sits on the clip threshold: the fixtures were generated under that condition, and the other cases
walk seeds until the float64 run keeps every |w| at least 1e-5 theta away from theta (ten to a hundred float32 roundings of w; a
property of the input, judged on the yardstick alone -- `separated`).  The recording forward must equal the plain one bit for bit, and
the gradient to the input must not depend on the blocking.
"""
import numpy as np
import torch

import dprox as dp
from dprox import _ops as ops
from conftest import assert_close, load_golden, record, rel_l2
import tv_cases as tc
from tv_cases import T, tune_get, tune_set

TOL_G = 1e-5
MARGIN = 1e-5
FIXTURES = ("a", "b", "d", "e")


def tv_torch64(y, lam, iters, dims):
    """tv_cases.tv_f64 in float64 torch ops (differentiable; the clip is torch.clamp with tensor bounds, whose backward counts equality as
    inside).  y [N, D0, D1, D2], lam [N].  Returns (out, the least | |w| - theta | / theta over every dual update)"""
    k, outs, margin = len(dims), [], float("inf")
    for n in range(y.shape[0]):
        yn, theta = y[n], lam[n] / 2
        axes = [d - 1 for d in dims]
        z = {a: torch.zeros([s - (i == a) for i, s in enumerate(yn.shape)], dtype=torch.float64) for a in axes}
        for t in range(iters):
            x = 0
            for a in axes:
                edge = torch.zeros([1 if i == a else s for i, s in enumerate(yn.shape)], dtype=torch.float64)
                zp = torch.cat([edge, z[a], edge], dim=a)                              # z[-1] = z[n_a - 1] = 0
                x = x + (yn - (zp.narrow(a, 0, yn.shape[a]) - zp.narrow(a, 1, yn.shape[a])))
            x = x / k
            if t + 1 < iters:
                for a in axes:
                    w = z[a] + torch.diff(x, dim=a) / 5
                    if w.numel() and float(theta.detach()) > 0:
                        margin = min(margin, float(((w.detach().abs() - theta.detach()).abs().min() / theta.detach())))
                    z[a] = torch.clamp(w, min=-theta, max=theta)
        outs.append(x)
    return torch.stack(outs), margin


def grads64(v, lam, g, iters, dims):
    """float64 autograd of <g, TV(v, lam)>: (out, d/dv, d/dlam [N], margin) as NumPy"""
    y = torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True)
    lm = torch.from_numpy(np.broadcast_to(np.asarray(lam, np.float64).reshape(-1), (y.shape[0],)).copy()).requires_grad_(True)
    out, margin = tv_torch64(y, lm, iters, dims)
    out.backward(torch.from_numpy(np.asarray(g, np.float64)))
    return out.detach().numpy(), y.grad.numpy(), lm.grad.numpy(), margin


def check_restatement():
    """tv_torch64's forward is tv_cases.tv_f64 (which test_tv_host.py pins to the reference's float64 outputs), and its gradients are the
    reference's float64 gradients on every fixture"""
    v = tc.noisy((2, 3, 9, 11), 5)
    for dims, iters in (((1, 2), 5), ((1, 2, 3), 4), ((2, 3), 7), ((3,), 3)):
        out, _ = tv_torch64(torch.from_numpy(v.astype(np.float64)), torch.tensor([0.05, 0.3], dtype=torch.float64), iters, dims)
        assert rel_l2(out.numpy(), tc.tv_f64(v, [0.05, 0.3], iters, dims)) <= 1e-14, dims
    for tag in FIXTURES:
        f = fixture(tag)
        out, gv, gl, margin = grads64(f["v"][None], f["sigma"], f["g"][None], f["iters"], f["dims"])
        assert margin >= 1e-4, (tag, margin)                                         # (the generator's own condition)
        worst = max(rel_l2(out[0], f["out64"]), rel_l2(gv[0], f["gv64"]), abs(gl[0] - f["gs64"]) / abs(f["gs64"]))
        record(f"tv_torch64 vs the reference's float64 autograd, fixture {tag}", worst, 1e-12)
        assert worst <= 1e-12, (tag, worst)


_fixtures = {}


def fixture(tag):
    """one case of make_golden_tv_bwd.py: v, g [C, H, W], sigma, iters, dims, and the reference's fp32 / float64 out, d/dv, d/dsigma"""
    if tag not in _fixtures:
        a, b = load_golden(f"g44_tv_bwd_{tag}"), load_golden(f"g44_tv_bwd_{tag}_grad")
        unbits = lambda r64, bits: (r64.astype(np.float32).view(np.int32) + bits).view(np.float32)
        assert float(a["margin"]) >= 1e-4 and 0.05 <= float(a["clipped"]) <= 0.95, tag
        _fixtures[tag] = dict(v=a["v"], g=a["g"], sigma=float(a["sigma"]), iters=int(a["iters"]), use_3d=bool(a["use_3d"]),
                              dims=(1, 2, 3) if bool(a["use_3d"]) else (1, 2), out64=a["out_f64"], out32=unbits(a["out_f64"], a["out_bits"]),
                              gv64=b["gv_f64"], gv32=unbits(b["gv_f64"], b["gv_bits"]), gs32=float(b["gsigma_f32"]), gs64=float(b["gsigma_f64"]))
    return _fixtures[tag]


def check_gy(gy, ref, what):
    r = rel_l2(gy, ref)
    record(what, r, TOL_G)
    print(f"{what}: rel-L2 {r:.3e} (bound {TOL_G:.0e})")
    assert r <= TOL_G, f"{what}: rel-L2 {r:.3e} > {TOL_G:.0e}"


def check_glam(glam, r64, r32, what):
    """per image: |glam - r64| <= |r32 - r64| + 1e-5 |r64| and |glam - r32| <= that + |r32 - r64|; r32 = None: float64 is the only yardstick"""
    glam, r64 = np.asarray(glam, np.float64).reshape(-1), np.asarray(r64, np.float64).reshape(-1)
    r32 = r64 if r32 is None else np.asarray(r32, np.float64).reshape(-1)
    for n in range(glam.size):
        gap = abs(r32[n] - r64[n])
        bound = gap + 1e-5 * abs(r64[n])
        d64, d32 = abs(glam[n] - r64[n]), abs(glam[n] - r32[n])
        record(f"{what} [image {n}] (relative to the float64 value)", d64 / max(abs(r64[n]), 1e-30), bound / max(abs(r64[n]), 1e-30))
        print(f"{what} [{n}]: {glam[n]:.9g} vs float64 {r64[n]:.9g} (|diff| {d64:.3e}, bound {bound:.3e}); vs fp32 |diff| {d32:.3e}")
        assert d64 <= bound, f"{what} [{n}]: {d64:.3e} from the float64 value > {bound:.3e}"
        assert d32 <= bound + gap, f"{what} [{n}]: {d32:.3e} from the float32 value > {bound + gap:.3e}"


def differentiate(device, v, lam, g, iters, dims, via="ops", use_3d=None):
    """(out, gy, glam as lam's own shape) of the drop-in API on `device`, all NumPy; asserts that the recording forward equals the plain one"""
    vt = T(v, device).requires_grad_(True)
    lt = lam if isinstance(lam, torch.Tensor) else T(np.asarray(lam, np.float32), device)
    lt = lt.detach().clone().requires_grad_(True)
    if via == "ops":
        out = ops.tv_denoise(vt, lt, iters, dims, differentiable=True)
    else:
        den = dp.TVDenoiser(iters, use_3d, differentiable=True) if use_3d is not None else dp.TVDenoiser(iters, dims=dims, differentiable=True)
        assert den.dims == tuple(dims)
        out = den.denoise(vt, lt)
    assert out.requires_grad
    with torch.no_grad():
        plain = ops.tv_denoise(vt, lt, iters, dims)
    assert torch.equal(out.detach(), plain), f"the recording forward differs from the plain one: {tuple(vt.shape)} dims {dims} iters {iters}"
    out.backward(T(g, device))
    assert tuple(lt.grad.shape) == tuple(lt.shape) and lt.grad.device == lt.device
    return out.detach().cpu().numpy(), vt.grad.cpu().numpy(), lt.grad.cpu().numpy()


def case_fixture(device, tag, via):
    """a fixture through ops.tv_denoise / TVDenoiser.denoise with a 0-d sigma on the host, as the reference is called"""
    f = fixture(tag)
    out, gy, gl = differentiate(device, f["v"][None], torch.tensor(f["sigma"]), f["g"][None], f["iters"], f["dims"], via, f["use_3d"])
    what = f"tv backward fixture {tag} ({via})"
    assert_close(out[0], f["out32"], tc.TOL_OP, what + ": out vs reference fp32")
    check_gy(gy[0], f["gv32"], what + ": d/dv vs reference fp32")
    check_glam(gl, f["gs64"], f["gs32"], what + ": d/dsigma")
    return gy, gl


_separated = {}


def separated(shape, lam, iters, dims, seed):
    """(v, g, float64 out, d/dv, d/dlam) for the first seed from `seed` on whose float64 run keeps every |w| MARGIN theta away from theta"""
    key = (tuple(shape), tuple(np.asarray(lam, np.float64).reshape(-1)), iters, tuple(dims), seed)
    if key not in _separated:
        for s in range(seed, seed + 40):
            v = tc.noisy(shape, s)
            g = np.random.RandomState(s + 1000).randn(*shape).astype(np.float32)
            out, gv, gl, margin = grads64(v, lam, g, iters, dims)
            if margin >= MARGIN:
                _separated[key] = (v, g, out, gv, gl)
                break
        else:
            raise AssertionError(f"no seed from {seed} on separates {shape} dims {dims} lam {lam}")
    return _separated[key]


def case_extension(device, shape, dims, iters=5, lam=None, seed=0):
    """shapes and axis sets the reference cannot run, against float64 autograd of the restatement; lam: [N] on the device"""
    lam = np.asarray(lam if lam is not None else [0.05 + 0.25 * i / max(shape[0] - 1, 1) for i in range(shape[0])], np.float32)
    v, g, out64, gv64, gl64 = separated(shape, lam, iters, dims, seed)
    out, gy, gl = differentiate(device, v, lam, g, iters, dims)
    what = f"tv backward {shape} dims {dims} iters {iters}"
    assert_close(out, out64, tc.TOL_OP, what + ": out vs float64 restatement")
    check_gy(gy, gv64, what + ": d/dv vs float64 autograd")
    check_glam(gl, gl64, None, what + ": d/dlam")
    return gy, gl


def case_iters1(device):
    """one step has no clip state: out = y, gy is g bit for bit, the gradient to lam is exactly zero"""
    v, g = tc.noisy((2, 3, 21, 30), 7), np.random.RandomState(8).randn(2, 3, 21, 30).astype(np.float32)
    for dims in ((1, 2), (1, 2, 3), (2, 3)):
        out, gy, gl = differentiate(device, v, [0.05, 0.3], g, 1, dims)
        assert np.array_equal(gy, g) and np.array_equal(gl, np.zeros(2, np.float32)), dims


def case_blocking(device, C, dims, kind):
    """on shapes chosen from the plan (tv_cases.blocking_shape; dpx_tv_bwd_plan must name the forward's tiles), d/dv is bit-identical between
    tv_steps = 1 and the blocked default, d/dlam agrees within 1e-5 relative and is bit-identical across two runs"""
    old = tune_get("tv_steps")
    try:
        tune_set("tv_steps", 0)
        shape, S, t = tc.blocking_shape(C, dims, kind)
        assert S > 1
        v, g = tc.noisy(shape, 11), np.random.RandomState(12).randn(*shape).astype(np.float32)
        for iters in sorted({S, 2 * S + 1}):
            res = {}
            for steps in (1, 0, 0):
                tune_set("tv_steps", steps)
                p = ops.tv_bwd_plan(shape, iters, dims)
                fwd = ops.tv_plan(shape, iters, dims)
                assert (p["steps"], p["launches"], p["tile"]) == (fwd["steps"], fwd["launches"], fwd["tile"]) and p["lds_bytes"] >= fwd["lds_bytes"]
                assert p["steps"] == min(steps or S, iters), (steps, iters, p)
                res.setdefault(steps, []).append(differentiate(device, v, 0.3, g, iters, dims)[1:])
            (gy1, gl1), (gy0, gl0), (gy0b, gl0b) = res[1][0], res[0][0], res[0][1]
            assert np.array_equal(gy1, gy0), (shape, dims, iters, f"d/dv: tv_steps 1 vs 0 (S = {S}, tile {t})")
            assert np.array_equal(gy0, gy0b) and np.array_equal(gl0, gl0b), (shape, dims, iters, "two runs differ")
            assert np.isfinite(gy0).all() and np.abs(gy0).max() > 0
            check_glam(gl0, gl1, None, f"tv backward blocking {shape} dims {dims} iters {iters}: d/dlam blocked vs one-step")
    finally:
        tune_set("tv_steps", old)


def case_saturation(device):
    """lam so large that nothing clips: d/dv is the linear operator's float64 result and d/dlam exactly zero; lam tiny against the data:
    almost every dual update clips, d/dv is close to g itself and d/dlam matches float64"""
    shape, dims, iters = (1, 3, 21, 30), (1, 2, 3), 5
    v, g, out64, gv64, gl64 = separated(shape, [100.0], iters, dims, 20)
    out, gy, gl = differentiate(device, v, [100.0], g, iters, dims)
    assert gl64[0] == 0.0 and gl[0] == 0.0, (gl, gl64)
    check_gy(gy, gv64, "tv backward, nothing clips: d/dv vs float64 autograd")
    assert rel_l2(gy, g) > 0.1                                    # (the operator smooths: far from the identity)
    v, g, out64, gv64, gl64 = separated(shape, [1e-4], iters, dims, 20)
    out, gy, gl = differentiate(device, v, [1e-4], g, iters, dims)
    check_gy(gy, gv64, "tv backward, almost everything clips: d/dv vs float64 autograd")
    check_glam(gl, gl64, None, "tv backward, almost everything clips: d/dlam")
    assert rel_l2(gy, g) < 0.05, rel_l2(gy, g)


def case_argument_errors(device):
    """dpx_tv_denoise_rec's and dpx_tv_backward's own argument checks surface as DpxError"""
    from dprox import _backend as be
    L, p = be.lib(), be.ptr
    v = T(tc.noisy((1, 3, 8, 8), 0), device)
    out, gy, lam = torch.empty_like(v), torch.empty_like(v), T(np.array([0.1], np.float32), device)
    codes = torch.zeros(L.query("dpx_tv_codes_bytes", 1, 3, 8, 8, 3, 5), dtype=torch.uint8, device=device)
    ws = torch.zeros(L.query("dpx_tv_bwd_ws_bytes", 1, 3, 8, 8, 3, 5), dtype=torch.uint8, device=device)
    glam = torch.empty(1, device=device)
    rec = [p(v), p(out), p(lam), p(codes), 1, 3, 8, 8, 3, 5, None, be.stream()]
    bwd = [p(v), p(codes), p(gy), p(glam), 1, 3, 8, 8, 3, 5, p(ws), be.stream()]
    for name, good, cases in (("dpx_tv_denoise_rec", rec, ((0, None, "null"), (1, None, "null"), (2, None, "null"), (3, None, "null"), (1, p(v), "in-place"),
                                                           (8, 0, "axes"), (9, 0, "iters"), (5, 0, "shape"))),
                              ("dpx_tv_backward", bwd, ((0, None, "null"), (1, None, "null"), (2, None, "null"), (2, p(v), "in-place"), (10, None, "workspace"),
                                                        (8, 8, "axes"), (9, 0, "iters"), (4, 0, "shape")))):
        for idx, bad, msg in cases:
            args = list(good)
            args[idx] = bad
            try:
                L.call(name, *args)
            except be.DpxError as e:
                assert msg in str(e), (name, msg, str(e))
            else:
                raise AssertionError(f"{name} accepted argument {idx} = {bad}")
    L.call("dpx_tv_backward", *bwd[:3], None, *bwd[4:10], None, be.stream())          # one launch, no gradient of lam: no workspace needed


def case_admm_grads(device):
    """end to end: 3 ADMM iterations on sum_squares(conv(x, psf) - b) + deep_prior(x, TVDenoiser(differentiable=True)) (the reference's default
    2-D form) at 1 x 3 x 32 x 32, loss = MSE to a target; the gradients to the per-step sigma schedule and to b against the reference's
    autograd.  Bound: tv_cases.case_admm's rule for amplified comparisons -- 1e-5, or 2 x the reference's own fp32-vs-float64 distance +
    1e-5 were that larger (it is 4.9e-7 for d/dsigma, 2.5e-6 for d/db, 1.7e-6 for x) -- against the fp32 and the float64 run alike.  The
    solve must have left the no-gradient plan for the unrolled mode; without a gradient to compute it stays on the fused plan."""
    g = load_golden("g44_tv_bwd_admm")
    assert float(g["margin"]) >= 1e-5 and 0.05 <= float(g["clipped"]) <= 0.95
    x = dp.Variable()
    bt = T(g["b"], device).clone().requires_grad_(True)
    sig = torch.tensor(g["sigmas"], requires_grad=True)
    prior = dp.deep_prior(x, denoiser=dp.TVDenoiser(differentiable=True))
    s = dp.compile(dp.sum_squares(dp.conv(x, g["psf"]) - bt) + prior, method="admm", device=device)
    xo = s.solve(x0=T(g["b"], device), rhos=T(g["rhos"], device), lams={prior: sig}, max_iter=3)
    assert s.last_path == "unrolled", f"the solve took {s.last_path!r}: not the unrolled mode autograd can see the TV prior in"
    loss = ((xo - T(g["gt"], device)) ** 2).mean()
    loss.backward()
    assert sig.grad is not None and bt.grad is not None
    for name, got in (("x", xo.detach()), ("g_sigma", sig.grad), ("g_b", bt.grad)):
        gap = float(g[f"{name}_ref_f32_vs_f64"])
        tol = tc.TOL if gap <= tc.TOL else 2 * gap + tc.TOL
        for ref, kind in ((g[name], "fp32"), (g[name + "_f64"], "float64")):
            r = rel_l2(got.cpu().numpy(), ref)
            record(f"tv backward, ADMM end to end: {name} vs reference {kind}", r, tol)
            print(f"ADMM end to end: {name} vs reference {kind}: rel-L2 {r:.3e} (bound {tol:.1e})")
            assert r <= tol, (name, kind, r, tol)
    with torch.no_grad():
        s.solve(x0=T(g["b"], device), rhos=T(g["rhos"], device), lams={prior: sig}, max_iter=3)
    assert s.last_path == "fused"
