"""TV denoiser cases shared by the GPU tests (-m gpu, real MI355X) and the emulated-kernel tests (CPU, the same kernel source under the
SIMT emulator).  Every case runs the drop-in API on `device` against the reference's stored outputs (tests/golden/g43_tv_*.npz,
make_golden_tv.py) or against `tv_f64`, a float64 NumPy restatement of the formula in csrc/dpx_tv.hip's header.

Gates: the operator within rel-L2 1e-6 (and max-abs 1e-6 of max|ref|) of the reference's fp32 and float64 outputs -- the project's
operator bar (nlm_cases.TOL_OP), 20x the reference's own fp32 round-off (3e-8 .. 5.5e-8 from its float64 run); `tv_f64` within 1e-12
of the stored float64 outputs; a 5-iteration solve within nlm_cases.case_admm's bounds: 1e-5 of the reference's fp32 iterate (or 2x the
reference's own fp32-vs-float64 distance + 1e-5, were that larger: it is 3.5e-6 / 2.7e-6 here), its float64 iterate within 0.3x that,
v within half of it and u within it on the iterate's scale (achieved on both paths: x 3.5e-6 / 2.7e-6 from the fp32 iterate -- the
reference's own distance -- and 2e-7 from the float64 iterate; both x-updates take the data term as its float64 spectrum).  Blocked and one-step launches must agree bit for bit.
"""
import ctypes

import numpy as np
import torch

import dprox as dp
from dprox import _backend as be
from dprox import _ops as ops
from conftest import assert_close, load_golden, record, rel_l2

TOL = 1e-5
TOL_OP = 1e-6
ITERS, LAMS = (1, 5, 13), (0.05, 0.3)
DIMS = {"fn2": (1, 2), "fn3": (1, 2, 3), "den2": (1, 2), "den3": (1, 2, 3)}
FN_KEYS = [(tag, vol, it, li) for tag in ("fn2", "fn3") for vol in ("a", "b") for it in ITERS for li in range(len(LAMS))]


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def tv_f64(y, lam, iters=5, dims=(1, 2)):
    """the formula in float64: y [N, D0, D1, D2], lam scalar or [N], dims out of NCHW dims {1, 2, 3}.  z_a has n_a - 1 entries along
    axis a (none for n_a = 1: the axis still counts in k); the last z update is not computed"""
    y = np.asarray(y, np.float64)
    lam = np.broadcast_to(np.asarray(lam, np.float64).reshape(-1), (y.shape[0],))
    out = np.empty_like(y)
    k = len(dims)
    for n in range(y.shape[0]):
        yn, theta = y[n], lam[n] / 2
        axes = [d - 1 for d in dims]
        z = {a: np.zeros([s - (i == a) for i, s in enumerate(yn.shape)]) for a in axes}
        for t in range(iters):
            x = np.zeros_like(yn)
            for a in axes:
                pad = [(1, 1) if i == a else (0, 0) for i in range(3)]
                zp = np.pad(z[a], pad)                                    # z[-1] = z[n_a - 1] = 0
                lo = tuple(slice(0, -1) if i == a else slice(None) for i in range(3))
                hi = tuple(slice(1, None) if i == a else slice(None) for i in range(3))
                x += yn - (zp[lo] - zp[hi])
            x /= k
            if t + 1 < iters:
                for a in axes:
                    z[a] = np.clip(z[a] + np.diff(x, axis=a) / 5, -theta, theta)
        out[n] = x
    return out


def fn_fixture(tag, vol, it, li):
    """(input [D0, D1, D2], the reference's fp32 output, its float64 output) of one fn2 / fn3 case"""
    g = _fn_files(tag)
    key = f"{vol}_i{it}_l{li}"
    r64 = g[key + "_f64"]
    r32 = (r64.astype(np.float32).view(np.int32) + g[key + "_bits"]).view(np.float32)
    return g[f"{vol}_v"], r32, r64


_files = {}


def _fn_files(tag):
    if tag not in _files:
        _files[tag] = load_golden(f"g43_tv_{tag}")
    return _files[tag]


def tune_set(name, value):
    be.lib().call("dpx_tune_set", name.encode(), int(value))


def tune_get(name):
    v = ctypes.c_int(0)
    be.lib().call("dpx_tune_get", name.encode(), ctypes.byref(v))
    return v.value


def case_fn(device, tag, vol, it, li):
    """ops.tv_denoise on a golden volume against TV_denoising / TV_denoising3d of the reference (fp32 and float64 runs)"""
    v, r32, r64 = fn_fixture(tag, vol, it, li)
    out = ops.tv_denoise(T(v[None], device), LAMS[li], it, DIMS[tag]).cpu().numpy()[0]
    what = f"tv {tag} {vol} iters {it} lam {LAMS[li]}"
    assert_close(out, r32, TOL_OP, what + " vs reference fp32")
    assert_close(out, r64, TOL_OP, what + " vs reference float64")
    return out


def case_den(device, tag):
    """TVDenoiser(5, use_3dtv).denoise on [1, 3, 33, 47] with a 0-d sigma against the reference's wrapper"""
    g = load_golden("g43_tv_denoiser")
    den = dp.TVDenoiser(5, tag == "den3")
    assert den.dims == DIMS[tag]
    out = den.denoise(T(g["den_v"], device), torch.tensor(float(g["den_sigma"]))).cpu().numpy()
    assert_close(out, g[f"{tag}_out"], TOL_OP, f"tv {tag} vs reference fp32")
    assert_close(out, g[f"{tag}_out_f64"], TOL_OP, f"tv {tag} vs reference float64")
    return out


def check_restatement():
    """tv_f64 against every stored float64 output of the reference (CPU; pins the restatement the extension cases lean on)"""
    worst = 0.0
    for tag, vol, it, li in FN_KEYS:
        v, _, r64 = fn_fixture(tag, vol, it, li)
        worst = max(worst, rel_l2(tv_f64(v[None], LAMS[li], it, DIMS[tag])[0], r64))
    g = load_golden("g43_tv_denoiser")
    for tag in ("den2", "den3"):
        worst = max(worst, rel_l2(tv_f64(g["den_v"], float(g["den_sigma"]), 5, DIMS[tag]), g[f"{tag}_out_f64"]))
    record("tv_f64 vs the reference's float64 outputs (worst of 26)", worst, 1e-12)
    assert worst <= 1e-12, worst


def noisy(shape, seed):
    rng = np.random.RandomState(seed)
    ramp = np.linspace(0, 1, shape[-1])[None, None, None, :] * np.linspace(1, 0.5, shape[-2])[None, None, :, None]
    return (0.3 + 0.4 * ramp + 0.1 * rng.randn(*shape)).astype(np.float32)


def case_restatement(device, shape, dims, iters=5, lam=None, seed=0):
    """ops.tv_denoise against tv_f64 on shapes the reference cannot run: batches with per-image lam, other axis sets, axes of length 1 / 2"""
    v = noisy(shape, seed)
    lam = np.asarray(lam if lam is not None else [0.05 + 0.25 * i / max(shape[0] - 1, 1) for i in range(shape[0])], np.float32)
    out = ops.tv_denoise(T(v, device), T(lam, device), iters, dims).cpu().numpy()
    assert_close(out, tv_f64(v, lam, iters, dims), TOL_OP, f"tv {shape} dims {dims} iters {iters} vs float64 restatement")
    return out


def case_axes_not_fixed(device):
    """the default 2-D form differences C and H, as the reference does: it equals the fixture and is far from the H-W result"""
    g = load_golden("g43_tv_denoiser")
    v, sigma = T(g["den_v"], device), torch.tensor(float(g["den_sigma"]))
    chw = dp.TVDenoiser(5).denoise(v, sigma).cpu().numpy()
    hw = dp.TVDenoiser(5, dims=(2, 3)).denoise(v, sigma).cpu().numpy()
    assert_close(chw, g["den2_out"], TOL_OP, "tv default 2-D axes vs reference fp32")
    assert rel_l2(chw, hw) > 1e-3, rel_l2(chw, hw)


def case_lam0(device):
    v = noisy((2, 3, 21, 70), 3)
    for dims in ((1, 2), (1, 2, 3), (2, 3)):
        for iters in (1, 5, 13):
            assert torch.equal(ops.tv_denoise(T(v, device), 0.0, iters, dims).cpu(), torch.from_numpy(v)), (dims, iters)
        lam = np.array([0.0, 0.2], np.float32)
        out = ops.tv_denoise(T(v, device), T(lam, device), 7, dims).cpu().numpy()
        assert np.array_equal(out[0], v[0]), dims
        assert_close(out[1], tv_f64(v[1:], lam[1:], 7, dims)[0], TOL_OP, f"tv lam = (0, 0.2) dims {dims}: image 1 vs float64 restatement")


def blocking_shape(C, dims, kind):
    """the smallest [1, C, H, W] whose own plan (dpx_tv_plan at tv_steps = 0) exercises the halo in the way `kind` names: `plus1` --
    H and W the shortest the plan splits at all (tile + 1, or the first extent past what it holds whole); `three` -- 2 t + 3 cells, not a multiple of the tile
    and three tiles along both; `short` -- as `three` along W, H shorter than the halo.  W is found first on tall volumes, then H for
    that W; the plan of the shape returned satisfies the rule (it is asked, not assumed).  Returns (shape, S, tile)"""
    want = (lambda n, t: n > t) if kind == "plus1" else (lambda n, t: n == 2 * t + 3)
    plan = lambda H, W: ops.tv_plan((1, C, H, W), 1000, dims)
    S = plan(4096, 4096)["steps"]
    if kind == "short":
        assert 2 in dims and 3 in dims, "`short` needs both spatial axes differenced"
        heights = [max(S - 2, 2)]
    else:
        heights = range(2, 1200)
    W = next(W for W in range(2, 600) if want(W, plan(4096 if kind != "short" else heights[0], W)["tile"][2]))
    for H in heights:
        p = plan(H, W)
        if want(W, p["tile"][2]) and (kind == "short" or want(H, p["tile"][1])):
            return (1, C, H, W), p["steps"], p["tile"]
    raise AssertionError(f"no shape for C={C} dims={dims} kind={kind} (W = {W})")


def case_blocking(device, C, dims, kind):
    """tv_steps = 1 (one step per launch), 2 and 0 (the plan's S) give torch.equal outputs for iters in {1, S, S + 1, 2 S + 1, 13}, and
    the one-step result matches tv_f64"""
    old = tune_get("tv_steps")
    try:
        tune_set("tv_steps", 0)
        shape, S, t = blocking_shape(C, dims, kind)
        assert S > 1, f"the plan does not block {shape} dims {dims}: S = {S}"
        v = noisy(shape, 11)
        assert 2000 <= v.size <= 400000, shape            # a few thousand to a few hundred thousand voxels
        lam = 0.3
        for iters in sorted({1, S, S + 1, 2 * S + 1, 13}):
            outs = {}
            for steps in (1, 2, 0):
                tune_set("tv_steps", steps)
                p = ops.tv_plan(shape, iters, dims)
                assert p["steps"] == min(steps or S, iters) and p["launches"] * p["steps"] >= iters, (steps, iters, p)
                outs[steps] = ops.tv_denoise(T(v, device), lam, iters, dims).cpu()
            assert torch.equal(outs[1], outs[2]), (shape, dims, iters, "tv_steps 1 vs 2")
            assert torch.equal(outs[1], outs[0]), (shape, dims, iters, f"tv_steps 1 vs 0 (S = {S}, tile {t})")
            if iters == 13:
                assert_close(outs[1].numpy(), tv_f64(v, lam, iters, dims), TOL_OP, f"tv blocking {shape} dims {dims} vs float64 restatement")
    finally:
        tune_set("tv_steps", old)


def admm_problem(g, device, tag, denoiser=None):
    x = dp.Variable()
    b = T(g["b"], device)
    prior = dp.deep_prior(x, denoiser=denoiser if denoiser is not None else dp.TVDenoiser(5, tag == "admm3"))
    fns = dp.sum_squares(dp.conv(x, g["psf"]) - b) + prior
    return fns, {prior: T(g["prior_lams"], device)}, b


def case_admm(device, tag, fused):
    """the reference's 5-iteration ADMM on sum_squares(conv(x, psf) - b) + deep_prior(x, TVDenoiser(5, use_3dtv)) through the fused plan
    or the generic splitting; nlm_cases.case_admm's tolerances."""
    g = load_golden("g43_tv_denoiser")
    fns, lams, b = admm_problem(g, device, tag)
    s = dp.compile(fns, method="admm", device=device)
    s.use_fused = fused
    with torch.no_grad():
        st = s.solve(x0=b, rhos=T(g["rhos"], device), lams=lams, max_iter=5, return_full_states=True)
    assert s.last_path == ("fused" if fused else "generic")
    ref_gap = float(g[f"{tag}_ref_f32_vs_f64"])
    tol = TOL if ref_gap <= TOL else 2 * ref_gap + TOL
    x = st[0].cpu().numpy()
    assert_close(x, g[f"{tag}_x"], tol, f"{tag} x vs reference fp32")
    r64 = rel_l2(x, g[f"{tag}_x_f64"])
    record(f"{tag} x vs reference float64", r64, 0.3 * tol)
    assert r64 <= 0.3 * tol, r64
    for name, got, bar in (("v0", st[1][0], tol / 2), ("u0", st[2][0], tol)):
        err = np.linalg.norm((got.cpu().numpy().astype(np.float64) - g[f"{tag}_{name}"]).ravel()) / np.linalg.norm(g[f"{tag}_x"].ravel())
        record(f"{tag} {name} (on the iterate's scale)", err, bar)
        assert err <= bar, (name, err)
    return st


def case_hqs_runs_fused(device):
    """half-quadratic splitting with the TV prior on the identity takes the fused plan (duals pinned to zero) and agrees with the
    generic splitting to the solve bar"""
    g = load_golden("g43_tv_denoiser")
    xs = {}
    for use_fused in (True, False):
        fns, lams, b = admm_problem(g, device, "admm2")
        s = dp.compile(fns, method="hqs", device=device)
        s.use_fused = use_fused
        with torch.no_grad():
            xs[use_fused] = s.solve(x0=b, rhos=T(g["rhos"], device), lams=lams, max_iter=5).cpu().numpy()
        assert s.last_path == ("fused" if use_fused else "generic")
    assert_close(xs[True], xs[False], TOL, "hqs + TV prior: fused plan vs generic splitting", maxabs_mult=4.0)


def case_registry_name(device, name):
    """deep_prior(x, denoiser="tv" / "tv3d") resolves without any file on disk and denoises like the class"""
    g = load_golden("g43_tv_denoiser")
    prior = dp.deep_prior(dp.Variable(), denoiser=name)
    assert isinstance(prior.denoiser, dp.TVDenoiser) and prior.denoiser.iter_num == 5 and prior.denoiser.use_3dtv == (name == "tv3d")
    out = prior.prox(T(g["den_v"], device), torch.tensor(float(g["den_sigma"]))).cpu().numpy()
    assert_close(out, g["den3_out" if name == "tv3d" else "den2_out"], TOL_OP, f'deep_prior(denoiser="{name}").prox vs reference fp32')


def case_argument_errors(device):
    """dpx_tv_denoise's own argument checks surface as DpxError"""
    L = be.lib()
    v = T(noisy((1, 3, 8, 8), 0), device)
    out, lam = torch.empty_like(v), T(np.array([0.1], np.float32), device)
    p = be.ptr
    good = [p(v), p(out), p(lam), 1, 3, 8, 8, 3, 5, None, be.stream()]
    for idx, bad, msg in ((0, None, "null"), (1, None, "null"), (2, None, "null"), (1, p(v), "in-place"), (7, 0, "axes"), (7, 8, "axes"),
                          (8, 0, "iters"), (3, 0, "shape"), (5, 0, "shape")):
        args = list(good)
        args[idx] = bad
        try:
            L.call("dpx_tv_denoise", *args)
        except be.DpxError as e:
            assert msg in str(e), (msg, str(e))
        else:
            raise AssertionError(f"dpx_tv_denoise accepted argument {idx} = {bad}")
    tune_old = tune_get("tv_steps")
    try:
        tune_set("tv_steps", 1)
        try:
            L.call("dpx_tv_denoise", p(v), p(out), p(lam), 1, 3, 8, 8, 3, 5, None, be.stream())     # a chain needs its workspace
        except be.DpxError as e:
            assert "workspace" in str(e)
        else:
            raise AssertionError("dpx_tv_denoise accepted a null workspace for a chain of launches")
    finally:
        tune_set("tv_steps", tune_old)
