"""Parity cases shared by the GPU tests (-m gpu, real MI355X through the C ABI) and the emulated-kernel
tests (CPU, same kernel sources under the SIMT emulator).  Every case rebuilds a golden fixture's problem
with the drop-in `dprox` API on `device` and compares with the reference's stored outputs.

Tolerance (north_star): rel-L2 <= 1e-5 on the iterate x.  The split variables v/u are
non-smooth functions of x (soft threshold / clip at lam) so their error is compared on the scale of x.
"""
import os

import numpy as np
import pytest
import torch

import dprox as dp
from conftest import assert_close, load_golden, record, rel_l2

TOL = 1e-5


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def close_on_scale(a, b, scale_ref, tol, what=""):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    err = np.linalg.norm((a - b).ravel()) / np.linalg.norm(np.asarray(scale_ref, dtype=np.float64).ravel())
    record(what + " (on the iterate's scale)", err, tol)
    assert err <= tol, f"{what}: error {err:.3e} relative to the iterate's norm > {tol:.1e}"


def tv_problem(b, psf, dims=(0, 1)):
    x = dp.Variable()
    fns = dp.sum_squares(dp.conv(x, psf) - b)
    regs = [dp.norm1(dp.grad(x, dim=d)) for d in dims]
    for r in regs:
        fns = fns + r
    return x, fns, regs


def case_linops(device, tag):
    g = load_golden(f"g1_linops_{tag}")
    x, y = T(g["x"], device), T(g["y"], device)
    v = dp.Variable()
    c = dp.conv(v, g["psf"]).to(device)
    assert_close(c.forward(x).cpu(), g["conv_fwd"], TOL, "conv fwd")
    assert_close(c.adjoint(y).cpu(), g["conv_adj"], TOL, "conv adj")
    assert_close(c.get_diag(x, freq=True).cpu(), g["conv_diag"], TOL, "conv diag")
    for d in (0, 1, 2):
        if f"grad{d}_fwd" not in g:
            continue
        gr = dp.grad(v, dim=d).to(device)
        assert_close(gr.forward(x).cpu(), g[f"grad{d}_fwd"], TOL, f"grad{d} fwd")
        assert_close(gr.adjoint(y).cpu(), g[f"grad{d}_adj"], TOL, f"grad{d} adj")
        assert_close(gr.get_diag(x, freq=True).cpu(), g[f"grad{d}_diag"], TOL, f"grad{d} diag")


def case_prox(device):
    g = load_golden("g3_prox")
    v, c = T(g["v"], device), T(g["c"], device)
    lam0, lamB = torch.tensor(0.3, device=device), T(g["lamB"], device)
    var = dp.Variable()
    var.value = torch.zeros_like(v)
    mk = lambda fn: fn.to(device)
    assert_close(dp.soft_threshold(v, 0.3).cpu(), g["soft_0p3"], 1e-6)
    assert_close(mk(dp.norm1(var)).prox(v, lam0).cpu(), g["norm1_scalar"], 1e-6)
    assert_close(mk(dp.norm1(var)).prox(v, lamB).cpu(), g["norm1_batch"], 1e-6)
    assert_close(mk(2.5 * dp.norm1(var)).prox(v, lamB).cpu(), g["norm1_alpha2p5"], 1e-6)
    assert_close(mk(dp.norm1(var - c)).prox(v, lamB).cpu(), g["norm1_offset"], 1e-6)
    assert_close(mk(dp.norm1(dp.grad(var, dim=1) - c)).prox(v, lam0).cpu(), g["norm1_grad1_offset"], 1e-6)
    assert_close(mk(dp.nonneg(var)).prox(v, lam0).cpu(), g["nonneg"], 1e-6)
    assert_close(mk(dp.nonneg(var - c)).prox(v, lam0).cpu(), g["nonneg_offset"], 1e-6)
    assert_close(mk(dp.sum_squares(var)).prox(v, lamB).cpu(), g["sumsq_batch"], 1e-6)
    assert_close(mk(dp.norm2(var)).prox(v, lam0).cpu(), g["norm2_scalar"], 1e-6)
    fn = mk(dp.norm1(var))
    fn.beta = 2.0
    assert_close(fn.prox(v, lam0).cpu(), g["norm1_beta2"], 1e-6)


def case_solve_direct(device):
    g = load_golden("g4_solve_direct")
    b = T(g["b"], device)
    x, fns, _ = tv_problem(b, g["psf"])
    s = dp.compile(fns, method="admm", device=device)
    s.Kall.update_vars([b])
    rhs = [T(g["rhs0"], device), T(g["rhs1"], device)]
    assert s.least_square.freq_diagonalizable and not s.least_square.diagonalizable
    assert_close(s.least_square.solve(rhs, torch.tensor(0.7, device=device)).cpu(), g["x_rho_scalar"], TOL)
    assert_close(s.least_square.solve(rhs, torch.tensor([0.7, 0.05], device=device)).cpu(), g["x_rho_batch"], TOL)
    x2 = dp.Variable()
    s2 = dp.compile(dp.sum_squares(dp.conv(x2, g["psf"]) - b) + dp.nonneg(x2), method="admm", device=device)
    s2.Kall.update_vars([b])
    assert_close(s2.least_square.solve([rhs[0]], torch.tensor(0.3, device=device)).cpu(), g["x_identity"], TOL)


def case_admm_tv_small(device, fused=True):
    g = load_golden("g5_admm_tv_small")
    b = T(g["b"], device)
    x, fns, _ = tv_problem(b, g["psf"])
    s = dp.compile(fns, method="admm", device=device)
    s.use_fused = fused
    st = s.solve(x0=b, rhos=T(g["rhos"], device), lams=0.004, max_iter=50, return_full_states=True)
    assert s.last_path == ("fused" if fused else "generic")
    assert_close(st[0].cpu(), g["x"], TOL, "x", maxabs_mult=4.0)    # at the reference's own fp32 noise floor, see conftest.assert_close
    assert x.value is st[0] or torch.equal(x.value, st[0])
    for i in range(2):
        close_on_scale(st[1][i], g[f"v{i}"], g["x"], TOL, f"v{i}")
        close_on_scale(st[2][i], g[f"u{i}"], g["x"], TOL, f"u{i}")


def case_admm_tv_config1(device):
    g = load_golden("g5_admm_tv_c1")
    b = T(g["b"], device)
    x, fns, _ = tv_problem(b, g["psf"])
    snaps = {}

    def cb(iter, state, rho, lam):
        if iter + 1 in (1, 5, 20):
            snaps[iter + 1] = (state[0].clone(), [e.clone() for e in state[1]], [e.clone() for e in state[2]])

    out = dp.Problem(fns).solve(method="admm", device=device, x0=b, rhos=0.1, lams=0.005, max_iter=20, callback=cb)
    assert_close(out.cpu(), g["x"], TOL, "final x", maxabs_mult=4.0)    # at the reference's own fp32 noise floor, see conftest.assert_close
    for it, (xs, vs, us) in snaps.items():
        assert_close(xs[..., ::4, ::4].cpu(), g[f"it{it}_x"], TOL, f"x@{it}", maxabs_mult=4.0 if it >= 5 else 1.0)
        for i in range(2):
            close_on_scale(vs[i][..., ::4, ::4], g[f"it{it}_v{i}"], g[f"it{it}_x"], TOL, f"v{i}@{it}")
            close_on_scale(us[i][..., ::4, ::4], g[f"it{it}_u{i}"], g[f"it{it}_x"], TOL, f"u{i}@{it}")
    psnr = 10 * np.log10(1.0 / np.mean((out.cpu().numpy() - g["gt"]) ** 2))
    assert abs(psnr - float(g["psnr"])) < 1e-3 and psnr > 31.0
    # context: the reference's fp32 schedule is 9e-6 away from the exact (float64) iterate; the HIP path must not be worse
    assert rel_l2(out.cpu(), g["x_f64"]) <= rel_l2(g["x"], g["x_f64"])


def case_admm_tv_misc(device):
    g = load_golden("g5_admm_tv_misc")
    b = T(g["b"], device)
    x = dp.Variable()
    data = dp.sum_squares(dp.conv(x, g["psf"]) - b)
    t0, t1, t2 = dp.norm1(dp.grad(x, dim=0)), 2.0 * dp.norm1(dp.grad(x, dim=1)), dp.norm1(dp.grad(x, dim=2))
    out = dp.Problem(data + t0 + t1 + t2).solve(method="admm", device=device, x0=np.ascontiguousarray(g["b"][0].transpose(1, 2, 0)))
    assert_close(out.cpu(), g["x_defaults"], TOL, "defaults (rho=1, lam=0.02, 24 it, HWC numpy x0)")
    out = dp.Problem(data + t0 + t1 + t2).solve(method="admm", device=device, x0=b, rhos=0.2, max_iter=6,
                                                lams={t0: 0.01, t1: torch.linspace(0.01, 0.02, 6), t2: 0.003})
    assert_close(out.cpu(), g["x_lams"], TOL, "per-term lams")


def case_pgd(device):
    g = load_golden("g10_pgd")
    b = T(g["b"], device)
    x = dp.Variable()
    out = dp.Problem(dp.sum_squares(dp.conv(x, g["psf"]) - b) + dp.norm1(x)).solve(
        method="pgd", device=device, x0=b, rhos=0.8, lams=0.01, max_iter=5)
    assert_close(out.cpu(), g["x_norm1"], TOL)
    x2 = dp.Variable()
    out = dp.Problem(dp.sum_squares(dp.conv(x2, g["psf"]) - b) + dp.nonneg(x2)).solve(
        method="pgd", device=device, x0=b, rhos=torch.tensor([[0.8] * 5, [0.4] * 5]), lams=0.01, max_iter=5)
    assert_close(out.cpu(), g["x_nonneg_rhoB"], TOL)


def case_pgd_pow2(device, tiny=False):
    """G34: proximal gradient descent on power-of-two planes = ONE fused call (dpx_pgd_run: column kernel + a row kernel that
    finishes the inverse transform, steps, applies the prox and starts the next forward transform).  Against the reference's
    iterates, and against the op-by-op path of the same backend (forced by passing a callback).  tiny (the SIMT emulator):
    1 x 2 x 256 x 256, 3 iterations, fused against op by op only."""
    import synthetic
    from dprox import _ops as ops
    g = load_golden("g34_pgd_pow2")
    shape, K = ((1, 2, 256, 256), 3) if tiny else ((2, 3, 256, 512), 8)
    gt, b0, psf = synthetic.deconv_case(*shape, seed=int(g["seed"]))
    b = T(b0, device)
    rhos, lams = torch.from_numpy(g["rhos"])[:shape[0], :K], torch.from_numpy(g["lams"])[:K]
    calls = []
    real = ops.pgd_run
    ops.pgd_run = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        for tag, mk in (("norm1", lambda x: 0.7 * dp.norm1(x)), ("nonneg", dp.nonneg), ("norm2", dp.norm2)):
            x = dp.Variable()
            term = mk(x)
            prob = dp.Problem(dp.sum_squares(dp.conv(x, psf) - b) + term)
            out = prob.solve(method="pgd", device=device, x0=b, rhos=rhos, lams={term: lams}, max_iter=K)
            assert len(calls) == 1, "the fused proximal-gradient path did not run"
            calls.clear()
            assert torch.equal(x.value, out)
            if not tiny:
                _check_packed(g, "x_" + tag, out, 4, TOL, what="pgd pow2 ")
            steps = []
            ref = prob.solve(method="pgd", device=device, x0=b, rhos=rhos, lams={term: lams}, max_iter=K,
                             callback=lambda **kw: steps.append(kw["iter"]))
            assert steps == list(range(K)) and not calls
            assert_close(out.cpu(), ref.cpu(), TOL, f"pgd pow2 {tag}: fused vs op by op")
            assert np.array_equal(b.cpu().numpy(), b0), "x0 / b modified in place"
    finally:
        ops.pgd_run = real


def case_pgd_pow2_shapes(device):
    """the fused proximal-gradient call on every row / column length of the power-of-two path against the op-by-op path (itself
    pinned by G10 / G34), K^T b absent (sum_squares(conv(x))) and present"""
    import synthetic
    for (B, C, H, W), with_b in (((1, 1, 256, 2048), True), ((1, 2, 512, 256), False), ((2, 1, 1024, 512), True), ((1, 1, 512, 1024), True)):
        gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=H + W)
        b = T(b0, device)
        x = dp.Variable()
        term = dp.norm1(x)
        data = dp.sum_squares(dp.conv(x, psf) - b) if with_b else dp.sum_squares(dp.conv(x, psf))
        prob = dp.Problem(data + term)
        kw = dict(method="pgd", device=device, x0=b, rhos=torch.linspace(0.9, 0.6, 4), lams={term: 0.01}, max_iter=4)
        out = prob.solve(**kw)
        ref = prob.solve(callback=lambda **k: None, **kw)
        assert_close(out.cpu(), ref.cpu(), TOL, f"pgd fused vs op by op {B}x{C}x{H}x{W}")


def case_h768(device, tiny=False):
    """G35: column length 768 = 3 * 256 on the register-radix path (three interleaved 256-point transforms + one radix-3 butterfly on
    registers, fft_reg_x3) -- the height of the reference's own example image (768 x 1024).  The convolution and its adjoint, the
    two-kernel ADMM iteration (state after 4 / 10 iterations) and the fused proximal-gradient call against the reference.
    tiny (the SIMT emulator): the 4-iteration state and the convolution only."""
    import synthetic
    from dprox import _ops as ops
    g = load_golden("g35_h768")
    gt, b0, psf = synthetic.deconv_case(1, 3, 768, 256, seed=int(g["seed"]))
    b = T(b0, device)
    assert ops.pgd_supported(768, 256, 1), "H = 768 is not on the register-radix path"
    x = dp.Variable()
    cv = dp.conv(x, g["k2"]).to(device)
    _check_packed(g, "conv_fwd", cv.forward(b), 8, TOL, what="h768 ")
    _check_packed(g, "conv_adj", cv.adjoint(b), 8, TOL, what="h768 ")
    for K in ((4,) if tiny else (4, 10)):
        x, fns, _ = tv_problem(b, psf)
        prob = dp.Problem(fns)
        xs, vs, us = prob.solve(method="admm", device=device, x0=b, rhos=0.1, lams=0.005, max_iter=K, return_full_states=True)
        assert prob.solver.last_path == "fused"
        _check_packed(g, f"it{K}_x", xs, 8, TOL, what="h768 ")
        for i in range(2):
            _check_packed(g, f"it{K}_v{i}", vs[i], 16, TOL, scale_key=f"it{K}_x", what="h768 ", scale_sub=2)
            _check_packed(g, f"it{K}_u{i}", us[i], 16, TOL, scale_key=f"it{K}_x", what="h768 ", scale_sub=2)
    if tiny:
        return
    x = dp.Variable()
    term = dp.norm1(x)
    out = dp.Problem(dp.sum_squares(dp.conv(x, psf) - b) + term).solve(method="pgd", device=device, x0=b, rhos=0.8, lams=0.01, max_iter=4)
    _check_packed(g, "pgd_x", out, 8, TOL, what="h768 ")


def case_other_plane_sizes(device, sizes=((384, 256), (1536, 256), (2048, 256), (256, 768), (768, 768), (512, 1536)), channels=None):
    """the other plane sizes of the register-radix path (3 * 2^k rows / columns: fft_reg_x3; 2048 rows on 4-column workgroups)
    against the oracle (the fp32 CPU restatement of the reference, pinned by the fixtures): convolution, adjoint, the ADMM
    iteration (two kernels -- 768-wide rows on one wave per row, fft384_wave -- or the staged kernels for 1536- and 2048-wide planes) and
    the fused proximal-gradient call"""
    import oracle as O
    import synthetic
    from dprox import _ops as ops
    for (H, W) in sizes:
        assert ops.pgd_supported(H, W, 1), f"{H}x{W} is not on the register-radix path"
        gt, b0, psf = synthetic.deconv_case(1, channels or (3 if H * W < 500000 else 1), H, W, seed=H + W)      # (the reference's conv takes 1 or 3 channels)
        b, bt = T(b0, device), torch.from_numpy(b0)
        x = dp.Variable()
        cv = dp.conv(x, psf).to(device)
        lin = O.lin_conv(psf)
        assert_close(cv.forward(b).cpu(), lin.fwd(bt), TOL, f"conv forward, {H}x{W}")
        assert_close(cv.adjoint(b).cpu(), lin.adj(bt), TOL, f"conv adjoint, {H}x{W}")
        x, fns, _ = tv_problem(b, psf)
        prob = dp.Problem(fns)
        out = prob.solve(method="admm", device=device, x0=b, rhos=0.1, lams=0.005, max_iter=6)
        assert prob.solver.last_path == "fused"
        ref = O.solve([O.sum_squares(O.lin_conv(psf).minus(bt)), O.norm1(O.lin_grad(0)), O.norm1(O.lin_grad(1))],
                      "admm", x0=bt, rhos=0.1, lams=0.005, max_iter=6)
        assert_close(out.cpu(), ref, TOL, f"ADMM x 6, {H}x{W}", maxabs_mult=4.0)   # (pointwise at the fp32 noise floor, as config 1: conftest.assert_close)
        x = dp.Variable()
        term = dp.norm1(x)
        out = dp.Problem(dp.sum_squares(dp.conv(x, psf) - b) + term).solve(method="pgd", device=device, x0=b, rhos=0.8, lams=0.01, max_iter=3)
        ref = O.solve([O.sum_squares(O.lin_conv(psf).minus(bt)), O.norm1(O.lin_identity())], "pgd", x0=bt, rhos=0.8, lams=0.01, max_iter=3)
        assert_close(out.cpu(), ref, TOL, f"PGD x 3, {H}x{W}")


def case_generic_interleaved(device, sizes=((1, 3, 45, 35), (2, 1, 30, 44), (1, 1, 52, 26), (1, 3, 63, 28), (1, 1, 100, 120), (1, 1, 24, 34),
                                             (1, 1, 1100, 24), (1, 1, 24, 2200)), oracle_sizes=((1, 3, 45, 35), (1, 1, 100, 120)), forms=(1, 4)):
    """size-generic transforms, second form (k_rows_r2c_il / k_rows_c2r_il: a row per one-wave workgroup, or eight rows interleaved on 512
    threads with knob value 4; k_cols_il: eight columns interleaved in one LDS image; passes in place) against the first form (knob
    generic_interleaved = 0: k_rows_r2c / k_cols / k_rows_c2r): same Stockham order, butterflies and table twiddles, so convolution, adjoint and
    the ADMM iterate must be BIT-IDENTICAL -- odd and even widths, radices 2 / 3 / 4 / 5 / 7 / 8 / 11 (13 stays on the first form), ragged last
    workgroups (135 rows, 18 columns), a 17-point row length that stays on the first form beside interleaved columns, and the four-sequence
    workgroups of lengths above 1024 -- and against the oracle (the reference's restatement) on two of the sizes."""
    import oracle as O
    import synthetic
    from dprox import _backend as be
    for (B, C, H, W) in sizes:
        gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=H + 3 * W)
        b, bt = T(b0, device), torch.from_numpy(b0)
        res = {}
        for form in tuple(forms) + (0,):
            with be.tuned(generic_interleaved=form):
                x = dp.Variable()
                cv = dp.conv(x, psf).to(device)
                fwd, adj = cv.forward(b).cpu(), cv.adjoint(b).cpu()
                x, fns, _ = tv_problem(b, psf)
                out = dp.Problem(fns).solve(method="admm", device=device, x0=b, rhos=0.3, lams=0.01, max_iter=3).cpu()
                res[form] = (fwd, adj, out)
        for form in forms:
            for name, p, q in zip(("conv forward", "conv adjoint", "ADMM x 3"), res[form], res[0]):
                assert torch.equal(p, q), f"{name} {B}x{C}x{H}x{W}: form {form} differs from the first form by {float((p - q).abs().max())}"
        if (B, C, H, W) in oracle_sizes:
            lin = O.lin_conv(psf)
            assert_close(res[1][0], lin.fwd(bt), TOL, f"conv forward, {H}x{W} (interleaved generic transforms)")
            ref = O.solve([O.sum_squares(O.lin_conv(psf).minus(bt)), O.norm1(O.lin_grad(0)), O.norm1(O.lin_grad(1))],
                          "admm", x0=bt, rhos=0.3, lams=0.01, max_iter=3)
            assert_close(res[1][2], ref, TOL, f"ADMM x 3, {H}x{W} (interleaved generic transforms)", maxabs_mult=4.0)


def case_merged_z_rhs(device, shapes=((2, 3, 40, 52), (1, 1, 33, 47), (2, 1, 30, 44))):
    """staged iteration on planes off the two-kernel iteration: the z / dual stage of iteration t and the right-hand side of iteration
    t + 1 as ONE pass (dpx_admm_zupdate_rhs: neighbours' updates recomputed, duals double-buffered) against the two separate passes
    (dpx_admm_zupdate, dpx_admm_rhs): the same expressions in the same order, so x, every v_i and every u_i must be BIT-IDENTICAL --
    ADMM and half-quadratic splitting, identity / grad_H / grad_W terms, soft threshold / nonneg proxes, per-image rho schedules, widths
    with and without 16-byte groups -- and the merged path against the op-by-op iteration to round-off."""
    import synthetic
    from dprox.algo import fused
    for (B, C, H, W) in shapes:
        gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=5 + H)
        b = T(b0, device)
        rhos = torch.linspace(0.5, 0.3, 5).repeat(B, 1) * torch.linspace(1.0, 1.4, B).view(B, 1)
        for method in ("admm", "hqs", "admm_vxu"):
            outs = {}
            for mode in ("merged", "staged", "op-by-op"):
                x = dp.Variable()
                fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1)) + dp.nonneg(x) + dp.norm1(x) * 0.3
                s = dp.compile(fns, method=method, device=device)
                s.use_fused = mode != "op-by-op"
                old = fused.FusedADMM.merge_z_rhs
                fused.FusedADMM.merge_z_rhs = mode == "merged"
                try:
                    outs[mode] = s.solve(x0=b, rhos=rhos, lams=0.01, max_iter=5, return_full_states=True)
                finally:
                    fused.FusedADMM.merge_z_rhs = old
                assert s.last_path == ("generic" if mode == "op-by-op" else "fused"), (mode, s.last_path)
            flat = lambda st: [st[0]] + [t for part in st[1:] for t in (part if isinstance(part, (list, tuple)) else [part])]
            for k, (p, q) in enumerate(zip(flat(outs["merged"]), flat(outs["staged"]))):
                assert torch.equal(p, q), f"{method} {B}x{C}x{H}x{W}: state tensor {k} of the merged pass differs by {float((p - q).abs().max())}"
            assert_close(outs["merged"][0].cpu(), outs["op-by-op"][0].cpu(), 2e-5, f"{method} {H}x{W}: merged z / rhs pass vs op by op")
    # with a callback the merged pass stores v in every iteration (without one only the loop's last stage does): the states a callback sees
    B, C, H, W = shapes[0]
    gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=11)
    b = T(b0, device)
    seen = {}
    for mode in ("merged", "staged"):
        x = dp.Variable()
        fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
        s = dp.compile(fns, method="admm", device=device)
        log = seen[mode] = []
        old = fused.FusedADMM.merge_z_rhs
        fused.FusedADMM.merge_z_rhs = mode == "merged"
        try:
            s.solve(x0=b, rhos=0.3, lams=0.01, max_iter=4, callback=lambda iter, state, **kw: log.append([t.clone() for t in [state[0]] + list(state[1]) + list(state[2])]))
        finally:
            fused.FusedADMM.merge_z_rhs = old
    assert len(seen["merged"]) == len(seen["staged"]) == 4
    for it, (pa, qa) in enumerate(zip(seen["merged"], seen["staged"])):
        for k, (p, q) in enumerate(zip(pa, qa)):
            assert torch.equal(p, q), f"callback state {k} of iteration {it}: merged pass differs by {float((p - q).abs().max())}"
    # the entry refuses what it cannot do in one pass: a dual updated in place (its neighbours are read while it is written)
    from dprox import _ops as ops, _backend as be
    z = torch.zeros(1, 1, 8, 8, device=device)
    v0, u0, rhs, rho = torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z), torch.ones(1, device=device)
    terms = ops.make_terms([dict(linop=1, prox=0, alpha=1.0, lam=rho, v=v0, u=u0)])
    try:
        ops.admm_zupdate_rhs(z, terms, 1, rhs, rho)
    except be.DpxError as e:
        assert "double-buffered" in str(e)
    else:
        raise AssertionError("dpx_admm_zupdate_rhs accepted an in-place dual")


def case_w768_two_kernel(device, H=256, B=2, methods=("admm", "hqs", "admm_vxu")):
    """768-wide rows on the two-kernel iteration (384 = 6 * 8 * 8 complex points per row on one wave, fft384_wave): ADMM, half-quadratic
    splitting and ADMM_vxu with full states against the op-by-op iteration on the size-generic kernels, and the fresh-state /
    touched-state seeds against each other.  (768 x 768 is the reference's own patch size, contrib/optic/utils.py:158-166.)"""
    import synthetic
    from dprox import _ops as ops
    x0 = torch.zeros(1, 1, H, 768, device=device)
    terms = ops.make_terms([dict(linop=1, prox=0, alpha=1.0, lam=None, v=x0, u=x0), dict(linop=2, prox=0, alpha=1.0, lam=None, v=x0, u=x0)])
    assert ops.iter_supported(H, 768, terms, 2), "768-wide planes must be on the two-kernel iteration"
    gt, b0, psf = synthetic.deconv_case(B, 1, H, 768, seed=3)
    b = T(b0, device)
    outs = {}
    for fused in (True, False):
        for method in methods:
            x = dp.Variable()
            fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
            s = dp.compile(fns, method=method, device=device)
            s.use_fused = fused
            outs[(fused, method)] = s.solve(x0=b, rhos=0.2, lams=0.01, max_iter=4, return_full_states=True)
            assert s.last_path == ("fused" if fused else "generic"), (method, s.last_path)
    for method in methods:
        a, c = outs[(True, method)], outs[(False, method)]
        assert_close(a[0].cpu(), c[0].cpu(), TOL, f"768-wide {method}: x, two-kernel vs op by op")
        for p, q in zip(a[1], c[1]):
            close_on_scale(p.cpu().numpy(), q.cpu().numpy(), c[0].cpu().numpy(), 5e-5, f"768-wide {method}: v on the scale of x")
    # a touched state takes the general seed (k_seed_rows), a fresh one the streaming seed: same iterate up to one transform's round-off
    x = dp.Variable()
    fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
    s = dp.compile(fns, method="admm", device=device)
    st = s.initialize(b.clone())
    st[2][0].add_(0.0)                                       # (touching the state disables the fresh-state shortcut)
    rh, lm = s.defaults(b, 0.2, 0.01, 3)[1:3]
    touched = s.iters(st, rh.to(device), {k: v.to(device) for k, v in lm.items()}, 3)[0]
    fresh = s.solve(x0=b, rhos=0.2, lams=0.01, max_iter=3)
    assert_close(touched.cpu(), fresh.cpu(), 2e-6, "768-wide: general seed vs fresh-state seed")


UNROLL_BWD_MODES = (("default", {}),                                            # two-kernel backward iteration on power-of-two planes (small launches: the row-parallel
                                                                                # kernel k_bwd_rows_par), else the image-domain fused stage
                    ("lock-step bands", dict(unroll_bwd_par_max_rows=-1)),          # two-kernel backward iteration on k_bwd_rows whatever the launch size
                    ("staged", dict(unroll_bwd_staged=1)),
                    ("image-domain fused stage", dict(unroll_bwd_staged=2)),
                    ("image-domain fused stage, reductions by its last workgroup", dict(unroll_bwd_staged=2, unroll_bwd_fold_finish=1)))


def _unrolled_bwd_run(device, data, terms, dtype, K, knobs, chain_history=None):
    """[loss, d loss / d rhos, d / d lams..., d / d b, d / d x0] (float64 numpy) of K unrolled ADMM iterations under the tuning `knobs`.
    chain_history ("f32" / "bf16"): on the stage-by-stage autograd path instead (DPX_UNROLL_CHAIN, read by autodiff.run at call time: one
    autograd node per stage), whose nodes save exactly what the one-node loop keeps as its history -- rhs (_Rhs), x (_Solve), v_i
    (_ZUpdate); "bf16" rounds those saved images to bf16 (round-to-nearest-even, as k_hist_pack_bf16 and the emitting row kernel do)
    through autograd's saved-tensor hooks, which makes that path keep the bf16 history's values.  A gradient autograd does not form
    there (lambda of a prox that ignores it) counts as zeros."""
    import contextlib
    import os
    from dprox import _backend as be
    gt, b, psf = data
    x = dp.Variable()
    bt = T(b, device).clone().requires_grad_(True)
    regs = []
    if "tv" in terms:
        regs += [dp.norm1(dp.grad(x, dim=0)), dp.norm1(dp.grad(x, dim=1))]
    if "nn" in terms:
        regs += [dp.nonneg(x)]
    if "l1" in terms:
        regs += [dp.norm1(x) * 0.5]
    fns = dp.sum_squares(dp.conv(x, psf) - bt)
    for r in regs:
        fns = fns + r
    solver = dp.specialize(dp.compile(fns, method="admm", device=device), method="unroll", device=device, max_iter=K, dtype=dtype)
    rhos = torch.linspace(0.4, 0.2, K).requires_grad_(True)
    lams = [torch.linspace(0.03, 0.01, K).requires_grad_(True) for _ in regs]
    x0 = T(b, device).clone().requires_grad_(True)
    image = lambda t: t.dtype == torch.float32 and tuple(t.shape) == tuple(b.shape)
    hooks = contextlib.nullcontext()
    if chain_history == "bf16":
        hooks = torch.autograd.graph.saved_tensors_hooks(lambda t: t.bfloat16().float() if image(t) else t, lambda t: t)
    old = os.environ.get("DPX_UNROLL_CHAIN")
    if chain_history:
        os.environ["DPX_UNROLL_CHAIN"] = "1"
    try:
        with be.tuned(**knobs):
            with hooks:                                      # (the solver's nodes only: the loss keeps what it saves)
                xo = solver.solve(x0=x0, rhos=rhos, lams=dict(zip(regs, lams)))
            loss = ((xo - T(gt, device)) ** 2).mean()
            loss.backward()
    finally:
        if chain_history and old is None:
            del os.environ["DPX_UNROLL_CHAIN"]
        elif chain_history:
            os.environ["DPX_UNROLL_CHAIN"] = old
    grad = lambda t: np.zeros(tuple(t.shape)) if (t.grad is None and chain_history) else t.grad.detach().cpu().double().numpy()
    return [float(loss.detach())] + [grad(t) for t in [rhos] + lams + [bt, x0]]


def case_unrolled_bwd_fused_vs_staged(device, shape=(2, 3, 32, 48), K=4, term_sets=("tv", "tv+nn", "nn+l1"), dtypes=("f32", "bf16"), modes=UNROLL_BWD_MODES,
                                      band=0):
    """the unrolled backward loop in its fused forms -- on power-of-two planes two kernels per backward iteration (k_bwd_rows: inverse
    row transform, rhs stage of iteration t + z stage of iteration t - 1, forward row transform; g_rhs / g_x stay in the Fourier domain),
    elsewhere the two stages as one image-domain pass (k_rhs_z_bwd4) -- against the staged loop (knob unroll_bwd_staged): same loss,
    gradients w.r.t. the rho / lambda schedules, the observation and x0 within fp32 round-off; three term sets (TV, TV + nonneg,
    nonneg + l1 on x), fp32 and bf16 history.  Returns {(terms, dtype): the staged loop's [loss, gradients...]}."""
    import synthetic
    data = synthetic.deconv_case(*shape, seed=17, ksize=5, ksigma=1.2)
    staged = {}
    for terms in term_sets:
        for dtype in dtypes:
            res = {name: _unrolled_bwd_run(device, data, terms, dtype, K, dict(unroll_bwd_band=band, **knobs)) for name, knobs in modes}
            for other in res:
                if other == "staged":
                    continue
                assert abs(res[other][0] - res["staged"][0]) <= 1e-7 * abs(res["staged"][0])
                for k, (a, c) in enumerate(zip(res[other][1:], res["staged"][1:])):
                    e = rel_l2(a, c)
                    record(f"unrolled backward, {other} vs staged, {shape[-2]} x {shape[-1]}, {terms}, {dtype}, gradient {k}", e, 1e-5)
                    assert e <= 1e-5, (terms, dtype, k, other, e)
            staged[terms, dtype] = res["staged"]
    return staged


def case_unrolled_bwd_shortest_loops(device, shapes=((1, 2, 32, 48),)):
    """the backward loops at K = 1 and K = 2, where a loop's start and end meet: at K = 1 the two-kernel loop is not selected and the
    image-domain fused loop is its first z stage and its last rhs stage with nothing in between, at K = 2 each loop body runs once.
    case_unrolled_bwd_fused_vs_staged (every mode against the staged loop, 1e-5), and the staged loop against the stage-by-stage
    autograd path keeping the same history format (_unrolled_bwd_run: chain_history), 1e-5 on every gradient in both formats.
    (Against that path with an fp32 history the bf16 history's d loss / d rho is 6e-5 ... 2e-2 away: that is the history's rounding in
    a sum that cancels, profiles/host_loops_refactor.txt, not something a loop can get wrong.)"""
    import synthetic
    for shape in shapes:
        data = synthetic.deconv_case(*shape, seed=17, ksize=5, ksigma=1.2)
        for K in (1, 2):
            staged = case_unrolled_bwd_fused_vs_staged(device, shape=shape, K=K, term_sets=("tv+nn",))
            for (terms, dtype), res in staged.items():
                chain = _unrolled_bwd_run(device, data, terms, "f32", K, {}, chain_history=dtype)
                assert abs(res[0] - chain[0]) <= TOL * abs(chain[0]), (shape, K, dtype, res[0], chain[0])
                for k, (a, c) in enumerate(zip(res[1:], chain[1:])):
                    e = rel_l2(a, c)
                    record(f"unrolled backward, staged vs stage-by-stage autograd, {'x'.join(map(str, shape))}, K = {K}, {dtype}, gradient {k}", e, 1e-5)
                    assert e <= 1e-5, (shape, K, dtype, k, e)


def case_unrolled_plane_sizes(device, shapes=((1, 3, 768, 1024), (1, 3, 768, 768))):
    """unrolled ADMM x 4 (forward on the two-kernel iteration / the staged kernels, hand-written backward stages) on the 3 * 2^k planes
    against float64 autograd through oracle.admm_f64: iterate and loss at 1e-5, gradients w.r.t. the rho / lambda schedules and
    the observation at 1e-3 (measured 6e-6 ... 1.5e-4, the same as on 512 x 512)"""
    import synthetic
    from oracle.dprox_oracle import admm_f64
    K = 4
    for shape in shapes:
        gt, b, psf = synthetic.deconv_case(*shape, seed=5)
        r0, a0, a1 = (np.linspace(lo, hi, K).astype("float32") for lo, hi in ((0.3, 0.1), (0.02, 0.005), (0.015, 0.006)))
        x = dp.Variable()
        bt = T(b, device).clone().requires_grad_(True)
        n0, n1 = dp.norm1(dp.grad(x, dim=0)), dp.norm1(dp.grad(x, dim=1))
        solver = dp.compile(dp.sum_squares(dp.conv(x, psf) - bt) + n0 + n1, method="admm", device=device)
        solver = dp.specialize(solver, method="unroll", device=device, max_iter=K)
        rhos, l0, l1 = (torch.tensor(t, requires_grad=True) for t in (r0, a0, a1))
        xo = solver.solve(x0=T(b, device), rhos=rhos, lams={n0: l0, n1: l1})
        loss = ((xo - T(gt, device)) ** 2).mean()
        loss.backward()
        r64, a64, b64 = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (r0, a0, a1))
        bt64 = torch.from_numpy(b).double().requires_grad_(True)
        x64, _, _ = admm_f64(bt64, psf, [("grad0", "norm1", 1.0), ("grad1", "norm1", 1.0)], r64, [a64, b64], K)
        loss64 = ((x64 - torch.from_numpy(gt).double()) ** 2).mean()
        loss64.backward()
        tag = "x".join(str(v) for v in shape)
        for name, got, ref, tol in (("x", xo, x64, 1e-5), ("g_rhos", rhos.grad, r64.grad, 1e-3), ("g_l0", l0.grad, a64.grad, 1e-3),
                                    ("g_l1", l1.grad, b64.grad, 1e-3), ("g_b", bt.grad, bt64.grad, 1e-3)):
            r = rel_l2(got.detach().cpu().double().numpy(), ref.detach().numpy())
            record(f"unrolled {tag} {name} vs float64 autograd", r, tol)
            assert r <= tol, (tag, name, r)
        assert abs(float(loss) - float(loss64)) <= 1e-5 * float(loss64)


def case_known_answers(device):
    """the reference's own exact tests, tests/problem/test_ml_problems.py:5-44"""
    g = load_golden("g13_known_answers")
    rhs = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    x = dp.Variable((3, 3))
    dp.Problem(dp.sum_squares(2 * x - rhs)).solve("admm", device=device, x0=np.zeros((3, 3)))
    assert (x.value.cpu().numpy() == rhs / 2).all()
    x = dp.Variable((3, 3))
    dp.Problem(dp.sum_squares(2 * x, rhs)).solve("admm", device=device, x0=np.zeros((3, 3)))
    assert (x.value.cpu().numpy() == rhs / 2).all()
    x = dp.Variable((3, 3, 1))
    rhs3 = np.array([[[1, 2, 3], [4, 5, 6], [7, 8, 9]]])
    kernel = np.array([[1, 1], [1, 1]]) / 4
    dp.Problem(dp.sum_squares(dp.conv(x, kernel) - rhs3)).solve("admm", device=device, x0=np.zeros((3, 3, 1)))
    out = dp.eval(dp.conv(x, kernel).to(device) - rhs3, x.value, zero_out_constant=False)
    assert (out.cpu() < 1e-5).all()
    assert_close(x.value.cpu(), g["lsq2_x"], TOL)
    x = dp.Variable((3))
    dp.Problem(dp.sum_squares(2 * x - np.array([1, 2, 3]))).solve("admm", device=device, x0=np.zeros(3))
    assert (x.value.cpu().numpy() == np.array([1, 2, 3]) / 2).all()


def case_cg(device, B):
    from dprox.linalg.solve import cg
    from dprox.utils import fft2, ifft2
    g = load_golden("g6_cg")
    mask, rhs, rho = T(g[f"B{B}_mask"], device), T(g[f"B{B}_rhs"], device), float(g["rho"])
    A = lambda x: (ifft2(mask * (mask * fft2(x))).real + rho * x).contiguous()
    x, n = cg(A, rhs, rtol=1e-6, max_iters=100, return_iters=True)
    assert abs(n - int(g[f"B{B}_iters"])) <= 1, (n, int(g[f"B{B}_iters"]))
    assert_close(x.cpu(), g[f"B{B}_x"], TOL)
    assert_close(cg(A, rhs, rtol=0.0, max_iters=10).cpu(), g[f"B{B}_x_10it"], TOL)


def case_numpy_observation_edits(device):
    """sum_squares(K, b) with a NumPy observation: the array is converted once and its caches (offset, data spectrum) are kept, but
    an in-place edit of the array between two solves must be seen -- the reference re-reads b on every use (proxfn/base.py unwrap).
    Also through a non-contiguous view (no shared memory with the converted tensor)."""
    import synthetic
    from dprox.contrib import masked_fft
    gt, b, psf = synthetic.deconv_case(2, 1, 32, 32, seed=5, ksize=5, ksigma=1.5)
    for view in (False, True):
        store = np.zeros((2, 1, 32, 64), np.float32)
        b_np = store[..., ::2] if view else np.ascontiguousarray(b.copy())
        b_np[...] = b
        x = dp.Variable()
        fn = dp.sum_squares(dp.conv(x, psf), b_np)
        s = dp.compile(fn + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1)), method="admm", device=device)
        x0 = T(b, device)
        out1 = s.solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu().clone()
        again = s.solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu()
        assert torch.equal(out1, again)
        xr = dp.Variable()
        ref1 = dp.compile(dp.sum_squares(dp.conv(xr, psf) - T(b, device)) + dp.norm1(dp.grad(xr, dim=0)) + dp.norm1(dp.grad(xr, dim=1)),
                          method="admm", device=device).solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu()
        assert rel_l2(out1.numpy(), ref1.numpy()) <= 1e-6
        b_np[...] = 0.5 * b                                   # in-place edit of the caller's array
        out2 = s.solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu()
        xr = dp.Variable()
        ref2 = dp.compile(dp.sum_squares(dp.conv(xr, psf) - T(0.5 * b, device)) + dp.norm1(dp.grad(xr, dim=0)) + dp.norm1(dp.grad(xr, dim=1)),
                          method="admm", device=device).solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu()
        assert rel_l2(out2.numpy(), ref2.numpy()) <= 1e-6, (view, rel_l2(out2.numpy(), ref2.numpy()))
        assert rel_l2(out2.numpy(), out1.numpy()) > 1e-2      # (the stale result would be bit-identical to out1)
        # the offset itself outside of a solve follows the array at once
        b_np[...] = 0.0
        off = fn.offset
        assert off is None or float(off.abs().max()) == 0.0
        # an explicit replacement (sum_squares.set_b: array or tensor) takes every dependent cache with it
        fn.set_b(np.ascontiguousarray(0.25 * b))
        out3 = s.solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu()
        xr = dp.Variable()
        ref3 = dp.compile(dp.sum_squares(dp.conv(xr, psf) - T(0.25 * b, device)) + dp.norm1(dp.grad(xr, dim=0)) + dp.norm1(dp.grad(xr, dim=1)),
                          method="admm", device=device).solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu()
        assert rel_l2(out3.numpy(), ref3.numpy()) <= 1e-6, (view, rel_l2(out3.numpy(), ref3.numpy()))
        fn.set_b(T(b, device))
        out4 = s.solve(x0=x0, rhos=0.2, lams=0.01, max_iter=3).cpu()
        assert rel_l2(out4.numpy(), ref1.numpy()) <= 1e-6


def case_merged_loop_keeps_the_callers_duals(device, shape=(1, 2, 30, 44)):
    """The merged z / rhs loop of the size-generic path double-buffers the duals; after an ODD number of iterations the current duals sit in
    the loop's second set of buffers -- they are copied back, so the tensors of the state that went into iters() hold the result (as with the
    in-place dual update of the un-merged stages) and ARE the returned state (round-4 advisor finding)."""
    import synthetic
    gt, b0, psf = synthetic.deconv_case(*shape, seed=3, ksize=5, ksigma=1.2)
    b = T(b0, device)
    for iters in (3, 4):
        x = dp.Variable()
        s = dp.compile(dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1)), method="admm", device=device)
        _, rhos, lams, _ = s.defaults(b, 0.3, 0.01, iters)
        rd, ld = rhos.to(device), {k: v.to(device) for k, v in lams.items()}
        st = s.initialize(b)
        st[2][0].add_(0.0)
        held = [t for t in st[2]]                              # the caller keeps its state's dual tensors
        out = s.iters(st, rd, ld, iters)
        assert s.last_path == "fused"
        for a, c in zip(held, out[2]):
            assert a is c or torch.equal(a, c), ("the caller's dual tensors hold stale values after an odd number of iterations", iters)
        ref = s.solve(x0=b, rhos=0.3, lams=0.01, max_iter=iters, return_full_states=True)
        for a, c in zip(held, ref[2]):
            assert rel_l2(a.cpu().numpy(), c.cpu().numpy()) <= 2e-6, iters


CG_BRANCHES = (("default", {}),
               ("fused", dict(cg_fused_max_b=32, cg_split_update=0, cg_unfused=0)),
               ("fused + split update", dict(cg_fused_max_b=32, cg_split_update=1, cg_unfused=0)),
               ("fused, slab Gram kernel", dict(cg_fused_max_b=32, cg_gram_small=2)),
               ("fused, no exit-iteration hint", dict(cg_fused_max_b=32, cg_no_hint=1)),
               ("fused, stop flag behind an event", dict(cg_fused_max_b=32, cg_event_wait=1)),
               ("fused, stop flag behind an event, no hint", dict(cg_fused_max_b=32, cg_event_wait=1, cg_no_hint=1)),
               ("fused, 2 rows / 4 columns per workgroup", dict(cg_fused_max_b=32, cg_rows_per_wg=2, cg_cols_per_wg=4)),
               ("step by step", dict(cg_fused_max_b=0)),
               ("step by step (cg_unfused)", dict(cg_fused_max_b=32, cg_unfused=1)))


def case_cg_branches(device, quick=False):
    """G6 / G6b -- BOTH branches of dpx_cg_masked_fft (the fused 4-launch iteration and the step-by-step sequence, selected through
    dpx_tune_set / dpx_cg_config) against the real reference's cg() on batches of 1, 4, 12 and 20 systems: solution, exit iteration,
    the iterate after 10 fixed iterations.  By default B <= 8 runs fused and B > 8 step by step, so without the switches the two
    batch sizes above 8 would never reach the fused kernels and the two below never the step-by-step ones."""
    from dprox import _backend as be
    from dprox import _ops as ops
    assert {"cg_fused_max_b", "cg_split_update", "cg_unfused"} <= set(be.tune_names())
    g6, g6b = load_golden("g6_cg"), load_golden("g6b_cg_large_batches")
    # (quick: the host emulator's share -- one batch on each side of the size rule, the branches that differ in kernels)
    branches = [br for br in CG_BRANCHES if not quick or br[0] in ("default", "fused", "fused, slab Gram kernel", "fused, stop flag behind an event", "step by step")]
    for B, g in (((4, g6), (12, g6b)) if quick else ((1, g6), (4, g6), (12, g6b), (20, g6b))):
        mask, rhs = T(g[f"B{B}_mask"], device), T(g[f"B{B}_rhs"], device).contiguous()
        rho = T(g[f"B{B}_rho"], device) if f"B{B}_rho" in g else torch.full((B,), float(g["rho"]), device=device)
        n_ref = int(g[f"B{B}_iters"])
        outs = {}
        for name, knobs in branches:
            with be.tuned(**knobs):
                x, n = ops.cg_masked_fft(rhs, mask, rho, 1.0, 1e-6, 100)
                x10, n10 = (None, 10) if quick else ops.cg_masked_fft(rhs, mask, rho, 1.0, 0.0, 10)
            assert abs(n - n_ref) <= 1, (B, name, n, n_ref)
            assert n10 == 10, (B, name, n10)
            assert_close(x.cpu(), g[f"B{B}_x"], TOL, f"cg branch '{name}' B={B}")
            if x10 is not None:
                assert_close(x10.cpu(), g[f"B{B}_x_10it"], TOL, f"cg branch '{name}' B={B}, 10 fixed iterations")
            outs[name] = (x.cpu().numpy(), n)
        # the branches run the same recurrences with differently ordered reductions: same exit iteration, solutions within round-off
        ns = {n for _, n in outs.values()}
        assert len(ns) == 1, (B, {k: v[1] for k, v in outs.items()})
        for name, (xv, _) in outs.items():
            e = rel_l2(xv, outs["step by step"][0])
            record(f"cg branch '{name}' vs step by step, B={B}", e, 2e-6)
            assert e <= 2e-6, (B, name, e)
    # the typed entry sets the same registry; negative arguments leave a switch alone; the fused kernels hold at most 32 systems
    L = be.lib()
    old = [be.tune_get(k) for k in ("cg_fused_max_b", "cg_split_update", "cg_unfused")]
    try:
        L.call("dpx_cg_config", 16, 1, -1)
        assert [be.tune_get(k) for k in ("cg_fused_max_b", "cg_split_update", "cg_unfused")] == [16, 1, old[2]]
        assert L.query("dpx_cg_config", 33, -1, -1) < 0
        assert L.query("dpx_tune_set", b"no_such_knob", 1) < 0
    finally:
        L.call("dpx_cg_config", old[0], old[1], old[2])


def case_cg_control_forms(device):
    """dpx_cg_direction and dpx_cg_update, called directly through ops.CgControl, in both forms of their kernels: 16-byte accesses
    (n_per_batch a multiple of 4, every buffer 16-byte aligned) and element by element (any other length or alignment).  B = 3 systems.

    Bounds, eps32 = 2^-23, everything on the right-hand sides from the float64 restatement:
      direction  p = r + beta p, one fused multiply-add per element: eps32 (|beta p| + |r|)
      <p, Ap>    a dot product over npb elements (tests/minres_cases.py): (sqrt(npb) + 4) eps32 sum |p Ap|
      update     alpha = gamma / pAp in float64 from the DEVICE's pAp; x within eps32 (|x| + 3 |alpha p|), r within
                 eps32 (|r| + 3 |alpha Ap|): one rounding each for the device's float32 division, the product and the sum
    With the same values the two forms apply the same fused multiply-add to every element: their p, x and r are bit-identical.
    A frozen solve (flags()[0] = 1) leaves every operand untouched in both forms."""
    from dprox import _ops as ops
    B, eps32 = 3, float(np.finfo(np.float32).eps)
    rng = np.random.RandomState(20)
    beta, gamma, gamma_prev = np.float32([0.37, -1.25, 2.5]), np.float32([1.7, 0.45, -0.8]), np.float32([0.9, 1.1, 1.3])
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)

    def fresh(a):                                        # a fresh allocation (on the CPU T() shares the array's memory): 16-byte aligned
        t = T(a, device).clone()
        assert t.data_ptr() % 16 == 0
        return t

    def shifted(a):                                      # the same values in a contiguous view 4 bytes into a larger allocation
        t = torch.empty(a.size + 1, dtype=torch.float32, device=device)[1:].view(a.shape)
        t.copy_(T(a, device))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t

    def run(v, place, frozen, what):
        npb = v["p"].shape[1]
        ctl = ops.CgControl(fresh(v["b"]), 1e-6)
        for i, s in enumerate((gamma, gamma_prev, beta)):         # the state block's layout (dpx_cg_dev.h): gamma, gamma_prev, beta, pAp, tol2
            ctl.state[i * B:(i + 1) * B].copy_(T(s, device))
        if frozen:
            ctl.flags[0:1].fill_(1)
        p, r, x, Ap = (place(v[k]) for k in ("p", "r", "x", "Ap"))
        ctl.direction(p, r)
        p_dev = p.clone()
        ctl.update(x, r, p, Ap)
        out = {"p": p_dev.cpu().numpy(), "p_end": p.cpu().numpy(), "x": x.cpu().numpy(), "r": r.cpu().numpy(), "Ap": Ap.cpu().numpy()}
        if frozen:
            for k, src in (("p", "p"), ("p_end", "p"), ("x", "x"), ("r", "r"), ("Ap", "Ap")):
                assert np.array_equal(out[k], v[src]), (what, "frozen solve", k)
            return out
        b64 = beta.astype(np.float64)[:, None]
        p0, r0, x0, q = (v[k].astype(np.float64) for k in ("p", "r", "x", "Ap"))
        worst = {}

        def within(name, got, ref, bound):
            ratio = float(np.max(np.abs(got.astype(np.float64) - ref) / bound))
            worst[name] = ratio
            print(f"case_cg_control_forms {what}: {name} error / bound = {ratio:.3f}")
            assert ratio <= 1.0, (what, name, ratio)

        within("direction", out["p"], r0 + b64 * p0, eps32 * (np.abs(b64 * p0) + np.abs(r0)))
        assert np.array_equal(out["p_end"], out["p"]) and np.array_equal(out["Ap"], v["Ap"]), what
        pd = out["p"].astype(np.float64)
        pAp = f64(ctl.pAp)
        within("pAp", pAp, np.sum(pd * q, axis=1), (np.sqrt(npb) + 4.0) * eps32 * np.sum(np.abs(pd * q), axis=1))
        alpha = (gamma.astype(np.float64) / pAp)[:, None]
        within("x", out["x"], x0 + alpha * pd, eps32 * (np.abs(x0) + 3 * np.abs(alpha * pd)))
        within("r", out["r"], r0 - alpha * q, eps32 * (np.abs(r0) + 3 * np.abs(alpha * q)))
        record(f"cg control forms, {what}: largest error / bound", max(worst.values()), 1.0)
        return out

    for npb in (5, 8):
        v = {k: rng.randn(B, npb).astype(np.float32) for k in ("b", "p", "r", "x", "Ap")}
        if npb % 4:                                      # element by element whatever the alignment
            run(v, fresh, False, f"npb={npb}")
            run(v, fresh, True, f"npb={npb}")
            continue
        a = run(v, fresh, False, f"npb={npb}, 16-byte aligned")
        s = run(v, shifted, False, f"npb={npb}, 4 bytes off")
        for k in ("p", "x", "r"):
            assert np.array_equal(a[k], s[k]), (npb, "16-byte and element-wise forms differ", k)
        run(v, fresh, True, f"npb={npb}, 16-byte aligned")
        run(v, shifted, True, f"npb={npb}, 4 bytes off")


def case_cg_wave_fft(device, sizes=(320, 384), B=3, iters=6):
    """the fused CG matvec on 320 x 320 and 384 x 384 planes -- every 1-D transform on one wave's registers (k_crows_real_in_w,
    k_ccols_mask_w, k_crows_real_out_w: radix 5 / 6, 8, 8) -- against the size-generic kernels (knob cg_wave_fft = 2, themselves pinned
    by G6 / G32) and against the oracle's dense-FFT CG: iterate after `iters` fixed iterations and the converged solve"""
    import oracle.dprox_oracle as orc
    from dprox import _backend as be
    from dprox import _ops as ops
    for N in sizes:
        rng = np.random.RandomState(N)
        mask = (rng.rand(1, N, N) < 0.3).astype(np.float32)
        mask[:, N // 2 - 8:N // 2 + 8] = 1
        rhs = rng.randn(B, N, N).astype(np.float32)
        rho = (0.3 + rng.rand(B)).astype(np.float32)
        mt, rt, rh = T(mask, device), T(rhs, device).contiguous(), T(rho, device)
        out = {}
        for name, knobs in (("wave", dict(cg_fused_max_b=32)), ("wave, step by step", dict(cg_fused_max_b=0)),
                            ("generic", dict(cg_fused_max_b=32, cg_wave_fft=2))):
            with be.tuned(**knobs):
                xk, nk = ops.cg_masked_fft(rt, mt, rh, 1.0, 0.0, iters)
                x, n = (xk, nk) if iters >= 100 else ops.cg_masked_fft(rt, mt, rh, 1.0, 1e-6, 100)
            assert nk == iters
            out[name] = (xk.cpu().numpy(), x.cpu().numpy(), n)
        for name in ("wave", "wave, step by step"):
            assert out[name][2] == out["generic"][2], (N, name, out[name][2], out["generic"][2])
            for i, what in ((0, f"{iters} fixed iterations"), (1, "converged")):
                e = rel_l2(out[name][i], out["generic"][i])
                record(f"cg matvec, one-wave transforms ({name}) vs size-generic kernels, {N} x {N}, {what}", e, 2e-6)
                assert e <= 2e-6, (N, name, what, e)
        m2 = torch.from_numpy(mask) ** 2
        rv = torch.from_numpy(rho).view(B, 1, 1)

        def normal(p):          # Re F^-1 mask^2 F p + rho p with the centred orthonormal transform (contrib masked_fft: utils fft2 / ifft2)
            f = torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(p, dim=(-2, -1)), norm="ortho"), dim=(-2, -1)) * m2
            return torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(f, dim=(-2, -1)), norm="ortho"), dim=(-2, -1)).real + rv * p

        xo, no = orc.cg(normal, torch.from_numpy(rhs), rtol=1e-6, max_iters=100, return_iters=True)
        assert abs(no - out["wave"][2]) <= 1, (N, no, out["wave"][2])
        assert_close(out["wave"][1], xo.numpy(), TOL, f"cg with one-wave transforms vs oracle, {N} x {N}")


def case_full_c4_batches(device, B):
    """G32b -- config 4 at the batch sizes of its 2-GPU and 1-GPU runs (16 and 32 x 1 x 320 x 320): LADMM with the CG x-update on the
    STEP-BY-STEP branch of dpx_cg_masked_fft (B > 8; what bench.py's config4_batch32 times), nonneg + gray FFDNet prior, 2 outer
    iterations, CG exit counts included -- and the same solve on the fused branch (cg_fused_max_b = 32)."""
    import synthetic
    from dprox import _backend as be
    from dprox.contrib import masked_fft
    from dprox.linalg import LinearSolveConfig
    from dprox.utils import ifft2
    g = load_golden("g32b_full_c4_batches")
    gt, mask, y = synthetic.csmri_case(B, 320, 320, seed=int(g[f"B{B}_seed"]), center=32)
    mask, y = T(mask, device), T(y, device)
    x0 = ifft2(y).real.float().contiguous()
    gB = {k[len(f"B{B}_"):]: g[k] for k in g if k.startswith(f"B{B}_")}
    for name, knobs in (("step by step", {}), ("fused", dict(cg_fused_max_b=32))):
        x = dp.Variable()
        fns = dp.sum_squares(masked_fft(x, mask), y) + dp.nonneg(x) + dp.deep_prior(x, denoiser=_ffdnet("gray", device))
        with torch.no_grad(), be.tuned(**knobs):
            assert be.tune_get("cg_fused_max_b") == (32 if knobs else 8) and not be.tune_get("cg_unfused")
            s = dp.compile(fns, method="ladmm", device=device, linear_solve_config=LinearSolveConfig(rtol=1e-6, max_iters=100))
            st = s.solve(x0=x0, rhos=0.5, lams=0.03, max_iter=2, return_full_states=True)
        assert s.last_path == "fused-cg", s.last_path
        its = list(s.least_square.cg_iters[-2:])
        assert all(abs(int(a) - int(r)) <= 1 for a, r in zip(its, gB["cg_iters"])), (name, its, gB["cg_iters"])
        what = f"c4 batch {B} ({name}) "
        _check_packed(gB, "x", st[0], 8, TOL, what=what)
        for i in range(2):
            _check_packed(gB, f"v{i}", st[1][i], 8, TOL, scale_key="x", what=what)
            _check_packed(gB, f"u{i}", st[2][i], 8, TOL, scale_key="x", what=what)


def case_cg_masked_fft_shapes(device):
    """dpx_cg_masked_fft (device-controlled CG whose matvec is three fused launches: real row transform, column transform - mask^2 -
    inverse column transform, inverse row transform + real part + rho p) on odd / non-square planes, broadcast and per-image masks:
    against a float64 torch solve of the same normal equations  (Re F^-1 M^2 F + c rho) x = b  (reference utils/misc.py:164-193)."""
    from dprox import _ops as ops
    rng = np.random.RandomState(77)
    for (B, H, W, per_image, c) in ((3, 20, 28, False, 1.0), (2, 33, 30, True, 2.0), (1, 64, 64, False, 1.0), (4, 27, 45, True, 1.0)):
        mask = (rng.rand(B if per_image else 1, 1, H, W) < 0.4).astype(np.float32)
        b = rng.randn(B, 1, H, W).astype(np.float32)
        rho = (0.3 + 0.2 * rng.rand(B)).astype(np.float32)
        x, n_it = ops.cg_masked_fft(T(b, device), T(mask, device), T(rho, device), c, 1e-7, 200)
        # float64 reference: the operator is diagonal in the (centred, orthonormal) Fourier domain only up to the real part --
        # solve by CG in float64 with the same operator built from torch.fft
        m2 = torch.from_numpy(mask.astype(np.float64)) ** 2
        bt, rt = torch.from_numpy(b.astype(np.float64)), torch.from_numpy(rho.astype(np.float64)).view(B, 1, 1, 1)
        f2 = lambda z: torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(z, dim=(-2, -1)), norm="ortho"), dim=(-2, -1))
        i2 = lambda z: torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(z, dim=(-2, -1)), norm="ortho"), dim=(-2, -1))
        A = lambda z: i2(m2 * f2(z)).real + c * rt * z
        xr, r = torch.zeros_like(bt), bt.clone()
        p, rs = r.clone(), (r * r).sum()
        for _ in range(400):
            Ap = A(p)
            al = rs / (p * Ap).sum()
            xr, r = xr + al * p, r - al * Ap
            rs_new = (r * r).sum()
            if rs_new.sqrt() < 1e-13 * bt.norm():
                break
            p, rs = r + (rs_new / rs) * p, rs_new
        e = rel_l2(x.cpu().numpy(), xr.numpy())
        record(f"cg_masked_fft {B}x1x{H}x{W} per-image-mask={per_image} vs float64 solve", e, 1e-5)
        assert e <= 1e-5, (B, H, W, per_image, e, n_it)
    # a mask the fused call does not take (one column profile, broadcast over the rows) must go down the generic cg() loop, not
    # trip an assertion: LADMM through the public API, against the same problem with the mask expanded to the plane
    from dprox.contrib import masked_fft
    from dprox.linalg import LinearSolveConfig
    B, H, W = 2, 24, 20
    col = (rng.rand(1, 1, 1, W) < 0.5).astype(np.float32)
    y = (rng.randn(B, 1, H, W) + 1j * rng.randn(B, 1, H, W)).astype(np.complex64)
    outs = []
    for m in (col, np.broadcast_to(col, (1, 1, H, W)).copy()):
        mt = T(m, device)
        yt = (torch.from_numpy(y).to(device) * mt).contiguous()
        xv = dp.Variable()
        s = dp.compile(dp.sum_squares(masked_fft(xv, mt), yt) + dp.nonneg(xv), method="ladmm", device=device,
                       linear_solve_config=LinearSolveConfig(rtol=1e-6, max_iters=50))
        outs.append(s.solve(x0=torch.zeros(B, 1, H, W, device=device), rhos=0.5, lams=0.1, max_iter=2).cpu().numpy())
    assert rel_l2(outs[0], outs[1]) <= 1e-5, rel_l2(outs[0], outs[1])


def case_dense_krylov(device):
    """The reference's own solver tests restated (tests/linalg/test_linear_solver.py:57-80, test_linear_solver_batch.py:27-49,
    test_linear_solver_torch.py:33-134): a 5 x 5 SPD matrix as the operator, 1-D vectors, cg / cg2 / pcg in float64 (kept in
    float64 on the device: 1e-8 like the reference) and float32, and the gradients of the solution w.r.t. b and the matrix
    against torch.linalg.solve's."""
    from dprox.linalg import linear_solve
    from dprox.linalg.solve import SOLVERS, cg, cg2, pcg
    assert set(SOLVERS) >= {"cg", "cg2", "pcg"}
    rng = np.random.RandomState(2023)
    P = rng.rand(5, 5)
    A64 = P.T @ P + 0.5 * np.eye(5)
    x64 = rng.rand(5)
    for dt, tol in ((torch.float64, 1e-8), (torch.float32, 2e-4)):          # (float32: rtol 1e-6 on the residual x the condition number)
        At, xt = torch.from_numpy(A64).to(device=device, dtype=dt), torch.from_numpy(x64).to(device=device, dtype=dt)
        bt = At @ xt
        K = lambda v: At @ v
        for name, fn, kw in (("cg", cg, dict(rtol=1e-10 if dt == torch.float64 else 1e-6)),
                             ("cg2", cg2, dict(rtol=1e-20 if dt == torch.float64 else 1e-10)),
                             ("pcg", pcg, dict(rtol=1e-10 if dt == torch.float64 else 1e-5))):
            xh = fn(K, bt, **kw)
            assert xh.dtype == dt and xh.shape == bt.shape
            e = float((xh - xt).abs().max() / xt.abs().max())
            record(f"{name} {dt} on a 5x5 SPD system", e, tol)
            assert e <= tol, (name, dt, e)
        jac = pcg(K, bt, rtol=1e-10 if dt == torch.float64 else 1e-5, Minv=lambda r: r / torch.diagonal(At))      # Jacobi preconditioner
        assert float((jac - xt).abs().max() / xt.abs().max()) <= tol

    class MatrixOp(dp.LinOp):                      # the plugin protocol of the reference's tests: parameters + forward / adjoint
        def __init__(self, M):
            super().__init__()
            self.A = torch.nn.Parameter(M)

        def forward(self, v):
            return self.A @ v

        def adjoint(self, v):
            return self.A.T @ v

    for solve in (lambda op, b: linear_solve(op, b), lambda op, b: cg(op, b, rtol=1e-7), lambda op, b: pcg(op, b, rtol=1e-6)):
        op = MatrixOp(torch.from_numpy(A64).float().to(device))
        b = (op.A.detach() @ torch.from_numpy(x64).float().to(device)).requires_grad_(True)
        xh = solve(op, b)
        xh.mean().backward()
        Ar = torch.from_numpy(A64).float().requires_grad_(True)
        br = b.detach().cpu().clone().requires_grad_(True)
        torch.linalg.solve(Ar, br).mean().backward()
        assert_close(b.grad.cpu(), br.grad, 1e-3, "implicit d/db of the solve")
        assert_close(op.A.grad.cpu(), Ar.grad, 1e-3, "implicit d/dA of the solve")


def case_adjoint_dot(device, shape=(2, 3, 96, 80)):
    """CompGraph.sanity_check dot-product test (reference comp_graph.py:342-371, tests/test_linop.py)"""
    import synthetic
    x = dp.Variable()
    psf = synthetic.point_spread_function(15, 5.0)
    for op in (dp.conv(x, psf), dp.grad(x, dim=0), dp.grad(x, dim=1), dp.vstack([dp.conv(x, psf), dp.grad(x, dim=1), x]),
               2.0 * dp.conv(x, psf) - 0.5 * dp.grad(x, dim=0)):
        assert dp.CompGraph(op.to(device)).sanity_check(eps=1e-4, shape=shape), str(op)


# ---- FFDNet / plug-and-play ---------------------------------------------------------------------------------
def _ffdnet(kind, device):
    import oracle as O          # weights generator only (tests may use the oracle)
    from dprox.proxfn.pnp.denoisers import FFDNetColorDenoiser, FFDNetDenoiser
    if kind == "color":
        return FFDNetColorDenoiser(O.ffdnet_weights(7)).to(device)
    return FFDNetDenoiser(O.ffdnet_weights(11, 1, 1, 64, 15)).to(device)


def case_ffdnet_f16_split(device, tiny=False):
    """split-f16 arithmetic of the FFDNet layers (the inference default): against the reference's fp32 output (G8) at the same
    1e-5 as the other modes, and the range trap -- an input outside the binary16 range makes denoise() / solve() raise instead of
    returning a wrong image, while "bf16x3" handles the same input.  tiny: a 3-layer 16-channel network against the f32 mode
    (the SIMT emulator needs minutes for the 12-layer one)."""
    import synthetic
    from dprox import _backend as be
    from dprox.proxfn.pnp.denoisers import FFDNetColorDenoiser
    g = load_golden("g8_ffdnet")
    sig = torch.tensor(0.02, device=device)
    if tiny:
        from dprox.proxfn.pnp.denoisers import FFDNet
        col = FFDNetColorDenoiser()
        col.model = FFDNet(in_nc=3, out_nc=3, nc=16, nb=3, act_mode="R").load_layers(synthetic.ffdnet_weights(5, 3, 3, 16, 3))
        col = col.to(device)
        x = T(g["odd_x"][:, :, :20, :28].copy(), device)
    else:
        col = _ffdnet("color", device)
        x = T(g["odd_x"], device)
    assert col.model.compute_mode == "f16x2"
    with torch.no_grad():
        out = col.denoise(x, sig)
        with be.tuned(conv_tile_rows=8):                      # (8-row workgroup tiles, a launch-geometry knob: the same bits)
            assert torch.equal(col.denoise(x, sig), out), "the workgroup's tile height must not change a bit"
        if tiny:
            col.model.compute_mode = "f32"
            assert_close(out.cpu(), col.denoise(x, sig).cpu(), TOL, "FFDNet split-f16 vs the f32 mode")
            col.model.compute_mode = "f16x2"
        else:
            assert_close(out.cpu(), g["odd_s0.02"], TOL, "FFDNet split-f16 odd sigma 0.02")
        big = (x * 3.0e5).contiguous()
        col.model.f16_fallback = "raise"
        with pytest.raises(be.F16RangeError, match="binary16"):
            col.denoise(big, sig)
        col.model.f16_fallback = "bf16x3"                    # the default: re-run on split-bf16, the network keeps that mode
        with pytest.warns(RuntimeWarning, match="split-bf16"):
            auto = col.denoise(big, sig)
        assert col.model.compute_mode == "bf16x3"
        ref = col.denoise(big, sig)
        col.model.compute_mode = "f32"
        r32 = col.denoise(big, sig)
    assert torch.isfinite(ref).all() and rel_l2(ref.cpu().numpy(), r32.cpu().numpy()) < 1e-5
    assert torch.equal(auto, ref)
    col.model.compute_mode = "f16x2"


def case_ffdnet_winograd(device, tiny=False):
    """compute_mode "f16x2w": the layers behind the first one (up to 64 output channels) as Winograd F(2x2, 3x3) on the split-f16 matrix
    instruction (dpx_conv_wino_dev.h; network_ffdnet.py:54-68, basicblock.py:61-98).  Gray FFDNet (64 channels: every middle layer and the last
    one) and the colour one's last layer against the reference's fp32 outputs (G8) at the same 1e-5 as the other modes; networks of 16 and 64
    channels on planes of several workgroup tiles (persistent workgroups: more tiles than workgroups), odd sizes, against the f32-input mode;
    the range trap.  tiny: the small networks only (the SIMT emulator)."""
    import synthetic
    from dprox import _backend as be
    from dprox.proxfn.pnp.denoisers import FFDNet, FFDNetColorDenoiser
    rng = np.random.RandomState(31)
    shapes = ((16, 3, (2, 3, 20, 28)), (64, 3, (2, 3, 40, 72))) if tiny else ((16, 3, (2, 3, 20, 28)), (64, 4, (3, 3, 135, 210)), (64, 4, (1, 3, 512, 640)))
    with torch.no_grad():
        for nc, nb, shape in shapes:
            col = FFDNetColorDenoiser()
            col.model = FFDNet(in_nc=3, out_nc=3, nc=nc, nb=nb, act_mode="R").load_layers(synthetic.ffdnet_weights(5, 3, 3, nc, nb))
            col = col.to(device)
            x = T(rng.rand(*shape).astype(np.float32), device)
            sig = torch.tensor(0.05, device=device)
            col.model.compute_mode = "f32"
            ref = col.denoise(x, sig).cpu()
            col.model.compute_mode = "f16x2w"
            out = col.denoise(x, sig)
            assert_close(out.cpu(), ref, TOL, f"FFDNet Winograd layers, {nc} channels, {shape} vs the f32 mode")
            assert torch.equal(col.denoise(x, sig), out), "run-to-run"
        # the range trap sees the transformed inputs
        col.model.f16_fallback = "raise"
        with pytest.raises(be.F16RangeError, match="binary16"):
            col.denoise((x * 3.0e5).contiguous(), sig)
        if tiny:
            return
        g = load_golden("g8_ffdnet")
        gray = _ffdnet("gray", device)
        gray.model.compute_mode = "f16x2w"
        out = gray.denoise(T(g["gray_x"], device), torch.tensor(0.1, device=device))
        assert_close(out.cpu(), g["gray_s0.1"], TOL, "gray FFDNet per band, Winograd layers")
        color = _ffdnet("color", device)
        color.model.compute_mode = "f16x2w"
        for tag in ("odd", "even"):
            out = color.denoise(T(g[f"{tag}_x"], device), torch.tensor(0.02, device=device))
            assert_close(out.cpu(), g[f"{tag}_s0.02"], TOL, f"colour FFDNet {tag}, last layer Winograd")


def case_ffdnet_wide_range(device):
    """G8b: a checkpoint with a large dynamic range (He-normal x 8: activations ~8x per layer, out of binary16 range after a few
    layers).  denoise() on the default split-f16 arithmetic trips the range trap, is re-run on split-bf16 automatically and matches
    the reference's fp32 forward at 1e-5; a solve() does the same (one re-run of the whole solve, same iterates as a solver that
    started on split-bf16)."""
    import synthetic
    from dprox.proxfn.pnp.denoisers import FFDNetColorDenoiser
    g = load_golden("g8b_ffdnet_wide_range")
    wts = synthetic.ffdnet_weights(7, gain=float(g["gain"]))
    col = FFDNetColorDenoiser(wts).to(device)
    assert col.model.compute_mode == "f16x2"
    x = T(g["x"], device)
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="split-bf16"):
            y = col.denoise(x, torch.tensor(float(g["sigma"]), device=device))
    assert col.model.compute_mode == "bf16x3"
    assert_close(y.cpu(), g["y"], TOL, "FFDNet wide-range weights: split-f16 -> split-bf16 fallback")
    # the same through a solve: PnP ADMM, 2 iterations
    gt, b0, psf = synthetic.deconv_case(1, 3, 32, 40, seed=88)
    b = T(b0, device)

    def solve(mode):
        den = FFDNetColorDenoiser(wts).to(device)
        den.model.compute_mode = mode
        xv = dp.Variable()
        prior = dp.deep_prior(xv, denoiser=den)
        s = dp.compile(dp.sum_squares(dp.conv(xv, psf) - b) + prior, method="admm", device=device)
        with torch.no_grad():
            out = s.solve(x0=b, rhos=0.5, lams={prior: 0.05}, max_iter=2)
        return out, den
    with pytest.warns(RuntimeWarning, match="split-bf16"):
        auto, den = solve("f16x2")
    assert den.model.compute_mode == "bf16x3"
    direct, _ = solve("bf16x3")
    assert torch.isfinite(auto).all() and torch.equal(auto, direct)


def case_ffdnet(device, which=("odd", "even", "batch", "gray")):
    """G8: FFDNet forward with seeded weights; odd sizes exercise the replicate-pad / crop path"""
    g = load_golden("g8_ffdnet")
    col = _ffdnet("color", device)
    with torch.no_grad():
        for tag in ("odd", "even"):
            if tag not in which:
                continue
            for s in (0.02, 0.2):
                out = col.denoise(T(g[f"{tag}_x"], device), torch.tensor(s, device=device))
                assert_close(out.cpu(), g[f"{tag}_s{s}"], TOL, f"ffdnet color {tag} sigma={s}")
        if "batch" in which:
            out = col.denoise(T(g["batch_sigma_x"], device), torch.tensor([0.05, 0.15], device=device))
            assert_close(out.cpu(), g["batch_sigma"], TOL, "per-image sigma")
            if getattr(col.model, "compute_mode", "") == "f16x2" and str(device) != "cpu":      # pre-split operand planes between the layers (an off-by-default knob; GPU only: half of this case's emulator time): the same bits
                from dprox import _backend as be
                with be.tuned(ffdnet_presplit=1):
                    pre = col.denoise(T(g["batch_sigma_x"], device), torch.tensor([0.05, 0.15], device=device))
                assert torch.equal(pre, out), "pre-split activations must not change a bit"
        if "gray" in which:
            gray = _ffdnet("gray", device)
            out = gray.denoise(T(g["gray_x"], device), torch.tensor(0.1, device=device))
            assert_close(out.cpu(), g["gray_s0.1"], TOL, "gray FFDNet per band")
            # 8-row and 16-row workgroup tiles of the split-arithmetic layers (launch geometry only): the same bits
            from dprox import _backend as be
            outs = []
            for rows in (8, 16):
                with be.tuned(conv_tile_rows=rows):
                    outs.append(gray.denoise(T(g["gray_x"], device), torch.tensor(0.1, device=device)))
            assert torch.equal(outs[0], outs[1]), "the workgroup's tile height must not change a bit"
            assert_close(outs[0].cpu(), g["gray_s0.1"], TOL, "gray FFDNet per band, 8-row tiles")


def case_admm_pnp(device):
    """G9: ADMM with deep_prior(FFDNet-color) z-update, rho/sigma from log_descent"""
    g = load_golden("g9_admm_pnp")
    b = T(g["b"], device)
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=_ffdnet("color", device))
    fns = dp.sum_squares(dp.conv(x, g["psf"]) - b) + prior
    rhos, sig = dp.log_descent(35, 5, 3)
    with torch.no_grad():
        s = dp.compile(fns, method="admm", device=device)
        st = s.solve(x0=b, rhos=rhos, lams={prior: sig}, max_iter=3, return_full_states=True)
    assert s.last_path == "fused"
    # The denoised variable is well conditioned: within 1e-5 of the reference.
    close_on_scale(st[1][0], g["v0"], g["x"], TOL, "v")
    # The x-update divides by |H|^2 + rho with rho down to 1.2e-5 (log_descent): fp32 round-off is amplified ~1e5 x and
    # the reference's own x is 7e-4 (rel-L2) away from the exact float64 iterate stored next to it.  Parity criterion for
    # such steps: at least as close to the exact iterate as the reference is (+ the 1e-5 budget).
    ref_err = rel_l2(g["x"], g["x_f64"])
    assert rel_l2(st[0].cpu(), g["x_f64"]) <= ref_err + TOL, (rel_l2(st[0].cpu(), g["x_f64"]), ref_err)
    assert rel_l2(st[0].cpu(), g["x"]) <= 2 * ref_err + TOL
    x2 = dp.Variable()
    prior2, nn2 = dp.deep_prior(x2, denoiser=_ffdnet("color", device)), dp.nonneg(x2)
    with torch.no_grad():
        out = dp.Problem(dp.sum_squares(dp.conv(x2, g["psf"]) - b) + prior2 + nn2).solve(
            method="admm", device=device, x0=b, rhos=rhos, lams={prior2: sig, nn2: 0.0}, max_iter=3)
    ref_err = rel_l2(g["x_nonneg"], g["x_nonneg_f64"])
    assert rel_l2(out.cpu(), g["x_nonneg_f64"]) <= ref_err + TOL, (rel_l2(out.cpu(), g["x_nonneg_f64"]), ref_err)


def case_pnp_scaled_sqrt(device):
    """G23: `0.6 * deep_prior(x, sqrt=True)` -- sigma = sqrt(alpha * lam) on the fused and on the op-by-op path"""
    g = load_golden("g23_pnp_scaled_sqrt")
    b = T(g["b"], device)
    for fused in (True, False):
        x = dp.Variable()
        prior = 0.6 * dp.deep_prior(x, denoiser=_ffdnet("color", device), sqrt=True)
        with torch.no_grad():
            s = dp.compile(dp.sum_squares(dp.conv(x, g["psf"]) - b) + prior, method="admm", device=device)
            s.use_fused = fused
            st = s.solve(x0=b, rhos=T(g["rhos"], device), lams={prior: T(g["lams"], device)}, max_iter=3, return_full_states=True)
        assert s.last_path == ("fused" if fused else "generic")
        assert_close(st[0].cpu(), g["x"], TOL, f"x (fused={fused})")
        close_on_scale(st[1][0], g["v0"], g["x"], TOL, f"v (fused={fused})")
        close_on_scale(st[2][0], g["u0"], g["x"], TOL, f"u (fused={fused})")


def case_x8_augment(device):
    """G21: deep_prior(x8=True) -- the dihedral transform cycles with the call count (non-square image: the denoiser sees
    transposed shapes on the odd quarter turns)"""
    g = load_golden("g21_x8_augment")
    prior = dp.deep_prior(dp.Variable(), denoiser=_ffdnet("color", device), x8=True)
    v = T(g["v"], device)
    with torch.no_grad():
        for k in range(9):
            out = prior._prox(v, torch.tensor(0.02 + 0.01 * k, device=device))
            assert_close(out.cpu(), g["outs"][k], TOL, f"x8 call {k} (mode {k % 8})")
    prior._reload()
    assert prior.denoiser.iter == 0


def case_ladmm_cg(device):
    """G7: user-defined masked-FFT LinOp (plugin surface) + nonneg + deep_prior(gray FFDNet), LADMM / ADMM with CG x-update"""
    from dprox.linalg import LinearSolveConfig
    from dprox.utils import fft2, ifft2
    g = load_golden("g7_ladmm_cg")
    mask, y, x0 = T(g["mask"], device), T(g["y"], device), T(g["x0"], device)

    class MaskedFFT(dp.LinOp):
        def __init__(self, arg, mask):
            super().__init__([arg])
            self.mask = mask

        def forward(self, x, **kw):
            return (self.mask * fft2(x)).contiguous()

        def adjoint(self, yy, **kw):
            return ifft2(self.mask * yy).real.contiguous()

    x = dp.Variable()
    fns = dp.sum_squares(MaskedFFT(x, mask), y) + dp.nonneg(x) + dp.deep_prior(x, denoiser=_ffdnet("gray", device))
    cfg = LinearSolveConfig(rtol=1e-6, max_iters=100)
    with torch.no_grad():
        st = dp.Problem(fns, linear_solve_config=cfg).solve(method="ladmm", device=device, x0=x0, rhos=0.5, lams=0.03, max_iter=5,
                                                            return_full_states=True)
        xa = dp.Problem(fns, linear_solve_config=cfg).solve(method="admm", device=device, x0=x0, rhos=0.5, lams=0.03, max_iter=3)
    assert_close(st[0].cpu(), g["x"], TOL, "ladmm x")
    close_on_scale(st[1][1], g["v1"], g["x"], TOL, "v1")
    close_on_scale(st[2][0], g["u0"], g["x"], TOL, "u0")
    assert_close(xa.cpu(), g["x_admm"], TOL, "admm+cg x")
    # the same operator from the backend's own building blocks (no PyTorch arithmetic in the CG matvec)
    from dprox.contrib import masked_fft
    x2 = dp.Variable()
    fns2 = dp.sum_squares(masked_fft(x2, mask), y) + dp.nonneg(x2) + dp.deep_prior(x2, denoiser=_ffdnet("gray", device))
    with torch.no_grad():
        x_native = dp.Problem(fns2, linear_solve_config=cfg).solve(method="ladmm", device=device, x0=x0, rhos=0.5, lams=0.03, max_iter=5)
    assert_close(x_native.cpu(), g["x"], TOL, "ladmm x with contrib.masked_fft")
    # the whole iteration in one C call (dpx_admm_cg_pnp_iter) -- with its folded passes (k_pnp_head: z / dual stage + the first layer's
    # input, issued ahead of the host's look at the CG's stop flag; k_pnp_tail: unpack + dual + the next right-hand side + the CG's start
    # state) and without -- against the stage-by-stage loop: the same arithmetic, the same bits, the
    # same CG exit iterations
    import os
    from dprox import _backend as be
    outs = {}
    for name, staged, knobs in (("one call, folded tail", False, {}), ("one call, folded, head not issued early", False, dict(pnp_cg_no_fold=2)),
                                ("one call", False, dict(pnp_cg_no_fold=1)), ("staged", True, {})):
        os.environ.pop("DPX_SPLIT_CG_STAGED", None)
        if staged:
            os.environ["DPX_SPLIT_CG_STAGED"] = "1"
        try:
            x3 = dp.Variable()
            ls_fns = dp.sum_squares(masked_fft(x3, mask), y) + dp.nonneg(x3) + dp.deep_prior(x3, denoiser=_ffdnet("gray", device))
            solver = dp.compile(ls_fns, method="ladmm", device=device, linear_solve_config=cfg)
            seen = []
            with torch.no_grad(), be.tuned(**knobs):
                st3 = solver.solve(x0=x0, rhos=0.5, lams=0.03, max_iter=5, return_full_states=True,
                                   callback=lambda iter, state, **kw: seen.append(state[0].clone()))
        finally:
            os.environ.pop("DPX_SPLIT_CG_STAGED", None)
        outs[name] = (st3, list(solver.least_square.cg_iters), getattr(solver, "last_split_cg_loop", None), seen)
    assert [outs[k][2] for k in outs] == ["one call", "one call", "one call", "staged"], [outs[k][2] for k in outs]
    sb, nb_, _, seen_b = outs["staged"]
    assert len(nb_) == 5 and len(seen_b) == 5
    for name in ("one call, folded tail", "one call, folded, head not issued early", "one call"):
        sa, na, _, seen_a = outs[name]
        assert na == nb_, (name, na, nb_)
        assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1][1], sb[1][1]) and torch.equal(sa[2][1], sb[2][1]) and torch.equal(sa[2][0], sb[2][0]), name
        assert all(torch.equal(p, q) for p, q in zip(seen_a, seen_b)), name        # (the iterates a callback sees, every iteration)
    assert_close(outs["one call, folded tail"][0][0].cpu(), g["x"], TOL, "ladmm x, one call per iteration")


def case_split_cg_loop_forms(device, B=2, H=48, W=48, iters=4, compute_mode=None):
    """The four forms of the plug-and-play loop with a CG x-update (FusedSplitCG.run: one C call per iteration with folded head / tail passes
    and the head issued ahead of the host's look at the CG's stop flag; the same without issuing it early; one C call, nothing folded; the
    stage-by-stage loop) on a small CS-MRI problem with a 3-layer gray FFDNet: same iterates in every iteration (what a callback sees), same
    final state, same CG exit iterations -- bit for bit.  (The staged form against the reference: fixtures G7 / G32.)"""
    import os
    import synthetic
    from dprox import _backend as be
    from dprox.contrib import masked_fft
    from dprox.linalg import LinearSolveConfig
    from dprox.proxfn.pnp.denoisers import FFDNet, FFDNetDenoiser
    from dprox.utils import ifft2
    gt, mask, y = synthetic.csmri_case(B, H, W, seed=5, center=8)
    mask_d, y_d = T(mask, device), torch.from_numpy(y).to(device)
    x0 = ifft2(y_d).real.contiguous()
    cfg = LinearSolveConfig(rtol=1e-6, max_iters=100)
    outs = {}
    forms = (("one call, folded", False, {}), ("one call, folded, head not issued early", False, dict(pnp_cg_no_fold=2)),
             ("one call", False, dict(pnp_cg_no_fold=1)), ("staged", True, {}))
    for name, staged, knobs in forms:
        os.environ.pop("DPX_SPLIT_CG_STAGED", None)
        if staged:
            os.environ["DPX_SPLIT_CG_STAGED"] = "1"
        try:
            x = dp.Variable()
            den = FFDNetDenoiser()
            den.model = FFDNet(in_nc=1, out_nc=1, nc=16, nb=3, act_mode="R").load_layers(synthetic.ffdnet_weights(3, 1, 1, 16, 3))   # (a small stand-in: the emulator's share)
            if compute_mode:
                den.model.compute_mode = compute_mode                # ("f32": the one-call loop without the folded passes -- the f32-input kernels' layout)
            fns = dp.sum_squares(masked_fft(x, mask_d), y_d) + dp.nonneg(x) + dp.deep_prior(x, denoiser=den)
            solver = dp.compile(fns, method="ladmm", device=device, linear_solve_config=cfg)
            seen = []
            with torch.no_grad(), be.tuned(**knobs):
                # without a callback (the folded tail also prepares the next iteration's right-hand side and CG start state) ...
                st = solver.solve(x0=x0, rhos=0.5, lams=0.03, max_iter=iters, return_full_states=True)
                n_plain = list(solver.least_square.cg_iters)
                solver.least_square.cg_iters.clear()
                # ... and with one (every call of the loop stands alone; the iterates a callback sees)
                st_cb = solver.solve(x0=x0, rhos=0.5, lams=0.03, max_iter=iters, return_full_states=True,
                                     callback=lambda iter, state, **kw: seen.append(state[0].clone()))
        finally:
            os.environ.pop("DPX_SPLIT_CG_STAGED", None)
        assert list(solver.least_square.cg_iters) == n_plain, (name, n_plain, list(solver.least_square.cg_iters))
        assert torch.equal(st[0], st_cb[0]) and all(torch.equal(p, q) for i in (1, 2) for p, q in zip(st[i], st_cb[i])), name
        outs[name] = (st, n_plain, getattr(solver, "last_split_cg_loop", None), seen, solver.last_path)
    assert [outs[k][2] for k, _, _ in forms] == ["one call", "one call", "one call", "staged"], [outs[k][2] for k, _, _ in forms]
    assert all(outs[k][4] == "fused-cg" for k in outs)
    sb, nb_, _, seen_b, _ = outs["staged"]
    assert len(nb_) == iters and len(seen_b) == iters and all(n > 0 for n in nb_), nb_
    assert bool(torch.isfinite(sb[0]).all()) and float(sb[0].abs().max()) > 0
    for name, _, _ in forms[:3]:
        sa, na, _, seen_a, _ = outs[name]
        assert na == nb_, (name, na, nb_)
        assert torch.equal(sa[0], sb[0]), name
        for i in range(2):
            assert torch.equal(sa[1][i], sb[1][i]) and torch.equal(sa[2][i], sb[2][i]), (name, i)
        assert all(torch.equal(p, q) for p, q in zip(seen_a, seen_b)), name


def case_unrolled_grads(device):
    """G11 (config 5 at fixture size): loss and gradients of 3 unrolled ADMM iterations w.r.t. the rho / lambda schedules,
    the observation b and x0 -- hand-written backward stages vs the reference's PyTorch autograd.
    Tolerances: forward 1e-5; gradients 1e-5 (measured ~2e-6; the reference's own gradient tests use rtol 1e-2..1e-3,
    tests/linalg/test_linear_solver_grad.py:101-123: soft-threshold masks make them piecewise constant in x)."""
    g = load_golden("g11_unrolled_grads")
    gt = T(g["gt"], device)
    for tag, with_nn in (("tv", False), ("tvnn", True)):
        x = dp.Variable()
        bt = T(g["b"], device).clone().requires_grad_(True)
        n0, n1 = dp.norm1(dp.grad(x, dim=0)), dp.norm1(dp.grad(x, dim=1))
        fns = dp.sum_squares(dp.conv(x, g["psf"]) - bt) + n0 + n1
        if with_nn:
            nn_ = dp.nonneg(x)
            fns = fns + nn_
        solver = dp.compile(fns, method="admm", device=device)
        solver = dp.specialize(solver, method="unroll", device=device, max_iter=3)
        rhos = torch.tensor(g["rhos"], requires_grad=True)
        l0, l1 = torch.tensor(g["l0"], requires_grad=True), torch.tensor(g["l1"], requires_grad=True)
        lams = {n0: l0, n1: l1}
        if with_nn:
            lams[nn_] = torch.zeros(3)
        x0 = T(g["b"], device).clone().requires_grad_(True)
        xo = solver.solve(x0=x0, rhos=rhos, lams=lams)
        loss = ((xo - gt) ** 2).mean()
        loss.backward()
        assert_close(xo.detach().cpu(), g[f"{tag}_x"], TOL, f"{tag} unrolled x")
        lv = float(loss.detach())
        assert abs(lv - float(g[f"{tag}_loss"])) <= 1e-5 * abs(float(g[f"{tag}_loss"])), (lv, float(g[f"{tag}_loss"]))
        for name, got in (("g_rhos", rhos.grad), ("g_l0", l0.grad), ("g_l1", l1.grad), ("g_b", bt.grad), ("g_x0", x0.grad)):
            assert got is not None, f"{tag} {name}: no gradient"
            assert_close(got.detach().cpu(), g[f"{tag}_{name}"], 1e-5, f"{tag} {name}", maxabs_mult=4.0)


def case_unrolled_grads_bf16(device, fixture="g11_unrolled_grads", K=3):
    """bf16 mode of the unrolled training step (BASELINE config 5): specialize(..., method='unroll', dtype='bf16').  The iteration
    itself is fp32 (forward and loss within 1e-5 of the reference); the backward pass reads a bf16 history.  Stated tolerances
    against the reference's fp32 autograd: d/d lambda_t and d/d b 1e-5 (threshold masks survive the rounding), d/d rho_t 1e-2
    (inner products with bf16-rounded x / rhs; measured ~1e-3)."""
    g = load_golden(fixture)
    gt = T(g["gt"], device)
    x = dp.Variable()
    bt = T(g["b"], device).clone().requires_grad_(True)
    n0, n1 = dp.norm1(dp.grad(x, dim=0)), dp.norm1(dp.grad(x, dim=1))
    solver = dp.compile(dp.sum_squares(dp.conv(x, g["psf"]) - bt) + n0 + n1, method="admm", device=device)
    solver = dp.specialize(solver, method="unroll", device=device, max_iter=K, dtype="bf16")
    rhos = torch.tensor(g["rhos"], requires_grad=True)
    l0, l1 = torch.tensor(g["l0"], requires_grad=True), torch.tensor(g["l1"], requires_grad=True)
    xo = solver.solve(x0=T(g["b"], device), rhos=rhos, lams={n0: l0, n1: l1})
    loss = ((xo - gt) ** 2).mean()
    loss.backward()
    assert_close(xo.detach().cpu(), g["tv_x"], TOL, "bf16-history unrolled x (fp32 iteration)")
    assert abs(float(loss.detach()) - float(g["tv_loss"])) <= 1e-5 * abs(float(g["tv_loss"]))
    assert_close(l0.grad.cpu(), g["tv_g_l0"], 1e-5, "bf16 mode d loss / d lam0", maxabs_mult=4.0)
    assert_close(l1.grad.cpu(), g["tv_g_l1"], 1e-5, "bf16 mode d loss / d lam1", maxabs_mult=4.0)
    assert_close(bt.grad.cpu(), g["tv_g_b"], 1e-5, "bf16 mode d loss / d b", maxabs_mult=4.0)
    assert_close(rhos.grad.cpu(), g["tv_g_rhos"], 1e-2, "bf16 mode d loss / d rho (bf16 history)")
    assert rel_l2(rhos.grad.cpu().numpy(), g["tv_g_rhos"]) > 1e-6, "the history should really be bf16"


def case_unrolled_solver(device):
    """G11 (second half): UnrolledSolver with one solver clone per step and learned rho / lambda parameters
    (specialization/unroll.py:21-58)"""
    g = load_golden("g11_unrolled_grads")
    x = dp.Variable()
    n1 = dp.norm1(x)
    b = T(g["b"], device)
    solver = dp.compile(dp.sum_squares(dp.conv(x, g["psf"]) - b) + n1, method="admm", device=device)
    us = dp.specialize(solver, method="unroll", device=device, max_iter=3, share=False, learned_params=True)
    assert len(us.solvers) == 3 and us.solvers[1] is not us.solvers[0]
    assert sorted(n for n, _ in us.named_parameters() if "." not in n) == ["norm1", "rhos"]      # the reference's names (unroll.py:35-38)
    with torch.no_grad():
        us.rhos.copy_(torch.tensor([0.3, 0.2, 0.1]))
        list(us.lams.values())[0].copy_(torch.tensor([0.03, 0.02, 0.012]))
    xo = us.solve(x0=b)
    loss = ((xo - T(g["gt"], device)) ** 2).mean()
    loss.backward()
    assert_close(xo.detach().cpu(), g["us_x"], TOL, "UnrolledSolver x")
    assert_close(us.rhos.grad.cpu(), g["us_g_rhos"], 1e-5, "UnrolledSolver d loss / d rhos", maxabs_mult=4.0)
    assert_close(list(us.lams.values())[0].grad.cpu(), g["us_g_lam"], 5e-5, "UnrolledSolver d loss / d lams")   # (measured 2.4e-5: a sum over threshold masks)
    # a checkpoint in the REFERENCE's format (unroll.py:35-38: `rhos` + one entry per term class, so two norm1 terms share "norm1")
    # loads with strict=True: the suffixed name of the earlier term starts from the class's entry
    xv = dp.Variable()
    two = dp.compile(dp.sum_squares(dp.conv(xv, g["psf"] if "psf" in g else np.ones((3, 3), np.float32) / 9) - b)
                     + dp.norm1(dp.grad(xv, dim=0)) + dp.norm1(dp.grad(xv, dim=1)), method="admm", device=device)
    us2 = dp.specialize(two, method="unroll", device=device, max_iter=3, share=False, learned_params=True)
    ref_ckpt = {k: v for k, v in us2.state_dict().items() if "#" not in k}
    ref_ckpt["rhos"] = torch.tensor([0.3, 0.2, 0.1])
    ref_ckpt["norm1"] = torch.tensor([0.03, 0.02, 0.012])
    us2.load_state_dict(ref_ckpt, strict=True)
    assert all(torch.equal(p.detach().cpu(), ref_ckpt["norm1"]) for p in us2.lams.values())


def case_train(device, tmpdir):
    """dp.train (primitives.py:112-205 restated): an unrolled TV-deconvolution solver with learned rho / lambda schedules trained for
    a few AdamW steps through the solver's own backward pass -- the loss goes down, ``last.pth`` holds what a resumed run needs, and
    resuming after epoch 2 reproduces an uninterrupted run's parameters (same shuffles: the generator is seeded by the epoch)."""
    import synthetic
    gt0, b0, psf = synthetic.deconv_case(4, 1, 32, 32, seed=31, ksize=5, ksigma=1.5)
    data = torch.from_numpy(gt0)
    blur = dp.conv(dp.Variable(), psf).to(device)

    class Schedules(torch.nn.Module):                      # the trained part (README.md:93-116: parameters live in a separate model)
        def __init__(self):
            super().__init__()
            self.rhos = torch.nn.Parameter(torch.full((3,), 0.5))
            self.lam0 = torch.nn.Parameter(torch.full((3,), 0.05))
            self.lam1 = torch.nn.Parameter(torch.full((3,), 0.05))

    def make():
        obs = dp.Placeholder()
        x = dp.Variable()
        n0, n1 = dp.norm1(dp.grad(x, dim=0)), dp.norm1(dp.grad(x, dim=1))
        base = dp.compile(dp.sum_squares(dp.conv(x, psf) - obs) + n0 + n1, method="admm", device=device)
        solver = dp.specialize(base, method="unroll", device=device, max_iter=3)
        m = Schedules().to(device)

        def step_fn(batch):
            g = batch.to(device)
            with torch.no_grad():
                inp = blur.forward(g.contiguous())
            obs.value = inp
            pred = solver.solve(x0=inp, rhos=m.rhos, lams={n0: m.lam0, n1: m.lam1})
            assert base.last_path == "fused", "a Placeholder observation must stay on the fused (differentiable) iteration"
            return g, inp, pred
        return m, step_fn

    us, step_fn = make()
    hist = dp.train(model=us, step_fn=step_fn, dataset=data, savedir=os.path.join(tmpdir, "a"), epochs=3, bs=2, lr=2e-2, weight_decay=0.0)
    assert [h["epoch"] for h in hist] == [0, 1, 2] and hist[-1]["loss"] < hist[0]["loss"], hist
    ck = torch.load(os.path.join(tmpdir, "a", "last.pth"))
    assert set(ck) == {"model", "optimizer", "epoch", "gstep", "psnr", "best_psnr"} and ck["epoch"] == 2 and ck["gstep"] == 6
    # interrupted after 2 epochs, resumed for the third: same parameters as the uninterrupted run
    us2, step2 = make()
    dp.train(model=us2, step_fn=step2, dataset=data, savedir=os.path.join(tmpdir, "b"), epochs=2, bs=2, lr=2e-2, weight_decay=0.0)
    us3, step3 = make()
    hist3 = dp.train(model=us3, step_fn=step3, dataset=data, savedir=os.path.join(tmpdir, "b"), epochs=3, bs=2, lr=2e-2, weight_decay=0.0, resume="last.pth")
    assert len(hist3) == 3
    for (n1, p1), (n3, p3) in zip(us.named_parameters(), us3.named_parameters()):
        assert n1 == n3 and torch.allclose(p1.detach().cpu(), p3.detach().cpu(), rtol=1e-5, atol=1e-7), (n1, p1, p3)
    with pytest.raises(ValueError, match="not supported"):
        dp.train(us)
    with pytest.raises(ValueError, match="no network"):
        dp.train(model=us, step_fn=step_fn, dataset="BSD500", savedir=os.path.join(tmpdir, "c"), epochs=1)


def _assert_grad_close(got, ref, what, tol=1e-4, flip_frac=0.08, flip_rel=5e-2):
    """Gradients through ReLU stacks are piecewise constant in the forward activations: an activation that rounds to the
    other side of 0 (fp32 summation order) flips one mask entry and changes the gradient on one receptive field
    (~10x10 pixels x C = 3 % of a 33x47 fixture) -- in the reference as much as here.  Accept: rel-L2 <= tol, or at most `flip_frac` of the entries
    off by more than tol * max|ref| with the total still within `flip_rel`."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    r = rel_l2(got, ref)
    if r <= tol:
        return
    bad = np.abs(got - ref) > tol * np.abs(ref).max()
    assert bad.mean() <= flip_frac and r <= flip_rel, f"{what}: rel-L2 {r:.3e}, {bad.mean():.2%} of entries off"


def case_ffdnet_grads(device, which=("odd", "even", "gray")):
    """G16: backward-data through the FFDNet stack (transposed MFMA convolutions, fused ReLU masks, adjoint of the
    pixel-unshuffle / replicate padding) vs the reference's autograd; gradients w.r.t. image and sigma.  Tolerance 1e-4
    (ReLU masks make the gradient piecewise constant in the forward activations)."""
    g = load_golden("g16_ffdnet_grads")
    col = _ffdnet("color", device)
    col.requires_grad_(False)
    for tag in ("odd", "even"):
        if tag not in which:
            continue
        x = T(g[f"{tag}_x"], device).requires_grad_(True)
        sig = T(g[f"{tag}_sigma"], device).requires_grad_(True)
        y = col.denoise(x, sig)
        (y * T(g[f"{tag}_w"], device)).sum().backward()
        assert_close(y.detach().cpu(), g[f"{tag}_y"], TOL, f"ffdnet {tag} y (training forward)")
        _assert_grad_close(x.grad.cpu(), g[f"{tag}_gx"], f"ffdnet {tag} d/dx")
        _assert_grad_close(sig.grad.cpu(), g[f"{tag}_gsigma"], f"ffdnet {tag} d/dsigma", tol=1e-2)   # a sum over the image: one mask flip moves it by ~1e-3
    if "gray" not in which:
        return
    gray = _ffdnet("gray", device)
    gray.requires_grad_(False)
    xg = T(g["gray_x"], device).requires_grad_(True)
    sg = torch.tensor(0.1, device=device, requires_grad=True)
    yg = gray.denoise(xg, sg)
    (yg * T(g["gray_w"], device)).sum().backward()
    assert_close(yg.detach().cpu(), g["gray_y"], TOL, "gray y")
    _assert_grad_close(xg.grad.cpu(), g["gray_gx"], "gray d/dx")
    _assert_grad_close(sg.grad.cpu(), g["gray_gsigma"], "gray d/dsigma (summed over bands and images)", tol=1e-2)


def case_ffdnet_split_backward(device, tiny=False):
    """Frozen FFDNet under autograd runs forward AND backward-data on the split kernels (_FFDNetSplitFn: dpx_ffdnet_forward_bf16_save /
    dpx_ffdnet_backward_bf16): d/dx and d/dsigma against the f32-input path (itself pinned against the reference's autograd by G16),
    odd sizes (adjoint of the replicate padding), per-image sigma, colour and gray; and against G16 directly.  tiny: a 3-layer
    16-channel network (the emulator needs minutes for the 12-layer one)."""
    import synthetic
    from dprox.proxfn.pnp.denoisers import FFDNet, FFDNetColorDenoiser
    rng = np.random.RandomState(616)
    shapes = ((2, 3, 17, 21),) if tiny else ((2, 3, 33, 47), (1, 3, 32, 40), (1, 3, 74, 106))     # (37 x 53 after the unshuffle: partial and odd strips of the weight-gradient GEMM)
    for shape in shapes:
        if tiny:
            col = FFDNetColorDenoiser()
            col.model = FFDNet(in_nc=3, out_nc=3, nc=16, nb=3, act_mode="R").load_layers(synthetic.ffdnet_weights(5, 3, 3, 16, 3))
            col = col.to(device)
        else:
            col = _ffdnet("color", device)
        col.requires_grad_(False)
        x0 = rng.rand(*shape).astype(np.float32)
        w0 = rng.randn(*shape).astype(np.float32)
        s0 = np.linspace(0.03, 0.12, shape[0]).astype(np.float32)
        res = {}
        for mode in ("f32", "bf16x3", "f16x2"):
            col.model.compute_mode = mode
            x = T(x0, device).requires_grad_(True)
            sig = T(s0, device).requires_grad_(True)
            y = col.denoise(x, sig)
            assert ("Split" in y.grad_fn.name()) == (mode != "f32"), (mode, y.grad_fn.name())
            (y * T(w0, device)).sum().backward()
            res[mode] = (y.detach().cpu().numpy(), x.grad.cpu().numpy(), sig.grad.cpu().numpy())
        for mode in ("bf16x3", "f16x2"):
            assert_close(res[mode][0], res["f32"][0], TOL, f"split backward {shape} {mode}: forward")
            _assert_grad_close(res[mode][1], res["f32"][1], f"split backward {shape} {mode}: d/dx", tol=1e-5)
            _assert_grad_close(res[mode][2], res["f32"][2], f"split backward {shape} {mode}: d/dsigma", tol=1e-5)
        # the split-f16 backward pass scales the incoming gradient by a power of two (max |gy| -> [8, 16)) and the results back: gradients of
        # the size a mean loss produces (1e-9 of the above, far below binary16's range) and huge ones come out as the same numbers times
        # that factor; the arithmetic of the two passes can also be chosen apart (a split-bf16 forward with a split-f16 backward and v.v.)
        assert col.model.backward_mode == "auto" and col.model.backward_mode_id() == 3
        for fwd, bwd, factor in (("f16x2", "auto", 1e-9), ("f16x2", "auto", 3e7), ("bf16x3", "f16x2", 1e-9), ("f16x2", "bf16x3", 1.0)):
            col.model.compute_mode, col.model.backward_mode = fwd, bwd
            x = T(x0, device).requires_grad_(True)
            sig = T(s0, device).requires_grad_(True)
            (col.denoise(x, sig) * T(w0, device)).sum().mul(factor).backward()
            _assert_grad_close(x.grad.cpu().numpy() / np.float32(factor), res["f32"][1], f"split backward {shape} {fwd}/{bwd} x {factor}: d/dx", tol=1e-5)
            _assert_grad_close(sig.grad.cpu().numpy() / np.float32(factor), res["f32"][2], f"split backward {shape} {fwd}/{bwd} x {factor}: d/dsigma", tol=1e-5)
        col.model.compute_mode, col.model.backward_mode = "f16x2", "auto"
        # trainable weights: forward / backward-data on the split kernels + the weight-gradient GEMM on their C8 planes
        # (k_wgrad_c8, dpx_ffdnet_backward_bf16_w) against everything on the f32-input kernels (dpx_ffdnet_backward): every layer's dW, db
        col.model.compute_mode = "f16x2"
        col.requires_grad_(True)
        wres = {}
        from dprox import _backend as be
        # (True: everything on the f32-input kernels; False: split kernels + the weight-gradient kernel on their C8 planes, k_wgrad_c8, in the
        #  backward pass's arithmetic -- split-f16 on scaled gradients; "c8_bf16x3": the same with a split-bf16 backward pass)
        for f32 in (True, False, "c8_bf16x3"):
            col.model.train_f32 = f32 is True
            col.model.backward_mode = "bf16x3" if f32 == "c8_bf16x3" else "auto"
            col.zero_grad()
            x = T(x0, device).requires_grad_(True)
            y = col.denoise(x, T(s0, device))
            assert ("Split" in y.grad_fn.name()) == (f32 is not True)
            (y * T(w0, device)).sum().mul(1.0 if f32 is True else 1e-6).backward()       # (a mean loss's magnitudes on the split paths)
            sc = np.float32(1.0 if f32 is True else 1e-6)
            wres[f32] = [p.grad.cpu().numpy() / sc for p in col.model.weights + col.model.biases] + [x.grad.cpu().numpy() / sc]
        for other in (False, "c8_bf16x3"):
            for k, (a_, b_) in enumerate(zip(wres[other], wres[True])):
                _assert_grad_close(a_, b_, f"split training path ({other}) {shape}: gradient {k} (weights, biases, d/dx)", tol=1e-5)
        col.requires_grad_(False)
        col.model.train_f32 = False
        col.model.backward_mode = "auto"
    col.model.compute_mode = "f16x2"
    # the range trap of the backward pass: weights that multiply a gradient by far more than the 2^12 of headroom (the forward pass on the
    # split-bf16 arithmetic, which has fp32's range) -- loss.backward() raises, the network's backward pass falls back to split-bf16, and
    # the repeated pass is right
    from dprox import _backend as be
    net = FFDNet(in_nc=3, out_nc=3, nc=16, nb=3, act_mode="R").load_layers(
        [(w * 600.0, b) for w, b in synthetic.ffdnet_weights(5, 3, 3, 16, 3)]).to(device)
    net.requires_grad_(False)
    net.compute_mode, net.backward_mode = "bf16x3", "f16x2"
    x0 = rng.rand(1, 3, 12, 16).astype(np.float32)
    w0 = rng.randn(1, 3, 12, 16).astype(np.float32)
    x = T(x0, device).requires_grad_(True)
    try:
        (net(x, T(np.float32([0.05]), device)) * T(w0, device)).sum().backward()
        raise AssertionError("a split-f16 backward pass whose gradients grow by 1e8 must trip the range trap")
    except be.F16RangeError:
        pass
    assert net.backward_mode == "bf16x3"
    x = T(x0, device).requires_grad_(True)
    (net(x, T(np.float32([0.05]), device)) * T(w0, device)).sum().backward()
    g_split = x.grad.cpu().numpy()
    net.compute_mode = "f32"
    x = T(x0, device).requires_grad_(True)
    (net(x, T(np.float32([0.05]), device)) * T(w0, device)).sum().backward()
    assert np.isfinite(g_split).all()
    _assert_grad_close(g_split, x.grad.cpu().numpy(), "split backward after the range trap's fallback: d/dx", tol=1e-5)


def case_wgrad_c8(device, tiny=False):
    """dpx_conv3x3_wgrad_c8 (k_wgrad_c8: the weight-gradient GEMM on the C8 planes, K = pixels) against the float64 sums it stands for
    (what autograd forms for a 3x3 convolution of network_ffdnet.py:54-68), both arithmetic modes, every instantiated channel-block shape,
    planes with partial / several column strips and fewer rows than a workgroup's share; the `mul` factor; bit-identical repeats."""
    import ctypes
    from dprox import _backend as be
    L = be.lib()
    rng = np.random.RandomState(4242)
    #         cout cin  (first layer, hidden, last layer of the colour and gray stacks; small widths)
    shapes = ((96, 96), (96, 13), (12, 96), (64, 64), (64, 5), (4, 64), (16, 16), (16, 64), (48, 16))
    planes = ((2, 9, 11), (1, 37, 70), (3, 5, 33))
    if tiny:                                                   # (the emulator: ~10 s per 96 -> 96 launch of a few rows)
        shapes, planes = ((96, 96), (64, 64), (16, 13)), ((1, 2, 35),)
    g16 = lambda c: 2 * ((c + 15) // 16)                       # channel groups of 8, whole 16-channel chunks (the split kernels' C8 planes)
    for cout, cin in shapes:
        for B, H, W in planes:
            Gg, Ga = g16(cout), g16(cin)
            g = np.zeros((B, Gg * 8, H, W), np.float32)
            a = np.zeros((B, Ga * 8, H, W), np.float32)
            g[:, :cout] = rng.randn(B, cout, H, W) * 3.0
            a[:, :cin] = np.maximum(rng.randn(B, cin, H, W), 0) * 0.7      # (post-ReLU activations)
            c8 = lambda t: np.ascontiguousarray(t.reshape(B, -1, 8, H, W).transpose(0, 1, 3, 4, 2))
            ap = np.pad(a.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
            ref_w = np.zeros((cout, cin, 3, 3))
            for dy in range(3):
                for dx in range(3):
                    ref_w[:, :, dy, dx] = np.einsum("bohw,bihw->oi", g[:, :cout].astype(np.float64), ap[:, :cin, dy:dy + H, dx:dx + W])
            ref_b = g[:, :cout].astype(np.float64).sum(axis=(0, 2, 3))
            gt, at = T(c8(g), device), T(c8(a), device)
            ws = torch.empty(L.query("dpx_conv3x3_wgrad_c8_ws_bytes", cout, cin), dtype=torch.uint8, device=device)
            mul = T(np.float32([0.25]), device)
            for mode in (3, 6):
                outs = []
                for rep in range(2):
                    gw = torch.full((cout, cin, 3, 3), float("nan"), device=device)
                    gb = torch.full((cout,), float("nan"), device=device)
                    L.call("dpx_conv3x3_wgrad_c8", be.ptr(gt), be.ptr(at), be.ptr(gw), be.ptr(gb), cout, cin, Gg, Ga, mode,
                           be.ptr(mul) if rep else None, B, H, W, be.ptr(ws), be.stream())
                    outs.append((gw.cpu().numpy().astype(np.float64) * (4.0 if rep else 1.0), gb.cpu().numpy().astype(np.float64) * (4.0 if rep else 1.0)))
                what = f"wgrad_c8 {cout}<-{cin} {B}x{H}x{W} mode {mode}"
                assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), what + ": `mul` = 2^-2 must only scale"
                assert_close(outs[0][0], ref_w, 2e-6, what + ": dW")
                assert_close(outs[0][1], ref_b, 2e-6, what + ": db")
    if not tiny:
        assert L.query("dpx_ffdnet_f16_overflow", 1) == 0
        big = T(np.full((1, 2, 4, 8, 8), 7.0e4, np.float32), device)          # an operand beyond the binary16 range trips the trap (mode 3 only)
        gw, gb = torch.empty(16, 16, 3, 3, device=device), torch.empty(16, device=device)
        ws = torch.empty(L.query("dpx_conv3x3_wgrad_c8_ws_bytes", 16, 16), dtype=torch.uint8, device=device)
        L.call("dpx_conv3x3_wgrad_c8", be.ptr(big), be.ptr(big), be.ptr(gw), be.ptr(gb), 16, 16, 2, 2, 6, None, 1, 4, 8, be.ptr(ws), be.stream())
        assert L.query("dpx_ffdnet_f16_overflow", 1) == 0
        L.call("dpx_conv3x3_wgrad_c8", be.ptr(big), be.ptr(big), be.ptr(gw), be.ptr(gb), 16, 16, 2, 2, 3, None, 1, 4, 8, be.ptr(ws), be.stream())
        assert L.query("dpx_ffdnet_f16_overflow", 1) == 1


def case_ffdnet_weight_grads(device):
    """G16 (third part): d/dW, d/db of the FFDNet stack (pixels-as-K MFMA GEMM + deterministic reduction) vs the
    reference's autograd -- first, a middle and the last layer."""
    g = load_golden("g16_ffdnet_grads")
    col = _ffdnet("color", device)
    col.train()
    x = T(g["wg_x"], device)
    # both arithmetic paths of a trainable stack: forward / backward-data on the split kernels + the weight-gradient GEMM on their
    # C8 planes, k_wgrad_c8 (the default), and everything on the f32-input kernels (train_f32)
    for f32 in (True, False):
        col.model.train_f32 = f32
        col.zero_grad()
        (col.denoise(x, torch.tensor([0.05, 0.2], device=device)) * T(g["wg_w"], device)).sum().backward()
        tag = "f32-input kernels" if f32 else "split kernels"
        for li in (0, 5, 11):
            _assert_grad_close(col.model.weights[li].grad.cpu(), g[f"wg_dw{li}"], f"dW layer {li} ({tag})", tol=1e-4, flip_frac=0.02)
            _assert_grad_close(col.model.biases[li].grad.cpu(), g[f"wg_db{li}"], f"db layer {li} ({tag})", tol=1e-4, flip_frac=0.05)
    assert getattr(col.model, "compute_mode", "") not in ("bf16x3", "f16x2") or col.model.last_train_path == "split"
    # run-to-run determinism of the two-stage reduction
    g1 = col.model.weights[5].grad.clone()
    col.zero_grad()
    (col.denoise(x, torch.tensor([0.05, 0.2], device=device)) * T(g["wg_w"], device)).sum().backward()
    assert torch.equal(g1, col.model.weights[5].grad)


def case_unrolled_pnp_grads(device):
    """G16 (second half): 2 unrolled plug-and-play ADMM iterations, gradients w.r.t. rho_t, sigma_t, x0"""
    g = load_golden("g16_ffdnet_grads")
    b = T(g["pnp_b"], device)
    x = dp.Variable()
    den = _ffdnet("color", device)
    den.requires_grad_(False)
    prior = dp.deep_prior(x, denoiser=den)
    solver = dp.compile(dp.sum_squares(dp.conv(x, g["pnp_psf"]) - b) + prior, method="admm", device=device)
    solver = dp.specialize(solver, method="unroll", device=device, max_iter=2)
    rhos = torch.tensor([0.4, 0.2], requires_grad=True)
    sigmas = torch.tensor([0.08, 0.04], requires_grad=True)
    x0 = b.clone().requires_grad_(True)
    xo = solver.solve(x0=x0, rhos=rhos, lams={prior: sigmas})
    loss = ((xo - T(g["pnp_gt"], device)) ** 2).mean()
    loss.backward()
    assert_close(xo.detach().cpu(), g["pnp_x"], TOL, "unrolled PnP x")
    _assert_grad_close(rhos.grad.cpu(), g["pnp_g_rhos"], "unrolled PnP d/d rhos", tol=1e-2)
    _assert_grad_close(x0.grad.cpu(), g["pnp_g_x0"], "unrolled PnP d/d x0")
    gs, rs = sigmas.grad.cpu().numpy(), g["pnp_g_sigmas"]
    assert abs(gs[1]) <= 1e-12 and abs(gs[0] - rs[0]) <= 1e-3 * abs(rs[0]) + 1e-9, (gs, rs)   # tiny: 5e-7 (random weights)


def case_mosaic_jd(device, solve=True):
    """G17: mosaic / mul_elementwise (dpx_mul) and joint demosaic + deconvolution: ADMM whose x-update is CG on
    (conv^T mosaic conv + rho I) with the FFDNet prior (tests/problem/test_jd23.py at fixture size)"""
    from dprox.linalg import LinearSolveConfig
    g = load_golden("g17_mosaic_jd")
    x = T(g["lin_x"], device)
    m = dp.mosaic(dp.Variable()).to(device)
    assert_close(m.forward(x).cpu(), g["mosaic_fwd"], 1e-7, "mosaic forward")
    assert_close(m.adjoint(x).cpu(), g["mosaic_adj"], 1e-7, "mosaic adjoint")
    assert np.array_equal(m.get_diag(x).cpu().numpy(), g["mosaic_diag"])
    me = dp.mul_elementwise(dp.Variable(), g["mul_w"]).to(device)
    assert_close(me.forward(x).cpu(), g["mul_fwd"], 1e-7, "mul_elementwise forward")
    assert_close(me.adjoint(x).cpu(), g["mul_adj"], 1e-7, "mul_elementwise adjoint")
    P = dp.Placeholder()
    mc = dp.mul_color(dp.Variable(), P).to(device)
    P.value = T(g["srf"], device)
    assert_close(mc.forward(x).cpu(), g["mulc_fwd"], 1e-6, "mul_color forward (3 -> 5 channels)")
    assert_close(mc.adjoint(T(g["mulc_x5"], device)).cpu(), g["mulc_adj"], 1e-6, "mul_color adjoint (5 -> 3 channels)")
    wss = dp.weighted_sum_squares(dp.Variable(), dp.mul_elementwise(dp.Variable(), g["mul_w"]), T(g["wss_b"], device)).to(device)
    assert_close(wss.prox(x, torch.tensor([0.3, 1.2], device=device)).cpu(), g["wss_prox"], TOL, "weighted_sum_squares prox")
    if not solve:
        return
    b = T(g["jd_b"], device)
    xv = dp.Variable()
    data = dp.sum_squares(dp.mosaic(dp.conv(xv, g["jd_psf"])) - b)
    reg = dp.deep_prior(xv, denoiser=_ffdnet("color", device))
    prob = dp.Problem(data + reg, linear_solve_config=LinearSolveConfig(max_iters=50))
    with torch.no_grad():
        st = prob.solve(method="admm", device=device, x0=b, rhos=torch.from_numpy(g["jd_rhos"]), lams={reg: torch.from_numpy(g["jd_sigmas"])},
                        max_iter=3, return_full_states=True)
    assert prob.solver.last_path == "fused-cg"           # CG x-update + a Psi term on x itself: the fused split-CG loop
    assert_close(st[0].cpu(), g["jd_x"], TOL, "JD x (CG x-update)")
    assert_close(st[1][0].cpu(), g["jd_v"], TOL, "JD v")


def case_conv2d_generic(device):
    """dpx_conv2d / dpx_space_to_depth / dpx_depth_to_space against plain PyTorch fp32: 3x3 and 1x1, output-channel blocks
    (Cout > 96), bias, fused ReLU, fused residual, odd spatial sizes; stride-2 conv and transposed conv built from them"""
    import torch.nn.functional as F
    from dprox import _ops as ops
    rng = np.random.RandomState(5)
    for (cin, cout, taps, H, W, relu, res, bias) in ((8, 128, 9, 9, 37, False, True, False), (6, 40, 9, 12, 20, True, False, True),
                                                      (16, 200, 1, 10, 33, False, False, True), (4, 3, 9, 7, 5, False, False, False)):
        k = 3 if taps == 9 else 1
        w = torch.from_numpy((rng.randn(cout, cin, k, k) * 0.2).astype("float32")).to(device)
        b = torch.from_numpy(rng.randn(cout).astype("float32")).to(device) if bias else None
        x = torch.from_numpy(rng.randn(2, cin, H, W).astype("float32")).to(device)
        r = torch.from_numpy(rng.randn(2, cout, H, W).astype("float32")).to(device) if res else None
        y = ops.conv2d(x, ops.conv_pack(w.reshape(cout, cin, taps).contiguous(), b, taps), cout, taps, relu=relu, res=r)
        ref = F.conv2d(x, w, b, padding=k // 2)
        ref = F.relu(ref) if relu else ref
        ref = ref + r if res else ref
        assert_close(y.cpu(), ref.cpu(), 2e-6, f"conv2d cin={cin} cout={cout} taps={taps}")
    for dil, (cin, cout, H, W, relu) in ((2, (8, 64, 11, 37, True)), (3, (6, 40, 9, 20, False)), (4, (8, 100, 12, 33, True))):
        w = torch.from_numpy((rng.randn(cout, cin, 3, 3) * 0.2).astype("float32")).to(device)
        b = torch.from_numpy(rng.randn(cout).astype("float32")).to(device)
        x = torch.from_numpy(rng.randn(2, cin, H, W).astype("float32")).to(device)
        y = ops.conv2d(x, ops.conv_pack(w.reshape(cout, cin, 9).contiguous(), b, 9), cout, 9, relu=relu, dilation=dil)
        ref = F.conv2d(x, w, b, padding=dil, dilation=dil)
        assert_close(y.cpu(), (F.relu(ref) if relu else ref).cpu(), 2e-6, f"dilated conv2d d={dil}")
    # weight / bias gradients (dpx_conv2d_wgrad) against PyTorch's autograd of the same fp32 convolution: 3x3 / 1x1, dilation,
    # odd channel counts, more than 96 output channels (blocks), image sizes that are not multiples of the 4x32 pixel tile
    for (cin, cout, taps, dil, H, W) in ((5, 7, 9, 1, 9, 37), (8, 130, 9, 1, 6, 40), (34, 20, 1, 1, 10, 33), (6, 12, 9, 2, 11, 21),
                                         (4, 40, 9, 3, 13, 9), (3, 9, 9, 4, 12, 35)):
        k = 3 if taps == 9 else 1
        w = torch.from_numpy((rng.randn(cout, cin, k, k) * 0.2).astype("float32")).requires_grad_(True)
        b = torch.from_numpy(rng.randn(cout).astype("float32")).requires_grad_(True)
        a = torch.from_numpy(rng.randn(2, cin, H, W).astype("float32"))
        gout = torch.from_numpy(rng.randn(2, cout, H, W).astype("float32"))
        (F.conv2d(a, w, b, padding=(k // 2) * dil, dilation=dil) * gout).sum().backward()
        gw, gb = ops.conv2d_wgrad(gout.to(device), a.to(device), taps, dilation=dil, want_bias=True)
        assert_close(gw.cpu().reshape(cout, cin, k, k), w.grad, 5e-6, f"conv2d_wgrad cin={cin} cout={cout} taps={taps} d={dil}")
        assert_close(gb.cpu(), b.grad, 5e-6, f"conv2d_wgrad bias cin={cin} cout={cout}")
    x = torch.from_numpy(rng.randn(2, 6, 8, 10).astype("float32")).to(device)
    assert torch.equal(ops.space_to_depth(x), F.pixel_unshuffle(x, 2))
    assert torch.equal(ops.depth_to_space(F.pixel_unshuffle(x, 2)), x)
    wd = torch.from_numpy((rng.randn(10, 6, 2, 2) * 0.3).astype("float32")).to(device)
    y = ops.conv2d(ops.space_to_depth(x), ops.conv_pack(wd.reshape(10, 24, 1).contiguous(), None, 1), 10, 1)
    assert_close(y.cpu(), F.conv2d(x, wd, stride=2).cpu(), 2e-6, "2x2 stride-2 conv = space_to_depth + 1x1")
    wt = torch.from_numpy((rng.randn(6, 10, 2, 2) * 0.3).astype("float32")).to(device)
    y = ops.depth_to_space(ops.conv2d(x, ops.conv_pack(wt.permute(1, 2, 3, 0).reshape(40, 6, 1).contiguous(), None, 1), 40, 1))
    assert_close(y.cpu(), F.conv_transpose2d(x, wt, stride=2).cpu(), 2e-6, "2x2 stride-2 transposed conv = 1x1 + depth_to_space")


def case_drunet(device):
    """G20: DRUNet (UNetRes on dpx_conv2d: 3x3 / 1x1 MFMA convolutions with up to 512 channels in blocks of 64, fused ReLU and
    residual adds, space-to-depth / depth-to-space around the strided / transposed 2x2 convolutions) behind
    DRUNetDenoiser: padded single pass, odd sizes, the four-quadrant path, per-image sigma"""
    import oracle as O          # seeded weight generator only
    from dprox.proxfn.pnp.denoisers import DRUNetDenoiser
    g = load_golden("g20_drunet")
    with torch.no_grad():
        den = DRUNetDenoiser(3, O.drunet_weights(21, 4, 3)).to(device)
        y = den.denoise(T(g["color0_x"], device), T(g["color0_sigma"], device))
        assert_close(y.cpu(), g["color0_y"], TOL, "DRUNet colour, 40x52 (padded to 48x64), per-image sigma")
        deng = DRUNetDenoiser(1, O.drunet_weights(22, 2, 1)).to(device)
        y = deng.denoise(T(g["gray0_x"], device), T(g["gray0_sigma"], device))
        assert_close(y.cpu(), g["gray0_y"], TOL, "DRUNet gray, 33x47")
        xb = torch.from_numpy(np.random.RandomState(201).rand(1, 1, 264, 260).astype("float32")).to(device)
        y = deng.denoise(xb, T(g["gray1_sigma"], device))
        assert_close(y.cpu(), g["gray1_y"], TOL, "DRUNet gray, 264x260 (four overlapping quadrants)")
    # input / sigma gradients (frozen weights): per-layer transposed convolutions on the same kernel
    xg = T(g["grad_x"], device).requires_grad_(True)
    sg = torch.tensor([0.05, 0.2], device=device, requires_grad=True)
    (den.denoise(xg, sg) * T(g["grad_w"], device)).sum().backward()
    _assert_grad_close(xg.grad.cpu(), g["grad_gx"], "DRUNet d/dx")
    _assert_grad_close(sg.grad.cpu(), g["grad_gsigma"], "DRUNet d/dsigma", tol=1e-2)
    # weight gradients (trainable denoiser): dpx_conv2d_wgrad for every layer kind -- 3x3 with 64..512 channels (output
    # channels in blocks of 96), the strided 2x2 (1x1 over space-to-depth) and transposed 2x2 (1x1 before depth-to-space)
    den.model.requires_grad_(True)
    (den.denoise(T(g["grad_x"], device), torch.tensor([0.05, 0.2], device=device)) * T(g["grad_w"], device)).sum().backward()
    grads = {n: den.model.ref_param(n).grad.cpu() for n in den.model.ref_keys}
    den.model.requires_grad_(False)
    for n in ("m_head.weight", "m_tail.weight"):
        _assert_grad_close(grads[n], g["wgrad_full_" + n], f"DRUNet dW {n}")
    for key in g:
        if key.startswith("wgrad_corner_"):
            n = key[len("wgrad_corner_"):]
            _assert_grad_close(grads[n][:8, :8], g[key], f"DRUNet dW {n} [:8,:8]")
    norms = dict(zip([str(n) for n in g["wgrad_names"]], g["wgrad_norms"]))
    for n, gr in grads.items():
        assert abs(float(gr.norm()) - norms[n]) <= 2e-3 * norms[n], (n, float(gr.norm()), norms[n])
    # IRCNN: seven dilated 3x3 convolutions (dilation 1,2,3,4,3,2,1), model chosen by the noise-level bin, per band
    import synthetic
    from dprox.proxfn.pnp.denoisers import IRCNNDenoiser
    ird = IRCNNDenoiser(1, {str(k): synthetic.ircnn_weights(31 + k) for k in (3, 12)}).to(device)
    xi = T(g["ircnn_x"], device)
    with torch.no_grad():
        assert_close(ird.denoise(xi, torch.tensor(8 / 255.0, device=device)).cpu(), g["ircnn_y3"], TOL, "IRCNN bin 3")
        assert_close(ird.denoise(xi, torch.tensor(25.5 / 255.0, device=device)).cpu(), g["ircnn_y12"], TOL, "IRCNN bin 12")
    # IRCNN gradients: backward-data through the dilated layers (same kernel, flipped weights, same dilation), weight and
    # bias gradients by dpx_conv2d_wgrad with the dilation-templated apron; accumulated over the two bands
    xig = T(g["ircnn_x"], device).requires_grad_(True)
    sig3 = torch.tensor(8 / 255.0, device=device)
    with torch.no_grad():
        ird.denoise(xig.detach(), sig3)                          # selects the bin-3 model
    ird.model.requires_grad_(True)
    (ird.denoise(xig, sig3) * T(g["ircnn_gw"], device)).sum().backward()
    _assert_grad_close(xig.grad.cpu(), g["ircnn_gx"], "IRCNN d/dx")
    gi = {f"model.{2 * i}.weight": ird.model.weights[i].grad.cpu() for i in range(7)}
    gi.update({f"model.{2 * i}.bias": ird.model.biases[i].grad.cpu() for i in range(7)})
    ird.model.requires_grad_(False)
    for key, name in (("ircnn_g_w0", "model.0.weight"), ("ircnn_g_b0", "model.0.bias"), ("ircnn_g_b6", "model.6.bias"),
                      ("ircnn_g_w12", "model.12.weight"), ("ircnn_g_b12", "model.12.bias")):
        _assert_grad_close(gi[name], g[key], f"IRCNN grad {name}")
    _assert_grad_close(gi["model.6.weight"][:8, :8], g["ircnn_g_w6_corner"], "IRCNN grad model.6.weight [:8,:8] (dilation 4)")
    inorms = dict(zip([str(n) for n in g["ircnn_gnames"]], g["ircnn_gnorms"]))
    for n, gr in gi.items():
        assert abs(float(gr.norm()) - inorms[n]) <= 2e-3 * inorms[n], (n, float(gr.norm()), inorms[n])
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=den)
    assert "deep_prior" in repr(prior)


def case_conv_doe(device):
    """G19: conv_doe -- OTF rebuilt on the device from the PSF value (dpx_cfft2 + dpx_otf_from_full), placeholder-driven,
    through the fused ADMM path"""
    g = load_golden("g19_conv_doe")
    for tag in ("odd", "even"):
        op = dp.conv_doe(dp.Variable(), T(g[f"{tag}_psf"], device)).to(device)
        x = T(g[f"{tag}_x"], device)
        assert_close(op.forward(x).cpu(), g[f"{tag}_fwd"], TOL, f"conv_doe {tag} forward")
        assert_close(op.adjoint(x).cpu(), g[f"{tag}_adj"], TOL, f"conv_doe {tag} adjoint")
        assert_close(op.get_diag(x, freq=True).cpu(), g[f"{tag}_diag"], TOL, f"conv_doe {tag} |OTF|^2")
    xv = dp.Variable()
    P, Y = dp.Placeholder(), dp.Placeholder()
    n0, n1 = dp.norm1(dp.grad(xv, dim=0)), dp.norm1(dp.grad(xv, dim=1))
    fns = dp.sum_squares(dp.conv_doe(xv, P, circular=True), Y) + n0 + n1
    y = T(g["tv_y"], device)
    P.value, Y.value = T(g["tv_psf"], device), y
    solver = dp.compile(fns, method="admm", device=device)
    st = solver.solve(x0=y, rhos=0.2, lams=0.01, max_iter=8, return_full_states=True)
    assert solver.last_path == "fused"
    assert_close(st[0].cpu(), g["tv_x"], TOL, "conv_doe TV x")
    # a new PSF value invalidates the OTF
    P.value = T(g["tv_psf"], device).flip(-1).contiguous()
    x2 = solver.solve(x0=y, rhos=0.2, lams=0.01, max_iter=8)
    assert rel_l2(x2.cpu(), g["tv_x"]) > 1e-3
    # circular=False: pad to 2H x 2H, circular product, crop; the solver takes the op-by-op path (adjoint is the padded one,
    # the denominators the circular |OTF|^2 of the unpadded size, like the reference)
    opl = dp.conv_doe(dp.Variable(), T(g["lin_psf"], device), circular=False).to(device)
    xl = T(g["lin_x"], device)
    assert_close(opl.forward(xl).cpu(), g["lin_fwd"], TOL, "conv_doe linear forward")
    assert_close(opl.adjoint(xl).cpu(), g["lin_adj"], TOL, "conv_doe linear adjoint")
    xv2, yl = dp.Variable(), T(g["lin_y"], device)
    fl = dp.sum_squares(dp.conv_doe(xv2, T(g["lin_psf"], device), circular=False), yl) + dp.norm1(dp.grad(xv2, dim=0)) + dp.norm1(dp.grad(xv2, dim=1))
    sl = dp.compile(fl, method="admm", device=device)
    xs = sl.solve(x0=yl, rhos=0.3, lams=0.01, max_iter=6)
    assert sl.last_path != "fused"
    assert_close(xs.cpu(), g["lin_tv_x"], TOL, "conv_doe linear TV x")


def case_doe_psf_grad(device):
    """G25 -- end-to-end optics (reference README.md:93-116): the PSF of a conv_doe data term is trained through the unrolled solver.
    Loss, x and the gradients w.r.t. the PSF, the observation and the rho / lambda schedules against the reference's autograd
    (there torch.fft ops; here dpx_otf_grad behind the Fourier x-update's backward + one adjoint transform)."""
    g = load_golden("g25_doe_psf_grad")
    for tag in ("a", "b"):
        K = int(g[f"{tag}_K"])
        gt, y0 = T(g[f"{tag}_gt"], device), T(g[f"{tag}_y"], device)
        psf = T(g[f"{tag}_psf"], device).clone().requires_grad_(True)
        y = y0.clone().requires_grad_(True)
        xv = dp.Variable()
        P, Y = dp.Placeholder(), dp.Placeholder()
        n0, n1 = dp.norm1(dp.grad(xv, dim=0)), dp.norm1(dp.grad(xv, dim=1))
        fns = dp.sum_squares(dp.conv_doe(xv, P, circular=True), Y) + n0 + n1
        P.value, Y.value = psf, y
        solver = dp.compile(fns, method="admm", device=device)
        solver = dp.specialize(solver, method="unroll", device=device, max_iter=K)
        rhos = torch.full((K,), 0.2, requires_grad=True, device=device)
        lam = torch.full((K,), 0.01, requires_grad=True, device=device)
        xo = solver.solve(x0=y0, rhos=rhos, lams={n0: lam, n1: lam})
        loss = ((xo - gt) ** 2).mean()
        loss.backward()
        assert_close(xo.detach().cpu(), g[f"{tag}_x"], TOL, f"doe {tag} x")
        lv, lr = float(loss.detach().double()), float(g[f"{tag}_loss"])
        assert abs(lv - lr) <= 1e-5 * abs(lr), (lv, lr)
        for name, got in (("g_psf", psf.grad), ("g_y", y.grad), ("g_rhos", rhos.grad), ("g_lam", lam.grad)):
            assert got is not None, f"doe {tag}: no gradient reached {name}"
            r = rel_l2(got.detach().cpu().numpy(), g[f"{tag}_{name}"])
            record(f"doe {tag} {name} vs the reference's autograd", r, 1e-4)
            assert r <= 1e-4, (tag, name, r)


def case_train_unrolled_pnp_full_size(device, tol_pred=1e-5, tol_grad=1e-4):
    """G39 -- the training workload `bench.py` times (`train_unrolled_pnp`: the reference's published throughput figure) at its own size: 2 x 3 x
    768 x 768, ADMM unrolled x 10 on a conv_doe data term + frozen FFDNet-colour prior, MSE loss; the first step's forward result, loss and the
    gradients w.r.t. the PSF (through the data term and through the simulated observation), rho_t and sigma_t^2 against the reference's
    autograd.  Bars: 1e-5 on the forward result and the loss, 1e-4 on the gradients (measured on the MI355X: prediction 2.3e-6, loss 8e-8,
    d/d rho_t 4e-8, d/d sigma_t^2 3.7e-6, d/d PSF 2.5e-7; profiles/r5_parity_achieved_gpu.json)."""
    import synthetic
    g = load_golden("g39_train_unrolled_pnp")
    bs, size, iters, k = 2, 768, 10, 15
    rng = np.random.RandomState(int(g["seed"]))
    gt = T(synthetic.synth_detail(rng, bs, 3, size, size), device)
    psf0 = synthetic.point_spread_function(k, 5.0)
    full = np.zeros((1, 3, size, size), np.float32)
    full[:, :, :k, :k] = psf0[:, :, 0]
    full = np.roll(full, (size // 2 - k // 2, size // 2 - k // 2), axis=(-2, -1))
    noise = T((rng.randn(bs, 3, size, size) * 7.65 / 255).astype(np.float32), device)
    psf = T(full, device).clone()
    psf = (psf / psf.sum(dim=(-2, -1), keepdim=True)).detach().requires_grad_(True)
    rhos = T(g["rhos"], device).clone().requires_grad_(True)
    lams = T(g["lams"], device).clone().requires_grad_(True)
    x, P, Bv = dp.Variable(), dp.Placeholder(), dp.Placeholder()
    reg = dp.deep_prior(x, denoiser=_ffdnet("color", device))
    solver = dp.compile(dp.sum_squares(dp.conv_doe(x, P, circular=True), Bv) + reg, method="admm", device=device)
    solver = dp.specialize(solver, method="unroll", device=device, max_iter=iters)
    blur = dp.conv_doe(dp.Variable(), P, circular=True).to(device)
    P.value = psf
    inp = blur.forward(gt) + noise
    Bv.value = inp
    pred = solver.solve(x0=inp.detach(), rhos=rhos, lams={reg: lams.sqrt()})
    loss = ((pred - gt) ** 2).mean()
    loss.backward()
    _check_packed(g, "inp", inp.detach(), 8, TOL, what="train step: observation ")
    r = rel_l2(pred.detach()[..., ::8, ::8].cpu().numpy(), g["pred"])
    record("train step 2 x 3 x 768^2: prediction samples vs the reference", r, tol_pred)
    assert r <= tol_pred, r
    lv, lr = float(loss.detach().double()), float(g["loss"])
    record("train step 2 x 3 x 768^2: loss", abs(lv - lr) / abs(lr), tol_pred)
    assert abs(lv - lr) <= tol_pred * abs(lr), (lv, lr)
    h0 = size // 2 - 16
    for name, got, ref in (("d/d rho_t", rhos.grad, g["g_rhos"]), ("d/d sigma_t^2", lams.grad, g["g_lams"]),
                           ("d/d PSF (32 x 32 window around its support)", psf.grad[..., h0:h0 + 32, h0:h0 + 32], g["g_psf"])):
        assert got is not None, name
        e = rel_l2(got.detach().cpu().numpy(), ref)
        record(f"train step 2 x 3 x 768^2: {name} vs the reference's autograd", e, tol_grad)
        assert e <= tol_grad, (name, e)
    e = abs(float(psf.grad.double().norm()) - float(g["g_psf_l2"])) / float(g["g_psf_l2"])
    record("train step 2 x 3 x 768^2: |d/d PSF|_2 over the whole plane", e, tol_grad)
    assert e <= tol_grad, e


def case_linop_autograd(device):
    """Built-in linear nodes under autograd (the reference's operators are eager torch ops: tests/test_linop.py:64-80 back-propagates
    through ``sum``): d/dx of <w, K x> is K^T w for every built-in K, including expressions with a shared variable, and uint8 /
    permuted inputs are accepted like the reference's operators accept them."""
    import synthetic
    rng = np.random.RandomState(31)
    psf = synthetic.point_spread_function(9, 2.0)
    x = dp.Variable()
    exprs = [dp.conv(x, psf), dp.grad(x, dim=0) + dp.grad(x, dim=1), 2.0 * dp.conv(x, psf) - 0.5 * dp.grad(x, dim=1), dp.mosaic(x)]
    for e in exprs:
        K = dp.CompGraph(e.to(device))
        xt = torch.from_numpy(rng.randn(2, 3, 24, 32).astype(np.float32)).to(device).requires_grad_(True)
        w = torch.from_numpy(rng.randn(2, 3, 24, 32).astype(np.float32)).to(device)
        y = K.forward(xt)
        (y * w).sum().backward()
        assert_close(xt.grad.cpu(), K.adjoint(w).cpu(), 1e-6, f"d/dx <w, Kx> = K^T w for {e}")
    x1, x2 = dp.Variable(), dp.Variable()
    K = dp.CompGraph((x1 + x2).to(device))
    v1 = torch.randn(4, 4, device=device, requires_grad=True)
    v2 = torch.randn(4, 4, device=device)
    out = K.forward(v1, v2)
    assert torch.allclose(out, v1 + v2)
    out.mean().backward()
    assert torch.allclose(v1.grad, torch.full_like(v1.grad, 1 / 16))
    img8 = torch.from_numpy((rng.rand(24, 32, 3) * 255).astype(np.uint8)).permute(2, 0, 1)[None].to(device)     # HWC uint8 -> NCHW view
    K = dp.CompGraph(dp.conv(dp.Variable(), psf).to(device))
    assert_close(K.forward(img8).cpu(), K.forward(img8.float().contiguous()).cpu(), 1e-7, "uint8 / permuted input")


def case_doe_op_autograd(device):
    """conv_doe.forward / adjoint under autograd (the reference's are torch.fft ops, linop/conv.py:97-135): gradients w.r.t. the
    image and the PSF against the same convolution written with torch.fft on the CPU (psf2otf2's padding and shift included)."""
    from dprox.linop.fourier import _doe_padded
    rng = np.random.RandomState(26)
    for (B, C, H, W, f) in ((2, 3, 24, 24, 7), (1, 1, 20, 24, 5)):
        psf0 = torch.from_numpy((rng.rand(1, C, f, f + (W - H)) ** 2).astype(np.float32))
        x0 = torch.from_numpy(rng.randn(B, C, H, W).astype(np.float32))
        w = torch.from_numpy(rng.randn(B, C, H, W).astype(np.float32))
        for adj in (False, True):
            psf, x = psf0.clone().to(device).requires_grad_(True), x0.clone().to(device).requires_grad_(True)
            op = dp.conv_doe(dp.Variable(), psf).to(device)
            y = op.adjoint(x) if adj else op.forward(x)
            (y * w.to(device)).sum().backward()
            pr, xr = psf0.clone().double().requires_grad_(True), x0.clone().double().requires_grad_(True)
            O = torch.fft.fft2(_doe_padded(pr, x0.shape))
            yr = torch.fft.ifft2((O.conj() if adj else O) * torch.fft.fft2(xr)).real
            (yr * w.double()).sum().backward()
            assert_close(y.detach().cpu(), yr.detach().float(), TOL, f"conv_doe {'adjoint' if adj else 'forward'} under autograd")
            assert_close(x.grad.cpu(), xr.grad.float(), 1e-5, "conv_doe d/d image")
            assert_close(psf.grad.cpu(), pr.grad.float(), 1e-5, "conv_doe d/d psf")


def case_sisr(device, solve=True):
    """G18: closed-form super-resolution data term (dpx_cfft2 + dpx_sisr_update), sf = 2 and 3, and the reference's
    super-resolution example (sisr + FFDNet prior, ADMM with the data term's own x-update)"""
    g = load_golden("g18_sisr")
    for sf in (2, 3):
        x = dp.Variable()
        fn = dp.sisr(x, T(g[f"sf{sf}_y"], device), kernel=g["psf"], sf=sf).to(device)
        v = T(g[f"sf{sf}_v"], device)
        assert_close(fn._prox(v, torch.tensor(0.4, device=device), 1).cpu(), g[f"sf{sf}_prox_scalar"], TOL, f"sisr sf={sf} scalar lam")
        assert_close(fn._prox(v, torch.tensor([0.2, 0.9], device=device), 2).cpu(), g[f"sf{sf}_prox_B"], TOL, f"sisr sf={sf} per-image lam")
    if not solve:
        return
    x = dp.Variable()
    data = dp.sisr(x, T(g["sr_y"], device), kernel=g["psf"], sf=2)
    reg = dp.deep_prior(x, denoiser=_ffdnet("color", device))
    prob = dp.Problem(data + reg)
    with torch.no_grad():
        st = prob.solve(method="admm", device=device, x0=T(g["sr_x0"], device), rhos=torch.from_numpy(g["sr_rhos"]),
                        lams={reg: torch.from_numpy(g["sr_sigmas"])}, max_iter=3, return_full_states=True)
    assert_close(st[0].cpu(), g["sr_x"], TOL, "super-resolution x")
    assert_close(st[1][0].cpu(), g["sr_v"], TOL, "super-resolution v")


def case_csmri(device, solve=True):
    """G15: closed-form csmri data term (native complex FFT + masked update) and CustomADMM on a complex iterate"""
    from dprox.contrib.csmri import CustomADMM
    g = load_golden("g15_csmri")
    y, mask = T(g["y"], device), T(g["mask"], device)
    x = dp.Variable()
    yp, mp = dp.Placeholder(), dp.Placeholder()
    yp.value, mp.value = y, mask
    fn = dp.csmri(x, mp, yp).to(device)
    v = T(g["prox_v"], device)
    assert_close(fn._prox(v, torch.tensor(0.7, device=device), 1).cpu(), g["prox_lam_scalar"], TOL, "csmri prox scalar lam")
    assert_close(fn._prox(v, torch.tensor([0.3, 1.9], device=device), 2).cpu(), g["prox_lam_B"], TOL, "csmri prox per-image lam")
    if not solve:
        return
    x2 = dp.Variable()
    y2, m2 = dp.Placeholder(), dp.Placeholder()
    data = dp.csmri(x2, m2, y2)
    reg = dp.deep_prior(x2, denoiser=_ffdnet("gray", device))
    solver = CustomADMM([reg], [data]).to(device)
    y2.value, m2.value = y, mask
    with torch.no_grad():
        st = solver.solve(x0=T(g["x0"], device), rhos=torch.from_numpy(g["rhos"]), lams={reg: torch.from_numpy(g["sigmas"])}, max_iter=4,
                          return_full_states=True)
    assert solver.last_path == "generic"
    assert_close(st[0].cpu(), g["x"], TOL, "CustomADMM x (prior output)")
    assert_close(st[1][0].cpu(), g["z"], TOL, "CustomADMM z (data-term output)")
    assert_close(st[2][0].cpu(), g["u"], TOL, "CustomADMM u")


def case_other_algorithms(device):
    """G14: ADMM_vxu / Pock-Chambolle through the generic path (same HIP primitives, different update order), HQS through the
    fused stages (dual variables pinned to zero) and op by op"""
    g = load_golden("g14_other_algorithms")
    b = T(g["b"], device)
    for method in ("admm_vxu", "hqs", "pc"):
        x = dp.Variable()
        fns = dp.sum_squares(dp.conv(x, g["psf"]) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1)) + dp.nonneg(x)
        prob = dp.Problem(fns)
        out = prob.solve(method=method, device=device, x0=b, rhos=0.3, lams=0.01, max_iter=6)
        assert_close(out.cpu(), g[method], TOL, method)
        if method in ("hqs", "admm_vxu"):   # recognised problems: the fused rhs / solve / z stages (hqs: duals pinned to zero) ...
            assert prob.solver.last_path == "fused"
            prob.solver.use_fused = False                        # ... and the op-by-op iteration give the same answer
            out2 = prob.solver.solve(x0=b, rhos=0.3, lams=0.01, max_iter=6)
            assert prob.solver.last_path == "generic"
            assert_close(out2.cpu(), g[method], TOL, f"{method} (op by op)")


def case_hqs_pow2(device):
    """G36: half-quadratic splitting on a power-of-two plane = the two-kernel ADMM iteration with DPX_TERM_NO_DUAL (duals counted as
    zero, right-hand side rho sum K_i^T v_i) against the reference's state, and against the op-by-op iteration"""
    import synthetic
    from dprox import _ops as ops
    g = load_golden("g36_hqs_pow2")
    gt, b0, psf = synthetic.deconv_case(1, 3, 256, 256, seed=int(g["seed"]))
    b = T(b0, device)
    x = dp.Variable()
    fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1)) + dp.nonneg(x)
    prob = dp.Problem(fns)
    rhos = torch.from_numpy(g["rhos"])
    calls = []
    real = ops.admm_run
    ops.admm_run = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        xs, vs = prob.solve(method="hqs", device=device, x0=b, rhos=rhos, lams=0.01, max_iter=6, return_full_states=True)
    finally:
        ops.admm_run = real
    assert calls and prob.solver.last_path == "fused", "half-quadratic splitting did not run on the two-kernel iteration"
    _check_packed(g, "x", xs, 4, TOL, what="hqs pow2 ")
    for i in range(3):
        _check_packed(g, f"v{i}", vs[i], 8, TOL, scale_key="x", what="hqs pow2 ", scale_sub=2)
    prob.solver.use_fused = False
    out2 = prob.solver.solve(x0=b, rhos=rhos, lams=0.01, max_iter=6)
    assert prob.solver.last_path == "generic"
    assert_close(xs.cpu(), out2.cpu(), TOL, "hqs pow2: two-kernel vs op by op")


def case_fresh_state(device, shapes=((2, 1, 256, 256),), iters=3):
    """The fresh-state shortcut (state straight from ADMM.initialize: the first right-hand side formed from x0 alone --
    dpx_admm_seed_rows_fresh -- and the zero duals not streamed in the first iteration -- DPX_TERM_U_ZERO) against the same solve
    started from a state that has been touched (general seed pass, duals read): x, v_i, u_i bit-identical where both seeds run the same
    transform code (plain kernels), within one transform's round-off where the fresh seed is the streaming kernel."""
    import synthetic
    from dprox import _backend as be
    from dprox import _ops as ops
    L = be.lib()
    try:
        for (B, C, H, W) in shapes:
            for rows_mode, with_h in ((1, True), (2, True), (1, False)):      # (1, False): no grad_H term -- the streaming seed's halo-free walk
                L.call("dpx_admm_iter_config", rows_mode, 0)
                gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=77 + H)
                b = T(b0, device)
                x = dp.Variable()
                fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=1)) + dp.nonneg(x)
                if with_h:
                    fns = fns + dp.norm1(dp.grad(x, dim=0))
                s = dp.compile(fns, method="admm", device=device)
                x0 = b.clone()
                seeds = []
                real = ops.admm_seed_rows
                ops.admm_seed_rows = lambda *a, **k: (seeds.append(k.get("fresh_x") is not None), real(*a, **k))[1]
                try:
                    fresh = s.solve(x0=x0, rhos=0.3, lams=0.01, max_iter=iters, return_full_states=True)
                    _, rhos, lams, _ = s.defaults(x0, 0.3, 0.01, iters)
                    st = s.initialize(x0)
                    st[2][0].add_(0.0)                       # a write: the state no longer counts as fresh
                    touched = s.iters(st, rhos.to(device), {k: v.to(device) for k, v in lams.items()}, iters)
                finally:
                    ops.admm_seed_rows = real
                assert seeds == [True, False], seeds
                for a, c in zip([fresh[0]] + list(fresh[1]) + list(fresh[2]), [touched[0]] + list(touched[1]) + list(touched[2])):
                    if rows_mode == 2:          # both seeds on k_seed_rows (one transform, two instantiations): bit-identical
                        assert torch.equal(a, c), ("fresh-state shortcut differs", (B, C, H, W), rows_mode, float((a - c).abs().max()))
                    else:                       # streaming seed (k_seed_rows_seq: the row kernel's transform) against k_seed_rows: round-off of one transform
                        err = float((a - c).abs().max())          # (images of O(1); the duals are clamped to lam / rho ~ 0.03)
                        assert err <= 2e-6, ("fresh-state shortcut differs", (B, C, H, W), rows_mode, err)
    finally:
        L.call("dpx_admm_iter_config", 0, 0)


def case_solve_x_only(device, shapes=((2, 1, 256, 256),), iters=4, configs=None):
    """solve() hands back x alone, so its last row pass stores x and skips the final z / dual update (emit mode 2: the no-dual
    instantiation of the streaming row kernel in its x-only mode, own rows of each band, no halo).  Against the same solve with
    return_full_states=True (the emitting pass: x, v and the duals, with its emit-aware wait counts) and against a callback run
    (every pass emits): BIT-identical x; ADMM and half-quadratic splitting; equal bands and ragged ones (bands of 8 and 9 rows)."""
    import synthetic
    from dprox import _backend as be
    L = be.lib()
    try:
        for (B, C, H, W) in shapes:
            gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=91 + H)
            b = T(b0, device)
            for method, bands in (configs or [(m_, b_) for m_ in ("admm", "hqs") for b_ in (0, H // 8, 30)]):
                if True:
                    L.call("dpx_admm_iter_config", 1, bands)
                    x = dp.Variable()
                    fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
                    s = dp.compile(fns, method=method, device=device)
                    kw = dict(x0=b, rhos=torch.linspace(0.4, 0.2, iters), lams=0.01, max_iter=iters)
                    xa = s.solve(**kw)
                    assert s.last_path == "fused"
                    full = s.solve(return_full_states=True, **kw)
                    seen = []
                    xc = s.solve(callback=lambda **k: seen.append(k["state"][0].clone()), **kw)
                    assert len(seen) == iters
                    assert torch.equal(xa, full[0]), ("x-only pass differs from the emitting pass", method, bands, float((xa - full[0]).abs().max()))
                    assert torch.equal(xa, xc) and torch.equal(xa, seen[-1]), ("callback run differs", method, bands)
                    # the full state is a state: continuing from it equals a longer solve
                    if method == "admm" and bands == 0:
                        sched = torch.cat([torch.linspace(0.4, 0.2, iters), torch.tensor([0.15, 0.1])])
                        _, rhos, lams, _ = s.defaults(b, sched, 0.01, iters + 2)
                        rd, ld = rhos.to(device), {k: v.to(device) for k, v in lams.items()}
                        longer = s.solve(x0=b, rhos=sched, lams=0.01, max_iter=iters + 2)
                        cont = s.iters(tuple(full), rd[..., iters:].contiguous(), {k: v[..., iters:].contiguous() for k, v in ld.items()}, 2)
                        rel = float((cont[0] - longer).norm() / longer.norm())
                        assert rel < 2e-6, ("continuing from the emitted state", rel)
    finally:
        L.call("dpx_admm_iter_config", 0, 0)


def case_sub_batch_chains(device, shapes=((4, 1, 256, 256),), iters=13, methods=("admm", "hqs"), nchs=(2, 3, 4), twice=True):
    """The two-kernel iteration run as independent sub-batch chains (FusedADMM._run_chains: own spectrum buffers and data spectrum per
    chain, separate streams on the GPU, launches issued in turns of 10 iterations) against the one-chain run: BIT-identical full
    states and x-only results, for 2 / 3 / 4 chains (uneven sub-batches included), ADMM and half-quadratic splitting, per-image rho."""
    import os
    import synthetic
    old = os.environ.get("DPX_CHAINS")
    try:
        for (B, C, H, W) in shapes:
            gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=17 + B + H)
            b = T(b0, device)
            rhos = torch.linspace(0.5, 0.2, iters)[None, :] * torch.linspace(1.0, 1.5, B)[:, None]     # [B, T]: every image its own schedule
            for method in methods:
                def run(nch, full):
                    os.environ["DPX_CHAINS"] = str(nch)
                    x = dp.Variable()
                    fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1)) + dp.nonneg(x)
                    s = dp.compile(fns, method=method, device=device)
                    out = s.solve(x0=b, rhos=rhos, lams=0.01, max_iter=iters, return_full_states=full)
                    assert s.last_path == "fused"
                    flat = lambda st: [st] if torch.is_tensor(st) else [t for part in st for t in (part if isinstance(part, (list, tuple)) else [part])]
                    if twice:
                        again = s.solve(x0=b, rhos=rhos, lams=0.01, max_iter=iters, return_full_states=full)      # cached data spectra of the chains
                        for p_, q_ in zip(flat(out), flat(again)):
                            assert torch.equal(p_, q_)
                    return flat(out)
                ref_full, ref_x = run(1, True), run(1, False)
                assert torch.equal(ref_full[0], ref_x[0])
                for nch in nchs:
                    if nch > B:
                        continue
                    for got, ref in ((run(nch, True), ref_full), (run(nch, False), ref_x)):
                        assert len(got) == len(ref)
                        for a, c in zip(got, ref):
                            assert torch.equal(a, c), ("sub-batch chains differ from the one-chain run", (B, C, H, W), method, nch, float((a - c).abs().max()))
            if str(device) != "cpu":                            # proximal gradient descent: the same split of dpx_pgd_run (streams: GPU only)
                def run_pgd(nch):
                    os.environ["DPX_CHAINS"] = str(nch)
                    x = dp.Variable()
                    s = dp.compile(dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(x) * 0.5, method="pgd", device=device)
                    return s.solve(x0=b, rhos=rhos * 0.5, lams=0.01, max_iter=iters)
                ref = run_pgd(1)
                for nch in nchs:
                    if nch <= B:
                        got = run_pgd(nch)
                        assert torch.equal(got, ref), ("pgd sub-batch chains differ", (B, C, H, W), nch, float((got - ref).abs().max()))
    finally:
        if old is None:
            os.environ.pop("DPX_CHAINS", None)
        else:
            os.environ["DPX_CHAINS"] = old


def case_row_parallel_kernel(device, shapes=((1, 2, 256, 256),), iters=5, methods=("admm", "hqs", "admm_vxu"), nterms_list=(2, 3, 4), hfirst=(True, False)):
    """The row-parallel kernel of launches with few planes (k_iter_rows_par, dpx_iter_par.hip: the rows of a band transformed side by
    side in one 16-wave workgroup, stencil neighbours through LDS) against the streaming band walker (k_iter_rows_seq): BIT-identical
    full states, x-only results and callback runs -- ADMM, half-quadratic splitting (no-dual instantiation) and the v, x, u order; two
    to four terms, the grad_H term first or behind the others (the accumulation order of the K^T terms is the streaming kernel's:
    terms behind grad_H wait for phase C), per-image rho schedules, ragged bands (H not a multiple of the workgroup's own rows)."""
    import synthetic
    from dprox import _backend as be
    L = be.lib()
    try:
        for (B, C, H, W) in shapes:
            gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=61 + W + B)
            b = T(b0, device)
            rhos = torch.linspace(0.5, 0.2, iters)[None, :] * torch.linspace(1.0, 1.3, B)[:, None]
            for method in methods:
                for nterms in nterms_list:
                    for hf in hfirst:
                        def run(mode, kind):
                            L.call("dpx_admm_iter_config", mode, 0)
                            x = dp.Variable()
                            gh, gw = dp.norm1(dp.grad(x, dim=0)), dp.norm1(dp.grad(x, dim=1))
                            fns = dp.sum_squares(dp.conv(x, psf) - b) + (gh + gw if hf else gw + gh)
                            if nterms >= 3:
                                fns = fns + dp.nonneg(x)
                            if nterms >= 4:
                                fns = fns + dp.norm1(x) * 0.5
                            if not hf and nterms >= 3:        # grad_H last: every other term in front of it
                                fns = dp.sum_squares(dp.conv(x, psf) - b) + gw + dp.nonneg(x) + (dp.norm1(x) * 0.5 + gh if nterms >= 4 else gh)
                            s = dp.compile(fns, method=method, device=device)
                            kw = dict(x0=b, rhos=rhos, lams=0.01, max_iter=iters)
                            if kind == "full":
                                st = s.solve(return_full_states=True, **kw)
                                out = [st[0]] + list(st[1]) + (list(st[2]) if len(st) > 2 else [])
                            elif kind == "x":
                                out = [s.solve(**kw)]
                            else:
                                seen = []
                                s.solve(callback=lambda **k: seen.append(k["state"][0].clone()), **kw)
                                out = seen
                            assert s.last_path == "fused"
                            return out
                        for kind in ("full", "x", "callback"):
                            seq, par = run(1, kind), run(3, kind)
                            assert len(seq) == len(par)
                            for a, c in zip(seq, par):
                                assert torch.equal(a, c), ("row-parallel kernel differs from the streaming kernel", (B, C, H, W), method, nterms, hf, kind,
                                                           float((a - c).abs().max()))
    finally:
        L.call("dpx_admm_iter_config", 0, 0)


def case_hqs_nodual_kernel(device, shapes=((1, 2, 256, 256),), iters=4, nterms_list=(1, 2, 3, 4)):
    """Half-quadratic splitting on the streaming row kernel's no-dual variant (k_iter_rows_seq<..., DUAL = false>: the duals are
    neither fetched nor stored, its wait counts are the general kernel's minus the dual streams) against the lock-step ring-buffer
    kernel (no LDS-DMA, no hand-counted waits), for one to four terms; bit-identical across band partitions."""
    import synthetic
    from dprox import _backend as be
    L = be.lib()
    try:
        for (B, C, H, W) in shapes:
            gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=55 + W)
            b = T(b0, device)
            for nterms in nterms_list:
                def run(mode, bands):
                    L.call("dpx_admm_iter_config", mode, bands)
                    x = dp.Variable()
                    fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0))
                    if nterms >= 2:
                        fns = fns + dp.norm1(dp.grad(x, dim=1))
                    if nterms >= 3:
                        fns = fns + dp.nonneg(x)
                    if nterms >= 4:
                        fns = fns + dp.norm1(x) * 0.5
                    s = dp.compile(fns, method="hqs", device=device)
                    st = s.solve(x0=b, rhos=torch.linspace(0.4, 0.2, iters), lams=0.01, max_iter=iters, return_full_states=True)
                    assert s.last_path == "fused"
                    return [st[0]] + list(st[1])
                seq = run(1, 0)
                seq2 = run(1, 16)
                lock = run(2, 0)
                for a, c in zip(seq, seq2):
                    assert torch.equal(a, c), ("no-dual kernel: band partitions differ", (B, C, H, W), nterms)
                tol = 2e-4 if nterms == 1 else 1e-5          # (one gradient term: a line of ~eps denominators)
                for a, c in zip(seq, lock):
                    assert float((a - c).abs().max()) <= tol * max(float(c.abs().max()), 1.0), ((B, C, H, W), nterms, float((a - c).abs().max()))
    finally:
        L.call("dpx_admm_iter_config", 0, 0)


def case_pgd_streaming_rows(device, shapes=((1, 2, 256, 256),), iters=4):
    """dpx_pgd_run's streaming row pass (k_pgd_rows_seq: LDS-DMA prefetch one row ahead, hand-counted waits) against the plain
    one-wave-per-row kernel (k_pgd_rows): the same arithmetic on the same table values, so the iterates agree to fp32 round-off of a few
    differently contracted multiply-adds; and BIT-identical across band partitions (a wait that returned early would read a stale or
    half-landed row in some partition).  With and without a K^T b term, three proxes."""
    import synthetic
    from dprox import _backend as be
    L = be.lib()
    try:
        for (B, C, H, W) in shapes:
            gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=73 + W)
            b = T(b0, device)
            T_lanes = W // 16
            per_block = 4 * (64 // T_lanes)
            cands = [nb for nb in (1, 2, 4, 8, 16, 32, 64, 128, 256) if nb <= H and (B * C * nb) % per_block == 0]
            for reg in ("l1", "nonneg", "l2"):
                def run(mode, bands):
                    L.call("dpx_admm_iter_config", mode, bands)
                    x = dp.Variable()
                    g = {"l1": dp.norm1(x), "nonneg": dp.nonneg(x), "l2": dp.norm2(x) if hasattr(dp, "norm2") else dp.norm1(x)}[reg]
                    s = dp.compile(dp.sum_squares(dp.conv(x, psf) - b) + g, method="pgd", device=device)
                    return s.solve(x0=b, rhos=0.8, lams=0.01, max_iter=iters)
                outs = [run(1, nb) for nb in (cands[0], cands[len(cands) // 2], cands[-1])]
                for o in outs[1:]:
                    assert torch.equal(outs[0], o), ("streaming PGD rows: band partitions differ", (B, C, H, W), reg)
                plain = run(2, 0)
                err = float((outs[0] - plain).abs().max()) / max(float(plain.abs().max()), 1e-30)
                record(f"pgd streaming rows vs plain kernel {B}x{C}x{H}x{W} {reg}", err, 1e-6)
                assert err <= 1e-6, ((B, C, H, W), reg, err)
    finally:
        L.call("dpx_admm_iter_config", 0, 0)


def case_vxu_two_kernel(device, shapes=((1, 2, 256, 256),), iters=5, nterms_list=(2, 3, 4)):
    """ADMM in the order v, x, u (admm.py:103-120) on the two-kernel iteration (DPX_TERM_VXU: the planes carry q = u' - v, the row pass
    forms the dual with the fresh x and the next v-update) against the op-by-op iteration of the same solver -- full state (z, v_i,
    u_i), one to four terms, both row kernels."""
    import synthetic
    from dprox import _backend as be
    from dprox import _ops as ops
    L = be.lib()
    try:
        for (B, C, H, W) in shapes:
            gt, b0, psf = synthetic.deconv_case(B, C, H, W, seed=91 + W)
            b = T(b0, device)
            for nterms in nterms_list:     # (a single gradient term leaves a line of ~eps denominators: two correct evaluation orders differ by 6e-3 there)
                def build():
                    x = dp.Variable()
                    fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0))
                    if nterms >= 2:
                        fns = fns + dp.norm1(dp.grad(x, dim=1))
                    if nterms >= 3:
                        fns = fns + dp.nonneg(x)
                    if nterms >= 4:
                        fns = fns + dp.norm1(x) * 0.5
                    return dp.compile(fns, method="admm_vxu", device=device)
                rhos = torch.linspace(0.4, 0.2, iters)
                s = build()
                s.use_fused = False
                ref = s.solve(x0=b, rhos=rhos, lams=0.01, max_iter=iters, return_full_states=True)
                assert s.last_path == "generic"
                for mode in (1, 2):
                    L.call("dpx_admm_iter_config", mode, 0)
                    calls = []
                    real = ops.admm_run
                    ops.admm_run = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
                    try:
                        s2 = build()
                        got = s2.solve(x0=b, rhos=rhos, lams=0.01, max_iter=iters, return_full_states=True)
                    finally:
                        ops.admm_run = real
                    assert calls and s2.last_path == "fused", "admm_vxu did not run on the two-kernel iteration"
                    tol = 1e-5
                    assert_close(got[0].cpu(), ref[0].cpu(), tol, f"admm_vxu two-kernel z ({nterms} terms, rows mode {mode})", maxabs_mult=4.0)
                    for i in range(nterms):
                        close_on_scale(got[1][i], ref[1][i].cpu().numpy(), ref[0].cpu().numpy(), tol, f"admm_vxu v{i}")
                        close_on_scale(got[2][i], ref[2][i].cpu().numpy(), ref[0].cpu().numpy(), tol, f"admm_vxu u{i}")
    finally:
        L.call("dpx_admm_iter_config", 0, 0)


def case_tiny_shapes(device):
    """degenerate planes against the oracle: 2x3, 3x3, 17x2 (every stage at its smallest size, prime lengths), and the
    reference's error for an axis shorter than the gradient stencil (utils/psf2otf.py:46-54 raises there too)"""
    import oracle as O
    for shape in ((1, 1, 2, 3), (1, 1, 3, 3), (2, 3, 4, 6), (1, 1, 17, 2)):
        B, C, H, W = shape
        rng = np.random.RandomState(sum(shape))
        b = rng.rand(*shape).astype("float32")
        psf = np.ones((1, 1), dtype="float32") if min(H, W) < 3 else rng.rand(3, 3).astype("float32")
        psf /= psf.sum()
        bt = torch.from_numpy(b).to(device)
        x = dp.Variable()
        fns = dp.sum_squares(dp.conv(x, psf) - bt) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
        out = dp.compile(fns, method="admm", device=device).solve(x0=bt, rhos=0.5, lams=0.02, max_iter=4)
        bc = torch.from_numpy(b)
        ref = O.solve([O.sum_squares(O.lin_conv(psf).minus(bc)), O.norm1(O.lin_grad(0)), O.norm1(O.lin_grad(1))], "admm", x0=bc, rhos=0.5,
                      lams=0.02, max_iter=4)
        assert_close(out.cpu(), ref, TOL, f"tiny plane {shape}")
    bt = torch.rand(2, 1, 5, 1).to(device)
    x = dp.Variable()
    with pytest.raises(Exception, match="cannot be smaller than the PSF"):
        dp.compile(dp.sum_squares(x - bt) + dp.norm1(dp.grad(x, dim=1)), method="admm", device=device).solve(x0=bt, rhos=0.5, lams=0.02, max_iter=2)



# ---- BASELINE-size cases (fixtures G30..G33: strided samples + per-image sums / L2 norms of the reference's outputs) -----------
def _check_packed(g, key, t, stride, tol, scale_key=None, what="", scale_sub=1, maxabs_mult=1.0):
    """compare tensor `t` with the packed reference entry `key`: strided samples (rel-L2, on the scale of `scale_key`'s
    samples for the split variables), per-image sum and L2 norm (float64 reductions of the full tensor)"""
    t = t.detach()
    samp = t[..., ::stride, ::stride].cpu().numpy()
    ref = g[key]
    if scale_key is None and (key + "_f64") in g and not (np.abs(samp - ref).max() <= tol * np.abs(ref).max()):
        # pointwise the reference itself sits ~1e-5 from the float64 result stored next to it (single pixels beside a threshold
        # decision after many iterations): the L2 criterion against the reference stays; the pointwise one is "within tol of the
        # reference, or at least as close to the float64 samples as the reference is"
        f64 = g[key + "_f64"]
        r = rel_l2(samp, ref)
        e_got, e_ref = np.abs(samp - f64).max() / np.abs(f64).max(), np.abs(ref - f64).max() / np.abs(f64).max()
        record(f"{what}{key} samples", r, tol, float(np.abs(samp - ref).max() / np.abs(ref).max()))
        record(f"{what}{key} samples: max-abs distance from float64 (reference's own: {e_ref:.2e})", float(e_got), float(e_ref))
        assert r <= tol, f"{what}{key} samples: rel-L2 {r:.3e}"
        assert e_got <= e_ref, f"{what}{key} samples: max-abs {e_got:.3e} from float64, the reference is {e_ref:.3e} away"
    elif scale_key is None:
        assert_close(samp, ref, tol, f"{what}{key} samples", maxabs_mult=maxabs_mult)
    else:
        close_on_scale(samp, ref, g[scale_key][..., ::scale_sub, ::scale_sub], tol, f"{what}{key} samples")
    d = t.double().reshape(t.shape[0], -1)
    l2, sm = d.norm(dim=1).cpu().numpy(), d.sum(1).cpu().numpy()
    n = d.shape[1]
    ref_l2 = np.maximum(g[key + "_l2"], 1e-30)
    scale_l2 = ref_l2 if scale_key is None else np.maximum(g[scale_key + "_l2"], ref_l2)
    e_l2 = float(np.max(np.abs(l2 - g[key + "_l2"]) / scale_l2))
    e_sum = float(np.max(np.abs(sm - g[key + "_sum"]) / (scale_l2 * np.sqrt(n))))      # |sum error| <= sqrt(n) * ||error||_2
    record(f"{what}{key} per-image L2 norm", e_l2, tol)
    record(f"{what}{key} per-image sum / (sqrt(n) L2)", e_sum, tol)
    assert e_l2 <= tol, f"{what}{key}: per-image L2 norms off by {e_l2:.3e}"
    assert e_sum <= tol, f"{what}{key}: per-image sums off by {e_sum:.3e} (relative to sqrt(n) * L2)"


def case_full_c2(device):
    """G30 -- config 2 at its real plane size (2 of the 8 images): state trajectory at iterations 1 / 5 / 10 against the
    reference run, through the two-kernel fused iteration (1024-point transforms)."""
    import synthetic
    g = load_golden("g30_full_c2")
    gt, b, psf = synthetic.deconv_case(2, 3, 1024, 1024, seed=int(g["seed"]))
    bt = T(b, device)
    x, fns, _ = tv_problem(bt, psf)
    snaps = {}

    def cb(iter, state, rho, lam):
        if iter + 1 in (1, 5, 10):
            snaps[iter + 1] = (state[0].clone(), [e.clone() for e in state[1]], [e.clone() for e in state[2]])

    s = dp.compile(fns, method="admm", device=device)
    out = s.solve(x0=bt, rhos=0.1, lams=0.005, max_iter=10, callback=cb)
    assert s.last_path == "fused"
    for it, (xs, vs, us) in sorted(snaps.items()):
        _check_packed(g, f"it{it}_x", xs, 8, TOL, what="c2 ", maxabs_mult=4.0 if it >= 5 else 1.0)   # noise floor of the reference from iteration ~5 on
        for i in range(2):
            _check_packed(g, f"it{it}_v{i}", vs[i], 16, TOL, scale_key=f"it{it}_x", what="c2 ", scale_sub=2)
            _check_packed(g, f"it{it}_u{i}", us[i], 16, TOL, scale_key=f"it{it}_x", what="c2 ", scale_sub=2)
    # without a callback the loop runs on the C side (dpx_admm_run): same final iterate
    out2 = s.solve(x0=bt, rhos=0.1, lams=0.005, max_iter=10)
    _check_packed(g, "it10_x", out2, 8, TOL, what="c2 (C-side loop) ", maxabs_mult=4.0)
    ref_err = rel_l2(g["it10_x"], g["x_f64"])
    got_err = rel_l2(out2[..., ::8, ::8].cpu().numpy(), g["x_f64"])
    record("c2 x vs the float64 iterate (reference's own distance: %.2e)" % ref_err, got_err, ref_err)
    assert got_err <= ref_err
    psnr = [10 * np.log10(1.0 / np.mean((out2[i].cpu().numpy() - gt[i]) ** 2)) for i in range(2)]
    assert np.allclose(psnr, g["psnr"], atol=2e-3), (psnr, g["psnr"])


def case_full_c2_batch8(device):
    """G30b -- config 2 exactly as BASELINE.json states it: the whole batch of 8 x 3 x 1024 x 1024 (the launch geometry bench.py
    times: 24 planes, 128 bands of 8 rows), 50 iterations on the C-side loop, against the real reference's run.
    After 50 iterations at this size the REFERENCE's own fp32 round-off has grown to 1.3e-5 of the float64 iterate of the same
    algorithm (stored next to it; it grows like sqrt(iterations): 4.7e-6 at iteration 10, G30), so a 1e-5 bar against the
    reference's samples cannot be met by anything that is not the reference's rounding sequence.  Acceptance here, stated:
      * the iterate after 25 iterations against the reference: rel-L2 <= 1e-5 (the reference is still below the bar there);
      * the final x against the float64 iterate: rel-L2 <= 1e-5 (measured ~3e-7) -- and therefore at most (the reference's own
        distance + 1e-5) from the reference, which is recorded;
      * per-image sums and L2 norms of the final x against the reference at 1e-5 (round-off averages out of them)."""
    import synthetic
    g = load_golden("g30b_full_c2_batch8")
    gt, b, psf = synthetic.deconv_case(8, 3, 1024, 1024, seed=int(g["seed"]))
    bt = T(b, device)
    x, fns, _ = tv_problem(bt, psf)
    s = dp.compile(fns, method="admm", device=device)
    x25 = s.solve(x0=bt, rhos=0.1, lams=0.005, max_iter=25)
    assert s.last_path == "fused"
    _check_packed(g, "it25_x", x25, 16, TOL, what="c2 batch 8 ", maxabs_mult=4.0)
    out = s.solve(x0=bt, rhos=0.1, lams=0.005, max_iter=50)
    samp = out[..., ::8, ::8].cpu().numpy()
    e_ref_f64 = rel_l2(g["x"], g["x_f64"])
    e_f64 = rel_l2(samp, g["x_f64"])
    e_ref = rel_l2(samp, g["x"])
    record("c2 batch 8, 50 it: x samples vs the float64 iterate", e_f64, TOL)
    record(f"c2 batch 8, 50 it: x samples vs the reference (the reference itself is {e_ref_f64:.2e} from float64)", e_ref, e_ref_f64 + TOL)
    assert e_f64 <= TOL, f"final x: {e_f64:.3e} from the float64 iterate"
    assert e_ref <= e_ref_f64 + TOL, (e_ref, e_ref_f64)
    d = out.double().reshape(8, -1)
    l2, sm = d.norm(dim=1).cpu().numpy(), d.sum(1).cpu().numpy()
    e_l2 = float(np.max(np.abs(l2 - g["x_l2"]) / g["x_l2"]))
    e_sum = float(np.max(np.abs(sm - g["x_sum"]) / (g["x_l2"] * np.sqrt(d.shape[1]))))
    record("c2 batch 8, 50 it: per-image L2 norm vs the reference", e_l2, TOL)
    record("c2 batch 8, 50 it: per-image sum / (sqrt(n) L2) vs the reference", e_sum, TOL)
    assert e_l2 <= TOL and e_sum <= TOL, (e_l2, e_sum)
    psnr = [float(10 * np.log10(1.0 / np.mean((out[i].cpu().numpy() - gt[i]) ** 2))) for i in range(8)]
    assert np.allclose(psnr, g["psnr"], atol=1e-3), (psnr, g["psnr"])


def case_generic_planes_full_size(device, tags=("1000", "720x1280")):
    """G37 -- the plane sizes bench.py times off the register-radix path AT THEIR FULL SIZE: 8 x 3 x 1000 x 1000 and 2 x 3 x 720 x 1280, 6 ADMM
    iterations, full state against the real reference's run (the small generic cases stop at 100 x 120: the XCD renumbering of the stencil
    passes, the 8-column interleave of k_cols_il and the merged z / rhs pass only see full grids here).  x at 1e-5 against the reference
    and at least as close to the reference's own float64 iterate as the reference's float32 output is."""
    import synthetic
    for tag in tags:
        g = load_golden("g37_generic_" + tag)
        shape = tuple(int(v) for v in g["shape"])
        gt, b, psf = synthetic.deconv_case(*shape, seed=int(g["seed"]))
        bt = T(b, device)
        x, fns, _ = tv_problem(bt, psf)
        s = dp.compile(fns, method="admm", device=device)
        st = s.solve(x0=bt, rhos=0.1, lams=0.005, max_iter=6, return_full_states=True)
        assert s.last_path == "fused"
        _check_packed(g, "x", st[0], 8, TOL, what=f"generic {tag} ")
        for i in range(2):
            _check_packed(g, f"v{i}", st[1][i], 16, TOL, scale_key="x", what=f"generic {tag} ", scale_sub=2)
            _check_packed(g, f"u{i}", st[2][i], 16, TOL, scale_key="x", what=f"generic {tag} ", scale_sub=2)
        out = s.solve(x0=bt, rhos=0.1, lams=0.005, max_iter=6)               # (x only: the loop's last stage without the state stores)
        _check_packed(g, "x", out, 8, TOL, what=f"generic {tag} (x only) ")
        ref_err = rel_l2(g["x"], g["x_f64"])
        got_err = rel_l2(out[..., ::8, ::8].cpu().numpy(), g["x_f64"])
        record(f"generic {tag}: x vs the reference's float64 iterate (reference's own distance: {ref_err:.2e})", got_err, ref_err + TOL)
        assert got_err <= ref_err + TOL, (tag, got_err, ref_err)
        psnr = [10 * np.log10(1.0 / np.mean((out[i].cpu().numpy() - gt[i]) ** 2)) for i in range(shape[0])]
        assert np.allclose(psnr, g["psnr"], atol=2e-3), (psnr, g["psnr"])
        del s, st, out, bt
        if str(device) != "cpu":
            torch.cuda.empty_cache()


def case_full_c3_batch8(device):
    """G38 -- config 3 as BASELINE.json states it (8 x 3 x 1024 x 1024, FFDNet-colour plug-and-play ADMM, log_descent(35, 5, 30)): the first 3
    and the last 3 steps of the 30-step schedule on the whole batch, against the real reference and its own float64 run (criterion as
    for G31 / G9: at least as close to the float64 iterate as the reference is, + the 1e-5 budget)."""
    import synthetic
    g = load_golden("g38_full_c3_batch8")
    gt, b, psf = synthetic.deconv_case(8, 3, 1024, 1024, seed=int(g["seed"]))
    bt = T(b, device)
    rhos30, sig30 = dp.log_descent(35, 5, 30)
    samp = lambda t: t[..., ::16, ::16].cpu().numpy()
    for tag, sl in (("first", slice(0, 3)), ("last", slice(27, 30))):
        assert np.allclose(rhos30[sl].numpy(), g[tag + "_rhos"], rtol=1e-6) and np.allclose(sig30[sl].numpy(), g[tag + "_sigmas"], rtol=1e-6)
        x = dp.Variable()
        prior = dp.deep_prior(x, denoiser=_ffdnet("color", device))
        fns = dp.sum_squares(dp.conv(x, psf) - bt) + prior
        with torch.no_grad():
            s = dp.compile(fns, method="admm", device=device)
            st = s.solve(x0=bt, rhos=rhos30[sl].clone(), lams={prior: sig30[sl].clone()}, max_iter=3, return_full_states=True)
        assert s.last_path == "fused"
        for key, got in (("x", samp(st[0])), ("v0", samp(st[1][0]))):
            ref_err = rel_l2(g[f"{tag}_{key}"], g[f"{tag}_{key}_f64"])
            got_err = rel_l2(got, g[f"{tag}_{key}_f64"])
            r = rel_l2(got, g[f"{tag}_{key}"])
            record(f"c3 batch 8, {tag} 3 steps: {key} vs the reference's float64 iterate (reference's own distance: {ref_err:.2e})", got_err, ref_err + TOL)
            record(f"c3 batch 8, {tag} 3 steps: {key} vs the reference (both fp32)", r, 2 * ref_err + TOL)
            assert got_err <= ref_err + TOL, (tag, key, got_err, ref_err)
            assert r <= 2 * ref_err + TOL, (tag, key, r, ref_err)
        d = st[1][0].double().reshape(8, -1).norm(dim=1).cpu().numpy()
        e = float(np.max(np.abs(d - g[tag + "_v0_f64_l2"]) / g[tag + "_v0_f64_l2"]))
        record(f"c3 batch 8, {tag} 3 steps: v per-image L2 norm vs float64", e, 1e-4)
        assert e <= 1e-4, (tag, e)
        del s, st
        if str(device) != "cpu":
            torch.cuda.empty_cache()


def case_full_c3_trajectory(device):
    """G38b -- config 3 at the length bench.py times: 8 x 3 x 1024 x 1024, FFDNet-colour plug-and-play ADMM, ALL 30 steps of log_descent(35, 5, 30)
    in one solve from x0 = b, x and v after 10, 20 and 30 iterations against the real reference and the reference's own float64 run of the same
    30 steps (criterion as G38 / G31 / G9: at least as close to the float64 iterate as the reference is, + the 1e-5 budget; and within the sum
    of the two fp32 distances of the reference).  Three solves of 10 / 20 / 30 iterations on the path bench.py times (no callback)."""
    import synthetic
    g = load_golden("g38b_full_c3_trajectory")
    gt, b, psf = synthetic.deconv_case(8, 3, 1024, 1024, seed=int(g["seed"]))
    bt = T(b, device)
    rhos30, sig30 = dp.log_descent(35, 5, 30)
    assert np.allclose(rhos30.numpy(), g["rhos"], rtol=1e-6) and np.allclose(sig30.numpy(), g["sigmas"], rtol=1e-6)
    samp = lambda t: t[..., ::16, ::16].cpu().numpy()
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=_ffdnet("color", device))
    fns = dp.sum_squares(dp.conv(x, psf) - bt) + prior
    with torch.no_grad():
        s = dp.compile(fns, method="admm", device=device)
        for it in (10, 20, 30):
            st = s.solve(x0=bt, rhos=rhos30[:it].clone(), lams={prior: sig30[:it].clone()}, max_iter=it, return_full_states=True)
            assert s.last_path == "fused"
            for key, got in (("x", samp(st[0])), ("v0", samp(st[1][0]))):
                ref_err = rel_l2(g[f"it{it}_{key}"], g[f"it{it}_{key}_f64"])
                got_err = rel_l2(got, g[f"it{it}_{key}_f64"])
                r = rel_l2(got, g[f"it{it}_{key}"])
                record(f"c3 batch 8, 30-step solve, iteration {it}: {key} vs the reference's float64 iterate (reference's own distance: {ref_err:.2e})", got_err,
                       ref_err + TOL)
                record(f"c3 batch 8, 30-step solve, iteration {it}: {key} vs the reference (both fp32)", r, 2 * ref_err + TOL)
                assert got_err <= ref_err + TOL, (it, key, got_err, ref_err)
                assert r <= 2 * ref_err + TOL, (it, key, r, ref_err)
            d = st[1][0].double().reshape(8, -1).norm(dim=1).cpu().numpy()
            e = float(np.max(np.abs(d - g[f"it{it}_v0_f64_l2"]) / g[f"it{it}_v0_f64_l2"]))
            record(f"c3 batch 8, 30-step solve, iteration {it}: v per-image L2 norm vs float64", e, 1e-4)
            assert e <= 1e-4, (it, e)
        psnr = [10 * np.log10(1.0 / np.mean((st[0][i].cpu().numpy() - gt[i]) ** 2)) for i in range(8)]
        assert np.allclose(psnr, g["psnr"], atol=5e-3), (psnr, g["psnr"])


def case_full_c4_trajectory(device):
    """G32c -- one GPU's shard of config 4 at the length bench.py times: 4 x 1 x 320 x 320, LADMM, CG x-update (rtol 1e-6, <= 100), nonneg + gray
    FFDNet prior, 10 outer iterations: the final state, x after 5 iterations (a second solve), and ALL TEN CG exit counts EQUAL to the reference's
    (linalg/solve/solver_cg.py:99-129)."""
    import synthetic
    from dprox.contrib import masked_fft
    from dprox.linalg import LinearSolveConfig
    from dprox.utils import ifft2
    g = load_golden("g32c_full_c4_trajectory")
    gt, mask, y = synthetic.csmri_case(4, 320, 320, seed=int(g["seed"]), center=32)
    mask, y = T(mask, device), T(y, device)
    x = dp.Variable()
    fns = dp.sum_squares(masked_fft(x, mask), y) + dp.nonneg(x) + dp.deep_prior(x, denoiser=_ffdnet("gray", device))
    x0 = ifft2(y).real.float().contiguous()
    with torch.no_grad():
        s = dp.compile(fns, method="ladmm", device=device, linear_solve_config=LinearSolveConfig(rtol=1e-6, max_iters=100))
        st = s.solve(x0=x0, rhos=0.5, lams=0.03, max_iter=10, return_full_states=True)
        its = [int(v) for v in s.least_square.cg_iters[-10:]]
        assert its == [int(v) for v in g["cg_iters"]], (its, list(g["cg_iters"]))
        x5 = s.solve(x0=x0, rhos=0.5, lams=0.03, max_iter=5)
    # Ten outer iterations of a truncated-CG x-update and a seeded denoiser amplify float32 round-off: the reference's own float32 x is `ref_err`
    # away from its float64 run with the SAME CG iteration counts (3.4e-5 on the stored ::4 lattice -- where the centred-FFT images happen to be
    # 4x smaller than their rms --, 3.8e-6 over the full tensor).  Criterion as for config 3: at least as close to the float64 iterate as the
    # reference is (+ the 1e-5 budget), within the sum of the two distances of the reference, and per-image norms / sums of the FULL tensors at 1e-5.
    samp = lambda t: t[..., ::4, ::4].cpu().numpy()
    for key, got in (("x", samp(st[0])), ("it5_x", samp(x5)), ("v0", samp(st[1][0])), ("u0", samp(st[2][0])), ("v1", samp(st[1][1])), ("u1", samp(st[2][1]))):
        scale = np.linalg.norm(g["x_f64"].astype(np.float64).ravel())                 # (split variables on the iterate's scale)
        f64 = g[key + "_f64"].astype(np.float64)
        ref_err = float(np.linalg.norm((g[key] - f64).ravel()) / scale)
        got_err = float(np.linalg.norm((got - f64).ravel()) / scale)
        r = float(np.linalg.norm((got.astype(np.float64) - g[key]).ravel()) / scale)
        record(f"c4, 10 outer iterations: {key} vs the reference's float64 run, same CG counts (reference's own distance: {ref_err:.2e})", got_err, ref_err + TOL)
        record(f"c4, 10 outer iterations: {key} vs the reference (both fp32)", r, 2 * ref_err + TOL)
        assert got_err <= ref_err + TOL, (key, got_err, ref_err)
        assert r <= 2 * ref_err + TOL, (key, r, ref_err)
    for key, t in (("x", st[0]), ("it5_x", x5)):
        d = t.double().reshape(4, -1)
        e_l2 = float(np.max(np.abs(d.norm(dim=1).cpu().numpy() - g[key + "_l2"]) / g[key + "_l2"]))
        e_sum = float(np.max(np.abs(d.sum(1).cpu().numpy() - g[key + "_sum"]) / (g[key + "_l2"] * np.sqrt(d.shape[1]))))
        record(f"c4, 10 outer iterations: {key} per-image L2 norm (full tensor)", e_l2, TOL)
        record(f"c4, 10 outer iterations: {key} per-image sum / (sqrt(n) L2) (full tensor)", e_sum, TOL)
        assert e_l2 <= TOL and e_sum <= TOL, (key, e_l2, e_sum)


def case_full_c3(device):
    """G31 -- config 3 at its real plane size (one 3x1024x1024 image): 3 plug-and-play ADMM iterations with the FFDNet-colour
    prior on the log_descent(35, 5, 30) schedule.  rho starts at 1.2e-3 * ... so the x-update amplifies fp32 round-off: the
    reference's x is itself `ref_err` away from the float64 iterate (printed); criterion as for G9."""
    import synthetic
    g = load_golden("g31_full_c3")
    gt, b, psf = synthetic.deconv_case(1, 3, 1024, 1024, seed=int(g["seed"]))
    bt = T(b, device)
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=_ffdnet("color", device))
    fns = dp.sum_squares(dp.conv(x, psf) - bt) + prior
    rhos, sig = dp.log_descent(35, 5, 30)
    assert np.allclose(rhos[:3].numpy(), g["rhos"], rtol=1e-6) and np.allclose(sig[:3].numpy(), g["sigmas"], rtol=1e-6)
    with torch.no_grad():
        s = dp.compile(fns, method="admm", device=device)
        st = s.solve(x0=bt, rhos=rhos[:3], lams={prior: sig[:3]}, max_iter=3, return_full_states=True)
    assert s.last_path == "fused"
    samp = lambda t: t[..., ::8, ::8].cpu().numpy()
    # rho = 1.2e-5: the x-update divides by |H|^2 + rho, fp32 round-off of EITHER implementation is amplified ~1e5 x.  The
    # reference's own x is `ref_err` (6e-3 at this size) and its denoised v 7e-5 away from the float64 iterates stored next to
    # them; criterion: at least as close to the exact iterate as the reference is (+ the 1e-5 budget), and the two fp32
    # results within the sum of their distances.
    for key, got in (("x", samp(st[0])), ("v0", samp(st[1][0]))):
        ref_err = rel_l2(g[key], g[key + "_f64"])
        got_err = rel_l2(got, g[key + "_f64"])
        record(f"c3 {key} vs the float64 iterate (reference's own distance: {ref_err:.2e})", got_err, ref_err + TOL)
        record(f"c3 {key} vs the reference (both fp32, round-off amplified by the x-update)", rel_l2(got, g[key]), 2 * ref_err + TOL)
        assert got_err <= ref_err + TOL, (key, got_err, ref_err)
        assert rel_l2(got, g[key]) <= 2 * ref_err + TOL, (key, rel_l2(got, g[key]), ref_err)
    d = st[1][0].double().reshape(1, -1)
    e = abs(float(d.norm()) - float(g["v0_f64_l2"][0])) / float(g["v0_f64_l2"][0])
    record("c3 v per-image L2 norm vs float64", e, 1e-4)
    assert e <= 1e-4


def case_full_c4(device):
    """G32 -- one GPU's shard of config 4 (4 x 1 x 320 x 320): LADMM, CG x-update (320-point mixed-radix transforms inside the
    matvec), nonneg + gray FFDNet prior, 2 outer iterations, CG exit counts included."""
    import synthetic
    from dprox.contrib import masked_fft
    from dprox.linalg import LinearSolveConfig
    from dprox.utils import ifft2
    g = load_golden("g32_full_c4")
    gt, mask, y = synthetic.csmri_case(4, 320, 320, seed=int(g["seed"]), center=32)
    mask, y = T(mask, device), T(y, device)
    x = dp.Variable()
    fns = dp.sum_squares(masked_fft(x, mask), y) + dp.nonneg(x) + dp.deep_prior(x, denoiser=_ffdnet("gray", device))
    x0 = ifft2(y).real.float().contiguous()
    with torch.no_grad():
        s = dp.compile(fns, method="ladmm", device=device, linear_solve_config=LinearSolveConfig(rtol=1e-6, max_iters=100))
        st = s.solve(x0=x0, rhos=0.5, lams=0.03, max_iter=2, return_full_states=True)
    its = list(s.least_square.cg_iters[-2:])
    assert all(abs(int(a) - int(r)) <= 1 for a, r in zip(its, g["cg_iters"])), (its, g["cg_iters"])
    _check_packed(g, "x", st[0], 4, TOL, what="c4 ")
    for i in range(2):
        _check_packed(g, f"v{i}", st[1][i], 4, TOL, scale_key="x", what="c4 ")
        _check_packed(g, f"u{i}", st[2][i], 4, TOL, scale_key="x", what="c4 ")


def case_full_c5(device, dtype="f32"):
    """G33 -- config 5 at its real size (4 x 3 x 512 x 512, ADMM unrolled 10 times, MSE loss): forward, loss and the gradients
    w.r.t. the rho / lambda schedules and the observation against the reference's autograd."""
    import synthetic
    g = load_golden("g33_full_c5")
    gt, b, psf = synthetic.deconv_case(4, 3, 512, 512, seed=int(g["seed"]))
    K = 10
    x = dp.Variable()
    bt = T(b, device).clone().requires_grad_(True)
    n0, n1 = dp.norm1(dp.grad(x, dim=0)), dp.norm1(dp.grad(x, dim=1))
    solver = dp.compile(dp.sum_squares(dp.conv(x, psf) - bt) + n0 + n1, method="admm", device=device)
    solver = dp.specialize(solver, method="unroll", device=device, max_iter=K, dtype=dtype)
    rhos, l0, l1 = (torch.tensor(g[k], requires_grad=True) for k in ("rhos", "l0", "l1"))
    xo = solver.solve(x0=T(b, device), rhos=rhos, lams={n0: l0, n1: l1})
    loss = ((xo - T(gt, device)) ** 2).mean()
    loss.backward()
    _check_packed(g, "x", xo, 8, TOL, what="c5 ")
    if dtype == "bf16":
        # bf16 history (the BASELINE's dtype for this config): fp32 forward as above; stated gradient tolerances vs the reference's
        # fp32 autograd: lambda schedules 1e-3 (masks survive the rounding; the sums still see bf16 x through the rho-coupling),
        # rho schedule 2e-2, observation gradient as in fp32 (decision flips dominate)
        for name, got, tol in (("g_rhos", rhos.grad, 2e-2), ("g_l0", l0.grad, 1e-3), ("g_l1", l1.grad, 1e-3)):
            r = rel_l2(got.detach().cpu().numpy(), g[name])
            record(f"c5 bf16-history {name} vs the reference's fp32 autograd", r, tol)
            assert r <= tol, (name, r)
        gb = bt.grad[..., ::8, ::8].cpu().numpy()
        r_64, ref_64 = rel_l2(gb, g["g_b_f64"]), rel_l2(g["g_b"], g["g_b_f64"])
        record(f"c5 bf16-history g_b samples vs the float64 gradient (reference's own distance: {ref_64:.2e})", r_64, 1.5 * ref_64)
        assert r_64 <= 1.5 * ref_64 + 1e-5
        return
    lv, lr = float(loss.detach().double()), float(g["loss"])
    record("c5 loss", abs(lv - lr) / abs(lr), 1e-5)
    assert abs(lv - lr) <= 1e-5 * abs(lr), (lv, lr)
    # d loss / d rho_t are sums of 3e6 signed products cancelling to ~1e-5: fp32 accumulation order alone moves them by ~1e-4
    # relative (the reference's own values are 1.6e-4 away from the float64 gradients stored next to them).  Criterion: within
    # 1e-4 of the reference, or at least as close to the float64 gradient as the reference is.
    for name, got in (("g_rhos", rhos.grad), ("g_l0", l0.grad), ("g_l1", l1.grad)):
        got = got.detach().cpu().numpy()
        r_ref, r_64, ref_64 = rel_l2(got, g[name]), rel_l2(got, g[name + "_f64"]), rel_l2(g[name], g[name + "_f64"])
        record(f"c5 {name} vs the reference's autograd", r_ref, 1e-4)
        record(f"c5 {name} vs the float64 gradient (reference's own distance: {ref_64:.2e})", r_64, max(ref_64, 1e-4))
        assert r_ref <= 1e-4 or r_64 <= ref_64, f"c5 {name}: {r_ref:.3e} from the reference, {r_64:.3e} from float64 (reference: {ref_64:.3e})"
    # d loss / d b goes through 10 x 2 soft-threshold Jacobians [|d| > lam] evaluated on 3e6 pixels each: every threshold
    # decision that fp32 round-off flips changes the gradient on one stencil -- in the reference as much as here (its own g_b
    # is ~1e-3 from the float64 gradient).  Criterion: within 1e-4 of the reference, or as close to the float64 gradient as the
    # reference is (x1.5: which of the two fp32 runs flips fewer decisions is chance).
    gb = bt.grad[..., ::8, ::8].cpu().numpy()
    r_ref, r_64, ref_64 = rel_l2(gb, g["g_b"]), rel_l2(gb, g["g_b_f64"]), rel_l2(g["g_b"], g["g_b_f64"])
    record("c5 g_b samples vs the reference's autograd", r_ref, 1e-4)
    record(f"c5 g_b samples vs the float64 gradient (reference's own distance: {ref_64:.2e})", r_64, 1.5 * ref_64)
    assert r_ref <= 1e-4 or r_64 <= 1.5 * ref_64 + 1e-5, (r_ref, r_64, ref_64)


def case_unet(device, grads=True):
    """G22: UNetDenoiser (reference wrapper.py:206-221, models/unet/unet.py:34-135) with seeded weights: forward on odd / even
    planes (MaxPool floor, zero-padded up path, per-image sigma), the backward-data pass (image and sigma gradients) and the
    weight / bias gradients against the reference's autograd."""
    import synthetic
    from dprox.proxfn.pnp.denoisers import UNetDenoiser
    g = load_golden("g22_unet")
    den = UNetDenoiser(synthetic.unet_weights(41)).to(device)
    with torch.no_grad():
        assert_close(den.denoise(T(g["odd_x"], device), torch.tensor(0.1, device=device)).cpu(), g["odd_y"], TOL, "unet odd 37x45, two bands")
        assert_close(den.denoise(T(g["even_x"], device), T(g["even_sigma"], device)).cpu(), g["even_y"], TOL, "unet even, per-image sigma")
        xe = T(g["even_x"], device)
        nm = torch.ones_like(xe) * T(g["even_sigma"], device).view(-1, 1, 1, 1)
        assert_close(den.model(torch.cat([xe, nm], dim=1).contiguous()).cpu(), g["even_raw"], TOL, "unet raw network output")
    # through deep_prior: the plug-and-play prox call
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=den).to(device)
    with torch.no_grad():
        out = prior.prox(T(g["even_x"], device), T(g["even_sigma"], device))
    assert_close(out.cpu(), g["even_y"], TOL, "deep_prior(denoiser=UNetDenoiser).prox")
    if not grads:
        return
    xg = T(g["grad_x"], device).requires_grad_(True)
    sg = torch.tensor([0.05, 0.2], device=device, requires_grad=True)
    w = T(g["grad_w"], device)
    (den.denoise(xg, sg) * w).sum().backward()
    _assert_grad_close(xg.grad.cpu(), g["grad_gx"], "unet d/dx", tol=1e-4)
    _assert_grad_close(sg.grad.cpu(), g["grad_gsigma"], "unet d/dsigma", tol=1e-4)
    # weight / bias gradients (trainable prior)
    den.model.requires_grad_(True)
    (den.denoise(xg.detach(), sg.detach()) * w).sum().backward()
    names = [str(n) for n in g["wgrad_names"]]
    got = {n: den.model.ref_param(n).grad.cpu() for n in names}
    norms = np.array([float(got[n].norm()) for n in names])
    assert np.allclose(norms, g["wgrad_norms"], rtol=2e-3), np.max(np.abs(norms / g["wgrad_norms"] - 1))
    for n in ("inc.conv.conv-0.conv2d.weight", "inc.conv.conv-0.conv2d.bias", "outc.conv.weight", "outc.conv.bias", "up4.conv.conv-2.conv2d.bias"):
        _assert_grad_close(got[n], g["wgrad_full_" + n], f"unet dW {n}", tol=2e-4)
    _assert_grad_close(got["down4.mpconv.1.conv-1.conv2d.weight"][:8, :8], g["wgrad_corner_down4"], "unet dW down4 corner", tol=2e-4)
    _assert_grad_close(got["up1.conv.conv-0.conv2d.weight"][:8, :8], g["wgrad_corner_up1"], "unet dW up1 corner", tol=2e-4)
    # the state dict keeps the reference's keys, also inside a parent module
    sd = den.state_dict()
    assert "model.inc.conv.conv-0.conv2d.weight" in sd and "model.outc.conv.bias" in sd and len(sd) == 56


def case_linear_solve_grad(device):
    """G24: linear_solve's implicit backward (reference linalg/custom.py:39-82) on the masked-Fourier normal operator with a
    trainable per-image rho: the solution, dL/db (one more CG solve with A^T) and dL/drho (operator VJP at the solution)."""
    from dprox.linalg import LinearSolveConfig, linear_solve
    from dprox.utils import fft2, ifft2
    g = load_golden("g24_linear_solve_grad")
    mask, w = T(g["mask"], device), T(g["w"], device)

    class Normal(torch.nn.Module):
        def __init__(self, rho):
            super().__init__()
            self.rho = torch.nn.Parameter(rho)

        def forward(self, x):
            return ifft2(mask * (mask * fft2(x.contiguous()))).real.float().contiguous() + self.rho.view(-1, 1, 1, 1) * x

        @property
        def T(self):
            return self

        def clone(self):
            return Normal(self.rho.detach().clone())

    A = Normal(T(g["rho"], device).clone()).to(device)
    b = T(g["b"], device).clone().requires_grad_(True)
    x = linear_solve(A, b, LinearSolveConfig(rtol=1e-6, max_iters=100))
    (x * w).sum().backward()
    assert_close(x.detach().cpu(), g["x"], TOL, "linear_solve x")
    assert_close(b.grad.cpu(), g["g_b"], 1e-5, "linear_solve dL/db (transposed solve)")
    assert_close(A.rho.grad.cpu(), g["g_rho"], 1e-5, "linear_solve dL/drho (operator VJP)")
    # without anything to differentiate the solver is called directly
    with torch.no_grad():
        x2 = linear_solve(A, b.detach(), LinearSolveConfig(rtol=1e-6, max_iters=100))
    assert_close(x2.cpu(), g["x"], TOL, "linear_solve x (no grad)")
