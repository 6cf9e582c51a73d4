"""DEQ cases shared by the GPU tests (-m gpu, real MI355X) and the emulated-kernel tests (CPU, the same kernel sources under the SIMT
emulator): the Anderson kernels against a float64 restatement written here, ``anderson()`` on a known contraction, and ``DEQSolver``
against the reference's stored runs (tests/golden/g41_deq*.npz, make_golden_deq.py).

Kernel bounds: Gram row and |F_k|^2 within 1e-5 sqrt(H_ii H_jj) (the project's 1e-5 bar on the Cauchy-Schwarz scale of the sum);
alpha sums to 1 within 1e-6 and is within 1e-5 |alpha|_inf of the float64 solve of the same float32 Gram matrix; X_new within
1e-5 max|alpha_i| max|F| of float64; everything bit-identical over two calls.
End to end (amplified round-off): output and rel_trace at least as close to the reference's float64 run as the reference's fp32 run
is, plus 1e-5, and within the sum of the two distances of the reference's fp32 output; nstep equal.
"""
import numpy as np
import torch

import dprox as dp
import oracle as O
import synthetic
from conftest import load_golden, record, rel_l2
from dprox import _ops as ops
from dprox.algo import deq

M = 6
LAM = 1e-4
RHO, LAM_TV = 0.3, 0.02          # make_golden_deq.py's schedule (the fixtures store it rounded to fp32; the float64 runs took these)


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def alpha_f64(Hm, n, lam):
    """rows 1 .. n of the solution of the bordered system, per image, in float64 from the given (float32) Gram matrices"""
    B = Hm.shape[0]
    out = np.zeros((B, n))
    for b in range(B):
        A = np.zeros((n + 1, n + 1))
        A[0, 1:] = A[1:, 0] = 1.0
        A[1:, 1:] = Hm[b, :n, :n].astype(np.float64) + lam * np.eye(n)
        y = np.zeros(n + 1)
        y[0] = 1.0
        out[b] = np.linalg.solve(A, y)[1:]
    return out


def case_kernels(device, shape, P, beta, steps=8, seed=0):
    """slots filled one after the other, k running past m (the slots wrap); after every fill the Gram row, and the mix at n = 1, 2, m - 1, m
    where that many slots are valid"""
    rng = np.random.RandomState(seed)
    B = shape[0]
    hist = ops.AndersonHistory(M, P, B, shape[1:], device)
    full = (P,) + tuple(shape)
    F32 = np.zeros((M,) + full, np.float32)
    G32 = np.zeros((M,) + full, np.float32)
    for k in range(steps):
        ks, nv = k % M, min(k + 1, M)
        X = rng.randn(*full).astype(np.float32)
        F = (X + (0.1 + 0.05 * k) * rng.randn(*full)).astype(np.float32)
        hist.X.copy_(T(X, device))
        hist.F[ks].copy_(T(F, device))
        nrm = hist.gram_row(ks, nv).cpu().numpy().copy()
        Hm = hist.Hm.cpu().numpy().copy()
        Gk = hist.G[ks].cpu().numpy().copy()
        F32[ks], G32[ks] = F, F - X
        assert np.array_equal(Gk, G32[ks])
        g64 = G32.astype(np.float64)
        per = lambda a: a.transpose(1, 0, *range(2, a.ndim)).reshape(B, -1)          # [P, B, ...] -> [B, P D]
        diag = np.array([[np.sum(per(g64[j])[b] ** 2) for j in range(nv)] for b in range(B)])
        assert diag.min() >= 1e-2
        for b in range(B):
            for j in range(nv):
                ref = float(np.dot(per(g64[ks])[b], per(g64[j])[b]))
                bound = 1e-5 * np.sqrt(diag[b, ks] * diag[b, j])
                assert abs(Hm[b, ks, j] - ref) <= bound and Hm[b, j, ks] == Hm[b, ks, j], (k, b, j, Hm[b, ks, j], ref)
            f2 = float(np.sum(per(F.astype(np.float64))[b] ** 2))
            assert abs(nrm[b, 1] - f2) <= 1e-5 * f2, (k, b, nrm[b, 1], f2)
            assert nrm[b, 0] == Hm[b, ks, ks]
        hist.gram_row(ks, nv)                                                        # bit-identical over two calls
        assert np.array_equal(hist.Hm.cpu().numpy(), Hm) and np.array_equal(hist.nrm.cpu().numpy(), nrm)
        assert np.array_equal(hist.G[ks].cpu().numpy(), Gk)
        for n in sorted({1, 2, M - 1, M}):
            if n > nv:
                continue
            al = hist.mix(n, beta, LAM).cpu().numpy().copy()
            Xn = hist.X.cpu().numpy().copy()
            assert abs(al.sum(1) - 1.0).max() <= 1e-6, (k, n, al.sum(1))
            a64 = alpha_f64(Hm, n, LAM)
            assert np.abs(al - a64).max() <= 1e-5 * np.abs(a64).max(), (k, n, al, a64)
            f64, x64 = F32[:n].astype(np.float64), (F32[:n].astype(np.float64) - g64[:n])
            ref = np.zeros(full)
            for b in range(B):
                ref[:, b] = beta * np.tensordot(a64[b], f64[:, :, b], 1) + (1 - beta) * np.tensordot(a64[b], x64[:, :, b], 1)
            err = np.abs(Xn - ref).max()
            bound = 1e-5 * np.abs(a64).max() * np.abs(F32[:n]).max()
            record(f"anderson mix {shape} x {P}, k={k}, n={n}, beta={beta}: max-abs", err, bound)
            assert err <= bound, (k, n, err, bound)
            al2 = hist.mix(n, beta, LAM).cpu().numpy()
            assert np.array_equal(al2, al) and np.array_equal(hist.X.cpu().numpy(), Xn)


def case_tiny_residuals(device, n=4):
    """|G|^2 = 1e-10 per slot: the ridge decides, alpha is uniform 1 / n"""
    shape, P = (2, 1, 5, 7), 3
    rng = np.random.RandomState(3)
    hist = ops.AndersonHistory(M, P, shape[0], shape[1:], device)
    hist.X.zero_()
    for k in range(n):
        g = rng.randn(P, *shape)
        g *= 1e-5 / np.sqrt((g.transpose(1, 0, 2, 3, 4).reshape(shape[0], -1) ** 2).sum(1)).reshape(1, -1, 1, 1, 1)
        hist.F[k].copy_(T(g.astype(np.float32), device))
        nrm = hist.gram_row(k, k + 1).cpu().numpy()
        assert np.allclose(nrm[:, 0], 1e-10, rtol=1e-5)
    al = hist.mix(n, 1.0, LAM).cpu().numpy()
    assert np.abs(al - 1.0 / n).max() <= 1e-5 / n, al


def contraction(device, seed=1):
    rng = np.random.RandomState(seed)
    shape = (2, 3, 9, 11)
    A = T(rng.uniform(-0.9, 0.9, shape).astype(np.float32), device)
    c = T(rng.randn(*shape).astype(np.float32), device)
    return A, c, (lambda z: A * z + c)


def case_contraction(device):
    """f(z) = A z + c, |A| <= 0.9 per pixel: the result is c / (1 - A) within 1e-5; an early stop pads the traces.
    The ridge: lam = 1e-12.  The method's ridge is absolute, and once |G|^2 falls below it the weights tend to uniform averaging
    (with the default 1e-4 the residual stalls near 1e-4 |F| here, in the reference's formula as in this one); a relative residual
    of 3e-7 on |F|^2 ~ 6e2 means |G|^2 ~ 5e-11, so the ridge has to sit below that."""
    A, c, f = contraction(device)
    thr = 60
    out = deq.anderson(f, torch.zeros_like(c), threshold=thr, eps=3e-7, lam=1e-12)
    want = (c.double() / (1 - A.double())).cpu().numpy()
    err = rel_l2(out["result"].cpu().numpy(), want)
    record("anderson on a contraction vs c / (1 - A)", err, 1e-5)
    assert err <= 1e-5, (err, out["rel_trace"])
    assert set(out) == {"result", "lowest", "nstep", "prot_break", "abs_trace", "rel_trace", "eps", "threshold"}
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == thr - 2
    assert out["nstep"] < thr - 1 and out["lowest"] < 3e-7                           # it stopped early ...
    k = out["nstep"]                                                                 # ... at step k: entries k - 1 .. are the padding
    assert all(v == out["lowest"] for v in out["rel_trace"][k - 1:])
    assert out["rel_trace"][k - 2] == out["lowest"]
    never = deq.anderson(f, torch.zeros_like(c), threshold=12, eps=0.0)
    assert len(never["rel_trace"]) == 10 and never["nstep"] <= 11


def tv_solver(b, psf, device, method="admm"):
    x = dp.Variable()
    fns = dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1))
    return dp.compile(fns, method=method, device=device)


def _amplified(got, ref32, ref64, what):
    """at least as close to the reference's float64 run as its fp32 run is, plus 1e-5; within the sum of the two distances of its fp32 run"""
    gap = rel_l2(ref32, ref64)
    d64, d32 = rel_l2(got, ref64), rel_l2(got, ref32)
    record(f"{what} vs reference float64 (reference fp32: {gap:.2e})", d64, gap + 1e-5)
    record(f"{what} vs reference fp32", d32, d64 + gap + 1e-5)
    assert d64 <= gap + 1e-5, (what, d64, gap)
    assert d32 <= d64 + gap + 1e-5, (what, d32, d64, gap)


def case_tv(device, which):
    """TV deconvolution through DEQSolver against the reference's runs: `small` 2 x 1 x 32 x 48, `256` 1 x 3 x 256 x 256"""
    if which == "small":
        g = load_golden("g41_deq_tv")
        b, psf, x64 = g["b"], g["psf"], g["fwd_x_f64"]
    else:
        g = load_golden("g41_deq_tv256")
        _, b, psf = synthetic.deconv_case(1, 3, 256, 256, seed=int(g["seed"]))
        assert float(np.asarray(b, np.float64).sum()) == float(g["b_checksum"])
        x64 = load_golden("g41_deq_tv256_f64")["fwd_x_f64_rounded"]
    bt = T(b, device)
    solver = tv_solver(bt, psf, device)
    model = dp.specialize(solver, method="deq", device=device)
    model.eps = float(g["eps"])
    model.eval()
    with torch.no_grad():
        x = model.solve(x0=bt.clone(), rhos=float(g["rho"]), lams=float(g["lam"]), f_thres=int(g["thres"]))
    info = model.last_forward
    assert info["nstep"] == int(g["fwd_nstep"]) == int(g["fwd_nstep_f64"])
    _amplified(x.cpu().numpy(), g["fwd_x"], x64, f"deq tv {which} x")
    _amplified(np.array(info["rel_trace"]), g["fwd_rel_trace"], g["fwd_rel_trace_f64"], f"deq tv {which} rel_trace")
    # the fixed-point residual at the returned z*: |f(z*) - z*| / |z*| no larger than the reference's final rel_trace entry + 1e-5
    n = len(solver.psi_fns)
    with torch.no_grad():
        z = [t.detach() for t in info["result"]]
        new = solver.iters((z[0].clone(), [t.clone() for t in z[1:1 + n]], [t.clone() for t in z[1 + n:]]), torch.tensor([float(g["rho"])]),
                           {fn: torch.tensor([float(g["lam"])]) for fn in solver.psi_fns}, 1)
    new = [new[0]] + list(new[1]) + list(new[2])
    num = np.sqrt(sum(float(((a - c).double() ** 2).sum()) for a, c in zip(new, z)))
    den = np.sqrt(sum(float((c.double() ** 2).sum()) for c in z))
    record(f"deq tv {which}: |f(z*) - z*| / |z*|", num / den, float(g["fwd_rel_trace"][-1]) + 1e-5)
    assert num / den <= float(g["fwd_rel_trace"][-1]) + 1e-5, (num / den, g["fwd_rel_trace"][-1])
    return x


def tv_iter_f64(z, b, psf, rho, lam):
    """One ADMM iteration of sum_squares(conv(x, psf) - b) + norm1(grad_H x) + norm1(grad_W x) restated in float64 torch with exact
    OTFs, differentiable in z, b, rho and lam: the x-update (conj(H) F b + rho sum_i conj(G_i) F (v_i - u_i) + 1e-7) /
    (|H|^2 + rho sum_i |G_i|^2 + 1e-7), then d_i = K_i x + u_i, v_i = soft(d_i, lam), u_i = d_i - v_i.  z: the packed state
    [B, 5 C, H, W] = (x, v_1, v_2, u_1, u_2); x does not enter an iteration."""
    B, C5, H, W = z.shape
    C = C5 // 5
    otf = lambda k: torch.from_numpy(np.transpose(O.psf2otf(np.asarray(k, dtype=np.float64), [H, W, C]), (2, 0, 1))[None])
    Hf, Gf = otf(np.asarray(psf)), [otf(O.grad_kernel(0).numpy()), otf(O.grad_kernel(1).numpy())]
    F2 = lambda a: torch.fft.fftn(a, dim=[-2, -1])
    Fi = lambda a: torch.real(torch.fft.ifftn(a, dim=[-2, -1]))
    _, v1, v2, u1, u2 = torch.split(z, C, dim=1)
    num = torch.conj(Hf) * F2(b) + rho * (torch.conj(Gf[0]) * F2(v1 - u1) + torch.conj(Gf[1]) * F2(v2 - u2))
    den = torch.abs(Hf) ** 2 + rho * (torch.abs(Gf[0]) ** 2 + torch.abs(Gf[1]) ** 2)
    x = Fi((num + 1e-7) / (den + 1e-7))
    vs, us = [], []
    for Gi, u in zip(Gf, (u1, u2)):
        d = Fi(Gi * F2(x)) + u
        v = torch.sign(d) * torch.clamp(d.abs() - lam, min=0)
        vs.append(v)
        us.append(d - v)
    return torch.cat([x] + vs + us, dim=1)


def check_restatement():
    """``tv_iter_f64`` at the z* of the reference's float64 run (the fixture's train_z_f64) reproduces that run's f(z*) (train_x_f64)"""
    g = load_golden("g41_deq_tv")
    assert np.float32(RHO) == g["rho"] and np.float32(LAM_TV) == g["lam"]
    z, b = torch.from_numpy(g["train_z_f64"]), torch.from_numpy(g["b"]).double()
    new = tv_iter_f64(z, b, g["psf"], RHO, LAM_TV)
    err = rel_l2(new[:, :b.shape[1]].numpy(), g["train_x_f64"])
    record("float64 restatement of one iteration vs the reference's float64 f(z*)", err, 1e-12)
    assert err <= 1e-12, err


def anderson_f64(f, x0, m=M, lam=LAM, threshold=12, beta=1.0):
    """Anderson acceleration restated in float64 torch on a packed [B, ...] state, never stopping early: X_0 = x0, X_1 = f(x0), then
    per step the bordered system [[0, 1^T], [1, G G^T + lam I]] [nu; alpha] = [1; 0] per image over the n = min(k, m) stored
    residuals G = F - X, X_k = beta alpha F + (1 - beta) alpha X into slot k % m.  Returns the X of the lowest relative residual
    |f(X) - X| / (1e-5 + |f(X)|) (whole-batch norms) and its step."""
    B = x0.shape[0]
    X = torch.zeros((B, m, x0[0].numel()), dtype=torch.float64)
    F = torch.zeros_like(X)
    X[:, 0], F[:, 0] = x0.reshape(B, -1), f(x0).reshape(B, -1)
    X[:, 1], F[:, 1] = F[:, 0], f(F[:, 0].reshape(x0.shape)).reshape(B, -1)
    best, best_k, best_x = 1e8, 0, None
    for k in range(2, threshold):
        n = min(k, m)
        G = F[:, :n] - X[:, :n]
        A = torch.zeros((B, n + 1, n + 1), dtype=torch.float64)
        A[:, 0, 1:] = A[:, 1:, 0] = 1.0
        A[:, 1:, 1:] = G @ G.transpose(1, 2) + lam * torch.eye(n, dtype=torch.float64)
        y = torch.zeros((B, n + 1, 1), dtype=torch.float64)
        y[:, 0] = 1.0
        alpha = torch.linalg.solve(A, y)[:, 1:, 0]
        X[:, k % m] = beta * (alpha[:, None] @ F[:, :n])[:, 0] + (1 - beta) * (alpha[:, None] @ X[:, :n])[:, 0]
        F[:, k % m] = f(X[:, k % m].reshape(x0.shape)).reshape(B, -1)
        rel = float((F[:, k % m] - X[:, k % m]).norm() / (1e-5 + F[:, k % m].norm()))
        if rel < best:
            best, best_k, best_x = rel, k, X[:, k % m].reshape(x0.shape).clone()
    return best_x, best_k


def check_backward_restatement():
    """The implicit backward restated in float64 -- ``tv_iter_f64`` at the fixture's train_z_f64, y = J^T y + g from zero through
    ``anderson_f64`` with the fixture's threshold, then (d f / d (r, l, b))^T y -- reproduces the reference's float64 gradients: an
    oracle for them that shares no code with the reference.  Bound 1e-10: the reference's own fp32 / float64 gradients differ by up to
    4.3e-5 = 7e2 fp32 roundings, and 7e2 float64 roundings are 8e-14."""
    g = load_golden("g41_deq_tv")
    z = torch.from_numpy(g["train_z_f64"]).requires_grad_()
    b = torch.from_numpy(g["b"]).double().requires_grad_()
    r = torch.ones((), dtype=torch.float64, requires_grad=True)
    l = torch.ones((), dtype=torch.float64, requires_grad=True)
    new = tv_iter_f64(z, b, g["psf"], r * RHO, l * LAM_TV)
    grad = torch.zeros_like(new)
    grad[:, :b.shape[1]] = torch.from_numpy(g["w"]).double()
    y, k = anderson_f64(lambda y: torch.autograd.grad(new, z, y, retain_graph=True)[0] + grad, torch.zeros_like(grad),
                        threshold=int(g["thres"]))
    assert k == int(g["bwd_nstep_f64"])
    for name, got in zip(("g_r", "g_l", "g_b"), torch.autograd.grad(new, (r, l, b), y)):
        err = rel_l2(got.numpy(), g[name + "_f64"])
        record(f"float64 restatement of the implicit backward, {name} vs the reference's float64", err, 1e-10)
        print(f"restated backward {name}: {err:.3e}")
        assert err <= 1e-10, (name, err)


def case_backward(device):
    """training mode, learned_params: gradients of sum(w x) w.r.t. r, l and the observation against the reference's float64 gradients
    under the amplified-round-off criterion; one AdamW step changes r and l.
    Not compared: the exact implicit gradient of the float64 restatement.  (I - J^T) y = g has no solution to 1e-10 at this z*: the
    plain iteration y <- J^T y + g still moves y by 4.4e-5 |y| per step after 20000 steps, and full GMRES in float64 does not reach
    1e-10 |g| within 3000 vectors.  Where the shrinkage is inactive u_new = K x + u, and x does not move with a dual direction in the
    null space of sum_i K_i^T, so J has the eigenvalue 1 there and I - J^T is singular."""
    g = load_golden("g41_deq_tv")
    bt = T(g["b"], device).requires_grad_()
    solver = tv_solver(bt, g["psf"], device)
    model = dp.specialize(solver, method="deq", device=device, learned_params=True)
    model.eps = float(g["eps"])
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    x = model.solve(x0=bt.detach().clone(), rhos=float(g["rho"]), lams=float(g["lam"]), f_thres=int(g["thres"]), b_thres=int(g["thres"]))
    assert model.last_forward["nstep"] == int(g["train_nstep"])
    _amplified(x.detach().cpu().numpy(), g["train_x"], g["train_x_f64"], "deq train x")
    (T(g["w"], device) * x).sum().backward()
    for name, got in (("g_r", model.r.grad), ("g_l", model.l.grad), ("g_b", bt.grad)):
        assert got is not None, name
        _amplified(got.detach().cpu().numpy(), g[name], g[name + "_f64"], f"deq grad {name}")
    r0, l0 = float(model.r), float(model.l)
    opt.step()
    assert float(model.r) != r0 and float(model.l) != l0
