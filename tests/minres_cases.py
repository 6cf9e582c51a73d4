"""MINRES cases shared by the GPU tests (-m gpu, real MI355X), the emulated-kernel tests (CPU, the same kernel sources under the SIMT
emulator) and the host tests: one Lanczos + update step against a float64 restatement written here, and ``minres`` against the
reference's stored float32 and float64 runs (tests/golden/g42_minres*.npz, make_golden_minres.py).

Single step (the only fixed, derived bounds; u = the element type's machine epsilon, every quantity of the right-hand sides taken
from the float64 restatement): a reduction over N products is within (sqrt(N) + 4) u sum|x_i y_i| -- sqrt(N) u for the sum, a few
u for the products and the final scale; beta_curr, a square root of such a sum, within the same factor of itself; an elementwise
result within 4 u (6 u for the search vector: three terms and a division) of the sum of the magnitudes of its terms, plus what the
error of an input computed in the same step contributes; the Givens scalars, float64 for both element types, within 1e-13 of
their scale.  Each stage is compared given the device's result of the stage before, so the bounds do not compound.

Solver (round-off amplified by the recurrences, so no number chosen in advance): the relative l2 distance of this backend's
float32 solution from the reference's float64 solution is at most the distance of the reference's own float32 run from it, plus
1e-5 (README "parity").  Float64 cases: at most the distance ``perm64`` between the reference's float64 solution and its float64
solution of the same system with the unknowns reversed (every sum in another order), plus 1e-5 u64 / u32 -- the same slack on
float64's scale.  The one-unknown case has no float32 yardstick (the reference's float32 run of it returns NaN: eps^2 underflows);
its float32 run here is held to 1e-5 of the float64 solution, the slack alone."""
import json
import os

import numpy as np
import torch

from conftest import load_golden, record, rel_l2
from dprox import _ops as ops

SLACK = 1e-5
SLACK64 = SLACK * float(np.finfo(np.float64).eps / np.finfo(np.float32).eps)
F32_CASES = ["dense33", "rag3", "rag5", "wide4", "many70", "zero", "shift3", "shift1", "prec", "long"]
ACHIEVED = {}          # case -> distances; written to the file DPX_MINRES_PARITY_OUT names, if it is set (write_achieved)

_golden = {}


def golden():
    if not _golden:
        for f in ("g42_minres", "g42_minres_long", "g42_minres_long_f64"):
            _golden.update(load_golden(f))
    return _golden


def T(a, device, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def tridiag(d, e):
    """x [..., N, K] -> T x for the symmetric tridiagonal T = diag(d) + diag(e, 1) + diag(e, -1), matrix-free"""
    def A(x):
        y = d[:, None] * x
        y[..., 1:, :] += e[:, None] * x[..., :-1, :]
        y[..., :-1, :] += e[:, None] * x[..., 1:, :]
        return y
    return A


def inputs(name, device, dtype=torch.float32):
    """(A, b, kwargs) of a stored case on ``device``"""
    g = golden()
    b = T(g[f"{name}_b"], device, dtype)
    if f"{name}_M" in g:
        M = T(g[f"{name}_M"], device, dtype)
        A = lambda v: M @ v
    else:
        A = tridiag(T(g[f"{name}_d"], device, dtype), T(g[f"{name}_e"], device, dtype))
    kw = {}
    if name == "dense33":
        kw["max_iters"] = 100
    if name in ("shift3", "shift1"):
        kw.update(shifts=torch.tensor([0.0, 0.5, 2.0] if name == "shift3" else [0.5]), value=0.5)
    if name == "prec":
        p = T(g["prec_p"], device, dtype)
        kw["Minv"] = lambda v: v / p[:, None]
    return A, b, kw


def solve(name, device, dtype=torch.float32):
    from dprox.linalg.solve import minres
    A, b, kw = inputs(name, device, dtype)
    calls = [0]

    def counted(v):
        calls[0] += 1
        return A(v)
    x = minres(counted, b, **kw)
    assert x.dtype == dtype and x.device.type == torch.device(device).type
    return x, calls[0]


def case_parity(device, name):
    """a float32 case against the reference's two runs"""
    g = golden()
    x, calls = solve(name, device)
    x = x.cpu().numpy()
    x32, x64 = g[f"{name}_x32"], g[f"{name}_x64"]
    assert x.shape == x64.shape, (x.shape, x64.shape)
    # operator applications: one per step and one per stop test, every tenth step; the exit is at a multiple of ten or after
    # max_iters + 2 steps.  The long vector's exit is far from the threshold (res32 in the fixture): there it is the reference's.
    ref_steps, last = int(g[f"{name}_steps"]), min(100, x64.shape[-2] + 1) + 2
    steps = next(s for s in range(calls + 1) if s + s // 10 == calls)
    assert steps == last or (steps % 10 == 0 and steps < last), (name, calls, steps)
    if name == "long":
        assert steps == ref_steps and steps % 10 == 0 and steps < last, (steps, ref_steps)
    ours, theirs = rel_l2(x, x64), rel_l2(x32, x64)
    ACHIEVED[name] = dict(dtype="float32", ours_vs_ref64=ours, ref32_vs_ref64=theirs, bound=theirs + SLACK, steps=steps)
    record(f"minres {name} vs the reference's float64 run", ours, theirs + SLACK)
    print(f"minres {name}: |x - x64| {ours:.3e}; the reference's float32 run {theirs:.3e}")
    assert np.isfinite(x).all()
    assert ours <= theirs + SLACK, (name, ours, theirs)
    if name == "zero":
        assert np.all(x[:, 1] == 0.0) and np.all(x[:, 0] != 0.0)
    if name == "shift3":
        assert x.shape == (3, 129, 2)
    if name == "shift1":
        assert x.shape == (129, 2)
    return x


def case_own(device):
    """the reference's tests/linalg/test_linear_solver.py::test_minres restated: float64, a 1-D right-hand side, rtol 1e-8"""
    g = golden()
    x, _ = solve("own", device, torch.float64)
    assert x.shape == (5,)
    assert torch.allclose(x.cpu(), torch.from_numpy(g["own_x"]), rtol=1e-8)
    _f64_criterion("own", x.cpu().numpy(), g)


def case_one_unknown(device):
    g = golden()
    A, b, kw = inputs("one", device, torch.float64)
    calls = [0]

    def counted(v):
        calls[0] += 1
        return A(v)
    from dprox.linalg.solve import minres
    x = minres(counted, b, **kw)
    assert calls[0] == 4 and x.shape == (1, 1, 1)                        # max_iters = min(100, N + 1) = 2: a loop of 4 steps
    _f64_criterion("one", x.cpu().numpy(), g)
    x32, _ = solve("one", device, torch.float32)
    d = rel_l2(x32.cpu().numpy(), g["one_x64"])
    ACHIEVED["one_float32"] = dict(dtype="float32", ours_vs_ref64=d, ref32_vs_ref64=None, bound=SLACK)
    print(f"minres one (float32): |x - x64| {d:.3e}")
    assert d <= SLACK, d


def _f64_criterion(name, x, g):
    ours, perm = rel_l2(x, g[f"{name}_x64"]), float(g[f"{name}_perm64"])
    ACHIEVED[name] = dict(dtype="float64", ours_vs_ref64=ours, ref64_permuted_vs_ref64=perm, bound=perm + SLACK64)
    record(f"minres {name} (float64) vs the reference's float64 run", ours, perm + SLACK64)
    print(f"minres {name} (float64): |x - x64| {ours:.3e}; the reference's permuted float64 run {perm:.3e}")
    assert ours <= perm + SLACK64, (name, ours, perm)


def case_deterministic(device):
    a, _ = solve("long", device)
    b, _ = solve("long", device)
    assert torch.equal(a, b)


def case_linear_solve(device):
    """``LinearSolve`` with solver_type="minres" on the dense indefinite system: the solution and the gradient of sum(w x) w.r.t. b
    (the implicit backward: one more solve with the transposed operator) against float64 dense solves computed here, at the bound
    the implicit-gradient tests of ``cg`` use (parity_cases.case_dense_krylov: 1e-3)"""
    import dprox as dp
    from conftest import assert_close
    from dprox.linalg import LinearSolveConfig, linear_solve
    g = golden()

    class MatrixOp(dp.LinOp):
        def __init__(self, M):
            super().__init__()
            self.A = torch.nn.Parameter(M)

        def forward(self, v):
            return self.A @ v

        def adjoint(self, v):
            return self.A.T @ v

    M64, b64 = g["dense33_M"].astype(np.float64), g["dense33_b"].astype(np.float64)
    w64 = np.cos(np.arange(33.0))[:, None]
    op = MatrixOp(T(g["dense33_M"], device))
    b = T(g["dense33_b"], device).clone().requires_grad_(True)
    x = linear_solve(op, b, LinearSolveConfig(rtol=1e-6, max_iters=100, solver_type="minres"))
    (x * T(w64, device, torch.float32)).sum().backward()
    assert_close(x.detach().cpu().numpy(), np.linalg.solve(M64, b64), 1e-3, "LinearSolve(minres) x")
    assert_close(b.grad.cpu().numpy(), np.linalg.solve(M64.T, w64), 1e-3, "LinearSolve(minres) implicit d/db")
    assert op.A.grad is not None and torch.isfinite(op.A.grad).all()


def write_achieved():
    """the measured distances of the cases run so far -> the JSON file the environment variable DPX_MINRES_PARITY_OUT names (how
    profiles/minres_parity_achieved.json is produced from a GPU run); without the variable nothing is written"""
    path = os.environ.get("DPX_MINRES_PARITY_OUT")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ACHIEVED, f, indent=1, sort_keys=True)


# ---- one step against float64 ---------------------------------------------------------------------------------------------------

def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def case_step(device, shape, dtype, prec=False, steps=3, seed=0):
    """``steps`` consecutive steps from a random state (so every role of the rings and of the rotation slots comes up), S = 2 shifts,
    value = 0.75; before each step the device's state is read back and the step restated in float64 (solver_minres.py:146-213,
    258-290); ``prec``: the split path around a preconditioner"""
    G, N, K = shape
    S, value, eps = 2, 0.75, 1e-25
    u = float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)
    red = np.sqrt(N) + 4.0
    rng = np.random.RandomState(seed)
    rnd = lambda *s: T(rng.randn(*s), device, dtype)
    ctl = ops.MinresControl(rnd(G, N, K), torch.tensor([0.0, 0.7]), value, eps)
    ctl.zring.copy_(rnd(2, G, N, K))
    ctl.search.copy_(rnd(2, S, G, N, K))
    ctl.solution.copy_(rnd(S, G, N, K))
    f = ctl.fields()
    f["beta"].copy_(T(0.5 + rng.rand(2, G, K), device))
    ang = rng.rand(3, S, G, K) * 2 * np.pi
    f["cos"].copy_(T(np.cos(ang), device))
    f["sin"].copy_(T(np.sin(ang), device))
    f["scale"].copy_(T(rng.randn(2, S, G, K), device))
    shifts = _np(f["shifts"])
    q = rnd(G, N, K) if prec else None
    pdiag = T(0.5 + rng.rand(N, 1), device, dtype)
    col = lambda a: a[:, None, :]                                         # a per-system scalar [G, K] against [G, N, K]
    for i in range(steps):
        assert int(f["step"][0]) == i
        cur = i & 1
        z, srch, sol = _np(ctl.zring), _np(ctl.search), _np(ctl.solution)
        beta, cos, sin, scale = _np(f["beta"]), _np(f["cos"]), _np(f["sin"]), _np(f["scale"])
        qv = _np(q) if prec else z[1 - cur]
        prod_t = rnd(G, N, K)
        prod = _np(prod_t)
        # alpha
        ctl.alpha(prod_t, q)
        al = _np(f["alpha"])
        al_ref = value * np.sum(prod * qv, axis=1)
        assert np.all(np.abs(al - al_ref) <= red * u * value * np.sum(np.abs(prod * qv), axis=1)), (i, "alpha", al, al_ref)
        # Lanczos vector and beta_curr (given the device's alpha)
        bp = beta[cur]
        z_ref = value * prod - col(al) * z[1 - cur] - col(bp) * z[cur]
        z_mag = np.abs(value * prod) + np.abs(col(al) * z[1 - cur]) + np.abs(col(bp) * z[cur])
        if prec:
            ctl.lanczos(prod_t, finish=False)
            zc = _np(ctl.zring[cur])
            qc = (ctl.zring[cur] / pdiag).contiguous()
            ctl.beta(qc)
            qcv = _np(qc)
            bc_ref = np.sqrt(np.sum(zc * qcv, axis=1))
            bc_tol = red * u * np.sum(np.abs(zc * qcv), axis=1) / (2 * bc_ref)
        else:
            ctl.lanczos(prod_t)
            zc = _np(ctl.zring[cur])
            bc_ref = np.sqrt(np.sum(zc * zc, axis=1))
            bc_tol = red * u * bc_ref
        assert np.all(np.abs(zc - z_ref) <= 4 * u * z_mag), (i, "z", np.abs(zc - z_ref).max())
        assert np.array_equal(_np(ctl.zring[1 - cur]), z[1 - cur])
        bc = _np(f["beta"])[1 - cur]
        assert np.all(np.abs(bc - bc_ref) <= bc_tol + 1e-300), (i, "beta", bc, bc_ref)
        assert np.array_equal(_np(f["beta"])[cur], bp)
        # the rotations (given the device's alpha and beta_curr), every shift
        c2, s2, c1, s1 = cos[(i + 1) % 3], sin[(i + 1) % 3], cos[(i + 2) % 3], sin[(i + 2) % 3]
        subsub = s2 * bp
        sub = c2 * bp
        ash = al[None] + shifts[:, None, None]
        diag = ash * c1 - s1 * sub
        sub = sub * c1 + s1 * ash
        radius = np.sqrt(diag * diag + bc[None] ** 2)
        cc, sc = diag / radius, bc[None] / radius
        diag = diag * cc + sc * bc[None]
        sp = scale[cur]
        scale_cur, scale_prev = -sp * sc, sp * cc
        big = 1e-13 * (1.0 + np.abs(ash) + bp[None] + bc[None])
        got = {k: _np(f[k]) for k in ("cos", "sin", "subsub", "sub", "diag", "scale")}
        for name, ref, dev in (("cos", cc, got["cos"][i % 3]), ("sin", sc, got["sin"][i % 3]), ("subsub", subsub, got["subsub"]),
                               ("sub", sub, got["sub"]), ("diag", diag, got["diag"]), ("scale_curr", scale_cur, got["scale"][1 - cur]),
                               ("scale_prev", scale_prev, got["scale"][cur])):
            assert np.all(np.abs(dev - ref) <= big * np.maximum(1.0, np.abs(sp))), (i, name, np.abs(dev - ref).max())
        assert np.array_equal(got["cos"][(i + 1) % 3], c2) and np.array_equal(got["cos"][(i + 2) % 3], c1)
        # normalisation, search vectors and solutions (given the device's scalars)
        if prec:
            ctl.update(q, qc)
            assert np.all(np.abs(_np(qc) - qcv / col(bc)) <= 4 * u * np.abs(qcv / col(bc))), (i, "qc")
        else:
            ctl.update()
        zn = _np(ctl.zring[cur])
        assert np.all(np.abs(zn - zc / col(bc)) <= 4 * u * np.abs(zc / col(bc))), (i, "z / beta")
        d_sub, d_subsub, d_diag, d_scale = (a[:, :, None, :] for a in (got["sub"], got["subsub"], got["diag"], got["scale"][cur]))
        s_ref = (qv[None] - d_sub * srch[1 - cur] - d_subsub * srch[cur]) / d_diag
        s_mag = (np.abs(qv[None]) + np.abs(d_sub * srch[1 - cur]) + np.abs(d_subsub * srch[cur])) / np.abs(d_diag)
        s_dev = _np(ctl.search[cur])
        assert np.all(np.abs(s_dev - s_ref) <= 6 * u * s_mag), (i, "search", np.abs(s_dev - s_ref).max())
        assert np.array_equal(_np(ctl.search[1 - cur]), srch[1 - cur])
        x_ref = sol + s_ref * d_scale
        x_tol = 4 * u * (np.abs(sol) + np.abs(s_ref * d_scale)) + 6 * u * s_mag * np.abs(d_scale)
        assert np.all(np.abs(_np(ctl.solution) - x_ref) <= x_tol), (i, "solution")
        assert int(f["step"][0]) == i + 1
        if prec:
            q = qc
