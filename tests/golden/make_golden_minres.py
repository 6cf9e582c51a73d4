#!/usr/bin/env python
"""Golden vectors of the MINRES solver -- runs ONLY in the build container (needs the reference checkout).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt) and runs the reference's
``minres`` (dprox/linalg/solve/solver_minres.py) on the CPU in float32 and in float64 on fixed-seed inputs.

Operators: a symmetric tridiagonal stored as its diagonal ``d[N]`` and off-diagonal ``e[N-1]`` (the tests rebuild the matrix-free
callable of tests/minres_cases.py:tridiag, restated below), or, for N <= 64, a dense symmetric matrix ``M``.  The tridiagonal entries
are multiples of 1/16 and 1/64 and the right-hand sides multiples of 1/8, so the arrays compress to a fraction of their size.

Per case ``<name>_*``: the inputs, ``x32`` / ``x64`` (the reference's float32 / float64 solutions; the float64 run takes the
float32 inputs promoted exactly), ``steps`` (operator applications of the float32 run's loop, i.e. its exit step), ``res32`` (the
largest scaled residual |(value A + shift) x - b| / |b| over the systems and shifts of the float32 run) and ``perm64`` (the relative
l2 distance between the float64 solution and the float64 solution of the same system with its unknowns in reversed order -- every
sum of the solve then runs in another order: the float64 yardstick).  The generator refuses a case whose float32 run does not reach
res32 < 1e-3: a test must not certify the agreement of two diverged iterates.

  g42_minres           every case but the long vector
  g42_minres_long      [70001, 1]: inputs and x32
  g42_minres_long_f64  its x64

The one-unknown case is stored from the float64 run only (``one_x32`` is absent): the reference's float32 run of it returns NaN --
``beta`` is clamped to eps = 1e-25, whose square underflows in float32, and the next rotation divides 0 by 0.

    python tests/golden/make_golden_minres.py
"""
import os
import runpy

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp, save = G["np"], G["torch"], G["dp"], G["save"]
from dprox.linalg.solve.solver_minres import minres  # noqa: E402   (the REFERENCE's)

assert dp.__file__.startswith(G["REF"]), dp.__file__


def tridiag(d, e):
    """x [..., N, K] -> T x for the symmetric tridiagonal T = diag(d) + diag(e, 1) + diag(e, -1)"""
    def A(x):
        y = d[:, None] * x
        y[..., 1:, :] += e[:, None] * x[..., :-1, :]
        y[..., :-1, :] += e[:, None] * x[..., 1:, :]
        return y
    return A


def tri_inputs(rng, N, shape, indefinite):
    """|d| in [2, 3) in steps of 1/16 (every third entry negative when indefinite), |e| <= 1/4 in steps of 1/64: strictly
    diagonally dominant, eigenvalues in +-[1.5, 3.5]; b in [-2, 2] in steps of 1/8"""
    d = 2.0 + rng.randint(0, 16, N) / 16.0
    if indefinite:
        d = np.where(np.arange(N) % 3 == 0, -d, d)
    e = rng.randint(-16, 17, max(N - 1, 0)) / 64.0
    b = rng.randint(-16, 17, shape) / 8.0
    return d.astype(np.float32), e.astype(np.float32), b.astype(np.float32)


def counted(A):
    calls = [0]

    def f(x):
        calls[0] += 1
        return A(x)
    return f, calls


def run_case(name, make_op, b, kw=None, minv=None, f32=True):
    """the reference in float32 and float64; ``make_op(dtype, flip)`` returns the operator, ``flip``: on reversed unknowns"""
    kw = dict(kw or {})
    out = {}

    def solve(dt, flip=False):
        bt = torch.from_numpy(b).to(dt)
        if flip:
            bt = torch.flip(bt, dims=(-2,) if bt.ndim > 1 else (0,))
        k = {a: (v.to(dt) if isinstance(v, torch.Tensor) else v) for a, v in kw.items()}
        if minv is not None:
            p = torch.from_numpy(minv).to(dt)
            p = torch.flip(p, dims=(0,)) if flip else p
            k["Minv"] = lambda v: v / p[:, None]
        A, calls = counted(make_op(dt, flip))
        with torch.no_grad():
            x = minres(A, bt.clone(), **k)
        if flip:
            x = torch.flip(x, dims=(-2,) if bt.ndim > 1 else (0,))
        n = calls[0] - 1                                  # (one application before the loop; one per stop test, every tenth step)
        return x, next(s for s in range(n + 1) if s + s // 10 == n), A

    x64, _, A64 = solve(torch.float64)
    p64, _, _ = solve(torch.float64, flip=True)
    out["x64"] = x64.numpy()
    out["perm64"] = float((p64 - x64).norm() / x64.norm())

    def residual(x, A, dt):
        bt = torch.from_numpy(b).to(dt)
        shifts = kw.get("shifts")
        xs = x if (shifts is not None and shifts.numel() > 1) else x[None]
        sh = [0.0] if shifts is None else [float(s) for s in shifts.reshape(-1)]
        worst = 0.0
        for s, xi in zip(sh, xs):
            Ax = A(xi.reshape(bt.shape) if bt.ndim > 1 else xi)
            r = kw.get("value", 1.0) * Ax + s * xi - bt
            ax = -2 if bt.ndim > 1 else 0
            bn = bt.norm(dim=ax)
            keep = bn > 1e-10
            worst = max(worst, float((r.norm(dim=ax)[keep] / bn[keep]).max()))
        return worst

    assert residual(x64, A64, torch.float64) < 1e-6, (name, residual(x64, A64, torch.float64))
    if f32:
        x32, steps, A32 = solve(torch.float32)
        out["x32"], out["steps"] = x32.numpy(), steps
        out["res32"] = residual(x32, A32, torch.float32)
        assert np.isfinite(out["res32"]) and out["res32"] < 1e-3, (name, out["res32"])
        print(f"{name:10s} steps {steps:3d}  res32 {out['res32']:.2e}  |x32 - x64| {float((x32.double() - x64).norm() / x64.norm()):.2e}  perm64 {out['perm64']:.2e}")
    else:
        print(f"{name:10s} float64 only  perm64 {out['perm64']:.2e}")
    return {f"{name}_{k}": v for k, v in out.items()}


def tri_case(name, rng, shape, indefinite=True, **more):
    N = shape[-2]
    d, e, b = tri_inputs(rng, N, shape, indefinite)
    b = more.pop("edit_b", lambda t: t)(b)

    def make_op(dt, flip):
        dd, ee = torch.from_numpy(d).to(dt), torch.from_numpy(e).to(dt)
        return tridiag(torch.flip(dd, (0,)), torch.flip(ee, (0,))) if flip else tridiag(dd, ee)
    out = run_case(name, make_op, b, **more)
    out.update({f"{name}_d": d, f"{name}_e": e, f"{name}_b": b})
    return out


def main():
    small = {}
    # the reference's own test (tests/linalg/test_linear_solver.py:6-14, 98-111): a 5 x 5 SPD matrix, a 1-D float64 right-hand side
    import dprox.utils
    dprox.utils.misc.seed_everything(2023)
    P = np.random.rand(5, 5)
    M5 = P.T @ P + 0.01 * np.eye(5)
    x5 = np.random.rand(5)
    b5 = M5 @ x5

    def dense_op(M):
        def make_op(dt, flip):
            Mt = torch.from_numpy(M).to(dt)
            Mt = torch.flip(Mt, (0, 1)) if flip else Mt
            return lambda v: Mt @ v
        return make_op
    small.update(run_case("own", dense_op(M5), b5, f32=False))
    small.update(own_M=M5, own_x=x5, own_b=b5)

    rng = np.random.RandomState(42)
    # one unknown: max_iters = 2, a loop of 4 steps, beta clamped to eps from the second step on
    M1, b1 = np.array([[2.5]], np.float32), np.array([[[0.75]]], np.float32)
    small.update(run_case("one", dense_op(M1), b1, f32=False))
    small.update(one_M=M1, one_b=b1)

    # dense indefinite 33 x 33: eigenvalues in +-[1, 3]
    Q, _ = np.linalg.qr(rng.randn(33, 33))
    lam = (1.0 + 2.0 * rng.rand(33)) * np.where(np.arange(33) % 2 == 0, 1.0, -1.0)
    M33 = (Q * lam) @ Q.T
    M33 = (0.5 * (M33 + M33.T)).astype(np.float32)
    b33 = (rng.randint(-16, 17, (33, 1)) / 8.0).astype(np.float32)
    small.update(run_case("dense33", dense_op(M33), b33, kw=dict(max_iters=100)))
    small.update(dense33_M=M33, dense33_b=b33)

    small.update(tri_case("rag3", rng, (257, 3)))
    small.update(tri_case("rag5", rng, (2, 130, 5)))
    small.update(tri_case("wide4", rng, (4096, 4)))
    small.update(tri_case("many70", rng, (64, 70)))

    def zero_col(b):
        b[:, 1] = 0.0
        return b
    small.update(tri_case("zero", rng, (40, 3), edit_b=zero_col))
    small.update(tri_case("shift3", rng, (129, 2), indefinite=False, kw=dict(shifts=torch.tensor([0.0, 0.5, 2.0]), value=0.5)))
    small.update(tri_case("shift1", rng, (129, 2), indefinite=False, kw=dict(shifts=torch.tensor([0.5]), value=0.5)))
    pdiag = (0.5 + rng.randint(0, 17, 257) / 16.0).astype(np.float32)
    small.update(tri_case("prec", rng, (257, 1), indefinite=False, minv=pdiag))
    small["prec_p"] = pdiag
    save("g42_minres", **small)

    long_ = tri_case("long", rng, (70001, 1), indefinite=False)
    assert long_["long_steps"] % 10 == 0 and long_["long_steps"] < 102, long_["long_steps"]      # the stop rule's exit is taken
    save("g42_minres_long_f64", long_x64=long_.pop("long_x64"))
    save("g42_minres_long", **long_)


if __name__ == "__main__":
    main()
