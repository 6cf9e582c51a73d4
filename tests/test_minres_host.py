"""CPU-only: the host side of ``dprox.linalg.solve.minres`` (kernels under the SIMT emulator): the registry, ``LinearSolve`` with
solver_type="minres" forward and backward, the reference's own test restated, the implicit gradient of a direct call, and how
arguments are taken."""
import numpy as np
import pytest
import torch

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import minres_cases as mc  # noqa: E402

DEV = "cpu"


def test_registry_lists_minres():
    import dprox as dp
    from dprox.linalg import solve
    from dprox.linalg.solve.minres import minres
    assert solve.available_solvers == ["cg", "cg2", "pcg", "minres"] and solve.__all__ == solve.available_solvers
    assert solve.SOLVERS["minres"] is minres and dp.linalg.solve.minres is minres
    assert sorted(solve.SOLVERS) == ["cg", "cg2", "minres", "pcg"]


def test_linear_solve_minres_gradient():
    mc.case_linear_solve(DEV)


def test_reference_test_minres_restated():
    mc.case_own(DEV)


def test_direct_call_carries_the_implicit_gradient():
    """b.requires_grad: the solution comes back with the implicit backward of krylov._ImplicitCG, as cg's does"""
    from dprox.linalg.solve import minres
    g = mc.golden()
    A, b, kw = mc.inputs("dense33", DEV)
    b = b.clone().requires_grad_(True)
    x = minres(A, b, **kw)
    assert x.requires_grad
    w = np.cos(np.arange(33.0))[:, None]
    (x * mc.T(w, DEV, torch.float32)).sum().backward()
    want = np.linalg.solve(g["dense33_M"].astype(np.float64).T, w)
    assert mc.rel_l2(b.grad.numpy(), want) <= 1e-3
    with pytest.raises(NotImplementedError, match="single shift"):
        minres(A, b, shifts=torch.tensor([0.0, 1.0]))


def test_shifts_are_cast_not_rejected():
    from dprox.linalg.solve import minres
    A, b, kw = mc.inputs("shift3", DEV)
    want = minres(A, b, **kw)
    assert torch.equal(minres(A, b, **dict(kw, shifts=kw["shifts"].double())), want)
    ints = minres(A, b, **dict(kw, shifts=torch.tensor([0, 2])))
    assert ints.dtype == torch.float32 and torch.equal(ints[1], want[2])
    assert torch.equal(minres(A, b, **dict(kw, shifts=[0.0, 0.5, 2.0])), want)


def test_non_callable_operator_raises():
    from dprox.linalg.solve import minres
    _, b, _ = mc.inputs("dense33", DEV)
    with pytest.raises(TypeError, match="callable"):
        minres(torch.eye(33), b)
    with pytest.raises(TypeError, match="Minv"):
        minres(lambda v: v, b, Minv=torch.eye(33))


def test_x0_is_ignored_and_other_dtypes_run_in_float32():
    from dprox.linalg.solve import minres
    A, b, kw = mc.inputs("dense33", DEV)
    want = minres(A, b, **kw)
    assert torch.equal(minres(A, b, x0=torch.ones_like(b), **kw), want)
    half = minres(A, b.to(torch.bfloat16), **kw)
    assert half.dtype == torch.float32


def test_verbose_prints_the_references_line(capsys):
    from dprox.linalg.solve import minres
    A, b, kw = mc.inputs("dense33", DEV)
    minres(A, b, verbose=True, **kw)
    assert capsys.readouterr().out.startswith(
        "Running MINRES on a torch.Size([33, 1]) RHS for 34 iterations (rtol=1e-06). Output: torch.Size([1, 33, 1]).")
