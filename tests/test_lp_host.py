"""CPU-only, no device and no kernel: the host side of ``dprox.algo.lp`` -- the preprocessing against the reference's stored
scalings, the three input forms, the refusals (each before anything is launched: the library is out of reach in this module), the
switches that are not built, the PCG tolerances, and the pieces ``Problem`` reads a linear program from."""
import numpy as np
import pytest
import torch

import lp_cases as lc


@pytest.fixture(autouse=True)
def _no_library(monkeypatch):
    """nothing here may load the library or launch: reaching for it fails the test"""
    from dprox import _backend as be

    def refuse():
        raise AssertionError("the host layer reached for the kernel library")
    monkeypatch.setattr(be, "lib", refuse)
    yield


@pytest.mark.parametrize("name", lc.CASES)
def test_preprocessing_is_the_references(name):
    lc.case_preprocess(name)


def test_the_package_does_not_import_scipy():
    import subprocess
    import sys
    code = "import sys; sys.path[:0] = %r; import dprox.algo.lp; assert 'scipy' not in sys.modules, 'scipy imported'" % (sys.path[:3],)
    subprocess.run([sys.executable, "-c", code], check=True)


class _Duck:
    """what a SciPy matrix looks like to the package: ``.tocsr()`` and indptr / indices / data / shape"""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, shape

    def tocsr(self):
        return self


def test_three_input_forms_give_identical_csr():
    from dprox.algo import lp
    g = lc.golden()
    for name in ("tiny", "longrow"):
        ub, eq = lc.csr_of(name, "ub"), lc.csr_of(name, "eq")
        args = lambda f: (g[f"{name}_c"], f(ub), g[f"{name}_b_ub"], f(eq), g[f"{name}_b_eq"])
        forms = [lp.LPProblem(*args(lambda t: t)), lp.LPProblem(*args(lambda t: _Duck(*t))), lp.LPProblem(*args(lambda t: lc._dense(*t))),
                 lp.LPProblem(*args(lambda t: torch.from_numpy(lc._dense(*t))))]
        for other in forms[1:]:
            for a, b in zip(forms[0].A + forms[0].AT, other.A + other.AT):
                assert np.array_equal(a, b)
            assert np.array_equal(forms[0].Acnorm, other.Acnorm) and forms[0].gamma_b == other.gamma_b
        A, AT = lc._dense(*forms[0].A, (forms[0].m, forms[0].n)), lc._dense(*forms[0].AT, (forms[0].n, forms[0].m))
        assert np.array_equal(A.T, AT)
        assert forms[0].A[0].dtype.kind == "i" and np.all(np.diff(forms[0].AT[0]) >= 1)


def _tiny(**edit):
    g = lc.golden()
    ub, eq = [list(lc.csr_of("tiny", t)) for t in ("ub", "eq")]
    args = dict(c=g["tiny_c"], ub=ub, b_ub=g["tiny_b_ub"], eq=eq, b_eq=g["tiny_b_eq"])
    for k, fn in edit.items():
        args[k] = fn(args[k])
    return args["c"], tuple(args["ub"]), args["b_ub"], tuple(args["eq"]), args["b_eq"]


def _with(i, fn):
    def edit(csr):
        csr = list(csr)
        csr[i] = fn(np.array(csr[i]))
        return csr
    return edit


@pytest.mark.parametrize("what, edit, match", [
    ("unsorted offsets", dict(ub=_with(0, lambda p: p[[0, 2, 1] + list(range(3, len(p)))])), "monotone"),
    ("an offset that does not end at nnz", dict(ub=_with(0, lambda p: np.concatenate([p[:-1], p[-1:] - 1]))), "indptr"),
    ("an index out of range", dict(eq=_with(1, lambda i: np.concatenate([i[:-1], [5]]))), "column index"),
    ("a negative index", dict(eq=_with(1, lambda i: np.concatenate([[-1], i[1:]]))), "column index"),
    ("an empty row", dict(ub=_with(0, lambda p: np.concatenate([p[:1], p[:1], p[2:]]))), "empty"),
    ("mismatched CSR lengths", dict(ub=_with(2, lambda d: d[:-1])), "lengths"),
    ("a right-hand side of another length", dict(b_ub=lambda b: b[:-1]), "b_ub"),
    ("matrices of another width", dict(c=lambda c: c[:-1]), "unknowns"),
])
def test_refusals(what, edit, match):
    from dprox.algo import lp
    with pytest.raises(ValueError, match=match):
        lp.LPProblem(*_tiny(**edit))


def test_float32_is_refused_by_name():
    from dprox.algo import lp
    for edit in (dict(c=lambda c: c.astype(np.float32)), dict(ub=_with(2, lambda d: d.astype(np.float32))),
                 dict(b_eq=lambda b: torch.from_numpy(b).float())):
        with pytest.raises(NotImplementedError, match="float32"):
            lp.LPProblem(*_tiny(**edit))
    with pytest.raises(NotImplementedError, match="float32"):
        lp.LPProblem(*_tiny(), dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="float32"):
        lp.LPSolverADMM(dtype=torch.float32)


def test_switches_that_are_not_built_raise_by_name():
    import dprox as dp
    from dprox.algo import lp
    p = lc.problem("tiny")
    solver = lp.LPSolverADMM(verbose=False).eval()
    for kw, match in ((dict(direct=True), "direct"), (dict(polish=True), "polish")):
        with pytest.raises(NotImplementedError, match=match):
            solver.solve(p, **kw)
    with pytest.raises(NotImplementedError, match="problem_scale"):
        lp.LPSolverADMM(problem_scale=p.problem_scale)
    with pytest.raises(NotImplementedError, match="optimize_params"):
        solver.optimize_params()
    with pytest.raises(NotImplementedError, match="norm_ord"):
        lp.LPSolverADMM(norm_ord=2)
    g = lc.golden()
    x = dp.Variable()
    prob = dp.Problem(g["tiny_c"] @ x, [lc._dense(*lc.csr_of("tiny", "ub")) @ x <= g["tiny_b_ub"], lc._dense(*lc.csr_of("tiny", "eq")) @ x == g["tiny_b_eq"]])
    with pytest.raises(NotImplementedError, match="optimize_params"):
        prob.solve(adapt_params=True)
    with pytest.raises(NotImplementedError, match="optimize_params"):
        prob.prob.optimize_params()


def test_pcg_tolerances_are_the_float32_logspace_values():
    from dprox.algo.lp import pcg_rtol
    ref = torch.logspace(-6, -10, 10000)
    assert ref.dtype == torch.float32
    for k in (0, 1, 9999):
        assert pcg_rtol(k) == float(ref[k]) and np.float32(pcg_rtol(k)) == ref[k].numpy()
    assert pcg_rtol(0) == float(np.float32(1e-6)) != 1e-6
    assert pcg_rtol(10000) == 1e-10 and pcg_rtol(20000) == 1e-10


def test_solver_parameters_are_the_references():
    """rho, sigma_log, alpha, gamma_c_mul and gamma_b_mul are float64 ``nn.Parameter``s, so a state dict of the reference's solver loads"""
    from dprox.algo import lp
    s = lp.LPSolverADMM(rho=0.25)
    state = {k: v.dtype for k, v in s.state_dict().items()}
    assert state == {k: torch.float64 for k in ("rho", "sigma_log", "alpha", "gamma_c_mul", "gamma_b_mul")}
    assert s.rho.item() == 0.25 and s.alpha.item() == 1.6 and abs(torch.exp(s.sigma_log).item() - 1e-6) < 1e-20
    s.load_state_dict({"rho": torch.tensor(0.5, dtype=torch.float64), "sigma_log": torch.tensor(-10.0, dtype=torch.float64),
                       "alpha": torch.tensor(1.5, dtype=torch.float64), "gamma_c_mul": torch.tensor(1.0, dtype=torch.float64),
                       "gamma_b_mul": torch.tensor(2.0, dtype=torch.float64)})
    assert s.rho.item() == 0.5 and s.gamma_b_mul.item() == 2.0


def test_the_pieces_of_a_linear_program():
    import dprox as dp
    from dprox.linop.constaints import equality, less, matmul
    x = dp.Variable()
    c, A, b = np.arange(3.0), np.eye(2, 3), np.ones(2)
    obj = c @ x
    assert isinstance(obj, matmul) and obj.A is c and obj.var is x
    assert isinstance(torch.from_numpy(c) @ x, matmul)
    le, eq = A @ x <= b, A @ x == b
    assert isinstance(le, less) and le.left.A is A and le.right is b
    assert isinstance(eq, equality) and eq.left.var is x and eq.right is b
    prob = dp.Problem(obj, [le, eq])
    assert prob.objective is obj and prob.solver.abstol == 1e-3 and prob.solver.reltol == 1e-6 and prob.solver.max_iters == 20000
    assert prob.solver.rho.item() == 1e-1
    with pytest.raises(ValueError, match="one"):
        dp.Problem(obj, [le, le])
    with pytest.raises(ValueError, match="one"):
        dp.Problem(obj, [le])
    with pytest.raises(ValueError, match="one variable"):
        dp.Problem(obj, [le, A @ dp.Variable() == b])
