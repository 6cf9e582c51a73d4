"""CPU-only: the LP kernels (csrc/dpx_lp.hip) and ``dprox.algo.lp`` under the SIMT emulator (tests/emul): every stage of an iteration
against a float64 restatement with the lane-group width forced to 1, 8 and 64, in both forms of the direction update, and the
solver against the reference's stored run.  A launch costs milliseconds here (one fiber per GPU thread), so the solver runs the one
case whose whole trajectory is a few hundred launches, ``tiny`` (its early stop included), and the first evaluation of ``odd``;
the five cases, the balance step of ``small`` among them, run in tests/test_gpu_lp.py on a real MI355X, which is the authoritative
numerics check."""
import numpy as np
import pytest
import torch

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import lp_cases as lc  # noqa: E402

DEV = "cpu"


# (odd at 64 lanes, 107 workgroups of fibers per launch, is the slowest here, about 12 s: the one combination in which a 64-lane group
# crosses a 256-thread block with several workgroups)
@pytest.mark.parametrize("lanes", [1, 8, 64])
@pytest.mark.parametrize("name", lc.STEP_CASES)
def test_lp_steps(name, lanes):
    lc.case_steps(DEV, name, lanes)


def test_lp_parity_tiny():
    lc.case_parity(DEV, "tiny")


def test_lp_objective_tiny():
    lc.case_objective(DEV, "tiny")


def test_lp_first_evaluation_of_odd():
    """one outer iteration of ``odd`` (several workgroups in every launch): its evaluation is the reference's first"""
    from dprox.algo import lp
    kw, balance = lc.settings("odd")
    solver = lp.LPSolverADMM(verbose=False, **dict(kw, max_iters=1)).eval()
    _, history, _ = solver.solve(lc.problem("odd", DEV), residual_balance=balance)
    ref = lc.golden()["odd_history"]
    bound = 8 * float(lc.golden()["odd_perm64"]) + lc.SLACK64
    for i, k in enumerate(lc.SERIES):
        assert len(history[k]) == 1 and lc.rel_l2(history[k], ref[i, :1]) <= bound, (k, history[k], ref[i, :1])


def test_lp_nan_residual_is_not_done():
    lc.case_nan_residual(DEV)


def test_lp_refused_shapes():
    lc.case_refused_shapes(DEV)


def test_lp_deterministic():
    lc.case_deterministic(DEV, "tiny", max_iters=26)
