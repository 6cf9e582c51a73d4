"""CPU-only, no emulator and no device: the DEQ specialization's public surface -- what it accepts, what it refuses by name, the
reference's parameter and checkpoint names, and the C entry points it stands on."""
import os
import re

import pytest
import torch

import dprox as dp
from dprox import _backend as be
from dprox.algo import deq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def host(monkeypatch):
    """solvers compile onto the CPU without a device (as under the emulator); nothing is launched"""
    monkeypatch.setattr(be, "_host_pointers", True)
    yield


def tv(method="admm", **kw):
    x = dp.Variable()
    b = torch.rand(1, 1, 8, 8)
    fns = dp.sum_squares(x - b) + dp.norm1(dp.grad(x, dim=0))
    if method != "pgd":                                        # (proximal gradient descent takes two terms)
        fns = fns + dp.norm1(dp.grad(x, dim=1))
    return dp.compile(fns, method=method, device="cpu", **kw)


def test_deq_solver_is_exported():
    assert dp.DEQSolver is deq.DEQSolver and dp.algo.DEQSolver is deq.DEQSolver
    assert dp.algo.api.SPECAILIZATIONS["deq"] is deq.DEQSolver


def test_specialize_deq_returns_a_deq_solver_on_the_solvers_device(host):
    solver = tv()
    model = dp.specialize(solver, method="deq", device="cpu")
    assert isinstance(model, dp.DEQSolver) and isinstance(model, torch.nn.Module)
    assert model.internal is solver and model.internal.device == solver.device
    assert (model.f_thres, model.b_thres) == (40, 40)
    assert [n for n, _ in model.named_parameters() if "." not in n] == []
    assert dp.specialize(tv(), device="cpu") is not None                       # the default method stays "unroll"


def test_learned_params_are_named_like_the_references_and_load(host):
    model = dp.DEQSolver(tv(), learned_params=True)
    assert sorted(n for n, _ in model.named_parameters() if "." not in n) == ["l", "r"]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["r"], sd["l"] = torch.tensor(0.7), torch.tensor(1.3)
    other = dp.DEQSolver(tv(), learned_params=True)
    other.load({"solver": sd, "rhos": 0.2, "lams": 0.01})
    assert other.r.item() == pytest.approx(0.7) and other.l.item() == pytest.approx(1.3)
    assert (other.rhos, other.lams) == (0.2, 0.01)


def test_unsupported_solvers_are_refused_by_name(host):
    with pytest.raises(NotImplementedError, match="ProximalGradientDescent"):
        dp.specialize(tv("pgd"), method="deq", device="cpu")
    with pytest.raises(NotImplementedError, match="compiled solver"):
        dp.specialize(None, method="deq")
    with pytest.raises(NotImplementedError, match="x-update"):
        dp.specialize(tv(try_diagonalize=False, try_freq_diagonalize=False), method="deq", device="cpu")
    with pytest.raises(NotImplementedError, match="rl"):
        dp.specialize(tv(), method="rl", device="cpu")


@pytest.mark.parametrize("threshold", [2, 1, 0])
def test_anderson_refuses_a_threshold_without_steps(threshold):
    with pytest.raises(ValueError, match="threshold"):
        deq.anderson(lambda z: z, torch.zeros(1, 1, 2, 2), threshold=threshold)


def test_anderson_c_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dpx.h")).read()
    for name in ("dpx_anderson_ws_bytes", "dpx_anderson_gram_row", "dpx_anderson_mix"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in be.SIGNATURES


def test_denoiser_priors_are_refused_by_name(host):
    x = dp.Variable()
    solver = dp.compile(dp.sum_squares(x - torch.rand(1, 1, 8, 8)) + dp.patch_nlm(x), method="admm", device="cpu")
    with pytest.raises(NotImplementedError, match="patch_nlm"):
        dp.specialize(solver, method="deq", device="cpu")


def test_float64_restatement_matches_the_references_float64_iteration():
    import deq_cases as dc
    dc.check_restatement()


def test_float64_restatement_of_the_backward_matches_the_references_float64_gradients():
    import deq_cases as dc
    dc.check_backward_restatement()
