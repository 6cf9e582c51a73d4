"""CPU-only, no kernel: compress_sensing is exported, ADMM routes it to its own x-update, the C symbols are declared and bound,
ops.cs_xupdate refuses what it cannot run before anything is launched, the float64 restatement is the reference's."""
import os
import re

import pytest
import torch

import dprox as dp
from dprox import _backend as be
from dprox import _ops as ops
from dprox.algo.splitting import ADMM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoLaunch:
    """a library stand-in that fails the test if any entry point is called"""

    def call(self, name, *args):
        raise AssertionError(f"{name} was launched")

    query = call


@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(be, "lib", lambda: _NoLaunch())
    monkeypatch.setattr(be, "_host_pointers", False)        # (as without the emulator, should its tests have run first in this process)
    yield


@pytest.fixture
def host(monkeypatch):
    """solvers compile onto the CPU without a device (as under the emulator); nothing is launched"""
    monkeypatch.setattr(be, "_host_pointers", True)
    yield


def test_cs_exports():
    from dprox.proxfn.fast.cs import compress_sensing
    assert dp.compress_sensing is compress_sensing and dp.proxfn.compress_sensing is compress_sensing
    assert dp.proxfn.fast.compress_sensing is compress_sensing
    assert issubclass(compress_sensing, dp.proxfn.ext_sum_squares)


def test_admm_routes_the_term_to_its_own_x_update(host):
    x = dp.Variable()
    mask, y = torch.rand(1, 4, 6, 5), torch.rand(1, 1, 6, 5)
    term, prior, nn = dp.compress_sensing(x, mask, y), dp.deep_prior(x, denoiser=dp.TVDenoiser(5, True)), dp.nonneg(x)
    psi, omega = ADMM.partition([term, prior, nn])
    assert len(omega) == 1 and omega[0] is term and [f is g for f, g in zip(psi, (prior, nn))] == [True, True]
    s = dp.compile(term + prior + nn, method="admm", device="cpu")
    assert s.least_square is term
    # a Psi term that is not on x itself: the term is one of least_squares' quadratic terms, not the solver
    s = dp.compile(dp.compress_sensing(x, mask, y) + dp.norm1(dp.grad(x, dim=1)), method="admm", device="cpu")
    assert isinstance(s.least_square, dp.proxfn.least_squares)


def test_cs_c_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dpx.h")).read()
    for name in ("dpx_cs_xupdate", "dpx_cs_bwd_ws_bytes", "dpx_cs_backward"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in be.SIGNATURES
    assert len(be.SIGNATURES["dpx_cs_xupdate"][1]) == 14 and len(be.SIGNATURES["dpx_cs_backward"][1]) == 18


V, Y, M = torch.rand(2, 3, 4, 5), torch.rand(2, 1, 4, 5), torch.rand(1, 3, 4, 5)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.complex64])
def test_cs_refuses_dtypes(no_launch, dtype):
    for bs, y, mask in (([V.to(dtype)], Y, M), ([V, V.to(dtype)], Y, M), ([V], Y.to(dtype), M), ([V], Y, M.to(dtype))):
        with pytest.raises(be.DpxError, match="float32"):
            ops.cs_xupdate(bs, y, mask, 0.1, len(bs))
    with pytest.raises(be.DpxError, match="float32"):
        dp.compress_sensing(dp.Variable(), M, Y)._prox(V.to(dtype), 0.1)


@pytest.mark.parametrize("mask", [torch.rand(3, 3, 4, 5), torch.rand(1, 2, 4, 5), torch.rand(4, 5), torch.rand(1, 3, 5, 4), torch.rand(1, 1, 3, 4, 5)])
def test_cs_refuses_masks_that_do_not_broadcast(no_launch, mask):
    with pytest.raises(be.DpxError, match="mask .* does not broadcast"):
        ops.cs_xupdate([V], Y, mask, 0.1, 1)


@pytest.mark.parametrize("y", [torch.rand(2, 3, 4, 5), torch.rand(3, 1, 4, 5), torch.rand(3, 4, 5), torch.rand(5, 4), torch.rand(5)])
def test_cs_refuses_measurements_that_do_not_broadcast(no_launch, y):
    with pytest.raises(be.DpxError, match="y .* does not broadcast"):
        ops.cs_xupdate([V], y, M, 0.1, 1)


def test_cs_refuses_host_lam_that_is_not_positive_no_inputs_and_bad_counts(no_launch):
    for lam in (0.0, -0.1, torch.tensor(0.0), torch.tensor([0.1, -1e-3])):
        with pytest.raises(be.DpxError, match="lam must be > 0"):
            ops.cs_xupdate([V], Y, M, lam, 1)
    with pytest.raises(be.DpxError, match="nb = 0"):
        ops.cs_xupdate([], Y, M, 0.1, 1)
    with pytest.raises(be.DpxError, match="nb = 0"):
        dp.compress_sensing(dp.Variable(), M, Y).solve([], 0.1)
    for num_psi in (0, -1, 1.5, True):
        with pytest.raises(be.DpxError, match="num_psi"):
            ops.cs_xupdate([V], Y, M, 0.1, num_psi)
    with pytest.raises(be.DpxError, match="shapes"):
        ops.cs_xupdate([V, V[:1]], Y, M, 0.1, 2)
    with pytest.raises(be.DpxError, match="NCHW"):
        ops.cs_xupdate([V[0]], Y, M, 0.1, 1)
    with pytest.raises(be.DpxError, match="HIP"):
        ops.cs_xupdate([V], Y, M, 0.1, 1)


def test_float64_restatement_matches_the_references_float64_outputs():
    import cs_cases as cc
    cc.check_restatement()
