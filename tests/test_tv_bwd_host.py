"""CPU-only, no kernel: the TV gradient is opt-in (the default stays forward-only through every entry point), dpx_tv_codes_bytes /
dpx_tv_bwd_ws_bytes / dpx_tv_bwd_plan are consistent with each other and with the forward's plan, argument errors are refused before any
launch, the new symbols are declared and bound, the float64 torch restatement the gradient cases lean on is the reference's."""
import ctypes
import os
import re

import pytest
import torch

import dprox as dp
from dprox import _backend as be
from dprox import _ops as ops
from dprox.algo import fused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpx_tv_codes_bytes", "dpx_tv_denoise_rec", "dpx_tv_bwd_ws_bytes", "dpx_tv_bwd_plan", "dpx_tv_backward")


@pytest.fixture(scope="module")
def hip_lib():
    if not os.path.exists(be.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return be.Library(be.LIB_PATH)


class _NoLaunch:
    """a library stand-in that fails the test if any entry point is called"""

    def call(self, name, *args):
        raise AssertionError(f"{name} was launched")

    query = call


@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(be, "lib", lambda: _NoLaunch())
    monkeypatch.setattr(be, "_host_pointers", False)
    yield


def _plan(lib, name, D, axes, iters):
    out = (ctypes.c_int * 6)()
    lib.call(name, *D, axes, iters, out)
    return list(out)


def test_tv_bwd_c_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dpx.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in be.SIGNATURES


def test_default_is_still_forward_only_through_every_entry_point(no_launch):
    v = torch.rand(1, 3, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward-only"):
        ops.tv_denoise(v, 0.1)
    with pytest.raises(NotImplementedError, match="forward-only"):
        ops.tv_denoise(v, 0.1, differentiable=False)
    with pytest.raises(NotImplementedError, match="forward-only"):
        dp.TVDenoiser().denoise(v, torch.tensor(0.1))
    with pytest.raises(NotImplementedError, match="forward-only"):
        dp.deep_prior(dp.Variable(), denoiser=dp.TVDenoiser()).prox(v, torch.tensor(0.1))
    with pytest.raises(NotImplementedError, match="forward-only"):
        ops.tv_denoise(torch.rand(1, 3, 8, 8), torch.tensor(0.1, requires_grad=True))
    assert dp.TVDenoiser().differentiable is False and dp.TVDenoiser(differentiable=True).differentiable is True
    assert dp.TVDenoiser(7, True, differentiable=True).dims == (1, 2, 3)


def test_differentiable_call_refuses_bad_arguments_before_any_launch(no_launch):
    v = torch.rand(1, 3, 8, 8, requires_grad=True)
    with pytest.raises(be.DpxError, match="HIP"):
        ops.tv_denoise(v, 0.1, differentiable=True)                      # (a host tensor without the emulator)
    with pytest.raises(be.DpxError, match="axes"):
        ops.tv_denoise(v, 0.1, 5, (0, 1), differentiable=True)
    with pytest.raises(be.DpxError, match="iters"):
        ops.tv_denoise(v, 0.1, 0, differentiable=True)
    with pytest.raises(be.DpxError, match="lam must be >= 0"):
        ops.tv_denoise(v, torch.tensor(-0.1, requires_grad=True), differentiable=True)
    with pytest.raises(be.DpxError, match="float32"):
        ops.tv_denoise(v.double(), 0.1, differentiable=True)


SHAPES = [(3, 1024, 1024), (3, 33, 47), (31, 40, 40), (31, 512, 512), (3, 21, 70), (1, 1, 1), (2, 3, 2), (1, 9, 7), (300, 7, 9)]


@pytest.mark.parametrize("tv_steps", [0, 1, 2])
def test_tv_bwd_sizes_and_plan_are_consistent(hip_lib, tv_steps):
    assert hip_lib.query("dpx_tune_set", b"tv_steps", tv_steps) == 0
    try:
        for D in SHAPES:
            V = D[0] * D[1] * D[2]
            for axes in range(1, 8):
                k = bin(axes).count("1")
                for iters in (1, 2, 5, 7, 13):
                    fwd = _plan(hip_lib, "dpx_tv_plan", D, axes, iters)
                    S, launches, t0, t1, t2, lds = _plan(hip_lib, "dpx_tv_bwd_plan", D, axes, iters)
                    assert [S, launches, t0, t1, t2] == fwd[:5], "the backward runs on the forward's tiles"
                    assert lds == max(fwd[5], 256) and lds <= 160 * 1024
                    tiles = -(-D[0] // t0) * -(-D[1] // t1) * -(-D[2] // t2)
                    for N in (1, 3):
                        assert hip_lib.query("dpx_tv_codes_bytes", N, *D, axes, iters) == (iters - 1) * N * V
                        ws = hip_lib.query("dpx_tv_bwd_ws_bytes", N, *D, axes, iters)
                        if iters == 1:
                            assert ws == 0
                            continue
                        head = 4 * N + 8 * N + 8 * N * tiles                  # tickets, running sums, one sum per workgroup
                        chain = 2 * (1 + k) * N * V * 4 if launches > 1 else 0     # two p and two x k q hand-over buffers
                        assert head + chain <= ws <= head + chain + 3 * 256 and ws % 4 == 0, (D, axes, iters, N, ws, head, chain)
    finally:
        hip_lib.call("dpx_tune_set", b"tv_steps", 0)


def test_tv_bwd_queries_refuse_bad_arguments(hip_lib):
    out = (ctypes.c_int * 6)()
    for args in ((0, 8, 8, 3, 5), (3, 8, 8, 0, 5), (3, 8, 8, 8, 5), (3, 8, 8, 3, 0)):
        with pytest.raises(be.DpxError, match="dpx_tv_bwd_plan"):
            hip_lib.call("dpx_tv_bwd_plan", *args, out)
        assert hip_lib.query("dpx_tv_bwd_ws_bytes", 1, *args) == 0
        assert hip_lib.query("dpx_tv_codes_bytes", 1, *args) == 0
    with pytest.raises(be.DpxError, match="null"):
        hip_lib.call("dpx_tv_bwd_plan", 3, 8, 8, 3, 5, None)


def test_tv_bwd_entry_points_refuse_null_pointers_before_any_launch(hip_lib):
    """host addresses never dereferenced: every call below must fail on its argument checks"""
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)
    for name, args, msg in (("dpx_tv_denoise_rec", (None, a, a, a, 1, 3, 8, 8, 3, 5, None, None), "null"),
                            ("dpx_tv_denoise_rec", (a, a + 4, a, None, 1, 3, 8, 8, 3, 5, None, None), "null"),
                            ("dpx_tv_denoise_rec", (a, a, a, a, 1, 3, 8, 8, 3, 5, None, None), "in-place"),
                            ("dpx_tv_backward", (None, a, a, None, 1, 3, 8, 8, 3, 5, None, None), "null"),
                            ("dpx_tv_backward", (a, None, a + 4, None, 1, 3, 8, 8, 3, 5, None, None), "null"),
                            ("dpx_tv_backward", (a, a, a, None, 1, 3, 8, 8, 3, 5, None, None), "in-place"),
                            ("dpx_tv_backward", (a, a, a + 4, a, 1, 3, 8, 8, 3, 5, None, None), "workspace"),
                            ("dpx_tv_backward", (a, a, a + 4, None, 1, 3, 8, 8, 9, 5, None, None), "axes"),
                            ("dpx_tv_backward", (a, a, a + 4, None, 0, 3, 8, 8, 3, 5, None, None), "shape")):
        with pytest.raises(be.DpxError, match=msg):
            hip_lib.call(name, *args)


def test_registry_names_of_the_differentiable_form(tmp_path, monkeypatch):
    from dprox.proxfn.pnp import prior
    monkeypatch.setattr(prior, "CACHE_DIR", str(tmp_path))
    d2, d3 = prior.get_denoiser("tv_diff"), prior.get_denoiser("tv3d_diff")
    assert type(d2) is dp.TVDenoiser and (d2.iter_num, d2.dims, d2.differentiable) == (5, (1, 2), True)
    assert type(d3) is dp.TVDenoiser and (d3.iter_num, d3.dims, d3.differentiable) == (5, (1, 2, 3), True)
    assert prior.get_denoiser("tv").differentiable is False and prior.get_denoiser("tv3d").differentiable is False


def test_fused_plan_knows_a_differentiable_tv_prior():
    x = dp.Variable()
    plain, diff = dp.deep_prior(x, denoiser=dp.TVDenoiser()), dp.deep_prior(x, denoiser=dp.TVDenoiser(differentiable=True))
    assert fused._psi_prox_code(diff) == be.PROX_EXTERNAL
    assert fused.differentiable_tv_priors([plain]) == [] and fused.differentiable_tv_priors([plain, diff]) == [diff]


def test_deq_still_refuses_the_differentiable_tv_prior(monkeypatch):
    monkeypatch.setattr(be, "_host_pointers", True)
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=dp.TVDenoiser(differentiable=True))
    solver = dp.compile(dp.sum_squares(x - torch.rand(1, 1, 8, 8)) + prior, method="admm", device="cpu")
    with pytest.raises(NotImplementedError, match="deep_prior"):
        dp.specialize(solver, method="deq", device="cpu")


def test_float64_torch_restatement_matches_the_references_float64_autograd():
    import tv_bwd_cases as bc
    bc.check_restatement()
