"""CPU-only, no kernel: dpx_tv_plan / dpx_tv_ws_bytes are consistent, ops.tv_denoise / TVDenoiser refuse what they cannot run before
anything is launched, the prior is forward-only, the registry names resolve, the float64 restatement is the reference's."""
import os
import re

import pytest
import torch

import dprox as dp
from dprox import _backend as be
from dprox import _ops as ops
from dprox.algo import fused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    monkeypatch.setattr(be, "_host_pointers", False)        # (as without the emulator, should its tests have run first in this process)
    yield


@pytest.fixture
def host(monkeypatch):
    """solvers compile onto the CPU without a device (as under the emulator); nothing is launched"""
    monkeypatch.setattr(be, "_host_pointers", True)
    yield


def _plan(lib, D, axes, iters):
    import ctypes
    out = (ctypes.c_int * 6)()
    lib.call("dpx_tv_plan", *D, axes, iters, out)
    return list(out)


SHAPES = [(3, 1024, 1024), (1, 1024, 1024), (3, 33, 47), (31, 17, 19), (31, 512, 512), (4, 100, 5000), (5, 100, 100), (1, 1, 1), (2, 3, 2),
          (3, 25, 235), (64, 64, 64), (300, 7, 9), (1, 9, 7)]


@pytest.mark.parametrize("tv_steps", [0, 1, 2, 3])
def test_tv_plan_is_consistent(hip_lib, tv_steps):
    old = hip_lib.query("dpx_tune_set", b"tv_steps", tv_steps)
    assert old == 0
    try:
        blocked = 0
        for D in SHAPES:
            V = D[0] * D[1] * D[2]
            for axes in range(1, 8):
                k = bin(axes).count("1")
                for iters in (1, 2, 5, 6, 13, 100):
                    S, launches, t0, t1, t2, lds = _plan(hip_lib, D, axes, iters)
                    assert 1 <= S <= iters and launches * S >= iters > (launches - 1) * S, (D, axes, iters, S, launches)
                    assert 0 < lds <= 160 * 1024 and lds % (4 * (2 + k)) == 0
                    assert 1 <= t0 <= D[0] and 1 <= t1 <= D[1] and t2 >= 1 and (t2 <= D[2] or not axes & 4)
                    if tv_steps:
                        assert S <= tv_steps and (tv_steps != 1 or S == 1)
                    elif iters >= 5 and (D[0] <= 4 or not axes & 1):
                        assert S > 1, ("gray / RGB volumes and per-plane axis sets take the blocked path", D, axes)
                    blocked += S > 1
                    for N in (1, 3):
                        ws = hip_lib.query("dpx_tv_ws_bytes", N, *D, axes, iters)
                        if launches == 1:
                            assert ws == 0
                        else:
                            assert 2 * k * N * V * 4 <= ws < 2 * k * N * V * 4 + 256
        assert (blocked > 0) == (tv_steps != 1)
    finally:
        hip_lib.call("dpx_tune_set", b"tv_steps", 0)


def test_tv_plan_refuses_bad_arguments(hip_lib):
    import ctypes
    out = (ctypes.c_int * 6)()
    for args in ((0, 8, 8, 3, 5), (3, 8, 8, 0, 5), (3, 8, 8, 8, 5), (3, 8, 8, 3, 0)):
        with pytest.raises(be.DpxError, match="dpx_tv_plan"):
            hip_lib.call("dpx_tv_plan", *args, out)
        assert hip_lib.query("dpx_tv_ws_bytes", 1, *args) == 0


def test_tv_c_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dpx.h")).read()
    for name in ("dpx_tv_ws_bytes", "dpx_tv_plan", "dpx_tv_denoise"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in be.SIGNATURES


@pytest.mark.parametrize("axes", [(), (0, 1), (1, 1), (4,), (1.5, 2), 3, (True, 2)])
def test_tv_refuses_axis_sets(no_launch, axes):
    with pytest.raises(be.DpxError, match="axes"):
        ops.tv_denoise(torch.rand(1, 3, 8, 8), 0.1, 5, axes)
    with pytest.raises(be.DpxError, match="axes"):
        dp.TVDenoiser(5, dims=axes)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.complex64])
def test_tv_refuses_dtypes(no_launch, dtype):
    with pytest.raises(be.DpxError, match="float32"):
        ops.tv_denoise(torch.rand(1, 3, 8, 8).to(dtype), 0.1)


def test_tv_refuses_host_tensors_shapes_iters_and_negative_lam(no_launch):
    with pytest.raises(be.DpxError, match="HIP"):
        ops.tv_denoise(torch.rand(1, 3, 8, 8), 0.1)
    with pytest.raises(be.DpxError, match="NCHW"):
        ops.tv_denoise(torch.rand(3, 8, 8), 0.1)
    with pytest.raises(be.DpxError, match="empty"):
        ops.tv_denoise(torch.rand(1, 3, 0, 8), 0.1)
    for iters in (0, -1, 2.5):
        with pytest.raises(be.DpxError, match="iters"):
            ops.tv_denoise(torch.rand(1, 3, 8, 8), 0.1, iters)
    for lam in (-0.1, torch.tensor(-0.1), torch.tensor([0.1, -1e-3])):
        with pytest.raises(be.DpxError, match="lam must be >= 0"):
            ops.tv_denoise(torch.rand(2, 3, 8, 8), lam)


def test_tv_is_forward_only(no_launch):
    v = torch.rand(1, 3, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward-only"):
        ops.tv_denoise(v, 0.1)
    with pytest.raises(NotImplementedError, match="forward-only"):
        dp.TVDenoiser().denoise(v, torch.tensor(0.1))
    with pytest.raises(NotImplementedError, match="forward-only"):
        dp.deep_prior(dp.Variable(), denoiser=dp.TVDenoiser()).prox(v, torch.tensor(0.1))
    with pytest.raises(NotImplementedError, match="forward-only"):
        ops.tv_denoise(torch.rand(1, 3, 8, 8), torch.tensor(0.1, requires_grad=True))


def test_tv_denoiser_api_and_registry_names(tmp_path, monkeypatch):
    from dprox.proxfn.pnp import prior
    monkeypatch.setattr(prior, "CACHE_DIR", str(tmp_path))          # an empty cache: no file on disk is involved
    d2, d3 = prior.get_denoiser("tv"), prior.get_denoiser("tv3d")
    assert type(d2) is dp.TVDenoiser and (d2.iter_num, d2.use_3dtv, d2.dims) == (5, False, (1, 2))
    assert type(d3) is dp.TVDenoiser and (d3.iter_num, d3.use_3dtv, d3.dims) == (5, True, (1, 2, 3))
    assert dp.proxfn.TVDenoiser is dp.TVDenoiser and dp.proxfn.pnp.TVDenoiser is dp.TVDenoiser
    assert dp.TVDenoiser(7, dims=(2, 3)).dims == (2, 3) and dp.TVDenoiser(7, True, dims=(3,)).dims == (3,)
    assert isinstance(dp.deep_prior(dp.Variable(), denoiser="tv").denoiser, dp.TVDenoiser)
    assert not list(dp.TVDenoiser().parameters())
    with pytest.raises(ValueError, match="tv3d"):
        prior.get_denoiser("no_such_denoiser")


def test_fused_plan_takes_the_tv_prior_as_external():
    x = dp.Variable()
    assert fused._psi_prox_code(dp.deep_prior(x, denoiser=dp.TVDenoiser())) == be.PROX_EXTERNAL
    assert fused._psi_prox_code(dp.deep_prior(x, denoiser=dp.TVDenoiser(), clamp=True)) is None
    assert fused._psi_prox_code(dp.deep_prior(x, denoiser=dp.TVDenoiser(), x8=True)) is None
    assert fused._psi_prox_code(dp.deep_prior(x, denoiser=dp.TVDenoiser(), unroll_step=2)) is None


def test_plan_fingerprint_distinguishes_two_tv_denoisers(host):
    x = dp.Variable()
    b = torch.rand(1, 3, 8, 8)
    prior = dp.deep_prior(x, denoiser=dp.TVDenoiser(5))
    s = dp.compile(dp.sum_squares(x - b) + prior, method="admm", device="cpu")
    f0 = fused.plan_fingerprint(s)
    assert fused.plan_fingerprint(s) == f0
    prior.denoiser = dp.TVDenoiser(5)                # an equal denoiser, another object
    f1 = fused.plan_fingerprint(s)
    assert f1 != f0
    prior.denoiser = dp.TVDenoiser(5, True)
    assert fused.plan_fingerprint(s) not in (f0, f1)


def test_deq_refuses_the_tv_prior_by_name(host):
    x = dp.Variable()
    solver = dp.compile(dp.sum_squares(x - torch.rand(1, 1, 8, 8)) + dp.deep_prior(x, denoiser="tv"), method="admm", device="cpu")
    with pytest.raises(NotImplementedError, match="deep_prior"):
        dp.specialize(solver, method="deq", device="cpu")


def test_float64_restatement_matches_the_references_float64_outputs():
    import tv_cases as tc
    tc.check_restatement()
