"""-m gpu: the TV denoiser's operator and ADMM cases on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py): the
ping-pong dual buffers of a chain of launches are exactly dpx_tv_ws_bytes long and start as NaN, so a tile that reads a neighbour's
dual the previous launch did not write, or writes past either end, fails here.

This module sorts in front of tests/test_gpu_guarded.py on purpose: that module's closing test counts every size query of the binding
(dpx_tv_ws_bytes is one now) among the queries its guarded runs have asked, so the runs here hand theirs to it."""
import pytest
import torch

import guarded_alloc as ga

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _hip_lib_loaded():
    from dprox import _backend as be
    assert torch.cuda.is_available()
    assert not be.host_mode()
    assert "libdpx_hip.so" in be.lib().path
    yield


import tv_cases as tc  # noqa: E402

RUNS = {
    "tv_fn2_chained": (tc.case_fn, ("fn2", "a", 13, 1)),
    "tv_fn3_chained": (tc.case_fn, ("fn3", "b", 13, 0)),
    "tv_blocking_three_tiles": (tc.case_blocking, (3, (1, 2, 3), "three")),
    "tv_admm_fused": (tc.case_admm, ("admm3", True)),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    import test_gpu_guarded                    # (the module pytest has collected: its SEEN is what its closing test reads)
    fn, args = RUNS[name]
    with ga.guarded(monkeypatch, label=name) as g:
        try:
            fn(DEV, *args)
            g.check()
        finally:
            test_gpu_guarded.SEEN.update(g.seen)
    assert "dpx_tv_ws_bytes" in g.seen
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"
