"""-m gpu: the compress_sensing gradient and its ADMM solve on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py): the
backward's workspace (one ticket per image, the workgroups' float64 sums of q r) is exactly dpx_cs_bwd_ws_bytes long and starts as
0xFF, so a partial the last workgroup reads but nobody wrote surfaces as NaN in glam, and a write past either end fails here.

Like tests/test_gpu_guard_tv.py this module sorts in front of tests/test_gpu_guarded.py, whose closing test counts every size query of
the binding among the queries its guarded runs have asked: the runs here hand theirs (dpx_cs_bwd_ws_bytes) to it."""
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


import cs_cases as cc  # noqa: E402

RUNS = {          # case, arguments, the size query its buffers come from (the solve has no backward: its guarded buffers are the TV prior's)
    "cs_grad_p_hsi": (cc.case_grad, ("p_hsi",), "dpx_cs_bwd_ws_bytes"),
    "cs_admm_tv3d": (cc.case_admm, ("admm_tv3d",), "dpx_tv_ws_bytes"),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    import test_gpu_guarded                    # (the module pytest has collected: its SEEN is what its closing test reads)
    fn, args, query = RUNS[name]
    with ga.guarded(monkeypatch, label=name) as g:
        try:
            fn(DEV, *args)
            g.check()
        finally:
            test_gpu_guarded.SEEN.update(g.seen)
    assert query in g.seen
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"
