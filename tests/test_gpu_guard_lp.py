"""-m gpu: the LP solver on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py): the state block and the reductions'
workspace are exactly dpx_lp_state_bytes / dpx_lp_ws_bytes long and sit between pattern bands, so a reduction that writes a partial
past its share, or a control word past the block, fails here.

This module sorts in front of tests/test_gpu_guarded.py on purpose: that module's closing test counts every size query of the binding
(dpx_lp_state_bytes and dpx_lp_ws_bytes are two now) among the queries its guarded runs have asked, so the runs here hand theirs to it."""
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


import lp_cases as lc  # noqa: E402

RUNS = {
    "lp_tiny": (lc.case_guarded, ("tiny",)),
    "lp_longrow": (lc.case_guarded, ("longrow",)),
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
    assert {"dpx_lp_state_bytes", "dpx_lp_ws_bytes"} <= g.seen
    assert g.buffers >= 2, "the case allocated no query-sized buffer: nothing was guarded"
