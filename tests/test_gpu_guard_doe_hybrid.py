"""-m gpu: the hybrid DOE model and the gradients to explicit arguments on exact-size, poisoned, guarded workspaces
(tests/guarded_alloc.py), as tests/test_gpu_guard_doe.py runs the base model: the workspace is exactly dpx_doe_ws_bytes long -- three
per-channel statistics and the per-channel partial sums of the reduction included -- and starts as 0xFF, so a statistic or a field
element that is read but was never written surfaces as NaN in the case's own comparison, and a write past either end fails here.

Like tests/test_gpu_guard_doe.py this module sorts in front of tests/test_gpu_guarded.py and hands its size queries to it."""
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


import doe_hybrid_cases as hc  # noqa: E402

RUNS = hc.GUARDED_RUNS


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    import test_gpu_guarded                    # (the module pytest has collected: its SEEN is what its closing test reads)
    fn, args, queries = RUNS[name]
    with ga.guarded(monkeypatch, label=name) as g:
        try:
            fn(DEV, *args)
            g.check()
        finally:
            test_gpu_guarded.SEEN.update(g.seen)
    assert set(queries) <= g.seen
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"
