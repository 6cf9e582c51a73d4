"""-m gpu: the TV denoiser's gradient on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py): the clip-state bytes are exactly
dpx_tv_codes_bytes long and the backward's workspace (tickets, sums, the hand-over buffers of a chain) exactly dpx_tv_bwd_ws_bytes, both
start as 0xFF -- a state byte the recording forward did not write reads as "clipped" on every axis, a hand-over cell the previous launch
did not write as NaN -- so a tile that reads what was never written, or writes past either end, fails here.

Like tests/test_gpu_guard_tv.py this module sorts in front of tests/test_gpu_guarded.py, whose closing test counts every size query of
the binding among the queries its guarded runs have asked: the runs here hand theirs (dpx_tv_codes_bytes, dpx_tv_bwd_ws_bytes) to it."""
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


import tv_bwd_cases as bc  # noqa: E402

RUNS = {
    "tv_bwd_fixture_chain_of_three": (bc.case_fixture, ("d", "ops")),
    "tv_bwd_fixture_two_launches": (bc.case_fixture, ("e", "denoiser")),
    "tv_bwd_spatial_dims_batch": (bc.case_extension, ((2, 3, 21, 70), (2, 3), 7)),
    "tv_bwd_blocking_three_tiles": (bc.case_blocking, (3, (1, 2, 3), "three")),
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
    assert {"dpx_tv_ws_bytes", "dpx_tv_codes_bytes", "dpx_tv_bwd_ws_bytes"} <= g.seen
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"
