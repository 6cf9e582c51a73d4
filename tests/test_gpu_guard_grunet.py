"""-m gpu: one GRUNet layer and one whole-network denoise on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py): the packed
weights and the workspaces are exactly as long as their queries say and start as 0xFF, so a cell of a concatenation buffer or a gate
plane that is read but never written surfaces as NaN in the case's own comparison, and a write past either end fails here.

Like tests/test_gpu_guard_cs.py this module sorts in front of tests/test_gpu_guarded.py, whose closing test counts every size query of
the binding among the queries its guarded runs have asked: the runs here hand theirs (dpx_qrnn3d_*_bytes, dpx_grunet_*_bytes) to it."""
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


import grunet_cases as gc  # noqa: E402


def _net(device):
    gc._nets.clear()                # (a fresh module: its packed weights are allocated inside the guarded context)
    try:
        gc.case_net(device, "n_2x32x48")
    finally:
        gc._nets.clear()


RUNS = {
    "grunet_layer_up": (gc.case_layer, ("up_fwd_s3b",), ("dpx_qrnn3d_packed_bytes", "dpx_qrnn3d_layer_ws_bytes")),
    "grunet_layer_residual": (gc.case_residual_offset, (), ("dpx_qrnn3d_packed_bytes", "dpx_qrnn3d_layer_ws_bytes")),
    "grunet_net": (_net, (), ("dpx_grunet_packed_bytes", "dpx_grunet_ws_bytes")),
}


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
