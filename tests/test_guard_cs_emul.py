"""CPU-only: the compress_sensing gradient and its ADMM solve on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py) under
the SIMT emulator -- the two runs of tests/test_gpu_guard_cs.py."""
import pytest

import emul_util
import guarded_alloc as ga


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import cs_cases as cc  # noqa: E402

DEV = "cpu"

RUNS = {          # case, arguments, the size query its buffers come from (the solve has no backward: its guarded buffers are the TV prior's)
    "cs_grad_p_hsi": (cc.case_grad, ("p_hsi",), "dpx_cs_bwd_ws_bytes"),
    "cs_admm_tv3d": (cc.case_admm, ("admm_tv3d",), "dpx_tv_ws_bytes"),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    fn, args, query = RUNS[name]
    g = ga.run(monkeypatch, name, fn, DEV, *args)
    assert query in g.seen
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"
