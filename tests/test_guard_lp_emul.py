"""CPU-only: the LP solver on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py) under the SIMT emulator: ``tiny``
whole, ``longrow`` cut short after its first evaluation, at 2 of its 18 outer iterations: a launch of it costs 20 ms here and the
whole run is 1700 of them, 36 s.  The GPU module (tests/test_gpu_guard_lp.py) runs both whole."""
import pytest

import emul_util
import guarded_alloc as ga


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import lp_cases as lc  # noqa: E402

DEV = "cpu"

RUNS = {
    "lp_tiny": (lc.case_guarded, ("tiny",), {}),
    "lp_longrow_first_evaluation": (lc.case_guarded, ("longrow",), dict(max_iters=2)),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    fn, args, kwargs = RUNS[name]
    g = ga.run(monkeypatch, name, fn, DEV, *args, **kwargs)
    assert {"dpx_lp_state_bytes", "dpx_lp_ws_bytes"} <= g.seen
    assert g.buffers >= 2, "the case allocated no query-sized buffer: nothing was guarded"
