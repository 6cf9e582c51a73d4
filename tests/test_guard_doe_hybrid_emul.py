"""CPU-only: the hybrid DOE model and the gradients to explicit arguments on exact-size, poisoned, guarded workspaces
(tests/guarded_alloc.py) under the SIMT emulator -- the runs of tests/test_gpu_guard_doe_hybrid.py."""
import pytest

import emul_util
import guarded_alloc as ga


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import doe_hybrid_cases as hc  # noqa: E402

DEV = "cpu"
RUNS = hc.GUARDED_RUNS


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    fn, args, queries = RUNS[name]
    g = ga.run(monkeypatch, name, fn, DEV, *args)
    assert set(queries) <= g.seen
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"
