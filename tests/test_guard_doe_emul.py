"""CPU-only: the DOE wave-optics model on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py) under the SIMT emulator --
the runs of tests/test_gpu_guard_doe.py."""
import pytest

import emul_util
import guarded_alloc as ga


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import doe_cases as dc  # noqa: E402

DEV = "cpu"
RUNS = dc.GUARDED_RUNS


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    fn, args, queries = RUNS[name]
    g = ga.run(monkeypatch, name, fn, DEV, *args)
    assert set(queries) <= g.seen
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"


def test_an_under_reported_workspace_is_caught(monkeypatch):
    """the self-test of the guard for this feature: with dpx_doe_ws_bytes handing out 8 bytes less, the last element of the propagated
    field lands in the arena's guard and the run is reported"""
    with ga.guarded(monkeypatch, shrink={"dpx_doe_ws_bytes": 8}, label="doe_shrunk") as g:
        try:
            dc.case_parity(DEV, 30, "pert")
        except AssertionError:
            pass                                # (the case's own comparison may fail first: the field's last element is lost)
        hits = g.damage()
    assert hits and all(h[0] == "dpx_doe_ws_bytes" and h[3] == "back" for h in hits), hits
