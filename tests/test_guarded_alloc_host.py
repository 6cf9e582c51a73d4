"""CPU-only, no kernel launched: the guarded allocator of tests/guarded_alloc.py checks what it claims to check (CPU tensors; the
run that proves it catches a wrong ``*_bytes`` formula through a real kernel is in tests/test_guarded_emul.py)."""
import pytest
import torch

import guarded_alloc as ga
from dprox import _backend as be
from dprox import _ops as ops


def _arena(g):
    return g.live[-1][0]


@pytest.mark.parametrize("n", [16, 100, 513, 4096])
def test_last_payload_byte_is_inside_and_byte_n_is_the_back_guard(monkeypatch, n):
    with ga.guarded(monkeypatch) as g:
        buf = ops._bytes(n, "cpu")
        assert buf.numel() == n and buf.dtype == torch.uint8 and buf.storage_offset() == ga.G
        buf[n - 1] = 0
        buf[0] = 0
        g.check()                                            # (releases the buffer: the next one is checked alone)
        buf = ops._bytes(n, "cpu")
        _arena(g)[ga.G + n] = 0
        assert g.damage() == [(None, (), n, "back", 0, 1)]


def test_byte_before_the_payload_is_a_front_guard_hit(monkeypatch):
    with ga.guarded(monkeypatch) as g:
        ops._bytes(100, "cpu")
        _arena(g)[ga.G - 1] = 0
        assert g.damage() == [(None, (), 100, "front", ga.G - 1, 1)]


def test_check_fails_the_test_and_names_the_query(monkeypatch):
    class Lib(be.Library):
        def __init__(self):
            pass
    monkeypatch.setattr(be.Library, "query", lambda self, name, *args: 48)
    with ga.guarded(monkeypatch) as g:
        lib = Lib()
        assert lib.query("dpx_version") == 48 and g.seen == set()
        buf = ops.workspace("some tag", lib.query("dpx_spectrum_bytes", 2, 3, 4), "cpu")
        assert buf.numel() == 48 and g.seen == {"dpx_spectrum_bytes"}
        _arena(g)[ga.G + 48 + 5:ga.G + 48 + 8] = 0
        with pytest.raises(AssertionError, match=r"dpx_spectrum_bytes\(2, 3, 4\): n = 48, back guard damaged from offset 5, 3 byte"):
            g.check()
        g.check()                                            # a checked buffer is released: nothing left to report
        assert len(g.hits) == 1 and g.buffers == 1


def test_small_requests_get_the_products_16_bytes(monkeypatch):
    with ga.guarded(monkeypatch) as g:
        assert ops._bytes(3, "cpu").numel() == 16
        assert g.live[-1][1] == 16 and _arena(g).numel() == 2 * ga.G + 16


def test_fresh_payload_is_nan_in_every_float_type_and_zero_on_request(monkeypatch):
    with ga.guarded(monkeypatch) as g:
        buf = ops._bytes(64, "cpu")
        for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
            assert torch.isnan(buf.view(dtype)).all(), dtype
        assert (buf.view(torch.int32) == -1).all()
        z = ops._bytes(64, "cpu", zero=True)
        assert (z == 0).all() and (z.view(torch.float64) == 0).all()
        g.check()


def test_guards_hold_neither_zero_nor_the_poison(monkeypatch):
    with ga.guarded(monkeypatch) as g:
        ops._bytes(32, "cpu")
        a = _arena(g)
        for guard in (a[:ga.G], a[ga.G + 32:]):
            assert guard.numel() == ga.G and int(guard.min()) > 0 and int(guard.max()) < 0xFF
    assert ga.G == 64 << 10 and ga.G % 512 == 0


def test_workspace_reuses_nothing(monkeypatch):
    with ga.guarded(monkeypatch) as g:
        a = ops.workspace("t", 4096, "cpu")
        b = ops.workspace("t", 64, "cpu")
        assert a.numel() == 4096 and b.numel() == 64 and a.data_ptr() != b.data_ptr()
        assert not ops._workspaces
        g.check()


def test_the_product_allocator_is_back_after_the_context(monkeypatch):
    real = (ops._bytes, ops.workspace, be.Library.query)
    with ga.guarded(monkeypatch):
        assert ops._bytes is not real[0] and ops.workspace is not real[1] and be.Library.query is not real[2]
        ops.workspace("t", 64, "cpu")
    assert (ops._bytes, ops.workspace, be.Library.query) == real
    assert not ops._workspaces and not ops._tables
    w = ops.workspace("t", 64, "cpu")
    assert w.storage_offset() == 0 and ops._workspaces
    assert ops._bytes(8, "cpu", zero=True).tolist() == [0] * 16
    ops.clear_caches()
    with pytest.raises(ZeroDivisionError):                   # an exception inside restores them too
        with ga.guarded(monkeypatch):
            1 / 0
    assert (ops._bytes, ops.workspace, be.Library.query) == real
