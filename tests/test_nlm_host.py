"""CPU-only, no emulator and no device: ops.nlm / patch_nlm refuse what they cannot run before anything is launched, and the prior is
forward-only (NotImplementedError where autograd would need its gradient)."""
import pytest
import torch

import dprox as dp
from dprox import _backend as be
from dprox import _ops as ops


class _NoLaunch:
    """a library stand-in that fails the test if any entry point is called"""

    def call(self, name, *args):
        raise AssertionError(f"{name} was launched")

    query = call


@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(be, "lib", lambda: _NoLaunch())
    monkeypatch.setattr(be, "_host_pointers", False)        # (as without the emulator, should its tests have run first in this process)
    yield


@pytest.mark.parametrize("shape", [(1, 2, 8, 8), (1, 4, 8, 8), (2, 0, 8, 8)])
def test_nlm_refuses_channel_counts(no_launch, shape):
    with pytest.raises(be.DpxError, match="channels"):
        ops.nlm(torch.rand(*shape), 0.1)


@pytest.mark.parametrize("search, patch", [(10, 5), (11, 4), (1, 1), (23, 5), (11, 11), (11, -1), (11, 0), (2.5, 5)])
def test_nlm_refuses_windows(no_launch, search, patch):
    with pytest.raises(be.DpxError, match="search window|patch"):
        ops.nlm(torch.rand(1, 3, 8, 8), 0.1, search, patch)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.complex64])
def test_nlm_refuses_dtypes(no_launch, dtype):
    with pytest.raises(be.DpxError, match="float32"):
        ops.nlm(torch.rand(1, 3, 8, 8).to(dtype), 0.1)


def test_nlm_refuses_host_tensors(no_launch):
    with pytest.raises(be.DpxError, match="HIP"):
        ops.nlm(torch.rand(1, 3, 8, 8), 0.1)


def test_nlm_refuses_non_images(no_launch):
    with pytest.raises(be.DpxError, match="NCHW"):
        ops.nlm(torch.rand(3, 8, 8), 0.1)


def test_patch_nlm_is_forward_only(no_launch):
    x = dp.Variable()
    fn = dp.patch_nlm(x)
    v = torch.rand(1, 3, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward-only.*NaN"):
        fn.prox(v, torch.tensor(0.01))
    lam = torch.tensor(0.01, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward-only"):
        fn._prox(torch.rand(1, 3, 8, 8), lam)


def test_patch_nlm_api():
    x = dp.Variable()
    fn = dp.patch_nlm(x)
    assert (fn.search_window_size, fn.patch_size) == (11, 5)
    assert dp.proxfn.patch_nlm is dp.patch_nlm
    fn2 = 0.5 * dp.patch_nlm(x, search_window_size=7, patch_size=3)
    assert (fn2.alpha, fn2.search_window_size, fn2.patch_size) == (0.5, 7, 3)
