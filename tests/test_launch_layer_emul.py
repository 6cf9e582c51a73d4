"""CPU-only: the launch layer (DPX_LAUNCH_LDS / lds_opt_in / launch_fail, csrc/dpx_common.h + dpx_core.hip) on the host emulator.

The emulator records every opt-in to large dynamic LDS (kernel address, current device, bytes), can refuse requests above a
limit, has a settable current device, and counts launches beyond 64 KB of LDS that held no grant (tests/emul/emul.cpp).  Each
test works on emulated devices of its own (5 .. 9): the grants are per (kernel instantiation, device) and the other emulator
tests of the same process have long been granted theirs on device 0."""
import ctypes

import pytest
import torch

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import dprox as dp  # noqa: E402
import synthetic  # noqa: E402
from dprox import _backend as be, _ops as ops  # noqa: E402
from parity_cases import tv_problem  # noqa: E402

DPX_ERR_ARG, DPX_ERR_LAUNCH = -1, -2
NO_OPT_IN = 48 * 1024


class Emul:
    def __init__(self):
        self.c = be.lib().cdll
        self.c.emul_lds_log.restype = ctypes.c_int
        self.c.emul_lds_log.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int]

    def log(self):
        cap = 4096
        k, d, b = (ctypes.c_void_p * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
        n = self.c.emul_lds_log(k, d, b, cap)
        assert n <= cap
        return [(k[i], d[i], b[i]) for i in range(n)]


@pytest.fixture
def emul():
    e = Emul()
    e.c.emul_lds_log_clear()
    unasked = e.c.emul_lds_unasked()
    yield e
    e.c.emul_lds_limit(-1)
    e.c.emul_set_device(0)
    e.c.emul_lds_log_clear()
    assert e.c.emul_lds_unasked() == unasked, "a kernel was launched with more than 64 KB of dynamic LDS and no grant on its device"


def _tv_256():
    """1 x 1 x 256 x 256 ADMM TV deconvolution: the two-kernel iteration (k_iter_rows_seq at 69 120 bytes of LDS per workgroup)"""
    _, b0, psf = synthetic.deconv_case(1, 1, 256, 256, seed=5)
    b = torch.from_numpy(b0)
    _, fns, _ = tv_problem(b, psf)
    return dp.Problem(fns), b


def _solve(prob, b):
    return prob.solve(method="admm", device="cpu", x0=b, rhos=0.1, lams=0.005, max_iter=2)


def test_one_opt_in_per_kernel_and_device(emul):
    prob, b = _tv_256()
    emul.c.emul_set_device(5)
    first = _solve(prob, b)
    asked = emul.log()
    assert asked, "the 256-wide two-kernel iteration needs more than 48 KB of LDS: it must have opted in"
    assert all(dev == 5 and nbytes > NO_OPT_IN for _, dev, nbytes in asked)
    assert len({k for k, _, _ in asked}) == len(asked), "a kernel instantiation asked twice on one device"
    for _ in range(3):                                   # N repeated solves: not one more call
        assert torch.equal(_solve(prob, b), first)
    assert emul.log() == asked

    emul.c.emul_set_device(6)                            # another device: every such kernel asks once more, there
    assert torch.equal(_solve(prob, b), first)
    again = emul.log()[len(asked):]
    assert sorted((k, nbytes) for k, _, nbytes in again) == sorted((k, nbytes) for k, _, nbytes in asked)
    assert all(dev == 6 for _, dev, _ in again)
    _solve(prob, b)
    emul.c.emul_set_device(5)                            # ... and back: nothing
    _solve(prob, b)
    assert len(emul.log()) == 2 * len(asked)


def test_refused_opt_in_is_a_launch_error_and_is_not_remembered(emul):
    prob, b = _tv_256()
    emul.c.emul_set_device(7)
    emul.c.emul_lds_limit(NO_OPT_IN)                     # every request is above it
    with pytest.raises(be.DpxError) as err:
        _solve(prob, b)
    refused = emul.log()
    assert refused, "nothing asked for large LDS"
    msg = str(err.value)
    assert f"failed ({DPX_ERR_LAUNCH})" in msg and "k_" in msg and f"{refused[-1][2]} bytes of LDS on device 7" in msg, msg
    # the mark is consumed by the entry that reported it: an entry without large LDS succeeds right behind it
    L = be.lib()
    table = torch.empty(L.query("dpx_fft_table_bytes", 16, 16), dtype=torch.uint8)
    L.call("dpx_fft_table_init", be.ptr(table), 16, 16, be.stream())
    emul.c.emul_lds_limit(-1)
    out = _solve(prob, b)                                # the failed attempt was not remembered as a grant: the kernel asks again
    assert all(call in emul.log()[len(refused):] for call in refused)
    emul.c.emul_set_device(5)
    assert torch.equal(out, _solve(prob, b))


def _conv_case(H, W, seed):
    _, b0, psf = synthetic.deconv_case(1, 1, H, W, seed=seed)
    x = torch.from_numpy(b0)
    otf = ops.make_otf(psf, 1, H, W, x.device)
    ops.fft_table(H, W, x.device)
    return x, otf


def test_refused_column_pass_leaves_the_output_untouched(emul):
    """The row pass in front of the refused column kernel needs no opt-in and does run (into the workspace); what the call guarantees is
    that the refused kernel's body does not, and that nothing behind it writes y: spectral_apply returns before its inverse row pass."""
    H, W = 700, 16                                       # size-generic column pass: k_cols_il at 700 x 80 = 56 000 bytes
    emul.c.emul_set_device(8)
    x, otf = _conv_case(H, W, seed=3)
    y = torch.full_like(x, -7.0)
    emul.c.emul_lds_log_clear()
    emul.c.emul_lds_limit(55999)
    with pytest.raises(be.DpxError) as err:
        ops.fft_conv(x, otf, out=y)
    msg = str(err.value)
    assert f"dpx_fft_conv failed ({DPX_ERR_LAUNCH})" in msg and "k_cols_il: opt-in to 56000 bytes of LDS on device 8 failed" in msg, msg
    assert bool((y == -7.0).all()), "the output of a call whose column pass could not be launched was written"
    emul.c.emul_lds_limit(56000)
    ops.fft_conv(x, otf, out=y)                          # the same call, now granted
    assert [nbytes for _, _, nbytes in emul.log()] == [56000, 56000]
    emul.c.emul_set_device(0)
    assert torch.equal(y, ops.fft_conv(x, otf))


def test_run_time_sized_kernel_asks_again_only_for_more(emul):
    emul.c.emul_set_device(9)
    small, large = _conv_case(700, 16, seed=3), _conv_case(900, 16, seed=4)
    emul.c.emul_lds_log_clear()
    ops.fft_conv(*small)
    ops.fft_conv(*large)
    ops.fft_conv(*small)
    ops.fft_conv(*large)
    asked = emul.log()
    assert [(dev, nbytes) for _, dev, nbytes in asked] == [(9, 700 * 80), (9, 900 * 80)] and asked[0][0] == asked[1][0]


def test_weight_gradients_reject_a_block_shape_without_instantiation(emul):
    """in_nc = 8, nc = 96: the first layer has 33 input channels against 96 outputs, 3 x 2 blocks of 32 -- k_wgrad_c8 has no such form"""
    L = be.lib()
    in_nc, nc, nb, B, H, W = 8, 96, 3, 1, 8, 8
    zeros = lambda n: torch.zeros(int(n), dtype=torch.uint8)
    acts = zeros(L.query("dpx_ffdnet_bf16_acts_bytes", B, in_nc, nc, nb, H, W))
    packed = zeros(L.query("dpx_ffdnet_bf16_packed_transposed_bytes", in_nc, nc, nb))
    ws = zeros(L.query("dpx_ffdnet_bf16_bwd_w_ws_bytes", B, in_nc, nc, H, W))
    gy = torch.zeros(B, in_nc, H, W)
    gx, gs = torch.full_like(gy, 3.0), torch.full((B,), 3.0)
    shapes = [(nc, 4 * in_nc + 1), (nc, nc), (4 * in_nc, nc)]
    gws = [torch.full((co, ci, 3, 3), 3.0) for co, ci in shapes]
    gbs = [torch.full((co,), 3.0) for co, _ in shapes]
    pw = (ctypes.c_void_p * nb)(*[t.data_ptr() for t in gws])
    pb = (ctypes.c_void_p * nb)(*[t.data_ptr() for t in gbs])
    with pytest.raises(be.DpxError) as err:
        L.call("dpx_ffdnet_backward_bf16_w", be.ptr(gy), be.ptr(gx), be.ptr(gs), pw, pb, be.ptr(packed), be.ptr(acts), in_nc, nc, nb, 6, B, H, W,
               be.ptr(ws), be.stream())
    msg = str(err.value)
    assert f"failed ({DPX_ERR_ARG})" in msg and "3 x 2 blocks" in msg, msg
    for t in gws + gbs + [gx, gs]:
        assert bool((t == 3.0).all()), "an output was written by a call that was rejected"
    # the same shape at the kernel's own entry point
    a = torch.zeros(B, 6, H, W, 8)
    g = torch.zeros(B, 12, H, W, 8)
    wsk = zeros(L.query("dpx_conv3x3_wgrad_c8_ws_bytes", 96, 33))
    with pytest.raises(be.DpxError) as err:
        L.call("dpx_conv3x3_wgrad_c8", be.ptr(g), be.ptr(a), be.ptr(gws[0]), be.ptr(gbs[0]), 96, 33, 12, 6, 6, None, B, H, W, be.ptr(wsk), be.stream())
    assert f"failed ({DPX_ERR_ARG})" in str(err.value)
    assert bool((gws[0] == 3.0).all())
