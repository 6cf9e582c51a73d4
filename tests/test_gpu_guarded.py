"""-m gpu: existing parity cases, unchanged, at their smallest shapes, on exact-size, poisoned, guarded workspaces
(tests/guarded_alloc.py) on a real MI355X -- the wave64, MFMA and LDS-DMA code paths the emulator's share
(tests/test_guarded_emul.py) never takes.  Every buffer the host layer sizes from a ``*_bytes`` query is exactly that long, starts
as NaN (or as zeros where the product asks for zeros) and sits between two 64 KiB pattern bands: a kernel that reads workspace it
has not written fails the case's own comparison, one that writes past either end fails ``check()`` with the query's name.  The
last test asserts that every size query of the C ABI has been asked under the guard."""
import pytest
import torch

import guarded_alloc as ga

pytestmark = pytest.mark.gpu
DEV = "cuda"

# size queries that need not be asked under the guard, with the reason (at most 3)
ALLOW = {}
SEEN = set()


@pytest.fixture(scope="module", autouse=True)
def _hip_lib_loaded():
    from dprox import _backend as be
    assert torch.cuda.is_available()
    assert not be.host_mode()
    assert "libdpx_hip.so" in be.lib().path
    yield
    ga.write_report(ALLOW)


import deq_cases as dc  # noqa: E402
import fft_cases as fc  # noqa: E402
import minres_cases as mc  # noqa: E402
import nlm_cases as nc  # noqa: E402
import parity_cases as pc  # noqa: E402

# name -> (case, arguments after the device, keyword arguments)
RUNS = {
    # operators and direct solves
    "linops_a": (pc.case_linops, ("a",), {}),
    "linops_b": (pc.case_linops, ("b",), {}),
    "linops_c": (pc.case_linops, ("c",), {}),
    "solve_direct": (pc.case_solve_direct, (), {}),
    # ADMM and PGD on the generic and register-radix paths
    "admm_tv_small_fused": (pc.case_admm_tv_small, (True,), {}),
    "admm_tv_small_generic": (pc.case_admm_tv_small, (False,), {}),
    "pgd": (pc.case_pgd, (), {}),
    "pgd_pow2_tiny": (pc.case_pgd_pow2, (), dict(tiny=True)),
    "h768_tiny": (pc.case_h768, (), dict(tiny=True)),
    "merged_z_rhs": (pc.case_merged_z_rhs, (), {}),
    "generic_interleaved": (pc.case_generic_interleaved, (), dict(sizes=((1, 3, 45, 35), (1, 1, 24, 34), (1, 1, 1100, 24)), oracle_sizes=((1, 3, 45, 35),))),
    "tiny_shapes": (pc.case_tiny_shapes, (), {}),
    # CG and Krylov
    "cg_B4": (pc.case_cg, (4,), {}),
    "cg_branches_quick": (pc.case_cg_branches, (), dict(quick=True)),
    "cg_masked_fft_shapes": (pc.case_cg_masked_fft_shapes, (), {}),
    "cg_wave_fft_320": (pc.case_cg_wave_fft, (), dict(sizes=(320,), B=1, iters=3)),
    "ladmm_cg": (pc.case_ladmm_cg, (), {}),
    "split_cg_loop_forms": (pc.case_split_cg_loop_forms, (), {}),
    "dense_krylov": (pc.case_dense_krylov, (), {}),
    # FFDNet and convolution
    "ffdnet_odd_gray": (pc.case_ffdnet, (), dict(which=("odd", "gray"))),
    "ffdnet_f16_split_tiny": (pc.case_ffdnet_f16_split, (), dict(tiny=True)),
    "ffdnet_winograd_tiny": (pc.case_ffdnet_winograd, (), dict(tiny=True)),
    "ffdnet_split_backward_tiny": (pc.case_ffdnet_split_backward, (), dict(tiny=True)),
    "ffdnet_grads": (pc.case_ffdnet_grads, (), {}),
    "conv2d_generic": (pc.case_conv2d_generic, (), {}),
    "unet": (pc.case_unet, (), {}),
    # unrolled solver and gradients
    "unrolled_grads": (pc.case_unrolled_grads, (), {}),
    "unrolled_grads_bf16": (pc.case_unrolled_grads_bf16, (), {}),
    "unrolled_bwd_fused_vs_staged": (pc.case_unrolled_bwd_fused_vs_staged, (), {}),
    "unrolled_bwd_shortest_loops": (pc.case_unrolled_bwd_shortest_loops, (), {}),
    "linear_solve_grad": (pc.case_linear_solve_grad, (), {}),
    # applications
    "sisr": (pc.case_sisr, (), {}),
    "csmri": (pc.case_csmri, (), {}),
    "conv_doe": (pc.case_conv_doe, (), {}),
    "doe_psf_grad": (pc.case_doe_psf_grad, (), {}),
    "admm_pnp": (pc.case_admm_pnp, (), {}),
    # launch forms
    "sub_batch_chains": (pc.case_sub_batch_chains, (), dict(shapes=((3, 1, 256, 256),), iters=3, methods=("admm",), nchs=(2,), twice=False)),
    "row_parallel_kernel": (pc.case_row_parallel_kernel, (), dict(shapes=((1, 1, 256, 256),), iters=2, methods=("admm",), nterms_list=(3,), hfirst=(True, False))),
    # Anderson / DEQ, MINRES, non-local means
    "anderson_kernels": (dc.case_kernels, ((1, 3, 33, 65), 3, 0.5), {}),
    "deq_tv_small": (dc.case_tv, ("small",), {}),
    "deq_backward": (dc.case_backward, (), {}),
    "minres_step_f32": (mc.case_step, ((2, 33, 3), torch.float32), {}),
    "minres_step_f64_preconditioned": (mc.case_step, ((2, 33, 3), torch.float64), dict(prec=True)),
    "minres_linear_solve": (mc.case_linear_solve, (), {}),
    "nlm_admm_fused": (nc.case_admm, ("admm", True), {}),
    # every FFT path against float64 with flat-spectrum operators (cases A and B of tests/fft_cases.py)
    **{f"fft_{fc.sid(s)}": (fc.case_guarded, (s,), {}) for s in fc.GUARDED},
}


@pytest.mark.parametrize("name", list(RUNS))
def test_guarded(monkeypatch, name):
    fn, args, kwargs = RUNS[name]
    with ga.guarded(monkeypatch, label=name) as g:
        try:
            fn(DEV, *args, **kwargs)
            g.check()
        finally:
            SEEN.update(g.seen)
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"


def test_wgrad_c8_kernel_asks_its_own_query(monkeypatch):
    """the case sizes the kernel's workspace itself, straight from dpx_conv3x3_wgrad_c8_ws_bytes (the host layer reaches that kernel
    through dpx_ffdnet_bf16_bwd_w_ws_bytes, which contains it): no buffer of the host layer's is guarded here, the query is recorded"""
    g = ga.run(monkeypatch, "wgrad_c8_tiny", pc.case_wgrad_c8, DEV, tiny=True)
    SEEN.update(g.seen)
    assert "dpx_conv3x3_wgrad_c8_ws_bytes" in g.seen


def test_every_size_query_was_asked_under_the_guard():
    """runs last: every ``*_bytes`` / ``*_floats`` query of the binding's signature table (the ``*_bytes_bf16`` ones included) has
    been asked at least once inside a guarded run of this module (ALLOW: the exceptions, one reason each, three at the most)"""
    from dprox import _backend as be
    queries = {n for n in be.SIGNATURES if ga.is_size_query(n)}
    assert len(queries) >= 33 and len(ALLOW) <= 3 and set(ALLOW) <= queries
    missing = sorted(queries - SEEN - set(ALLOW))
    assert not missing, f"size queries never asked under the guard: {missing}"
