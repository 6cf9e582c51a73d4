"""CPU-only: existing parity cases, unchanged, on exact-size, poisoned, guarded workspaces (tests/guarded_alloc.py) under the SIMT
emulator.  A case's own comparisons turn a read of unwritten workspace into a NaN failure; ``check()`` fails on a write past
either end of a buffer sized by a ``*_bytes`` query.  The emulator's share is the cases that take under about 30 s here; the
GPU module (tests/test_gpu_guarded.py) runs the wave64 / MFMA / LDS-DMA code paths and asserts the coverage of the queries."""
import pytest

import emul_util
import guarded_alloc as ga


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield
    ga.write_report()


import deq_cases as dc  # noqa: E402
import fft_cases as fc  # noqa: E402
import minres_cases as mc  # noqa: E402
import nlm_cases as nc  # noqa: E402
import parity_cases as pc  # noqa: E402
import torch  # noqa: E402

DEV = "cpu"

RUNS = {
    "linops_a": (pc.case_linops, ("a",), {}),
    "solve_direct": (pc.case_solve_direct, (), {}),
    "pgd": (pc.case_pgd, (), {}),
    "pgd_pow2_tiny": (pc.case_pgd_pow2, (), dict(tiny=True)),
    "tiny_shapes": (pc.case_tiny_shapes, (), {}),
    "generic_interleaved": (pc.case_generic_interleaved, (), dict(sizes=((1, 3, 45, 35), (1, 1, 24, 34)), oracle_sizes=((1, 3, 45, 35),))),
    "admm_tv_small_fused": (pc.case_admm_tv_small, (True,), {}),
    "admm_tv_small_generic": (pc.case_admm_tv_small, (False,), {}),
    "admm_tv_config1": (pc.case_admm_tv_config1, (), {}),
    "merged_z_rhs": (pc.case_merged_z_rhs, (), {}),
    "cg_B4": (pc.case_cg, (4,), {}),
    "cg_masked_fft_shapes": (pc.case_cg_masked_fft_shapes, (), {}),
    "dense_krylov": (pc.case_dense_krylov, (), {}),
    "split_cg_loop_forms": (pc.case_split_cg_loop_forms, (), dict(B=1, H=32, W=32, iters=3)),
    "ffdnet_f16_split_tiny": (pc.case_ffdnet_f16_split, (), dict(tiny=True)),
    "ffdnet_split_backward_tiny": (pc.case_ffdnet_split_backward, (), dict(tiny=True)),
    "conv2d_generic": (pc.case_conv2d_generic, (), {}),
    "unrolled_grads": (pc.case_unrolled_grads, (), {}),
    "unrolled_grads_bf16": (pc.case_unrolled_grads_bf16, (), {}),
    "unrolled_bwd_shortest_loops": (pc.case_unrolled_bwd_shortest_loops, (), {}),
    "unrolled_bwd_bf16_history": (pc.case_unrolled_bwd_fused_vs_staged, (), dict(K=2, term_sets=("nn+l1",), dtypes=("bf16",),
                                                                                  modes=[m for m in pc.UNROLL_BWD_MODES if m[0] in ("default", "staged")])),
    "linear_solve_grad": (pc.case_linear_solve_grad, (), {}),
    "conv_doe": (pc.case_conv_doe, (), {}),
    "doe_psf_grad": (pc.case_doe_psf_grad, (), {}),
    "sisr_ops": (pc.case_sisr, (), dict(solve=False)),
    "csmri_ops": (pc.case_csmri, (), dict(solve=False)),
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
    g = ga.run(monkeypatch, name, fn, DEV, *args, **kwargs)
    assert g.buffers > 0, "the case allocated no query-sized buffer: nothing was guarded"


def _pow2_conv(device):
    """one forward FFT convolution on a 256 x 256 plane: the power-of-two column pass is out of place and fills both halves of the
    spectrum workspace"""
    import dprox as dp
    import synthetic
    x = torch.rand(1, 1, 256, 256, device=device)
    dp.conv(dp.Variable(), synthetic.point_spread_function(5, 1.0)).to(device).forward(x)


@pytest.mark.parametrize("query, case", [("dpx_denominator_bytes", pc.case_solve_direct), ("dpx_spectrum_bytes", _pow2_conv)])
def test_an_under_reported_bytes_formula_is_caught(monkeypatch, query, case):
    """the harness's own proof: with the payload of every buffer sized by one query 64 bytes shorter than the query says (as if its
    formula under-reported by 64 bytes), the kernels' accesses of those last bytes land in the arena's own back guard, from its
    first byte on, and check() names the query.

    case_solve_direct is paired with dpx_denominator_bytes, not with dpx_spectrum_bytes: the spectrum workspace is two half-spectrum
    buffers, and on planes off the power-of-two path (the fixture's 24 x 32) nothing touches the second one (measured: written
    extent 18432 of 36864 bytes), so a spectrum workspace 64 bytes short is never overrun there.  dpx_spectrum_bytes is shrunk under
    a convolution on a 256 x 256 plane, whose out-of-place column pass writes the second buffer to its end."""
    with ga.guarded(monkeypatch, shrink={query: 64}, label=f"shrunken {query}") as g:
        try:
            case(DEV)
        except AssertionError:
            pass                                             # (what the kernels compute from a truncated table is not the point)
        with pytest.raises(AssertionError, match=query + r"\(\d+, \d+, \d+\): n = \d+, back guard damaged from offset 0, "):
            g.check()
    assert g.hits and all(h[0] == query and h[3] == "back" for h in g.hits), g.hits
