"""CPU-only: the unchanged HIP kernel sources compiled for the host by the SIMT emulator (tests/emul)
run the same parity cases as the GPU tests (small fixtures only).  Catches indexing / barrier / layout
bugs without a GPU; the authoritative numerics check is tests/test_gpu_parity.py on a real MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import parity_cases as pc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_linops(tag):
    pc.case_linops(DEV, tag)


def test_prox():
    pc.case_prox(DEV)


def test_solve_direct():
    pc.case_solve_direct(DEV)


def test_admm_tv_small_fused():
    pc.case_admm_tv_small(DEV, True)


def test_admm_tv_config1_pow2_path():
    pc.case_admm_tv_config1(DEV)          # 256x256: register-radix power-of-two kernels


def test_admm_tv_misc():
    pc.case_admm_tv_misc(DEV)


def test_pgd():
    pc.case_pgd(DEV)


def test_column_length_768():
    pc.case_h768(DEV, tiny=True)


def test_768_wide_rows_on_the_two_kernel_iteration():
    pc.case_w768_two_kernel(DEV, B=1, methods=("admm",))


def test_merged_z_rhs():
    pc.case_merged_z_rhs(DEV)


def test_generic_interleaved():
    pc.case_generic_interleaved(DEV, sizes=((1, 3, 45, 35), (2, 1, 30, 44), (1, 1, 52, 26), (1, 1, 63, 28), (1, 1, 24, 34), (1, 1, 1100, 24)),
                                oracle_sizes=((1, 3, 45, 35),))


def test_other_plane_sizes():
    pc.case_other_plane_sizes(DEV, sizes=((384, 256), (256, 768)), channels=1)


def test_hqs_two_kernel():
    pc.case_hqs_pow2(DEV)


def test_fresh_state_shortcut_matches_the_general_seed():
    pc.case_fresh_state(DEV)


def test_solve_returns_x_alone_from_an_x_only_last_pass():
    pc.case_solve_x_only(DEV, iters=3, configs=(("admm", 0), ("admm", 30), ("hqs", 0)))


def test_sub_batch_chains_are_bit_identical_to_one_chain():
    pc.case_sub_batch_chains(DEV, shapes=((3, 1, 256, 256),), iters=3, methods=("admm",), nchs=(2,), twice=False)      # (a 1- and a 2-image chain)


def test_hqs_no_dual_row_kernel():
    pc.case_hqs_nodual_kernel(DEV, iters=3, nterms_list=(2, 4))


def test_admm_vxu_two_kernel():
    pc.case_vxu_two_kernel(DEV, iters=3, nterms_list=(3,))


def test_pgd_streaming_row_kernel():
    pc.case_pgd_streaming_rows(DEV)


def test_pgd_pow2_fused():
    pc.case_pgd_pow2(DEV, tiny=True)


def test_known_answers():
    pc.case_known_answers(DEV)


@pytest.mark.parametrize("B", [1, 4])
def test_cg(B):
    pc.case_cg(DEV, B)


def test_numpy_observation_edited_in_place_is_seen():
    pc.case_numpy_observation_edits(DEV)


def test_cg_both_branches_of_the_fused_call():
    pc.case_cg_branches(DEV, quick=True)


def test_cg_control_kernels_in_both_forms():
    pc.case_cg_control_forms(DEV)


def test_cg_matvec_with_one_wave_transforms_320():
    pc.case_cg_wave_fft(DEV, sizes=(320,), B=1, iters=3)


def test_cg_masked_fft_odd_and_per_image_masks():
    pc.case_cg_masked_fft_shapes(DEV)


def test_dense_systems_cg_cg2_pcg_and_implicit_gradients():
    pc.case_dense_krylov(DEV)


def test_doe_psf_gradient_through_the_unrolled_solver():
    pc.case_doe_psf_grad(DEV)
    pc.case_doe_op_autograd(DEV)


def test_builtin_linear_nodes_under_autograd():
    pc.case_linop_autograd(DEV)


def test_ffdnet_split_f16_and_its_range_trap():
    pc.case_ffdnet_f16_split(DEV, tiny=True)


def test_ffdnet_winograd_layers():
    pc.case_ffdnet_winograd(DEV, tiny=True)


def test_linear_solve_implicit_backward():
    pc.case_linear_solve_grad(DEV)


def test_ffdnet_mfma_layout():
    pc.case_ffdnet(DEV, which=("batch",))       # 2x3x16x24: the f32 MFMA lane layouts + pack / unpack, emulated


def test_other_algorithms():
    pc.case_other_algorithms(DEV)


def test_plug_and_play_cg_loop_forms_are_bit_identical():
    pc.case_split_cg_loop_forms(DEV, B=1, H=32, W=32, iters=3)          # (the emulator's share; the GPU suite runs 2 x 48 x 48 and config 4's shard)


def test_csmri_custom_admm():
    pc.case_csmri(DEV, solve=False)          # the 4-iteration solve with the 15-layer gray FFDNet runs on the GPU only


def test_conv2d_generic():
    pc.case_conv2d_generic(DEV)


def test_tiny_shapes():
    pc.case_tiny_shapes(DEV)


def test_conv_doe():
    pc.case_conv_doe(DEV)


def test_sisr_super_resolution():
    pc.case_sisr(DEV, solve=False)


def test_mosaic_joint_demosaic_deconv():
    pc.case_mosaic_jd(DEV, solve=False)      # the ADMM + CG + FFDNet solve runs on the GPU only


def test_unrolled_backward_fused_stage_matches_the_staged_loop():
    # (32 x 48 planes: off the two-kernel backward iteration -- its row-kernel choice is exercised at 256 x 256 below)
    pc.case_unrolled_bwd_fused_vs_staged(DEV, modes=[m for m in pc.UNROLL_BWD_MODES if m[0] != "lock-step bands"], term_sets=("tv+nn", "nn+l1"))


def test_unrolled_backward_two_kernel_iteration_256():
    # 2 x 2 planes of 256 x 256, bands of 14 and 5 rows (the last band of a plane shorter / a band inside one lock-step round)
    modes = [m for m in pc.UNROLL_BWD_MODES if m[0] in ("default", "lock-step bands", "staged")]
    pc.case_unrolled_bwd_fused_vs_staged(DEV, shape=(1, 2, 256, 256), K=3, term_sets=("tv+nn",), dtypes=("f32",), modes=modes)
    pc.case_unrolled_bwd_fused_vs_staged(DEV, shape=(1, 1, 256, 256), K=2, term_sets=("nn+l1",), dtypes=("bf16",), modes=modes, band=5)


def test_unrolled_backward_shortest_loops():
    pc.case_unrolled_bwd_shortest_loops(DEV)


def test_unrolled_plane_sizes_one_pixel_per_thread():
    """widths with W % 4 = 2, 3 and 1, an odd height, two images x three channels: the forward pass runs the one-pixel forms of
    k_zupdate_rhs / k_rhs / k_zupdate, the backward pass the one-pixel forms of the staged loop's stages"""
    pc.case_unrolled_plane_sizes(DEV, shapes=((2, 3, 30, 46), (2, 3, 31, 43), (2, 3, 30, 41)))


def test_unrolled_backward_shortest_loops_one_pixel_per_thread():
    pc.case_unrolled_bwd_shortest_loops(DEV, shapes=((1, 2, 31, 43),))


def _shifted(t, shift):
    """a contiguous copy of t that starts `shift` floats into its (64-byte aligned) storage"""
    import torch
    buf = torch.empty(t.numel() + 4, dtype=torch.float32)
    view = buf[shift:shift + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * shift
    return view


def test_staged_backward_passes_take_misaligned_planes():
    """planes that start one float into their storage (W % 4 == 0: the width alone would pick the 16-byte forms) go through the one-pixel
    forms of the staged backward passes: dpx_admm_zupdate_bwd, and the unrolled backward's staged loop -- selected by its knob, and as what
    the image-domain fused stage falls back to (the launch log shows k_zupdate_bwd per iteration and no k_rhs_z_bwd; on aligned planes the
    same setting does launch k_rhs_z_bwd) -- give the same planes bit for bit as on aligned planes, and per-image sums within 1e-5 (the
    bound case_unrolled_bwd_fused_vs_staged uses between forms that add in different orders)"""
    import os
    import re
    import ctypes
    import numpy as np
    import torch
    import synthetic
    from conftest import rel_l2
    from dprox import _backend as be, _ops as ops
    L = be.lib()
    B, C, H, W = shape = (1, 2, 16, 24)
    px = B * C * H * W

    # ---- dpx_admm_zupdate_bwd
    gen = torch.Generator().manual_seed(3)
    codes = ((be.LIN_GRAD_H, be.PROX_NORM1, 1.0), (be.LIN_GRAD_W, be.PROX_NORM1, 1.0), (be.LIN_IDENTITY, be.PROX_NONNEG, 1.0),
             (be.LIN_IDENTITY, be.PROX_SUMSQ, 0.5))
    n = len(codes)
    lam = [0.05 + 0.1 * torch.rand(B, generator=gen) for _ in codes]
    vs = [ops.prox(pk, torch.randn(shape, generator=gen), lam[i], alpha=al) for i, (_, pk, al) in enumerate(codes)]
    gvs, guns = ([torch.randn(shape, generator=gen) for _ in codes] for _ in range(2))
    ws_floats = L.query("dpx_admm_bwd_ws_bytes", B, C, H, W) // 4

    def zupdate_bwd(shift):
        place = lambda t: _shifted(t, shift)
        keep = [[place(t) for t in ts] for ts in (vs, gvs, guns)]
        gx, ws, gus = place(torch.zeros(shape)), place(torch.zeros(ws_floats)), [place(torch.zeros(shape)) for _ in codes]
        arr = (be.BwdTerm * n)()
        for i, (lc, pk, al) in enumerate(codes):
            arr[i].linop, arr[i].prox, arr[i].alpha, arr[i].lam = lc, pk, al, lam[i].data_ptr()
            arr[i].v, arr[i].gv, arr[i].gu_new, arr[i].gu = keep[0][i].data_ptr(), keep[1][i].data_ptr(), keep[2][i].data_ptr(), gus[i].data_ptr()
        glam = torch.empty(n, B)
        L.call("dpx_admm_zupdate_bwd", be.ptr(gx), arr, n, be.ptr(glam), B, C, H, W, be.ptr(ws), be.stream())
        return [gx, *gus], glam

    (planes_a, sums_a), (planes_m, sums_m) = zupdate_bwd(0), zupdate_bwd(1)
    for k, (a, m) in enumerate(zip(planes_a, planes_m)):
        assert torch.equal(a, m), f"dpx_admm_zupdate_bwd: plane {k} differs on misaligned planes"
    assert rel_l2(sums_m.numpy(), sums_a.numpy()) <= 1e-5

    # ---- the unrolled backward's staged loop: the arguments of a real training step's call, replayed on buffers of our own
    decl = re.search(r"\bdpx_admm_unrolled_backward\s*\(([^;]*?)\)\s*;", open(os.path.join(emul_util.ROOT, "include", "dpx.h")).read(), re.S).group(1)
    names = [re.search(r"(\w+)\s*$", prm).group(1) for prm in decl.split(",")]       # the parameters' names, in the header's order

    def launches():
        buf = ctypes.create_string_buffer(1 << 16)
        L.call("dpx_timing_report", buf, len(buf))
        return {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines() if ln.split()}

    def replay(args, shift, staged):
        assert len(args) == len(names)
        a = dict(zip(names, args))
        n, T = a["nterms"], a["T"]
        place = lambda t: _shifted(t, shift)
        take = lambda p, count: torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * count).from_address(p.value)).copy())
        hist = place(take(a["hist"], T * (2 + 2 * n) * px))
        gx = None if a["gx"] is None else place(take(a["gx"], px).view(shape))
        assert all(p is None for p in list(a["gv_in"]) + list(a["gu_in"])), "the loss uses x alone"
        gv0, gu0 = ([place(torch.zeros(shape)) for _ in range(n)] for _ in range(2))
        goff = [None if p is None else place(torch.zeros(shape)) for p in list(a["goff"])[:a["n_off"]]]
        g_rho, g_lam = torch.empty(T, B), torch.empty(T, n, B)
        ws = place(torch.zeros(L.query("dpx_admm_unrolled_bwd_ws_bytes", n, B, C, H, W) // 4))
        ptrs = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
        a.update(hist=be.ptr(hist), gx=be.ptr(gx), gv0=ptrs(gv0), gu0=ptrs(gu0), grho=be.ptr(g_rho), glam=be.ptr(g_lam), goff=ptrs(goff), ws=be.ptr(ws))
        orig("dpx_timing_enable", 1)
        try:
            launches()                                       # (reading the log resets it)
            with be.tuned(unroll_bwd_staged=staged):
                orig("dpx_admm_unrolled_backward", *[a[k] for k in names])
            log = launches()
        finally:
            orig("dpx_timing_enable", 0)
        return [*gv0, *gu0, *[t for t in goff if t is not None]], torch.cat([g_rho.flatten(), g_lam.flatten()]), log, T

    runs = []

    def spy(name, *args):
        if name == "dpx_admm_unrolled_backward" and not runs:
            runs.extend([replay(args, 0, 1), replay(args, 1, 1), replay(args, 1, 2), replay(args, 0, 2)])
        return orig(name, *args)

    orig = L.call
    L.call = spy
    try:
        pc._unrolled_bwd_run(DEV, synthetic.deconv_case(*shape, seed=17, ksize=5, ksigma=1.2), "tv+nn", "f32", 3, dict(unroll_bwd_staged=1))
    finally:
        del L.call
    assert len(runs) == 4
    (planes_a, sums_a, log_a, T), (planes_m, sums_m, log_m, _), (planes_f, sums_f, log_f, _), (_, _, log_fused, _) = runs
    for log in (log_a, log_m, log_f):                        # the staged loop: one z stage per iteration, never the fused stage
        assert log.get("k_zupdate_bwd") == T and "k_rhs_z_bwd" not in log, log
    assert log_fused.get("k_rhs_z_bwd") == T - 1 and log_fused.get("k_zupdate_bwd") == 1, log_fused      # (aligned planes: the fused stage runs)
    assert float(sums_a.abs().max()) > 0 and all(float(p.abs().max()) > 0 for p in planes_a)
    for what, planes, sums in (("staged loop", planes_m, sums_m), ("staged loop in place of the fused stage", planes_f, sums_f)):
        for k, (a, m) in enumerate(zip(planes_a, planes)):
            assert torch.equal(a, m), f"{what}: plane {k} differs on misaligned planes"
        assert rel_l2(sums.numpy(), sums_a.numpy()) <= 1e-5, what


def test_unrolled_forward_refuses_fresh_x0_off_the_two_kernel_iteration():
    """both history formats: a lazy fresh state (fresh_x0) exists only for the two-kernel iteration; on a plane that is not on it the
    entry point says so and launches nothing (it used to be the fp32 entry's rule alone)"""
    import ctypes
    import torch
    from dprox import _backend as be
    B, C, H, W, n, K = 1, 1, 12, 20, 1, 1
    t = lambda *shape: torch.zeros(*shape)
    planes = [t(B, C, H, W) for _ in range(6)]
    arr = lambda ts: (ctypes.c_void_p * n)(*[x.data_ptr() for x in ts])
    lin, prx, alp = (ctypes.c_int * n)(be.LIN_IDENTITY), (ctypes.c_int * n)(be.PROX_NONNEG), (ctypes.c_float * n)(1.0)
    rho, lam, dummy = t(K, B), t(K, B), t(64)
    tail = (arr(planes[0:1]), arr(planes[1:2]), lin, prx, alp, n, be.ptr(rho), arr([lam]), K, be.ptr(dummy), be.ptr(dummy), ctypes.c_float(0.0), B, C, H, W,
            be.ptr(dummy), be.ptr(dummy), be.ptr(planes[2]), be.stream())
    with pytest.raises(be.DpxError, match=r"dpx_admm_unrolled_forward: fresh_x0 needs the two-kernel iteration \(plane 12 x 20 is not on it\)"):
        be.lib().call("dpx_admm_unrolled_forward", be.ptr(t(K, 2 + 2 * n, B, C, H, W)), *tail)
    with pytest.raises(be.DpxError, match=r"dpx_admm_unrolled_forward_bf16: fresh_x0 needs the two-kernel iteration \(plane 12 x 20 is not on it\)"):
        be.lib().call("dpx_admm_unrolled_forward_bf16", be.ptr(t(K, 2 + n, B, C, H, W)), be.ptr(t(2 + 4 * n, B, C, H, W)), be.ptr(planes[3]), arr(planes[4:5]),
                      arr(planes[5:6]), *tail)


def test_unrolled_gradients():
    pc.case_unrolled_grads(DEV)


def test_unrolled_gradients_bf16_history():
    pc.case_unrolled_grads_bf16(DEV)


def test_unrolled_solver_learned_params():
    pc.case_unrolled_solver(DEV)


def test_train_driver_and_resume(tmp_path):
    pc.case_train(DEV, str(tmp_path))


@pytest.mark.skipif(not __import__("os").environ.get("DPX_EMUL_SLOW"), reason="~4 min on the emulator (runs on the GPU in test_gpu_parity); DPX_EMUL_SLOW=1 enables it")
def test_ffdnet_weight_gradients():
    pc.case_ffdnet_weight_grads(DEV)


def test_wgrad_c8_kernel():
    pc.case_wgrad_c8(DEV, tiny=True)


def test_ffdnet_split_backward():
    pc.case_ffdnet_split_backward(DEV, tiny=True)


@pytest.mark.skipif(not __import__("os").environ.get("DPX_EMUL_SLOW"), reason="~1 min on the emulator (runs on the GPU in test_gpu_parity; the split-kernel backward below stays); DPX_EMUL_SLOW=1 enables it")
def test_ffdnet_backward():
    pc.case_ffdnet_grads(DEV, which=("even",))      # one small image: the emulator runs MFMA layers at ~1 s each


def test_adjoint_dot_product():
    pc.case_adjoint_dot(DEV, shape=(1, 3, 24, 20))


def test_unet_layer_kernels_vs_torch():
    """the U-Net's non-convolution layers (dpx_unet.hip) against ATen on the CPU: MaxPool2d(2) with odd sizes and ties,
    bilinear x2 (align_corners=True) + zero pad + concat, their adjoints (dot-product test + autograd), LeakyReLU backward"""
    import torch
    import torch.nn.functional as F
    from dprox import _ops as ops
    torch.manual_seed(3)
    x = torch.rand(2, 3, 9, 11)
    x[0, 0, 0, 0] = x[0, 0, 0, 1] = 0.99                      # a tie: the gradient goes to the first maximum
    assert torch.equal(ops.maxpool2(x), F.max_pool2d(x, 2))
    xr = x.clone().requires_grad_(True)
    gy = torch.randn(2, 3, 4, 5)
    (F.max_pool2d(xr, 2) * gy).sum().backward()
    assert torch.equal(ops.maxpool2_bwd(x, gy), xr.grad)
    for (h, w), (H, W) in (((4, 5), (9, 11)), ((1, 3), (2, 6)), ((6, 6), (12, 13))):
        low, skip = torch.rand(2, 3, h, w), torch.rand(2, 2, H, W)
        up = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=True)
        dy, dx = H - 2 * h, W - 2 * w
        ref = torch.cat([skip, F.pad(up, (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))], dim=1)
        got = ops.concat_skip_upsampled(skip, low)
        assert float((got - ref).abs().max()) <= 2e-7, float((got - ref).abs().max())
        g = torch.randn_like(ref)
        gskip, glow = ops.concat_skip_upsampled_bwd(g, 2, (h, w))
        lr = low.clone().requires_grad_(True)
        upr = F.pad(F.interpolate(lr, scale_factor=2, mode="bilinear", align_corners=True), (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))
        (upr * g[:, 2:]).sum().backward()
        assert torch.equal(gskip, g[:, :2]) and float((glow - lr.grad).abs().max()) <= 2e-6
    y, g = torch.randn(2, 3, 5, 7), torch.randn(2, 3, 5, 7)
    assert torch.equal(ops.leaky_relu_bwd(y, g, 0.2), torch.where(y > 0, g, 0.2 * g))


def test_leaky_conv_layer_vs_torch():
    """dpx_conv2d_leaky (bias + LeakyReLU(0.2) epilogue on the MFMA kernel) against F.conv2d on a small layer"""
    import torch
    import torch.nn.functional as F
    from dprox import _ops as ops
    torch.manual_seed(4)
    x, w, b = torch.randn(1, 2, 9, 13), torch.randn(32, 2, 3, 3) * 0.3, torch.randn(32) * 0.1
    blob = ops.conv_pack(w.reshape(32, 2, 9).contiguous(), b, 9)
    ref = F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.2)
    got = ops.conv2d_leaky(x, blob, 32, 0.2)
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_row_parallel_kernel_is_bit_identical_to_the_streaming_kernel():
    pc.case_row_parallel_kernel(DEV, shapes=((1, 1, 256, 256),), iters=2, methods=("admm",), nterms_list=(3,), hfirst=(True, False))
    pc.case_row_parallel_kernel(DEV, shapes=((1, 1, 256, 256),), iters=2, methods=("hqs", "admm_vxu"), nterms_list=(2,), hfirst=(True,))


def test_merged_loop_keeps_the_callers_duals():
    pc.case_merged_loop_keeps_the_callers_duals(DEV)
