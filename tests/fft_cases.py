"""TEST INFRASTRUCTURE: every FFT path (csrc/dpx_fft.hip, dpx_fft_pow2.hip / dpx_fft_reg.h, dpx_otf.hip) against numpy's float64 FFT
with operators whose spectrum is flat, shared by tests/test_gpu_fft.py (MI355X), tests/test_fft_emul.py (SIMT emulator) and the
guarded tables (tests/test_gpu_guarded.py, tests/test_guarded_emul.py).

Inputs that make every bin count: a white image ``randn(B, C, H, W)`` and a dense real kernel of the plane's own size,
``h = randn(C, H, W) / sqrt(H W)``; its full-grid spectrum ``fft2(h)`` is rounded to complex64 and handed over with
``ops.otf_from_full``, and the float64 reference uses the same rounded table (table rounding is not charged to the kernels).  The
seed is a function of (H, W).

  A  ops.fft_conv, conj = False / True           vs  ifft2(fft2(x) F), ifft2(fft2(x) conj(F))
  B  ops.data_spectrum + ops.fourier_solve       vs  ifft2((fft2(rhs) + conj(F) fft2(b) + eps) / (|F|^2 + rho + eps)), F = psf2otf(k) in
     numpy (zero-pad, roll by -floor(k / 2), fft2) of a dense random kernel k: 1 x 1, 4 x 5 (clipped to the plane) and, where
     H W <= 1200, the whole plane -- dpx_psf2otf (both of its kernels), the fp64 row / column pass, OP_SOLVE with spec_add
  C  ops.cfft2, the eight combinations of inverse / centred / ortho   vs  fftshift(fft2 | ifft2 (ifftshift(x), norm))
  D  planes do not interact: fft_conv of one plane with its channel's table equals its slice of the batch result bit for bit
  E  refused lengths: DpxError, the output untouched, the neighbouring accepted length still works

Bounds (measured against the reference, no number chosen in advance): every comparison also evaluates the same formula with
torch.fft in float32 / complex64 on the CPU; its rel-L2 and max-abs (over max|ref|) distance from float64 is e32, floored at 2^-23
(it is 0 on a 1 x 1 plane).  The gate, on both metrics, is  err <= 3 e32 g:  g = 1 when every radix of both plans is <= 13, and
g = max(1, sqrt(p / 97)) when p is the largest generic prime of either plan (stockham_pass_any adds p terms per output where
pocketfft uses Bluestein; on the emulator ours / e32 = 1.1 at p = 97, 2.0 at 683, 5.6 at 3413).  The factor 3 covers the
difference between the emulator's and the GPU's contraction of multiply-adds (emulator ratios <= 1.2 at g = 1)."""
import functools
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import record
from dprox import _backend as be
from dprox import _ops as ops

FLOOR = 2.0 ** -23
FACTOR = 3.0
EPS = 1e-7

# ---- shapes, B x C x H x W -----------------------------------------------------------------------------------------------------------
SMALL = ((1, 1, 1, 8), (1, 1, 6, 1), (1, 1, 2, 2), (1, 1, 8, 6), (2, 2, 12, 7), (1, 1, 17, 19), (1, 2, 26, 34), (1, 1, 13, 39), (1, 1, 23, 58),
         (3, 1, 30, 44), (1, 1, 6, 97), (1, 1, 97, 6), (1, 1, 289, 4), (1, 1, 4, 578))
# il_seqs on the row length M = W / 2 (W when odd): one row per wave up to 1024, four-sequence workgroups up to 2048, else the first form
ROWS = ((1, 1, 4, 2000), (1, 1, 4, 2048), (1, 1, 4, 2050), (1, 1, 4, 2400), (1, 1, 3, 1125), (1, 1, 3, 675), (1, 1, 4, 4096), (1, 1, 4, 4320),
        (1, 1, 4, 4100), (1, 1, 6, 1664), (1, 1, 3, 2049))
COLS = ((1, 2, 1000, 6), (1, 1, 1024, 6), (2, 1, 1080, 6), (1, 1, 2048, 18), (1, 1, 2160, 6), (1, 1, 2197, 4), (1, 1, 1025, 3))
LARGEST = ((1, 1, 10239, 2), (1, 1, 2, 20478), (1, 1, 2, 10239))
REG = tuple((1, 2, H, 256) for H in (256, 384, 512, 768, 1024, 1536, 2048)) + tuple((1, 2, 256, W) for W in (512, 768, 1024, 1536, 2048)) \
    + ((1, 2, 768, 768), (2, 3, 256, 256))
SHAPES = SMALL + ROWS + COLS + LARGEST + REG
# the emulator's share: everything that takes a few seconds at the most there (not the 10239 / 20478 lengths, nor the register-radix
# planes of 2^18 points and more)
EMUL_SHAPES = tuple(s for s in SHAPES if s not in LARGEST and not (s in REG and s[2] * s[3] >= 1 << 18))
# case D: the multi-plane shapes above, and three more plane counts on the ragged sizes
PLANES_EXTRA = ((2, 3, 12, 7), (2, 2, 26, 34), (2, 1, 3, 1125))
PLANES = tuple(s for s in SHAPES if s[0] * s[1] > 1) + PLANES_EXTRA
EMUL_PLANES = tuple(s for s in PLANES if s not in REG) + ((2, 3, 256, 256),)
# the fp64 data spectrum keeps two columns (one row) of padded double2 sequences in 160 KB: it refuses these lengths, case B solves without it
DS_REFUSED = LARGEST
# case C, P x H x W
CFFT_SHAPES = ((1, 1, 1), (1, 1, 7), (2, 5, 1), (1, 2, 2), (2, 7, 9), (1, 8, 6), (3, 17, 12), (1, 13, 11), (1, 33, 26), (1, 6, 97), (1, 97, 6),
               (1, 4, 1023), (1, 1023, 3), (1, 3, 2047), (1, 3640, 2), (1, 3838, 2), (1, 3839, 2), (1, 256, 256), (1, 2, 4095))
# case E: (function, refused shape, accepted neighbour, what the message names)
REFUSALS = {
    "conv_cols_10240": ("fft_conv", (1, 1, 10240, 2), (1, 1, 10239, 2), "column length 10240 too large for the LDS-resident generic FFT"),
    "conv_rows_20480": ("fft_conv", (1, 1, 2, 20480), (1, 1, 2, 20478), "row length 20480 too large for the LDS-resident generic FFT"),
    "conv_rows_10241": ("fft_conv", (1, 1, 2, 10241), (1, 1, 2, 10239), "row length 10241 too large for the LDS-resident generic FFT"),
    "cfft2_4096": ("cfft2", (1, 2, 4096), (1, 2, 4095), "dpx_cfft2: plane 2x4096 too large for the LDS-resident transform"),
}
# the emulator's share of case E: the accepted neighbours of the 10240 / 20480 lengths take seconds there
EMUL_REFUSALS = ("cfft2_4096",)
GUARDED = ((2, 2, 12, 7), (1, 2, 26, 34), (1, 1, 3, 1125), (1, 1, 2048, 18), (1, 1, 4, 4096), (1, 2, 384, 256))

ACHIEVED = {}          # comparison -> figures; written to the file DPX_FFT_PARITY_OUT names, if it is set (write_achieved)


def sid(shape):
    return "x".join(str(s) for s in shape)


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- the plans, restated (csrc/dpx_fft.hip make_plan; dpx_fft_pow2.hip pow2_path_available) --------------------------------------------
def radices(n):
    out = []
    for r in (8, 4, 2, 3, 5, 7, 11, 13):
        while n % r == 0 and n > 1:
            out.append(r)
            n //= r
    q = 17
    while n > 1:
        while n % q == 0:
            out.append(q)
            n //= q
        q += 2
    return out


def pow2_path(H, W):
    return H in (256, 384, 512, 768, 1024, 1536, 2048) and W in (256, 512, 768, 1024, 1536, 2048)


def growth(H, W, real=True):
    """g of the gate: the plans of a real transform are make_plan(W / 2 or W) and make_plan(H), of dpx_cfft2 make_plan(W) and make_plan(H)"""
    if real and pow2_path(H, W):
        return 1.0
    M = W // 2 if real and W % 2 == 0 else W
    p = max(radices(M) + radices(H) + [1])
    return max(1.0, math.sqrt(p / 97.0)) if p > 13 else 1.0


# ---- metrics and the gate ------------------------------------------------------------------------------------------------------------
def distances(a, ref):
    """(rel-L2, max-abs over max|ref|) in float64 / complex128"""
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    wide = np.complex128 if np.iscomplexobj(a) or np.iscomplexobj(ref) else np.float64
    d = a.astype(wide) - ref.astype(wide)
    return (float(np.linalg.norm(d.ravel()) / max(np.linalg.norm(ref.ravel()), 1e-300)),
            float(np.max(np.abs(d)) / max(np.max(np.abs(ref)), 1e-300)))


def gate(ours, f32, ref, g, what):
    """err <= 3 e32 g on rel-L2 and on max-abs, e32 = the float32 torch.fft evaluation's distance from float64, floored at 2^-23"""
    assert np.isfinite(np.asarray(ours)).all(), f"{what}: non-finite output"
    e, e32 = distances(ours, ref), tuple(max(v, FLOOR) for v in distances(f32, ref))
    bound = tuple(FACTOR * v * g for v in e32)
    record(what, e[0], bound[0], e[1])
    ACHIEVED[what] = dict(rel_l2=e[0], maxabs=e[1], e32_rel_l2=e32[0], e32_maxabs=e32[1], g=g, bound_rel_l2=bound[0], bound_maxabs=bound[1])
    print(f"{what}: rel-L2 {e[0]:.3e} (e32 {e32[0]:.3e}, gate {bound[0]:.3e}), max-abs {e[1]:.3e} (e32 {e32[1]:.3e}, gate {bound[1]:.3e}), g {g:.2f}")
    assert e[0] <= bound[0], f"{what}: rel-L2 {e[0]:.3e} > 3 x {e32[0]:.3e} x {g:.2f}"
    assert e[1] <= bound[1], f"{what}: max-abs {e[1]:.3e} > 3 x {e32[1]:.3e} x {g:.2f}"


def write_achieved():
    """the figures of the comparisons run so far -> the JSON file the environment variable DPX_FFT_PARITY_OUT names (how
    profiles/fft_parity_achieved.json is produced from a GPU run); without the variable nothing is written"""
    path = os.environ.get("DPX_FFT_PARITY_OUT")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ACHIEVED, f, indent=1, sort_keys=True)


# ---- inputs and references (computed once per shape, never modified) -------------------------------------------------------------------
def _rng(H, W, salt=0):
    return np.random.RandomState((7919 * H + W + 104729 * salt) % (2 ** 31))


@functools.lru_cache(maxsize=None)
def conv_inputs(shape):
    """(x [B, C, H, W] float32 white, F [C, H, W] complex64: the spectrum of a dense real kernel of the plane's size)"""
    B, C, H, W = shape
    rng = _rng(H, W)
    x = rng.randn(B, C, H, W).astype(np.float32)
    h = rng.randn(C, H, W) / math.sqrt(H * W)
    return x, np.fft.fft2(h).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def conv_refs(shape, conj):
    """(float64 reference, the float32 torch.fft evaluation) of the convolution / its adjoint"""
    x, F = conv_inputs(shape)
    F64 = F.astype(np.complex128)
    ref = np.fft.ifft2(np.fft.fft2(x.astype(np.float64)) * (F64.conj() if conj else F64)).real
    Ft = torch.from_numpy(F)
    f32 = torch.fft.ifft2(torch.fft.fft2(torch.from_numpy(x)) * (Ft.conj() if conj else Ft)).real.numpy()
    return ref, f32


def conv_table(shape, device, channel=None):
    _, C, H, W = shape
    F = conv_inputs(shape)[1]
    if channel is not None:
        F, C = F[channel:channel + 1], 1
    return ops.otf_from_full(T(F, device), C, H, W)


def case_conv(device, shape):
    """A. forward and adjoint FFT convolution with a flat-spectrum operator"""
    _, _, H, W = shape
    x = T(conv_inputs(shape)[0], device)
    otf = conv_table(shape, device)
    for conj in (False, True):
        y = ops.fft_conv(x, otf, conj=conj).cpu().numpy()
        ref, f32 = conv_refs(shape, conj)
        gate(y, f32, ref, growth(H, W), f"A fft_conv{' adjoint' if conj else ''} {sid(shape)}")


def psf2otf64(k, H, W):
    """psf2otf in numpy: zero-pad, the kernel's centre (floor(k / 2)) rolled to the origin, fft2"""
    pad = np.zeros((H, W), np.float64)
    pad[:k.shape[0], :k.shape[1]] = k
    return np.fft.fft2(np.roll(pad, (-(k.shape[0] // 2), -(k.shape[1] // 2)), (0, 1)))


def kernel_sizes(H, W):
    sizes = [(1, 1), (min(4, H), min(5, W))] + ([(H, W)] if H * W <= 1200 else [])
    return tuple(dict.fromkeys(sizes))


@functools.lru_cache(maxsize=None)
def solve_inputs(shape):
    B, C, H, W = shape
    rng = _rng(H, W, salt=1)
    rhs, b = rng.randn(B, C, H, W).astype(np.float32), rng.randn(B, C, H, W).astype(np.float32)
    kernels = tuple(rng.randn(kh, kw) / math.sqrt(kh * kw) for kh, kw in kernel_sizes(H, W))
    return rhs, b, kernels, np.linspace(0.3, 0.7, B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def solve_refs(shape, ki, with_data):
    """(float64 reference, float32 torch.fft evaluation) of the x-update with kernel ki (without the data term where the library refuses
    the plane's fp64 data spectrum)"""
    B, C, H, W = shape
    rhs, b, kernels, rho = solve_inputs(shape)
    F = psf2otf64(kernels[ki], H, W)
    r64 = rho.astype(np.float64).reshape(B, 1, 1, 1)
    num = np.fft.fft2(rhs.astype(np.float64)) + (F.conj() * np.fft.fft2(b.astype(np.float64)) if with_data else 0.0) + EPS
    ref = np.fft.ifft2(num / (np.abs(F) ** 2 + r64 + EPS)).real
    Ft, rt = torch.from_numpy(F.astype(np.complex64)), torch.from_numpy(rho).view(B, 1, 1, 1)
    num = torch.fft.fft2(torch.from_numpy(rhs)) + (Ft.conj() * torch.fft.fft2(torch.from_numpy(b)) if with_data else 0.0) + EPS
    f32 = torch.fft.ifft2(num / (Ft.abs() ** 2 + rt + EPS)).real.numpy()
    return ref, f32


def case_solve(device, shape):
    """B. the x-update: OTF and |OTF|^2 tables from dpx_psf2otf, the fp64 data spectrum, OP_SOLVE with spec_add, per-image rho"""
    B, C, H, W = shape
    rhs, b, kernels, rho = solve_inputs(shape)
    rhs_d, b_d, rho_d = T(rhs, device), T(b, device), T(rho, device)
    for ki, k in enumerate(kernels):
        otf = ops.make_otf(k, C, H, W, device)
        d0 = ops.accumulate_diag(ops.new_diag(C, H, W, device), k, 1.0, C, H, W)
        try:
            FK = ops.data_spectrum(b_d, otf, conj=True)
        except be.DpxError as e:
            assert shape in DS_REFUSED and "too large for the LDS-resident fp64 transform" in str(e), e
            FK = None
        else:
            assert shape not in DS_REFUSED, f"{sid(shape)}: the fp64 data spectrum was expected to refuse this plane"
        x = ops.fourier_solve(rhs_d, d0, None, 0.0, 1.0, rho_d, EPS, spec_add=FK).cpu().numpy()
        ref, f32 = solve_refs(shape, ki, FK is not None)
        gate(x, f32, ref, growth(H, W), f"B solve {sid(shape)} kernel {k.shape[0]}x{k.shape[1]}")


@functools.lru_cache(maxsize=None)
def cfft_input(shape):
    P, H, W = shape
    rng = _rng(H, W, salt=2)
    return (rng.randn(P, H, W) + 1j * rng.randn(P, H, W)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def cfft_refs(shape, inverse, centred, ortho):
    x, norm, ax = cfft_input(shape), "ortho" if ortho else "backward", (-2, -1)
    z = x.astype(np.complex128)
    z = np.fft.ifftshift(z, axes=ax) if centred else z
    z = (np.fft.ifft2 if inverse else np.fft.fft2)(z, norm=norm)
    ref = np.fft.fftshift(z, axes=ax) if centred else z
    t = torch.from_numpy(x)
    t = torch.fft.ifftshift(t, dim=ax) if centred else t
    t = (torch.fft.ifft2 if inverse else torch.fft.fft2)(t, norm=norm)
    f32 = (torch.fft.fftshift(t, dim=ax) if centred else t).numpy()
    return ref, f32


def case_cfft2(device, shape):
    """C. the complex 2-D transform (k_crows / k_ccols) in all eight flag combinations; odd lengths tell fftshift from ifftshift"""
    _, H, W = shape
    x = T(cfft_input(shape), device)
    for inverse, centred, ortho in itertools.product((False, True), repeat=3):
        y = ops.cfft2(x, inverse=inverse, centred=centred, ortho=ortho).cpu().numpy()
        ref, f32 = cfft_refs(shape, inverse, centred, ortho)
        gate(y, f32, ref, growth(H, W, real=False), f"C cfft2 {sid(shape)} inverse={int(inverse)} centred={int(centred)} ortho={int(ortho)}")


def case_planes(device, shape):
    """D. every plane of a batch alone, with its channel's table alone, equals its slice of the batch result bit for bit (ragged last
    workgroups, plane and channel offsets)"""
    B, C, H, W = shape
    assert B * C > 1
    x = T(conv_inputs(shape)[0], device)
    otf = conv_table(shape, device)
    batch = {conj: ops.fft_conv(x, otf, conj=conj).cpu() for conj in (False, True)}
    for c in range(C):
        otf_c = conv_table(shape, device, channel=c)
        for bi, conj in itertools.product(range(B), (False, True)):
            one = ops.fft_conv(x[bi:bi + 1, c:c + 1].contiguous(), otf_c, conj=conj).cpu()
            assert torch.isfinite(one).all() and float(one.abs().max()) > 0
            assert torch.equal(one[0, 0], batch[conj][bi, c]), \
                f"{sid(shape)} plane ({bi}, {c}) conj={conj}: alone differs from its slice of the batch by {float((one[0, 0] - batch[conj][bi, c]).abs().max())}"


SENTINEL = -77.25


def _cfft2_into(x, out):
    H, W = int(x.shape[-2]), int(x.shape[-1])
    be.lib().call("dpx_cfft2", be.ptr(x), be.ptr(out), 0, 1, 1, x.numel() // (H * W), H, W, be.ptr(ops.fft_table(H, W, x.device)), be.stream())


def case_refusal(device, name, neighbour=True):
    """E. a length whose workgroup does not fit the LDS is refused by the argument check (status -3, DPX_ERR_UNSUPPORTED): DpxError with
    its message, the output untouched, and the neighbouring accepted length still works afterwards"""
    fn, refused, accepted, message = REFUSALS[name]
    if fn == "fft_conv":
        _, C, H, W = refused
        x = T(_rng(H, W, salt=3).randn(*refused).astype(np.float32), device)
        otf = ops.otf_from_full(T(np.ones((C, H, W), np.complex64), device), C, H, W)
        out = torch.full_like(x, SENTINEL)
        with pytest.raises(be.DpxError, match=r"dpx_fft_conv failed \(-3\): " + message):
            ops.fft_conv(x, otf, out=out)
    else:
        x = T(cfft_input(refused), device)
        out = torch.full_like(x, SENTINEL)
        with pytest.raises(be.DpxError, match=r"dpx_cfft2 failed \(-3\): " + message):
            _cfft2_into(x, out)
    if out.is_cuda:
        torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), f"{name}: the refused call wrote to its output"
    if neighbour:
        (case_conv if fn == "fft_conv" else case_cfft2)(device, accepted)


# ---- the guarded tables' entry ---------------------------------------------------------------------------------------------------------
def case_guarded(device, shape):
    """A and B at one shape (run on exact-size, poisoned workspaces: dpx_spectrum_bytes, dpx_otf_bytes, dpx_data_spectrum_ws_bytes at odd
    widths and at the tile-rounded column counts)"""
    case_conv(device, shape)
    case_solve(device, shape)
