"""TEST INFRASTRUCTURE: the cases of the data spectrum's column-pass order (csrc/dpx_common.h, spec_cols_order_index), shared by
tests/test_gpu_data_spectrum_order.py (MI355X) and tests/test_data_spectrum_order_emul.py (SIMT emulator).

The buffer dpx_data_spectrum writes is opaque, so the layout is tested through its one consumer: the x-update
``dpx_fourier_solve(rhs = 0, spec_add = dpx_data_spectrum(b, OTF))`` against

    irfft2((conj(OTF) rfft2(b) + eps) / (|OTF|^2 + rho SUM G + eps))

evaluated in float64 with torch, SUM G = |F grad_H|^2 + |F grad_W|^2 = 4 sin^2(pi k / H) + 4 sin^2(pi l / W).  Every column length H
of the register-radix path at W = 256 (16 column groups of 8, 32 of 4 at H = 2048), B x C = 2 x 3 (plane and channel offsets; the
packed DC + i Nyquist column is in group 0 of every plane), a seeded 5 x 5 PSF, per-image rho = (0.1, 0.3).  The bound is the
repository's x-update bound, rel-L2 <= 1e-5; one misplaced element of the spectrum is an O(1) error.
"""
import functools

import numpy as np
import torch

from dprox import _ops as ops

HS = (256, 384, 512, 768, 1024, 1536, 2048)
B, C, W = 2, 3, 256
RHO = (0.1, 0.3)
EPS = 1e-7
BOUND = 1e-5


def rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).norm() / ref.norm())


@functools.lru_cache(maxsize=None)
def inputs(H):
    """(b [B, C, H, W] float32, psf [5, 5] float64): seeded, the same arrays for every test of one H (never modified)"""
    rng = np.random.RandomState(4100 + H)
    b = torch.from_numpy(rng.rand(B, C, H, W).astype(np.float32))
    psf = rng.rand(5, 5) + 0.1
    return b, psf / psf.sum()


@functools.lru_cache(maxsize=None)
def _spectral_parts(H):
    """float64: (conj(OTF) on the half grid [H, W/2 + 1], the denominator [B, 1, H, W/2 + 1])"""
    _, psf = inputs(H)
    pad = torch.zeros(H, W, dtype=torch.float64)
    pad[:5, :5] = torch.from_numpy(psf)
    otf = torch.fft.rfft2(torch.roll(pad, (-2, -2), (0, 1)))           # psf2otf: the kernel's centre at the origin
    k = torch.arange(H, dtype=torch.float64)[:, None]
    l = torch.arange(W // 2 + 1, dtype=torch.float64)[None, :]
    sum_g = 4 * torch.sin(np.pi * k / H) ** 2 + 4 * torch.sin(np.pi * l / W) ** 2
    rho = torch.tensor(RHO, dtype=torch.float64).view(B, 1, 1, 1)
    return otf.conj(), otf.abs() ** 2 + rho * sum_g + EPS


def reference(H, b):
    """the float64 x-update of the observation b (computed on the CPU)"""
    cotf, den = _spectral_parts(H)
    return torch.fft.irfft2((cotf * torch.fft.rfft2(b.double()) + EPS) / den, s=(H, W))


@functools.lru_cache(maxsize=None)
def reference_of_inputs(H):
    return reference(H, inputs(H)[0])


class Plane:
    """the library's tables of one H on one device: OTF, |OTF|^2 and SUM G"""

    def __init__(self, H, device):
        _, psf = inputs(H)
        self.H, self.device = H, device
        self.otf = ops.make_otf(psf, C, H, W, device)
        self.d0 = ops.accumulate_diag(ops.new_diag(C, H, W, device), psf, 1.0, C, H, W)
        k = torch.arange(H, dtype=torch.float64)[:, None]
        l = torch.arange(W, dtype=torch.float64)[None, :]
        full = (4 * torch.sin(np.pi * k / H) ** 2 + 4 * torch.sin(np.pi * l / W) ** 2).float().expand(1, C, H, W)
        self.d1 = ops.diag_from_full(full, C, H, W, device)
        self.zero = torch.zeros(B, C, H, W, dtype=torch.float32, device=device)
        self.rho = torch.tensor(RHO, dtype=torch.float32, device=device)

    def spectrum(self, b, out=None):
        return ops.data_spectrum(b.to(self.device).contiguous(), self.otf, conj=True, out=out, accumulate=out is not None)

    def solve(self, FK):
        return ops.fourier_solve(self.zero, self.d0, self.d1, 0.0, 0.0, self.rho, EPS, spec_add=FK)


def check(x, ref, what):
    r = rel_l2(x, ref)
    print(f"{what}: rel-L2 {r:.3e} (bound {BOUND:.0e})")
    assert r <= BOUND, f"{what}: rel-L2 {r:.3e} > {BOUND:.0e}"


def case_placement(device, H):
    """1. every element of the data spectrum reaches the frequency it belongs to"""
    pl = Plane(H, device)
    check(pl.solve(pl.spectrum(inputs(H)[0])), reference_of_inputs(H), f"placement H={H}")


def case_accumulate(device, H):
    """2. accumulate = 1 reads and writes the slot accumulate = 0 writes: a second, all-zero observation leaves the bits of the first
    (old + 0 is exact), and two observations b1, b2 in one buffer give the x-update of b1 + b2 (the x-update is linear in the data
    spectrum; float(double(float(s1)) + s2) is not float(s1 + s2) bit for bit, so this half has test 1's bound)"""
    pl = Plane(H, device)
    b1 = inputs(H)[0]
    b2 = torch.flip(b1, dims=(0, 2)) * 0.5
    used = lambda FK: FK.view(torch.float32)[:B * C * H * W]             # (the main part: a data spectrum has no side array)
    one = pl.spectrum(b1)
    acc = pl.spectrum(torch.zeros_like(b1), out=one.clone())
    assert torch.equal(used(acc), used(one)), f"H={H}: accumulating a zero observation changed the data spectrum"
    acc = pl.spectrum(b2, out=acc)
    check(pl.solve(acc), reference(H, b1.double() + b2.double()), f"accumulate H={H}")


def case_per_image(device, H):
    """3. the planes of one image stay that image's: with image 1 of b all zero, image 1 of the x-update is the solve without a data
    spectrum bit for bit, and image 0 is inside test 1's bound"""
    pl = Plane(H, device)
    b = inputs(H)[0].clone()
    b[1] = 0
    x = pl.solve(pl.spectrum(b))
    bare = pl.solve(None)
    assert torch.equal(x[1], bare[1]), f"H={H}: image 1 (zero observation) differs from the solve without a data spectrum"
    assert not torch.equal(x[0], bare[0])
    check(x[0], reference_of_inputs(H)[0], f"per-image H={H}, image 0")


def case_chains(device):
    """4. the two-kernel iteration as two sub-batch chains (each with its own data spectrum) against one chain: bit-identical full
    states -- the smallest ADMM case of parity_cases.case_sub_batch_chains"""
    import parity_cases as pc
    pc.case_sub_batch_chains(device, shapes=((3, 1, 256, 256),), iters=3, methods=("admm",), nchs=(2,), twice=False)
