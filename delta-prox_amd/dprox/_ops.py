"""Tensor-level wrappers around the C ABI (device pointers + current stream from PyTorch-ROCm).

PyTorch is used for device memory and streams only; every arithmetic pass below is a HIP kernel
of ``libdpx_hip.so``.
"""
import ctypes
from ctypes import c_double, c_float, c_void_p

import numpy as np
import torch

from . import _backend as be
from ._backend import Term, ptr, require

EPS = 1e-7   # least_squares.solve default (reference dprox/proxfn/sum_square.py:115)


# ----------------------------------------------------------------------------------------------
# cached tables / workspaces
# ----------------------------------------------------------------------------------------------
_tables = {}
_workspaces = {}


def _bytes(n, device, zero=False):
    """the one allocation of every buffer whose size a ``*_bytes`` query of the C ABI reports (uint8; callers that need another
    element type take ``.view(dtype)``) -- and the one hook tests/guarded_alloc.py substitutes"""
    return (torch.zeros if zero else torch.empty)(max(int(n), 16), dtype=torch.uint8, device=device)


def fft_table(H, W, device):
    key = (str(device), H, W)
    t = _tables.get(key)
    if t is None:
        L = be.lib()
        t = _bytes(L.query("dpx_fft_table_bytes", H, W), device)
        L.call("dpx_fft_table_init", ptr(t), H, W, be.stream())
        _tables[key] = t
    return t


_zero_scalars = {}


def zero_scalar(device):
    """a cached 0-d zero on ``device`` (a stand-in for an absent offset in the differentiable path: never written)"""
    key = str(device)
    if key not in _zero_scalars:
        _zero_scalars[key] = torch.zeros((), device=device)
    return _zero_scalars[key]


def workspace(tag, nbytes, device):
    key = (str(device), tag)
    w = _workspaces.get(key)
    if w is None or w.numel() < nbytes:
        w = _bytes(nbytes, device)
        _workspaces[key] = w
    return w


def spectrum_ws(P, H, W, device):
    return workspace("spectrum", be.lib().query("dpx_spectrum_bytes", P, H, W), device)


def clear_caches():
    _tables.clear()
    _workspaces.clear()
    _psf_dev.clear()
    _dd_cache.clear()
    _doe_contexts.clear()


def _shape4(x):
    if x.ndim != 4:
        raise be.DpxError(f"expected an NCHW tensor, got shape {tuple(x.shape)}")
    return tuple(int(s) for s in x.shape)


def as_batch_vec(v, B, device):
    """scalar / 0-d / [B] / [B,1,1,1] -> contiguous float32 [B] on device."""
    if not isinstance(v, torch.Tensor):
        v = torch.tensor(float(v))
    v = v.detach().to(device=device, dtype=torch.float32).reshape(-1)
    if v.numel() == 1:
        v = v.expand(B)
    elif v.numel() != B:
        raise be.DpxError(f"per-image scalar has {v.numel()} entries for a batch of {B}")
    return v.contiguous()


# ----------------------------------------------------------------------------------------------
# OTF tables
# ----------------------------------------------------------------------------------------------
_psf_dev = {}           # (kernel bytes, shape, device) -> fp64 device copy: a kernel is uploaded once, not once per table built from it


def psf_to_device(psf, device):
    """kernel (2-D, or HWC 3-D) -> contiguous fp64 [kh,kw,kc] on device."""
    k = np.asarray(psf, dtype=np.float64)
    if k.ndim == 1:
        k = k[None, :, None]
    elif k.ndim == 2:
        k = k[:, :, None]
    elif k.ndim != 3:
        raise ValueError(f"kernel must be 1-D, 2-D or HWC 3-D, got shape {k.shape}")
    k = np.ascontiguousarray(k)
    if k.nbytes <= 1 << 16:
        key = (k.tobytes(), k.shape, str(device))
        hit = _psf_dev.get(key)
        if hit is None:
            if len(_psf_dev) >= 64:
                _psf_dev.pop(next(iter(_psf_dev)))
            hit = _psf_dev[key] = torch.from_numpy(k).to(device)     # (a pageable upload blocks the host behind everything queued: once)
        return hit, k.shape
    return torch.from_numpy(k).to(device), k.shape


def make_otf(psf, C, H, W, device):
    """complex OTF table for dpx_fft_conv (opaque layout)."""
    L = be.lib()
    kd, (kh, kw, kc) = psf_to_device(psf, device)
    if kh > H or kw > W or kc > C:
        raise ValueError(f"outsize {[H, W, C]} cannot be smaller than the PSF array size {[kh, kw, kc]} in any dimension.")
    otf = _bytes(L.query("dpx_otf_bytes", C, H, W), device)
    L.call("dpx_psf2otf", ptr(kd), kh, kw, kc, C, H, W, ptr(otf), None, c_float(1.0), 0, be.stream())
    return otf


def new_diag(C, H, W, device):
    return _bytes(be.lib().query("dpx_diag_bytes", C, H, W), device, zero=True).view(torch.float32)


def accumulate_diag(diag, psf, weight, C, H, W):
    """diag += weight * |OTF(psf)|^2"""
    L = be.lib()
    kd, (kh, kw, kc) = psf_to_device(psf, diag.device)
    L.call("dpx_psf2otf", ptr(kd), kh, kw, kc, C, H, W, None, ptr(diag), c_float(weight), 1, be.stream())
    return diag


def diag_to_full(diag, C, H, W):
    """opaque diag table -> full [1,C,H,W] |OTF|^2 array on the table's device (setup-time interop)"""
    full = torch.empty(1, C, H, W, dtype=torch.float32, device=diag.device)
    be.lib().call("dpx_table_to_full", ptr(diag), ptr(full), C, H, W, be.stream())
    return full


def otf_from_full(full, C, H, W):
    """complex64 OTF on the full grid [.., C, H, W] -> opaque half-spectrum OTF table for fft_conv"""
    f = full.reshape(-1, C, H, W)[0].to(torch.complex64).contiguous()
    require(f, dtype=torch.complex64, what="full OTF")
    tab = _bytes(be.lib().query("dpx_otf_bytes", C, H, W), f.device)
    be.lib().call("dpx_otf_from_full", ptr(f), ptr(tab), C, H, W, be.stream())
    return tab


def diag_from_full(full, C, H, W, device):
    """full-spectrum real diagonal [.., C, H, W] -> opaque table (user-supplied BlackBox diagonals)"""
    f = torch.as_tensor(full).real.float().reshape(-1, C, H, W)[0].contiguous().to(device)
    tab = new_diag(C, H, W, device)
    be.lib().call("dpx_table_from_full", ptr(f), ptr(tab), C, H, W, be.stream())
    return tab


_dd_cache = {}


def denominator(d0, c0, d1, c1, C, H, W, device):
    """interleaved (d0 + c0, d1 + c1) table for fourier_solve; cached on the identity of its inputs"""
    key = (None if d0 is None else (d0.data_ptr(), d0._version), float(c0), None if d1 is None else (d1.data_ptr(), d1._version),
           float(c1), C, H, W, str(device))
    hit = _dd_cache.get(key)
    if hit is None:
        L = be.lib()
        dd = _bytes(L.query("dpx_denominator_bytes", C, H, W), device)
        L.call("dpx_denominator_pack", ptr(d0), c_float(c0), ptr(d1), c_float(c1), ptr(dd), C, H, W, be.stream())
        if len(_dd_cache) > 64:
            _dd_cache.clear()
        hit = (dd, d0, d1)            # keep the sources alive so data_ptr keys stay unique
        _dd_cache[key] = hit
    return hit[0]


# ----------------------------------------------------------------------------------------------
# Fourier-domain operators
# ----------------------------------------------------------------------------------------------
def fft_conv(x, otf, conj=False, out=None):
    require(x, what="fft_conv input")
    B, C, H, W = _shape4(x)
    y = torch.empty_like(x) if out is None else out
    be.lib().call("dpx_fft_conv", ptr(x), ptr(y), ptr(otf), int(bool(conj)), B, C, H, W,
                  ptr(fft_table(H, W, x.device)), ptr(spectrum_ws(B * C, H, W, x.device)), be.stream())
    return y


def pgd_supported(H, W, kind):
    return bool(be.lib().query("dpx_pgd_supported", int(H), int(W), int(kind)))


def pgd_run(x, ktb, gram_otf, kind, alpha, rho_tab, lam_tab, T, ws=None):
    """T fused proximal-gradient iterations on x, in place (two kernels per iteration; rho_tab / lam_tab: [T, B] device tables).
    ws: a spectrum workspace of the caller's (concurrent calls on different streams must not share the cached one)"""
    require(x, what="pgd iterate")
    B, C, H, W = _shape4(x)
    if ws is None:
        ws = spectrum_ws(B * C, H, W, x.device)
    be.lib().call("dpx_pgd_run", ptr(x), ptr(ktb), ptr(gram_otf), int(kind), c_float(alpha), ptr(rho_tab), ptr(lam_tab), int(T),
                  B, C, H, W, ptr(fft_table(H, W, x.device)), ptr(ws), be.stream())
    return x


def data_spectrum(b, otf=None, conj=True, out=None, accumulate=False):
    """packed fp32 half spectrum of op(OTF) * F(b), transform evaluated in fp64 (once per solve)"""
    require(b, what="data_spectrum input")
    B, C, H, W = _shape4(b)
    L = be.lib()
    if out is None:
        out = _bytes(L.query("dpx_spectrum_bytes", B * C, H, W) // 2, b.device)
        accumulate = False
    ws = workspace("data_spectrum", L.query("dpx_data_spectrum_ws_bytes", B * C, H, W), b.device)
    L.call("dpx_data_spectrum", ptr(b), ptr(otf), int(bool(conj)), ptr(out), int(bool(accumulate)), B, C, H, W, ptr(ws), be.stream())
    return out


def fourier_solve(rhs, d0, d1, c0, c1, rho, eps=EPS, out=None, spec_add=None):
    require(rhs, what="fourier_solve rhs")
    B, C, H, W = _shape4(rhs)
    rho = as_batch_vec(rho, B, rhs.device)
    x = torch.empty_like(rhs) if out is None else out
    dd = denominator(d0, c0, d1, c1, C, H, W, rhs.device)
    be.lib().call("dpx_fourier_solve", ptr(rhs), ptr(x), ptr(spec_add), ptr(dd), ptr(rho),
                  c_float(eps), B, C, H, W, ptr(fft_table(H, W, rhs.device)),
                  ptr(spectrum_ws(B * C, H, W, rhs.device)), be.stream())
    return x


def fourier_apply_inv(g, d0, d1, c0, c1, rho, eps=EPS):
    """irFFT2[rFFT2(g) / (d0 + c0 + rho (d1 + c1) + eps)]: the self-adjoint linear part of fourier_solve (its backward)"""
    require(g, what="fourier_apply_inv input")
    B, C, H, W = _shape4(g)
    rho = as_batch_vec(rho, B, g.device)
    out = torch.empty_like(g)
    dd = denominator(d0, c0, d1, c1, C, H, W, g.device)
    be.lib().call("dpx_fourier_apply_inv", ptr(g), ptr(out), ptr(dd), ptr(rho), c_float(eps), B, C, H, W,
                  ptr(fft_table(H, W, g.device)), ptr(spectrum_ws(B * C, H, W, g.device)), be.stream())
    return out


def prox_bwd(kind, d, g, lam, alpha=1.0, off=None, want_dlam=True):
    """(J(d)^T g, d prox / d lam at d) of ops.prox -- see dpx_prox_bwd"""
    require(d, what="prox_bwd point")
    require(g, what="prox_bwd gradient")
    B = int(d.shape[0])
    npb = d.numel() // max(B, 1)
    lam_v = as_batch_vec(lam, B, d.device)
    gd = torch.empty_like(d)
    dl = torch.empty_like(d) if want_dlam else None
    be.lib().call("dpx_prox_bwd", int(kind), ptr(d), ptr(g), ptr(gd), ptr(dl), ptr(lam_v), c_float(alpha), ptr(off), B, npb, be.stream())
    return gd, dl


# ----------------------------------------------------------------------------------------------
# spatial / elementwise
# ----------------------------------------------------------------------------------------------
def grad(x, dim, adjoint=False):
    require(x, what="grad input")
    B, C, H, W = _shape4(x)
    y = torch.empty_like(x)
    be.lib().call("dpx_grad", ptr(x), ptr(y), int(dim), int(bool(adjoint)), B, C, H, W, be.stream())
    return y


def _flat_real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def lincomb(terms, out=None):
    """out = sum_i coef_i * x_i, terms = [(coef, x)] with coef a python float or a per-image [B] tensor.
    Real fp32 tensors, or complex64 tensors with real coefficients (handled as interleaved floats)."""
    xs = [t[1] for t in terms]
    ref = xs[0]
    if ref.dtype == torch.float64:
        return _lincomb_f64(terms, out)
    cplx = ref.is_complex()
    for x in xs:
        require(x, dtype=torch.complex64 if cplx else torch.float32, what="lincomb operand")
        if x.shape != ref.shape:
            raise be.DpxError(f"lincomb: shape mismatch {tuple(x.shape)} vs {tuple(ref.shape)}")
    res = torch.empty_like(ref) if out is None else out
    B = int(ref.shape[0]) if ref.ndim > 0 else 1
    npb = (ref.numel() // max(B, 1)) * (2 if cplx else 1)
    if ref.numel() == 0:
        return res
    i, first = 0, True
    while i < len(terms):
        take = 4 if first else 3
        ops = ([] if first else [(1.0, res)]) + list(terms[i:i + take])
        i += take
        first = False
        n = len(ops)
        px = (c_void_p * n)(*[_flat_real(o[1]).data_ptr() for o in ops])
        cf = (c_float * n)()
        pb = (c_void_p * n)()
        keep = []
        for j, (c, _) in enumerate(ops):
            if isinstance(c, torch.Tensor) and c.numel() > 1:
                cb = as_batch_vec(c, B, ref.device)
                keep.append(cb)
                cf[j] = 1.0
                pb[j] = cb.data_ptr()
            else:
                cf[j] = float(c)
                pb[j] = None
        be.lib().call("dpx_lincomb", ptr(_flat_real(res)), n, px, cf, pb, B, npb, be.stream())
    return res


def _lincomb_f64(terms, out=None):
    """float64 operands (the Krylov solvers keep a float64 system in float64): dpx_lincomb_f64"""
    ref = terms[0][1]
    for _, x in terms:
        require(x, dtype=torch.float64, what="lincomb operand")
        if x.shape != ref.shape:
            raise be.DpxError(f"lincomb: shape mismatch {tuple(x.shape)} vs {tuple(ref.shape)}")
    res = torch.empty_like(ref) if out is None else out
    if ref.numel() == 0:
        return res
    B = int(ref.shape[0]) if ref.ndim > 0 else 1
    npb = ref.numel() // max(B, 1)
    i, first = 0, True
    while i < len(terms):
        take = 4 if first else 3
        grp = ([] if first else [(1.0, res)]) + list(terms[i:i + take])
        i += take
        first = False
        n = len(grp)
        px = (c_void_p * n)(*[o[1].data_ptr() for o in grp])
        cf, pb, keep = (c_double * n)(), (c_void_p * n)(), []
        for j, (c, _) in enumerate(grp):
            if isinstance(c, torch.Tensor) and c.numel() > 1:
                cb = c.detach().to(device=ref.device, dtype=torch.float64).reshape(-1).contiguous()
                if cb.numel() != B:
                    raise be.DpxError(f"per-image scalar has {cb.numel()} entries for a batch of {B}")
                keep.append(cb)
                cf[j], pb[j] = 1.0, cb.data_ptr()
            else:
                cf[j], pb[j] = float(c), None
        be.lib().call("dpx_lincomb_f64", ptr(res), n, px, cf, pb, B, npb, be.stream())
    return res


def absmax(x):
    """max |x| over all elements (float32 or float64) as a 0-d tensor on x's device -- pcg's stop rule"""
    f64 = x.dtype == torch.float64
    require(x, dtype=torch.float64 if f64 else torch.float32, what="absmax operand")
    out = torch.empty((), dtype=x.dtype, device=x.device)
    ws = workspace("absmax", 256 * 8, x.device)
    be.lib().call("dpx_absmax", ptr(x), ptr(out), x.numel(), 1 if f64 else 0, ptr(ws), be.stream())
    return out


def _f64_or_f32(t):
    """(element type, C symbol suffix, workspace tag) of the float64 or the float32 dot / Gram kernels"""
    return (torch.float64, "_f64", "dot64") if t.dtype == torch.float64 else (torch.float32, "", "dot")


def bdot(x, y):
    dtype, sfx, tag = _f64_or_f32(x)
    require(x, dtype=dtype, what="bdot x"), require(y, dtype=dtype, what="bdot y")
    B = int(x.shape[0])
    npb = x.numel() // B
    L = be.lib()
    out = torch.empty(B, dtype=dtype, device=x.device)
    ws = workspace(tag, L.query(f"dpx_bdot{sfx}_ws_bytes", B, npb), x.device)
    L.call(f"dpx_bdot{sfx}", ptr(x), ptr(y), ptr(out), B, npb, ptr(ws), be.stream())
    return out


def bgram(r):
    dtype, sfx, tag = _f64_or_f32(r)
    require(r, dtype=dtype, what="bgram r")
    B = int(r.shape[0])
    npb = r.numel() // B
    L = be.lib()
    out = torch.empty(B, B, dtype=dtype, device=r.device)
    ws = workspace(tag, L.query(f"dpx_bdot{sfx}_ws_bytes", B, npb), r.device)
    L.call(f"dpx_bgram{sfx}", ptr(r), ptr(out), B, npb, ptr(ws), be.stream())
    return out


ANDERSON_MAX_M = 8


class AndersonHistory:
    """The piece-major history of an Anderson solve (dpx_anderson_gram_row / dpx_anderson_mix): ``F`` and ``G = F - X`` are
    [m, P, B, *piece] (m slots of P pieces; ``F[slot, p]`` is a contiguous image stack an iteration kernel writes directly), ``X``
    [P, B, *piece] is the point the next evaluation of f starts from, ``Hm`` [B, m, m] the Gram matrices kept across steps."""

    def __init__(self, m, P, B, piece_shape, device):
        if not 1 <= int(m) <= ANDERSON_MAX_M:
            raise be.DpxError(f"anderson: history of m={m} slots (1 .. {ANDERSON_MAX_M})")
        if not be.host_mode() and torch.device(device).type != "cuda":
            raise be.DpxError(f"anderson history on {device}: the MI355X backend only runs on HIP devices (no CPU fallback)")
        self.m, self.P, self.B = int(m), int(P), int(B)
        piece_shape = tuple(int(s) for s in piece_shape)
        self.D = int(np.prod(piece_shape))
        if self.P < 1 or self.B < 1 or self.D < 1:
            raise be.DpxError(f"anderson: empty state (P={P}, B={B}, piece {piece_shape})")
        f32 = dict(dtype=torch.float32, device=device)
        self.F = torch.empty((self.m, self.P, self.B) + piece_shape, **f32)
        self.G = torch.empty_like(self.F)
        self.X = torch.empty((self.P, self.B) + piece_shape, **f32)
        self.Hm = torch.zeros(self.B, self.m, self.m, **f32)
        self.nrm = torch.zeros(self.B, 2, **f32)
        self._alpha = torch.zeros(self.B * self.m, **f32)
        # (the reduction's tickets live at the head of the workspace and must start from zero: not the shared scratch of workspace())
        self.ws = _bytes(be.lib().query("dpx_anderson_ws_bytes", self.B, self.P, self.D), device, zero=True)

    def gram_row(self, ks, n, X=None):
        """after f(X) has been written into slot ``ks`` of F: G[ks] = F[ks] - X, row / column ks of Hm over the slots j < n, and
        nrm[b] = (|G_ks|^2, |F_ks|^2).  ``X``: the point f was evaluated at when it is not ``self.X`` (another slot of F, say)"""
        X = self.X if X is None else require(X, what="anderson point")
        if X.numel() != self.X.numel():
            raise be.DpxError(f"anderson: point of shape {tuple(X.shape)} for a state of shape {tuple(self.X.shape)}")
        be.lib().call("dpx_anderson_gram_row", ptr(X), ptr(self.F), ptr(self.G), ptr(self.Hm), ptr(self.nrm), int(ks), int(n), self.m, self.P,
                      self.B, self.D, ptr(self.ws), be.stream())
        return self.nrm

    def mix(self, n, beta=1.0, lam=1e-4):
        """X = beta sum_i alpha_i F_i + (1 - beta) sum_i alpha_i X_i over the slots i < n; returns alpha [B, n]"""
        be.lib().call("dpx_anderson_mix", ptr(self.F), ptr(self.G), ptr(self.Hm), ptr(self.X), ptr(self._alpha), int(n), self.m, c_float(beta),
                      c_float(lam), self.P, self.B, self.D, be.stream())
        return self._alpha[:self.B * int(n)].view(self.B, int(n))


def cg_masked_fft(b, mask, rho, n_identity, rtol, max_iters):
    """the whole CG x-update of a masked-Fourier data term in one C call (dpx_cg_masked_fft); returns (x, exit iteration)"""
    require(b, what="cg right-hand side")
    B = int(b.shape[0])
    H, W = int(b.shape[-2]), int(b.shape[-1])
    assert b.numel() == B * H * W, "one plane per system"
    mask = mask.to(device=b.device, dtype=torch.float32).contiguous()
    mimg = B if mask.numel() == b.numel() else 1
    assert mask.numel() == mimg * H * W
    L = be.lib()
    x = torch.empty_like(b)
    ws = workspace("cg_masked_fft", L.query("dpx_cg_masked_fft_ws_bytes", B, H, W, mimg), b.device)
    n = L.query("dpx_cg_masked_fft", ptr(x), ptr(b), ptr(mask), mimg, ptr(as_batch_vec(rho, B, b.device)), c_float(n_identity), c_float(rtol),
                int(max_iters), B, H, W, ptr(fft_table(H, W, b.device)), ptr(ws), be.stream())
    if n < 0:
        raise be.DpxError(f"dpx_cg_masked_fft failed ({n}): {L.cdll.dpx_last_error().decode()}")
    return x, int(n)


def zeros_like(t):
    """torch.zeros_like through the C ABI's stream memset"""
    out = torch.empty_like(t)
    if be.host_mode():
        return out.zero_()
    be.lib().call("dpx_zero", ptr(out), out.numel() * out.element_size(), be.stream())
    return out


class CgControl:
    """device-resident control block of one cg() solve (dpx_cg_*): stop rule, beta / alpha and the iterate updates run on the
    GPU; the host only issues kernels and polls the `done` flag without blocking"""

    MAX_B = 64

    def __init__(self, b, rtol):
        L = be.lib()
        self.B = int(b.shape[0])
        self.npb = b.numel() // self.B
        self.dev = b.device
        self.state = _bytes(L.query("dpx_cg_state_bytes", self.B), b.device).view(torch.float32)
        self.flags = self.state[5 * self.B:].view(torch.int32)                  # done, n_done, it, pad
        self.pAp = self.state[3 * self.B:4 * self.B]
        self.gram = torch.empty(self.B, self.B, dtype=torch.float32, device=b.device)
        self.ws = workspace("dot", L.query("dpx_bdot_ws_bytes", self.B, self.npb), b.device)
        self.bnorm2 = bdot(b, b)                                                # <b_i, b_i> (kept alive: the call below is asynchronous)
        L.call("dpx_cg_init", ptr(self.state), ptr(self.bnorm2), c_float(rtol), self.B, be.stream())

    def test(self, r):
        L = be.lib()
        L.call("dpx_bgram", ptr(r), ptr(self.gram), self.B, self.npb, ptr(self.ws), be.stream())
        L.call("dpx_cg_test", ptr(self.state), ptr(self.gram), self.B, be.stream())

    def direction(self, p, r):
        be.lib().call("dpx_cg_direction", ptr(p), ptr(r), ptr(self.state), self.B, self.npb, be.stream())

    def update(self, x, r, p, Ap):
        L = be.lib()
        L.call("dpx_bdot", ptr(p), ptr(Ap), ptr(self.pAp), self.B, self.npb, ptr(self.ws), be.stream())
        L.call("dpx_cg_update", ptr(x), ptr(r), ptr(p), ptr(Ap), ptr(self.state), self.B, self.npb, be.stream())


class MinresControl:
    """device-resident state of one minres() solve (dpx_minres_*): vectors are [G, N, K] (G leading systems, K contiguous columns,
    every dot product per (g, k)), float32 or float64.  ``zring`` [2, G, N, K] is the ring of Lanczos vectors, ``search``
    [2, S, G, N, K] the ring of search vectors, ``solution`` [S, G, N, K]; the scalars of every (shift, system) pair and the step
    counter live in ``state`` (float64), and which slot of a ring is "prev" or "curr" follows from that counter on the device --
    the host only issues launches.  ``fields()`` names the state's parts."""

    def __init__(self, b, shifts, value=None, eps=1e-25):
        if b.ndim != 3 or b.numel() == 0:
            raise be.DpxError(f"minres: right-hand side of shape {tuple(b.shape)} (expected a non-empty [G, N, K])")
        self.f64 = b.dtype == torch.float64
        require(b, dtype=b.dtype if self.f64 else torch.float32, what="minres right-hand side")
        self.G, self.N, self.K = (int(s) for s in b.shape)
        shifts = shifts.detach().reshape(-1).to(device=b.device, dtype=torch.float64)
        self.S = int(shifts.numel())
        if self.S < 1:
            raise be.DpxError("minres: empty shifts")
        self.value = 1.0 if value is None else float(value)
        self.eps = float(eps)
        L = be.lib()
        self.state = _bytes(L.query("dpx_minres_state_bytes", self.S, self.G, self.K), b.device, zero=True).view(torch.float64)
        # (the reductions' tickets live at the head of the workspace and must start from zero: not the shared scratch of workspace())
        self.ws = _bytes(L.query("dpx_minres_ws_bytes", self.G, self.N, self.K), b.device, zero=True)
        self.fields()["shifts"].copy_(shifts)
        kw = dict(dtype=b.dtype, device=b.device)
        self.zring = torch.zeros((2,) + tuple(b.shape), **kw)
        self.search = torch.zeros((2, self.S) + tuple(b.shape), **kw)
        self.solution = torch.zeros((self.S,) + tuple(b.shape), **kw)
        self._dims = (self.S, self.G, self.N, self.K, 1 if self.f64 else 0)

    def fields(self):
        """views into the state block: alpha [G, K], beta [2, G, K], norm, zero [G, K], cos, sin [3, S, G, K], subsub, sub, diag
        [S, G, K], scale [2, S, G, K], shifts [S], step (int64 [1])"""
        S, G, K = self.S, self.G, self.K
        out, off = {}, 0
        for name, shape in (("alpha", (G, K)), ("beta", (2, G, K)), ("norm", (G, K)), ("zero", (G, K)), ("cos", (3, S, G, K)),
                            ("sin", (3, S, G, K)), ("subsub", (S, G, K)), ("sub", (S, G, K)), ("diag", (S, G, K)),
                            ("scale", (2, S, G, K)), ("shifts", (S,)), ("step", (1,))):
            n = int(np.prod(shape))
            out[name] = self.state[off:off + n].view(shape)
            off += n
        out["step"] = out["step"].view(torch.int64)
        return out

    def _vec(self, t, what, shape=None):
        require(t, dtype=torch.float64 if self.f64 else torch.float32, what=what)
        if tuple(t.shape) != (shape or (self.G, self.N, self.K)):
            raise be.DpxError(f"minres: {what} of shape {tuple(t.shape)} for systems of shape {(self.G, self.N, self.K)}")
        return t

    def init(self, phase):
        be.lib().call("dpx_minres_init", ptr(self.state), int(phase), self.S, self.G, self.K, be.stream())

    def colscale(self, out, inp, mode):
        """per system: mode 0 out = inp / norm, 1 out = inp / beta[0], 2 out = 0 where the right-hand side vanished, else inp * norm"""
        be.lib().call("dpx_minres_colscale", ptr(self._vec(out, "output")), ptr(self._vec(inp, "input")), ptr(self.state), int(mode),
                      *self._dims, be.stream())

    def alpha(self, prod, q=None, value=None):
        """alpha = value <prod, q> per system; ``q=None``: the ring's previous vector (the identity preconditioner's q)"""
        q = None if q is None else self._vec(q, "q")
        be.lib().call("dpx_minres_alpha", ptr(self._vec(prod, "operator product")), ptr(q), ptr(self.zring),
                      c_double(self.value if value is None else value), ptr(self.state), *self._dims, ptr(self.ws), be.stream())

    def lanczos(self, prod, finish=True):
        be.lib().call("dpx_minres_lanczos", ptr(self._vec(prod, "operator product")), ptr(self.zring), c_double(self.value), c_double(self.eps),
                      1 if finish else 0, ptr(self.state), *self._dims, ptr(self.ws), be.stream())

    def beta(self, qc):
        be.lib().call("dpx_minres_beta", ptr(self.zring), ptr(self._vec(qc, "preconditioned vector")), c_double(self.eps), ptr(self.state),
                      *self._dims, ptr(self.ws), be.stream())

    def update(self, q=None, qc=None):
        q = None if q is None else self._vec(q, "q")
        qc = None if qc is None else self._vec(qc, "preconditioned vector")
        be.lib().call("dpx_minres_update", ptr(self.zring), ptr(q), ptr(qc), ptr(self.search), ptr(self.solution), ptr(self.state), *self._dims,
                      ptr(self.ws), be.stream())


class LpControl:
    """device-resident state of one LPSolverADMM.solve (dpx_lp_*, csrc/dpx_lp.hip): the two CSR copies of the scaled constraint
    matrix, the ADMM iterates x, xt, z, y, the PCG vectors and the state block; the host only issues launches and reads the state
    block where the reference synchronises too.  Everything is float64; the inputs are NumPy arrays (``csr`` = (indptr, indices,
    data), validated by the caller).  ``fields()`` names the state's parts; ``launches`` counts the kernels issued."""
    TABLE = ("a_ptr", "a_idx", "a_val", "at_ptr", "at_idx", "at_val", "x", "xt", "z", "y", "t", "c", "acn", "right", "r", "yv", "p", "Ap",
             "lb", "ub", "d", "e", "state", "ws")
    MAX_INNER = 1000                       # the reference's pcg(..., max_iters=int(1e3))

    def __init__(self, csr_a, csr_at, m, n, c, acn, lb, ub, d, e, device):
        self.m, self.n, self.nnz = int(m), int(n), int(len(csr_a[2]))
        dev = torch.device(device)
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        b = {}
        for tag, (indptr, indices, data), rows in (("a", csr_a, self.m), ("at", csr_at, self.n)):
            if len(indptr) != rows + 1 or len(indices) != self.nnz or len(data) != self.nnz or self.nnz > 2 ** 31 - 65:
                raise be.DpxError(f"lp: CSR arrays of lengths {len(indptr)}, {len(indices)}, {len(data)} for {rows} rows and {self.nnz} entries")
            b[f"{tag}_ptr"], b[f"{tag}_idx"], b[f"{tag}_val"] = put(indptr, np.int32), put(indices, np.int32), put(data, np.float64)
        for name, a, length in (("c", c, n), ("acn", acn, n), ("d", d, n), ("lb", lb, m), ("ub", ub, m), ("e", e, m)):
            if np.shape(a) != (length,):
                raise be.DpxError(f"lp: {name} of shape {np.shape(a)} (expected ({length},))")
            b[name] = put(a, np.float64)
        for name, length in (("x", n), ("xt", n), ("right", n), ("r", n), ("yv", n), ("p", 2 * n), ("Ap", n), ("z", m), ("y", m), ("t", m)):
            b[name] = torch.zeros(length, dtype=torch.float64, device=dev)
        L = be.lib()
        b["state"] = _bytes(L.query("dpx_lp_state_bytes"), dev, zero=True)
        # (the reductions' ticket lives at the head of the workspace and must start from zero: not the shared scratch of workspace())
        b["ws"] = _bytes(L.query("dpx_lp_ws_bytes", self.m, self.n), dev, zero=True)
        for t in b.values():
            require(t, dtype=None, what="lp buffer")
        self.buf = b
        self.tab = (c_void_p * len(self.TABLE))(*[b[k].data_ptr() for k in self.TABLE])
        self._dims = (self.m, self.n, self.nnz)
        self.words = b["state"][14 * 8:17 * 8].view(torch.int64)          # done, inner, ops
        self.launches = 0

    def __getattr__(self, name):
        buf = self.__dict__.get("buf", {})
        if name in buf:
            return buf[name]
        raise AttributeError(name)

    def fields(self):
        """views into the state block: ry, a, beta, rtol, pAp, rmax (float64 [1]), eval (float64 [8]: objval, r_norm, s_norm, |A x|,
        |z|, |AT y|, |c|, |z - clip(z)|), done, inner, ops (int64 [1])"""
        f64 = self.buf["state"][:14 * 8].view(torch.float64)
        out = {k: f64[i:i + 1] for i, k in enumerate(("ry", "a", "beta", "rtol", "pAp", "rmax"))}
        out["eval"] = f64[6:14]
        out.update({k: self.words[i:i + 1] for i, k in enumerate(("done", "inner", "ops"))})
        return out

    def lanes(self):
        """(lanes per row of A, of AT) the kernels use now"""
        L = be.lib()
        return L.query("dpx_lp_lanes", self.m, self.nnz), L.query("dpx_lp_lanes", self.n, self.nnz)

    def spmv(self, which, v, reps=1):
        """A v (``which`` = "a", v [n]) or AT v ("at", v [m]): the plain row product (``reps``: issued that often from one call)"""
        rows, cols = (self.m, self.n) if which == "a" else (self.n, self.m)
        require(v, dtype=torch.float64, what="lp vector")
        if tuple(v.shape) != (cols,):
            raise be.DpxError(f"lp: a vector of shape {tuple(v.shape)} for a matrix with {cols} columns")
        out = torch.empty(rows, dtype=torch.float64, device=v.device)
        b = self.buf
        be.lib().call("dpx_lp_spmv_chain", ptr(out), ptr(b[f"{which}_ptr"]), ptr(b[f"{which}_idx"]), ptr(b[f"{which}_val"]), ptr(v), rows, self.nnz,
                      int(reps), be.stream())
        self.launches += int(reps)
        return out

    def pcg_start(self, rho, sigma, rtol):
        be.lib().call("dpx_lp_pcg_start", self.tab, *self._dims, c_double(rho), c_double(sigma), c_double(rtol), be.stream())
        self.launches += 1

    def pcg_iters(self, rho, sigma, iters=1):
        be.lib().call("dpx_lp_pcg_iters", self.tab, *self._dims, c_double(rho), c_double(sigma), self.MAX_INNER, int(iters), be.stream())
        self.launches += int(iters) * (4 if be.tune_get("lp_split_direction") else 3)

    def tail(self, alpha, rho):
        be.lib().call("dpx_lp_tail", self.tab, *self._dims, c_double(alpha), c_double(rho), be.stream())
        self.launches += 1

    def eval(self, gamma_c, gamma_b):
        be.lib().call("dpx_lp_eval", self.tab, *self._dims, c_double(gamma_c), c_double(gamma_b), be.stream())
        self.launches += 2


def prox(kind, v, lam, alpha=1.0, off=None, out=None):
    require(v, what="prox input")
    B = int(v.shape[0])
    npb = v.numel() // B
    lam_v = None if lam is None else as_batch_vec(lam, B, v.device)
    if off is not None:
        off = require(off.expand_as(v).contiguous(), what="prox offset")
    res = torch.empty_like(v) if out is None else out
    be.lib().call("dpx_prox", int(kind), ptr(v), ptr(res), ptr(lam_v), c_float(alpha), ptr(off), B, npb, be.stream())
    return res


def _bwd_ws(B, C, H, W, device):
    return workspace("admm_bwd", be.lib().query("dpx_admm_bwd_ws_bytes", B, C, H, W), device)


def admm_zupdate_bwd(specs, shape, device):
    """specs: dict(linop, prox, alpha, lam[B], v, gv|None, gu_new|None) per term -> (gx, [gu_i], [glam_i [B]])"""
    B, C, H, W = shape
    n = len(specs)
    arr = (be.BwdTerm * n)()
    gus = [torch.empty(shape, dtype=torch.float32, device=device) for _ in specs]
    keep = []
    for i, s_ in enumerate(specs):
        arr[i].linop, arr[i].prox, arr[i].alpha = s_["linop"], s_["prox"], float(s_.get("alpha", 1.0))
        for name in ("lam", "v", "gv", "gu_new"):
            t = s_.get(name)
            if t is not None:
                t = t.contiguous()
                keep.append(t)
            setattr(arr[i], name, None if t is None else t.data_ptr())
        arr[i].gu = gus[i].data_ptr()
    gx = torch.empty(shape, dtype=torch.float32, device=device)
    glam = torch.empty(n, B, dtype=torch.float32, device=device)
    be.lib().call("dpx_admm_zupdate_bwd", ptr(gx), arr, n, ptr(glam), B, C, H, W, ptr(_bwd_ws(B, C, H, W, device)), be.stream())
    return gx, gus, [glam[i] for i in range(n)]


def admm_solve_rho_grad(g_rhs, x, linops):
    B, C, H, W = _shape4(x)
    n = len(linops)
    codes = (ctypes.c_int * max(n, 1))(*linops)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    be.lib().call("dpx_admm_solve_rho_grad", ptr(g_rhs.contiguous()), ptr(x.contiguous()), codes, n, ptr(out), B, C, H, W,
                  ptr(_bwd_ws(B, C, H, W, x.device)), be.stream())
    return out


def admm_rhs_bwd(g, rhs, rho, linops, want_v=True, want_u=True):
    B, C, H, W = _shape4(g)
    n = len(linops)
    codes = (ctypes.c_int * n)(*linops)
    gv = [torch.empty_like(g) if want_v else None for _ in range(n)]
    gu = [torch.empty_like(g) if want_u else None for _ in range(n)]
    pv = (c_void_p * n)(*[None if t is None else t.data_ptr() for t in gv])
    pu = (c_void_p * n)(*[None if t is None else t.data_ptr() for t in gu])
    grho = torch.empty(B, dtype=torch.float32, device=g.device)
    be.lib().call("dpx_admm_rhs_bwd", ptr(g.contiguous()), ptr(rhs), ptr(rho.contiguous()), codes, n, pv, pu, ptr(grho), B, C, H, W,
                  ptr(_bwd_ws(B, C, H, W, g.device)), be.stream())
    return gv, gu, grho


def make_terms(specs):
    """specs: list of dict(linop, prox, alpha, lam[B] tensor or None, v, u) -> (ctypes array, keepalive)."""
    n = len(specs)
    if n > be.MAX_TERMS:
        raise be.DpxError(f"at most {be.MAX_TERMS} fused terms")
    arr = (Term * max(n, 1))()
    for i, s in enumerate(specs):
        arr[i].linop, arr[i].prox, arr[i].alpha = s["linop"], s["prox"], float(s.get("alpha", 1.0))
        arr[i].lam = None if s.get("lam") is None else s["lam"].data_ptr()
        arr[i].v, arr[i].u = s["v"].data_ptr(), s["u"].data_ptr()
        arr[i].u_out = None if s.get("u_out") is None else s["u_out"].data_ptr()
    return arr


def admm_rhs(rhs, ktb, rho, term_arr, nterms):
    B, C, H, W = _shape4(rhs)
    be.lib().call("dpx_admm_rhs", ptr(rhs), ptr(ktb), ptr(rho), term_arr, nterms, B, C, H, W, be.stream())
    return rhs


def split_rhs(rhs, ktb, x, rho, term_arr, nterms, mode):
    """rhs = ktb + rho sum_i K_i^T (x - K_i^T q_i): mode 0 Pock-Chambolle (q = z), 1 linearised ADMM (q = K x - v + u)"""
    B, C, H, W = _shape4(rhs)
    be.lib().call("dpx_split_rhs", ptr(rhs), ptr(ktb), ptr(x), ptr(rho), term_arr, nterms, int(mode), B, C, H, W, be.stream())
    return rhs


def pc_dual(xbar, term_arr, nterms):
    B, C, H, W = _shape4(xbar)
    be.lib().call("dpx_pc_dual", ptr(xbar), term_arr, nterms, B, C, H, W, be.stream())


def admm_pnp_iter(x, rhs, term_arr, nterms, ext, v_new, rho, sigma, spec_add, dd, eps, net):
    """one plug-and-play ADMM iteration in one C call (dpx_admm_pnp_iter); `net`: the FFDNet module of term `ext`"""
    B, C, H, W = _shape4(x)
    L = be.lib()
    mode = be.FFDNET_MODES[net.compute_mode]
    if mode in (3, 4):
        be.note_f16_launch()
    Bn = B if net.in_nc == C else B * C
    if mode == 0:
        packed = net.packed()
        ws = workspace("ffdnet", L.query("dpx_ffdnet_ws_bytes", Bn, net.in_nc, net.nc, H, W), x.device)
    else:
        packed = net.packed_bf16(mode)
        ws = workspace("ffdnet_bf16", L.query("dpx_ffdnet_bf16_ws_bytes", Bn, net.in_nc, net.nc, H, W), x.device)
    L.call("dpx_admm_pnp_iter", ptr(x), ptr(rhs), term_arr, nterms, int(ext), ptr(v_new), ptr(rho), ptr(sigma), ptr(spec_add), ptr(dd),
           c_float(eps), ptr(packed), net.in_nc, net.nc, net.nb, mode, B, C, H, W, ptr(fft_table(H, W, x.device)),
           ptr(spectrum_ws(B * C, H, W, x.device)), ptr(ws), be.stream())


class CgPnpIter:
    """One plug-and-play iteration with the masked-Fourier CG x-update in one C call (dpx_admm_cg_pnp_iter), set up once per run: everything
    that does not change between iterations (workspaces, packed weights, the table, the mask) is resolved here, the per-iteration call
    passes pointers only.  `net`: the gray FFDNet of term `ext`; x: [B, 1, H, W]."""

    def __init__(self, x, rhs, ktb, term_arr, nterms, ext, mask, n_identity, rtol, max_iters, net):
        B, C, H, W = _shape4(x)
        assert C == 1 and net.in_nc == 1
        L = be.lib()
        self.L = L
        self.mode = be.FFDNET_MODES[net.compute_mode]
        mask = mask.to(device=x.device, dtype=torch.float32).contiguous()
        mimg = B if mask.numel() == x.numel() else 1
        assert mask.numel() == mimg * H * W
        if self.mode == 0:
            packed = net.packed()
            ffd_ws = workspace("ffdnet", L.query("dpx_ffdnet_ws_bytes", B, net.in_nc, net.nc, H, W), x.device)
        else:
            packed = net.packed_bf16(self.mode)
            ffd_ws = workspace("ffdnet_bf16", L.query("dpx_ffdnet_bf16_ws_bytes", B, net.in_nc, net.nc, H, W), x.device)
        cg_ws = workspace("cg_masked_fft", L.query("dpx_cg_masked_fft_ws_bytes", B, H, W, mimg), x.device)
        self.keep = (mask, packed, ffd_ws, cg_ws, ktb, rhs, fft_table(H, W, x.device))
        self.fixed = (ptr(mask), mimg, c_float(n_identity), c_float(rtol), int(max_iters), ptr(packed), net.in_nc, net.nc, net.nb, self.mode, B, H, W,
                      ptr(self.keep[6]), ptr(cg_ws), ptr(ffd_ws))
        self.head = (ptr(rhs), ptr(ktb), term_arr, nterms, int(ext))
        self.folds = bool(L.query("dpx_admm_cg_pnp_iter_folds", self.mode, B))
        self.ready = False        # the previous call prepared this call's right-hand side

    def __call__(self, x, v_new, rho, sigma, rho_next=None, x_next=None, cg_hint=-1):
        """x (written), v_new (receives the denoised image); returns the CG exit iteration.  rho_next / x_next (self.folds only): the pass
        behind the denoiser also prepares the next call's right-hand side and CG start state (x_next zeroed: the next call's x) -- the next
        call then skips its rhs stage by itself"""
        if self.mode in (3, 4):
            be.note_f16_launch()
        L = self.L
        ready, self.ready = self.ready, rho_next is not None
        n = L.query("dpx_admm_cg_pnp_iter", ptr(x), *self.head, ptr(v_new), ptr(rho), ptr(sigma), *self.fixed, ptr(rho_next), ptr(x_next), int(ready),
                    int(cg_hint), be.stream())
        if n < 0:
            raise be.DpxError(f"dpx_admm_cg_pnp_iter failed ({n}): {L.cdll.dpx_last_error().decode()}")
        return int(n)


def admm_zupdate(x, term_arr, nterms):
    B, C, H, W = _shape4(x)
    be.lib().call("dpx_admm_zupdate", ptr(x), term_arr, nterms, B, C, H, W, be.stream())


def admm_zupdate_rhs(x, term_arr, nterms, rhs, rho_next, dual=True, emit_v=True, ktb=None):
    """z / dual update of this iteration and the right-hand side of the next one in one pass (dpx_admm_zupdate_rhs: every term's dual is
    double-buffered, u_out != u; emit_v=False: v is not stored -- the loop's last stage must be admm_zupdate)"""
    B, C, H, W = _shape4(x)
    be.lib().call("dpx_admm_zupdate_rhs", ptr(x), term_arr, nterms, ptr(rhs), ptr(ktb), ptr(rho_next), int(bool(dual)), int(bool(emit_v)), B, C, H, W, be.stream())


def iter_supported(H, W, term_arr, nterms):
    return bool(be.lib().query("dpx_admm_iter_supported", H, W, term_arr, nterms))


def spectrum_buffer(P, H, W, device):
    """one half-spectrum buffer (dpx_spectrum_bytes covers two)"""
    return _bytes(be.lib().query("dpx_spectrum_bytes", P, H, W) // 2, device)


def rfft_rows(x, spec):
    B, C, H, W = _shape4(x)
    be.lib().call("dpx_rfft_rows", ptr(x), ptr(spec), B, C, H, W, ptr(fft_table(H, W, x.device)), be.stream())


def iter_cols(spec_in, spec_out, spec_add, dd, rho, eps, shape, device):
    B, C, H, W = shape
    be.lib().call("dpx_admm_iter_cols", ptr(spec_in), ptr(spec_out), ptr(spec_add), ptr(dd), ptr(rho), c_float(eps),
                  B, C, H, W, ptr(fft_table(H, W, device)), be.stream())


def iter_rows(spec_in, spec_out, term_arr, nterms, rho_next, x_out, emit_v, shape, device):
    B, C, H, W = shape
    be.lib().call("dpx_admm_iter_rows", ptr(spec_in), ptr(spec_out), term_arr, nterms, ptr(rho_next), ptr(x_out),
                  int(bool(emit_v)), B, C, H, W, ptr(fft_table(H, W, device)), be.stream())


def admm_seed_rows(spec, rho, term_arr, nterms, shape, device, fresh_x=None, stream=None):
    """spec = row transform of rho_b sum_i K_i^T (v_i - u_i): the seed of admm_run in one pass.  ``fresh_x``: the state is
    ADMM.initialize(fresh_x) untouched (v_i = K_i x0, u_i = 0) -- the pass then reads x0 alone (bit-identical result).
    stream: a raw stream handle (default: the current stream)"""
    B, C, H, W = shape
    st = be.stream() if stream is None else stream
    if fresh_x is not None:
        be.lib().call("dpx_admm_seed_rows_fresh", ptr(spec), ptr(rho), ptr(fresh_x), term_arr, nterms, B, C, H, W, ptr(fft_table(H, W, device)), st)
        return spec
    be.lib().call("dpx_admm_seed_rows", ptr(spec), ptr(rho), term_arr, nterms, B, C, H, W, ptr(fft_table(H, W, device)), st)
    return spec


def stream_fork(frm, to):
    """every raw stream of ``to`` waits for what has been issued on ``frm`` (dpx_stream_fork; no-op on the CPU emulator)"""
    if be.host_mode():
        return
    arr = (c_void_p * len(to))(*to)
    be.lib().call("dpx_stream_fork", c_void_p(frm), arr, len(to))


def stream_join(into, frm):
    """``into`` waits for what has been issued on every raw stream of ``frm``"""
    if be.host_mode():
        return
    arr = (c_void_p * len(frm))(*frm)
    be.lib().call("dpx_stream_join", c_void_p(into), arr, len(frm))


def admm_run(spec_a, spec_b, spec_add, dd, term_arr, nterms, rho_tab, lam_tabs, eps, it0, n_iters, total, x_out, emit_last,
             shape, device):
    """n_iters fused iterations on the C side; returns the u-buffer parity (0: terms[i].u current, 1: u_out).
    emit_last: 0 nothing / 1 x and v (and the duals) / 2 x alone when the call ends the solve (v and u are then NOT updated)"""
    B, C, H, W = shape
    lt = (c_void_p * nterms)(*[None if t is None else t.data_ptr() for t in lam_tabs])
    L = be.lib()
    rc = L.query("dpx_admm_run", ptr(spec_a), ptr(spec_b), ptr(spec_add), ptr(dd), term_arr, nterms, ptr(rho_tab), lt,
                 c_float(eps), it0, n_iters, total, ptr(x_out), int(emit_last), B, C, H, W,
                 ptr(fft_table(H, W, device)), be.stream())
    if rc < 0:
        raise be.DpxError(f"dpx_admm_run failed ({rc}): {L.cdll.dpx_last_error().decode()}")
    return rc


def _addr(t):
    """device address of a tensor, or the address itself"""
    return t if isinstance(t, int) else t.data_ptr()


def admm_run_chains(chains, dd, nterms, eps, it0, n_iters, total, emit_last, shape, device):
    """dpx_admm_run for several sub-batch chains at once.  chains: dicts with spec_a, spec_b, spec_add (tensor / None), terms (ctypes
    array), rho_tab, lam_tabs (tensors), x_out, B, stream (raw handle), optionally seed (0 / 1 / 2) and seed_x0.  Returns the dual-buffer parity."""
    _, C, H, W = shape
    arr = (be.Chain * len(chains))()
    keep = []
    for i, ch in enumerate(chains):
        lt = (c_void_p * nterms)(*[None if t is None else t.data_ptr() for t in ch["lam_tabs"]])
        keep.append(lt)
        arr[i].spec_a, arr[i].spec_b = _addr(ch["spec_a"]), _addr(ch["spec_b"])
        arr[i].spec_add = None if ch["spec_add"] is None else _addr(ch["spec_add"])
        arr[i].terms = ctypes.cast(ch["terms"], ctypes.POINTER(Term))
        arr[i].rho_tab = ch["rho_tab"].data_ptr()
        arr[i].lam_tabs = ctypes.cast(lt, ctypes.POINTER(c_void_p))
        arr[i].x_out = _addr(ch["x_out"])
        arr[i].B = int(ch["B"])
        arr[i].stream = ch["stream"]
        arr[i].seed = int(ch.get("seed", 0))
        arr[i].seed_x0 = None if ch.get("seed_x0") is None else _addr(ch["seed_x0"])
    L = be.lib()
    rc = L.query("dpx_admm_run_chains", arr, len(chains), ptr(dd), nterms, c_float(eps), it0, n_iters, total, int(emit_last), C, H, W,
                 ptr(fft_table(H, W, device)))
    if rc < 0:
        raise be.DpxError(f"dpx_admm_run_chains failed ({rc}): {L.cdll.dpx_last_error().decode()}")
    return rc


def mul(x, w):
    """x * w with w one image ([1,C,H,W] or [C,H,W]) or a batch of them"""
    require(x, what="mul input")
    B = int(x.shape[0])
    npb = x.numel() // B
    w = w.to(device=x.device, dtype=torch.float32).contiguous()
    if w.numel() == npb:
        wimg = 1
    elif w.numel() == x.numel():
        wimg = B
    else:
        raise be.DpxError(f"mul: weight {tuple(w.shape)} matches neither one image nor the batch {tuple(x.shape)}")
    out = torch.empty_like(x)
    be.lib().call("dpx_mul", ptr(x), ptr(w), ptr(out), B, npb, wimg, be.stream())
    return out


def wss_prox(v, ktb, diag, lam):
    """(ktb + lam v) / (diag + lam) with per-image lam; ktb / diag one image or a batch"""
    require(v, what="wss_prox input")
    B = int(v.shape[0])
    npb = v.numel() // B
    ktb = ktb.to(device=v.device, dtype=torch.float32).contiguous()
    diag = diag.to(device=v.device, dtype=torch.float32).contiguous()

    def images(t, what):
        if t.numel() == npb:
            return 1
        if t.numel() == v.numel():
            return B
        raise be.DpxError(f"wss_prox: {what} {tuple(t.shape)} matches neither one image nor the batch {tuple(v.shape)}")
    out = torch.empty_like(v)
    be.lib().call("dpx_wss_prox", ptr(v), ptr(ktb), images(ktb, "Ktb"), ptr(diag), images(diag, "diag"), ptr(as_batch_vec(lam, B, v.device)),
                  ptr(out), B, npb, be.stream())
    return out


def mul_color(x, srf, transpose=False):
    """channel mixing by srf [C, C2]: forward srf.T @ x (C -> C2 channels), adjoint srf @ x (C2 -> C)"""
    require(x, what="mul_color input")
    B, Cx, H, W = _shape4(x)
    srf = srf.to(device=x.device, dtype=torch.float32).contiguous()
    C, C2 = int(srf.shape[0]), int(srf.shape[1])
    if Cx != (C2 if transpose else C):
        raise be.DpxError(f"mul_color: input has {Cx} channels, srf is {C}x{C2} (transpose={transpose})")
    out = torch.empty(B, C if transpose else C2, H, W, dtype=torch.float32, device=x.device)
    be.lib().call("dpx_mul_color", ptr(x), ptr(srf), ptr(out), int(bool(transpose)), B, C, C2, H * W, be.stream())
    return out


def upsample_zero(y, sf):
    require(y, what="upsample input")
    B, C, h, w = _shape4(y)
    out = torch.empty(B, C, h * sf, w * sf, dtype=torch.float32, device=y.device)
    be.lib().call("dpx_upsample_zero", ptr(y), ptr(out), int(sf), B * C, h, w, be.stream())
    return out


def cplx_mul(a, b, conj_a=False):
    """(conj) a * b, complex64; a is one image [1,...] shared by the batch or a batch like b"""
    require(b, dtype=torch.complex64, what="cplx_mul b")
    a = a.to(torch.complex64).contiguous()
    B = int(b.shape[0])
    npb = b.numel() // B
    a = a.expand(*([1] * (b.ndim - a.ndim)), *a.shape) if a.ndim < b.ndim else a
    if a.numel() == npb:
        aimg = 1
    elif a.numel() == b.numel():
        aimg = B
    else:
        a = a.expand_as(b).contiguous()
        aimg = B
    out = torch.empty_like(b)
    be.lib().call("dpx_cplx_mul", ptr(out), ptr(a), ptr(b), int(bool(conj_a)), B, npb, aimg, be.stream())
    return out


def sisr_update(FR, FB, lam, I, sf):
    """FX of sr.py:66-72 from FR [B,C,H,W] and the kernel spectrum FB ([1|B, 1|C, H, W])"""
    require(FR, dtype=torch.complex64, what="sisr FR")
    B, C, H, W = _shape4(FR)
    FB = FB.to(torch.complex64).contiguous()
    planes = FB.numel() // (H * W)
    if planes not in (1, C, B * C):
        FB = FB.expand(B, C, H, W).contiguous()
        planes = B * C
    buf = torch.empty(2, B, C, H, W, dtype=torch.complex64, device=FR.device)
    buf[0].copy_(FR)
    be.lib().call("dpx_sisr_update", ptr(buf), ptr(FB), planes, ptr(as_batch_vec(lam, B, FR.device)), float(I), int(sf), B, C, H, W,
                  be.stream())
    return buf[1]


def conv_pack(w, b, taps):
    """w [cout, cin, taps] float32 device tensor (+ optional bias) -> packed blob for conv2d"""
    require(w, what="conv weight")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    L = be.lib()
    blob = _bytes(L.query("dpx_conv_packed_bytes", cin, cout, taps), w.device)
    L.call("dpx_conv_pack", ptr(blob), ptr(w), ptr(b), cin, cout, taps, be.stream())
    return blob


def conv2d(x, packed, cout, taps, relu=False, res=None, dilation=1):
    """stride-1 3x3 (pad = dilation) / 1x1 convolution on the fp32 matrix cores; optional ReLU or residual add"""
    require(x, what="conv input")
    B, C, H, W = _shape4(x)
    out = torch.empty(B, cout, H, W, dtype=torch.float32, device=x.device)
    if res is not None:
        require(res, what="conv residual")
    be.lib().call("dpx_conv2d", ptr(x), ptr(out), ptr(packed), ptr(res), int(bool(relu)), C, cout, taps, int(dilation), B, H, W, be.stream())
    return out


def conv2d_leaky(x, packed, cout, neg_slope=0.2):
    """3x3 / pad 1 convolution + bias + LeakyReLU(neg_slope) fused (the U-Net denoiser's ConvLayer)"""
    require(x, what="conv input")
    B, C, H, W = _shape4(x)
    out = torch.empty(B, cout, H, W, dtype=torch.float32, device=x.device)
    be.lib().call("dpx_conv2d_leaky", ptr(x), ptr(out), ptr(packed), float(neg_slope), C, cout, 9, B, H, W, be.stream())
    return out


def leaky_relu_bwd(y, g, neg_slope=0.2):
    """g * (y > 0 ? 1 : neg_slope): backward of the fused LeakyReLU from the layer's saved output"""
    require(y, what="activation")
    require(g, what="gradient")
    out = torch.empty_like(g)
    be.lib().call("dpx_leaky_relu_bwd", ptr(y), ptr(g), ptr(out), y.numel(), float(neg_slope), be.stream())
    return out


def maxpool2(x):
    """MaxPool2d(2) (floor)"""
    require(x, what="maxpool input")
    B, C, H, W = _shape4(x)
    y = torch.empty(B, C, H // 2, W // 2, dtype=torch.float32, device=x.device)
    be.lib().call("dpx_maxpool2", ptr(x), ptr(y), B, C, H, W, be.stream())
    return y


def maxpool2_bwd(x, gy):
    require(x, what="maxpool input")
    require(gy, what="maxpool output gradient")
    B, C, H, W = _shape4(x)
    gx = torch.empty_like(x)
    be.lib().call("dpx_maxpool2_bwd", ptr(x), ptr(gy), ptr(gx), B, C, H, W, be.stream())
    return gx


def concat_skip_upsampled(skip, low):
    """torch.cat([skip, pad(upsample_x2_bilinear_align_corners(low))], dim=1) without the intermediates: the interpolated,
    zero-padded tensor is written straight into its channel slice (reference models/unet/unet.py:96-117)"""
    require(skip, what="skip tensor")
    require(low, what="low-resolution tensor")
    B, C2, H, W = _shape4(skip)
    _, C1, h, w = _shape4(low)
    out = torch.empty(B, C2 + C1, H, W, dtype=torch.float32, device=skip.device)
    L = be.lib()
    L.call("dpx_copy_channels", ptr(skip), ptr(out), 1, B, C2, H, W, C2 + C1, 0, be.stream())
    L.call("dpx_upsample2_into", ptr(low), ptr(out), B, C1, h, w, C2 + C1, C2, H, W, be.stream())
    return out


def concat_skip_upsampled_bwd(g, C2, low_shape):
    """gradients of concat_skip_upsampled w.r.t. (skip, low)"""
    require(g, what="concat gradient")
    B, Ct, H, W = _shape4(g)
    C1, (h, w) = Ct - C2, low_shape
    gskip = torch.empty(B, C2, H, W, dtype=torch.float32, device=g.device)
    glow = torch.empty(B, C1, h, w, dtype=torch.float32, device=g.device)
    L = be.lib()
    L.call("dpx_copy_channels", ptr(g), ptr(gskip), 0, B, C2, H, W, Ct, 0, be.stream())
    L.call("dpx_upsample2_into_bwd", ptr(g), ptr(glow), B, C1, h, w, Ct, C2, H, W, be.stream())
    return gskip, glow


def conv2d_wgrad(g, a, taps, dilation=1, want_bias=False):
    """weight (and bias) gradient of one conv2d layer: g [B,cout,H,W] gradient of the pre-activation output, a [B,cin,H,W] the
    layer's input -> gw [cout, cin, taps] (, gb [cout])"""
    require(g, what="conv output gradient")
    require(a, what="conv input")
    B, cout, H, W = _shape4(g)
    cin = int(a.shape[1])
    L = be.lib()
    gw = torch.empty(cout, cin, taps, dtype=torch.float32, device=g.device)
    gb = torch.empty(cout, dtype=torch.float32, device=g.device) if want_bias else None
    ws = workspace("conv_wgrad", L.query("dpx_conv2d_wgrad_ws_bytes", cin, cout, taps, B, H, W), g.device)
    L.call("dpx_conv2d_wgrad", ptr(g), ptr(a), ptr(gw), ptr(gb), cin, cout, taps, int(dilation), B, H, W, ptr(ws), be.stream())
    return gw, gb


def space_to_depth(x):
    require(x, what="space_to_depth input")
    B, C, H, W = _shape4(x)
    y = torch.empty(B, 4 * C, H // 2, W // 2, dtype=torch.float32, device=x.device)
    be.lib().call("dpx_space_to_depth", ptr(x), ptr(y), B, C, H, W, be.stream())
    return y


def depth_to_space(x):
    require(x, what="depth_to_space input")
    B, C4, H, W = _shape4(x)
    y = torch.empty(B, C4 // 4, 2 * H, 2 * W, dtype=torch.float32, device=x.device)
    be.lib().call("dpx_depth_to_space", ptr(x), ptr(y), B, C4 // 4, H, W, be.stream())
    return y


def cplx_scale(a, w):
    """w * a with a complex64 and w a real weight (one image or a batch)"""
    require(a, dtype=torch.complex64, what="cplx_scale input")
    B = int(a.shape[0])
    npb = a.numel() // B
    w = w.to(device=a.device, dtype=torch.float32).contiguous()
    if w.numel() == npb:
        wimg = 1
    elif w.numel() == a.numel():
        wimg = B
    else:
        raise be.DpxError(f"cplx_scale: weight {tuple(w.shape)} matches neither one image nor the batch {tuple(a.shape)}")
    out = torch.empty_like(a)
    be.lib().call("dpx_cplx_scale", ptr(out), ptr(a), ptr(w), B, npb, wimg, be.stream())
    return out


def clincomb(terms, out_complex=True):
    """sum_i coef_i * x_i over up to 4 real-fp32 / complex64 tensors of one shape; complex64 result, or its real part
    as fp32 (out_complex=False).  coef_i are python floats."""
    xs = [t[1].contiguous() for t in terms]
    ref = xs[0]
    if not 1 <= len(xs) <= 4:
        raise be.DpxError("clincomb: 1..4 operands")
    for x in xs:
        if x.dtype not in (torch.float32, torch.complex64):
            raise be.DpxError(f"clincomb operand must be float32 or complex64, got {x.dtype}")
        require(x, dtype=None, what="clincomb operand")
        if x.shape != ref.shape:
            raise be.DpxError(f"clincomb: shape mismatch {tuple(x.shape)} vs {tuple(ref.shape)}")
    res = torch.empty(ref.shape, dtype=torch.complex64 if out_complex else torch.float32, device=ref.device)
    if ref.numel() == 0:
        return res
    n = len(xs)
    px = (c_void_p * n)(*[x.data_ptr() for x in xs])
    cx = (ctypes.c_int * n)(*[int(x.is_complex()) for x in xs])
    cf = (c_float * n)(*[float(t[0]) for t in terms])
    be.lib().call("dpx_cplx_lincomb", ptr(res), int(bool(out_complex)), n, px, cx, cf, ref.numel(), be.stream())
    return res


def csmri_update(z, y, mask, lam, num_psi):
    """in place on the complex64 spectrum z [B,C,H,W]: z[mask] = ((lam z + y) / (1 + lam num_psi))[mask]"""
    require(z, dtype=torch.complex64, what="csmri spectrum")
    B = int(z.shape[0])
    npi = z.numel() // B
    y = y.to(torch.complex64).contiguous()
    if y.shape != z.shape:
        raise be.DpxError(f"csmri: y {tuple(y.shape)} does not match the iterate {tuple(z.shape)}")
    mk = (mask != 0).to(torch.uint8).contiguous()
    if mk.numel() == z.numel():
        mimg = B
    elif mk.numel() == npi:
        mimg = 1
    else:
        raise be.DpxError(f"csmri: mask {tuple(mask.shape)} matches neither one image nor the batch {tuple(z.shape)}")
    lam_v = as_batch_vec(lam, B, z.device)
    be.lib().call("dpx_csmri_update", ptr(z), ptr(y), ptr(mk), mimg, ptr(lam_v), float(num_psi), B, npi, be.stream())
    return z


def otf_grad(A, X, Y, O):
    """dL/dO of the Fourier x-update (dpx_otf_grad): A, X, Y complex64 [B,C,H,W] (Y may be None), O complex64 [1,C,H,W] -> [1,C,H,W]"""
    B, C, H, W = (int(v) for v in A.shape)
    for t, what in ((A, "A"), (O, "O")) + (((X, "X"),) if X is not None else ()) + (((Y, "Y"),) if Y is not None else ()):
        require(t, dtype=torch.complex64, what=f"otf_grad {what}")
    G = torch.empty_like(O)
    be.lib().call("dpx_otf_grad", ptr(A), ptr(X), ptr(Y), ptr(O), ptr(G), B, C, H, W, 0, be.stream())
    return G


def cfft2(x, inverse=False, centred=True, ortho=True):
    """complex64 2-D FFT over the last two dims (hand-written kernels; centring shifts and normalisation fused)"""
    if not x.is_complex():
        x = clincomb([(1.0, x.float())], out_complex=True)
    x = x.to(torch.complex64).contiguous()
    require(x, dtype=torch.complex64, what="cfft2 input")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    P = x.numel() // (H * W)
    out = torch.empty_like(x)
    be.lib().call("dpx_cfft2", ptr(x), ptr(out), int(bool(inverse)), int(bool(centred)), int(bool(ortho)), P, H, W,
                  ptr(fft_table(H, W, x.device)), be.stream())
    return out


def nlm(v, sigma, search=11, patch=5):
    """non-local means of [B, C, H, W] fp32 images (C = 3: the reference's luminance patch distance; C = 1: the plane itself) at the
    per-image noise level sigma (0-d / [B]): NonLocalMeansFast.forward of the reference in one kernel (dpx_nlm); a new tensor"""
    if not isinstance(v, torch.Tensor):
        raise be.DpxError(f"nlm: expected a torch.Tensor, got {type(v)}")
    if v.is_complex() or v.dtype != torch.float32:
        raise be.DpxError(f"nlm: expected a real float32 image, got {v.dtype}")
    B, C, H, W = _shape4(v)
    if C not in (1, 3):
        raise be.DpxError(f"nlm: {C} channels (1 or 3)")
    for name, n, lo, hi in (("search window", search, 3, 21), ("patch", patch, 1, 9)):
        if int(n) != n or n % 2 != 1 or not lo <= n <= hi:
            raise be.DpxError(f"nlm: {name} {n} (odd, {lo} .. {hi})")
    v = require(v.contiguous(), what="nlm input")
    sig = as_batch_vec(sigma, B, v.device)          # (held until the call returns: a temporary's memory may be reused before the launch)
    out = torch.empty_like(v)
    be.lib().call("dpx_nlm", ptr(v), ptr(out), ptr(sig), B, C, H, W, int(search), int(patch), be.stream())
    return out


def _tv_axes_mask(axes):
    """NCHW dims out of {1, 2, 3} -> dpx_tv_denoise's bit mask (bit 0 = dim 1)"""
    try:
        dims = tuple(axes)
    except TypeError:
        raise be.DpxError(f"tv_denoise: axes {axes!r} (a tuple of NCHW dims out of 1, 2, 3)")
    if not dims or len(set(dims)) != len(dims) or any(isinstance(d, bool) or int(d) != d or d not in (1, 2, 3) for d in dims):
        raise be.DpxError(f"tv_denoise: axes {axes!r} (a non-empty tuple of distinct NCHW dims out of 1, 2, 3)")
    return sum(1 << (int(d) - 1) for d in dims)


def tv_plan(shape, iters=5, axes=(1, 2)):
    """what dpx_tv_denoise would do on an [N, C, H, W] volume: dict(steps, launches, tile, lds_bytes) (dpx_tv_plan)"""
    _, D0, D1, D2 = (int(n) for n in shape)
    out = (ctypes.c_int * 6)()
    be.lib().call("dpx_tv_plan", D0, D1, D2, _tv_axes_mask(axes), int(iters), out)
    return dict(steps=out[0], launches=out[1], tile=(out[2], out[3], out[4]), lds_bytes=out[5])


def tv_bwd_plan(shape, iters=5, axes=(1, 2)):
    """what dpx_tv_backward would do on an [N, C, H, W] cotangent: dict(steps, launches, tile, lds_bytes) (dpx_tv_bwd_plan)"""
    _, D0, D1, D2 = (int(n) for n in shape)
    out = (ctypes.c_int * 6)()
    be.lib().call("dpx_tv_bwd_plan", D0, D1, D2, _tv_axes_mask(axes), int(iters), out)
    return dict(steps=out[0], launches=out[1], tile=(out[2], out[3], out[4]), lds_bytes=out[5])


def tv_denoise_rec(v, lam, iters, mask):
    """the recording forward on a checked, contiguous volume and an [N] lam: (out, the clip states of dpx_tv_denoise_rec as uint8)"""
    N, D0, D1, D2 = _shape4(v)
    L = be.lib()
    nb = L.query("dpx_tv_codes_bytes", N, D0, D1, D2, mask, int(iters))
    codes = _bytes(nb, v.device)[:nb] if nb else None           # (kept by the autograd node: not the shared scratch of workspace())
    ws = workspace("tv", L.query("dpx_tv_ws_bytes", N, D0, D1, D2, mask, int(iters)), v.device)
    out = torch.empty_like(v)
    L.call("dpx_tv_denoise_rec", ptr(v), ptr(out), ptr(lam), ptr(codes), N, D0, D1, D2, mask, int(iters), ptr(ws), be.stream())
    return out, codes


def tv_backward(g, codes, iters, mask, want_lam=True):
    """(gy, glam [N] or None) of dpx_tv_backward for the cotangent g [N, C, H, W] and the states tv_denoise_rec recorded"""
    g = require(g.contiguous(), what="tv_backward cotangent")
    N, D0, D1, D2 = _shape4(g)
    L = be.lib()
    ws = workspace("tv_bwd", L.query("dpx_tv_bwd_ws_bytes", N, D0, D1, D2, mask, int(iters)), g.device)
    gy = torch.empty_like(g)
    glam = torch.empty(N, dtype=torch.float32, device=g.device) if want_lam else None
    L.call("dpx_tv_backward", ptr(g), ptr(codes), ptr(gy), ptr(glam), N, D0, D1, D2, mask, int(iters), ptr(ws), be.stream())
    return gy, glam


class _TVDenoiseFn(torch.autograd.Function):
    """ops.tv_denoise(..., differentiable=True) under autograd: the recording forward, its state bytes saved for dpx_tv_backward"""

    @staticmethod
    def forward(ctx, v, lam, lam_vec, iters, mask):
        out, codes = tv_denoise_rec(v, lam_vec, iters, mask)
        ctx.codes, ctx.iters, ctx.mask = codes, iters, mask
        ctx.lam_shape = tuple(lam.shape) if isinstance(lam, torch.Tensor) else None
        ctx.lam_device = lam.device if isinstance(lam, torch.Tensor) else None
        return out

    @staticmethod
    def backward(ctx, g):
        want_lam = ctx.needs_input_grad[1]
        gy, glam = tv_backward(g, ctx.codes, ctx.iters, ctx.mask, want_lam)
        if want_lam:
            N = glam.shape[0]
            n_lam = int(np.prod(ctx.lam_shape)) if ctx.lam_shape else 1
            glam = (glam if n_lam == N else glam.sum()).reshape(ctx.lam_shape).to(ctx.lam_device)     # (one lam for N images: their sum)
        return (gy if ctx.needs_input_grad[0] else None), glam, None, None, None


def tv_denoise(v, lam, iters=5, axes=(1, 2), differentiable=False):
    """anisotropic TV denoising of an [N, C, H, W] fp32 volume: `iters` projected dual-ascent steps (step 1/5, threshold lam / 2) with
    differences along the NCHW dims in `axes` -- the reference's TV_denoising ((1, 2): its 2-D form differences C and H) / TV_denoising3d
    ((1, 2, 3)) in one dpx_tv_denoise call; lam: per-image (0-d / [N]), >= 0 (checked where it is a host value; a device tensor is not
    read back); a new tensor.

    The gradient is opt-in.  With the default a call autograd would have to differentiate raises NotImplementedError (forward-only).
    With ``differentiable=True`` such a call runs the recording forward (dpx_tv_denoise_rec: the same output bit for bit, plus the clip
    state of every dual update, one byte per voxel and step -- (iters - 1) bytes per voxel kept until the backward pass, which is why it
    has to be asked for) and its backward is dpx_tv_backward: the gradient to `v`, and to `lam` in lam's own shape where lam requires it.
    A call that needs no gradient takes the plain forward and records nothing, whatever the flag."""
    if not isinstance(v, torch.Tensor):
        raise be.DpxError(f"tv_denoise: expected a torch.Tensor, got {type(v)}")
    if v.is_complex() or v.dtype != torch.float32:
        raise be.DpxError(f"tv_denoise: expected a real float32 volume, got {v.dtype}")
    needs_grad = torch.is_grad_enabled() and (v.requires_grad or (isinstance(lam, torch.Tensor) and lam.requires_grad))
    if needs_grad and not differentiable:
        raise NotImplementedError("tv_denoise is forward-only unless asked: pass differentiable=True (TVDenoiser(differentiable=True)) for the "
                                  "backward kernel, which records (iters - 1) bytes per voxel in the forward pass, or call it under torch.no_grad()")
    N, D0, D1, D2 = _shape4(v)
    if min(N, D0, D1, D2) < 1:
        raise be.DpxError(f"tv_denoise: empty volume {tuple(v.shape)}")
    mask = _tv_axes_mask(axes)
    if int(iters) != iters or iters < 1:
        raise be.DpxError(f"tv_denoise: iters {iters} (an integer >= 1)")
    host_lam = lam if not isinstance(lam, torch.Tensor) else (lam.detach() if lam.device.type == "cpu" else None)
    if host_lam is not None and bool((torch.as_tensor(host_lam) < 0).any()):
        raise be.DpxError("tv_denoise: lam must be >= 0")
    v = require(v.contiguous(), what="tv_denoise input")
    lam_in = lam
    lam = as_batch_vec(lam, N, v.device)            # (held until the call returns)
    if needs_grad:
        return _TVDenoiseFn.apply(v, lam_in if isinstance(lam_in, torch.Tensor) else None, lam, int(iters), mask)
    L = be.lib()
    ws = workspace("tv", L.query("dpx_tv_ws_bytes", N, D0, D1, D2, mask, int(iters)), v.device)
    out = torch.empty_like(v)
    L.call("dpx_tv_denoise", ptr(v), ptr(out), ptr(lam), N, D0, D1, D2, mask, int(iters), ptr(ws), be.stream())
    return out


# ----------------------------------------------------------------------------------------------
# compress_sensing: the coded-aperture x-update (dpx_cs_xupdate / dpx_cs_backward, csrc/dpx_cs.hip)
# ----------------------------------------------------------------------------------------------
CS_MAX_IN = 4            # right-hand sides one dpx_cs_xupdate launch adds up


def _cs_operands(shape, y, mask):
    """(y as [Ny, H, W], the mask as [Nm, C, H, W]) for an [N, C, H, W] iterate (Ny, Nm: 1 = shared by the batch, or N): checked,
    contiguous fp32"""
    N, C, H, W = shape
    for t, what in ((mask, "mask"), (y, "y")):
        if not isinstance(t, torch.Tensor):
            raise be.DpxError(f"cs_xupdate: {what}: expected a torch.Tensor, got {type(t)}")
        if t.is_complex() or t.dtype != torch.float32:
            raise be.DpxError(f"cs_xupdate: {what}: expected real float32, got {t.dtype}")
    ms = tuple(mask.shape)
    if ms == (C, H, W):
        ms = (1,) + ms
    if ms not in ((1, C, H, W), (N, C, H, W)):
        raise be.DpxError(f"cs_xupdate: mask {tuple(mask.shape)} does not broadcast to the iterate {tuple(shape)} ([C,H,W], [1,C,H,W] or [N,C,H,W])")
    ys = tuple(y.shape)
    if ys not in ((H, W), (1, H, W), (N, H, W), (1, 1, H, W), (N, 1, H, W)):
        raise be.DpxError(f"cs_xupdate: y {ys} does not broadcast to the iterate {tuple(shape)} ([N,1,H,W], [1,1,H,W], [N,H,W] or [H,W])")
    Ny = 1 if len(ys) == 2 else ys[0]
    y3, mask4 = y.detach().reshape(Ny, H, W).contiguous(), mask.detach().reshape(ms).contiguous()
    return require(y3, what="cs_xupdate y"), require(mask4, what="cs_xupdate mask")


def _cs_forward(bs, y3, mask4, lam_vec, num_psi):
    """one dpx_cs_xupdate launch on checked operands; more than CS_MAX_IN right-hand sides: the leading ones are added up first"""
    if len(bs) > CS_MAX_IN:
        k = len(bs) - CS_MAX_IN + 1
        bs = [lincomb([(1.0, t) for t in bs[:k]])] + list(bs[k:])
    N, C, H, W = _shape4(bs[0])
    x = torch.empty_like(bs[0])
    pb = (c_void_p * len(bs))(*[t.data_ptr() for t in bs])
    be.lib().call("dpx_cs_xupdate", pb, len(bs), ptr(y3), ptr(mask4), ptr(lam_vec), int(num_psi), ptr(x), N, C, H, W, int(mask4.shape[0]),
                  int(y3.shape[0]), be.stream())
    return x


def cs_backward(g, v, y3, mask4, lam_vec, num_psi, want=(True, True, True, True)):
    """(gv, gy, glam [N], gmask) of dpx_cs_backward for the cotangent g [N, C, H, W]; an entry of `want` that is False is not computed
    (None): gy and gmask come in the shapes of y3 [Ny, H, W] and mask4 [Nm, C, H, W], summed over the batch where those are shared"""
    g = require(g.contiguous(), what="cs_backward cotangent")
    N, C, H, W = _shape4(g)
    L = be.lib()
    gv = torch.empty_like(g) if want[0] else None
    gy = torch.empty_like(y3) if want[1] else None
    glam = torch.empty(N, dtype=torch.float32, device=g.device) if want[2] else None
    gmask = torch.empty_like(mask4) if want[3] else None
    ws = workspace("cs_bwd", L.query("dpx_cs_bwd_ws_bytes", N, C, H, W), g.device) if want[2] else None
    L.call("dpx_cs_backward", ptr(g), ptr(v), ptr(y3), ptr(mask4), ptr(lam_vec), int(num_psi), ptr(gv), ptr(gy), ptr(glam), ptr(gmask), N, C, H, W,
           int(mask4.shape[0]), int(y3.shape[0]), ptr(ws), be.stream())
    return gv, gy, glam, gmask


class _CSXUpdateFn(torch.autograd.Function):
    """ops.cs_xupdate under autograd: the forward launch as it stands (its inputs are kept, nothing else), dpx_cs_backward recomputes from them"""

    @staticmethod
    def forward(ctx, y, mask, lam, y3, mask4, lam_vec, num_psi, *bs):
        ctx.y3, ctx.mask4, ctx.lam_vec, ctx.num_psi, ctx.bs = y3, mask4, lam_vec, num_psi, [b.detach() for b in bs]
        ctx.y_shape, ctx.mask_shape = tuple(y.shape), tuple(mask.shape)
        ctx.lam_shape = tuple(lam.shape) if isinstance(lam, torch.Tensor) else None
        ctx.lam_device = lam.device if isinstance(lam, torch.Tensor) else None
        return _cs_forward(ctx.bs, y3, mask4, lam_vec, num_psi)

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        want = (any(need[7:]), need[0], need[2], need[1])
        v = ctx.bs[0] if len(ctx.bs) == 1 else lincomb([(1.0, t) for t in ctx.bs])
        gv, gy, glam, gmask = cs_backward(g, v, ctx.y3, ctx.mask4, ctx.lam_vec, ctx.num_psi, want)
        if want[2]:
            N = glam.shape[0]
            n_lam = int(np.prod(ctx.lam_shape)) if ctx.lam_shape else 1
            glam = (glam if n_lam == N else glam.sum()).reshape(ctx.lam_shape).to(ctx.lam_device)     # (one lam for N images: their sum)
        gy = gy.reshape(ctx.y_shape) if want[1] else None
        gmask = gmask.reshape(ctx.mask_shape) if want[3] else None
        return (gy, gmask, glam, None, None, None, None) + tuple(gv if n else None for n in need[7:])


def cs_xupdate(bs, y, mask, lam, num_psi):
    """compress_sensing's closed-form x-update on the sum v of the [N, C, H, W] fp32 right-hand sides `bs` (ADMM hands over num_psi of
    them; a prox call one, num_psi = 1), in one dpx_cs_xupdate launch that adds them up itself (more than four: the leading ones by
    ops.lincomb first):

        s = sum_c m_c v_c,  phi = sum_c m_c^2,  d = phi + num_psi lam,  r = (num_psi y - s) / d,  x_c = (v_c + m_c r) / num_psi

    mask: real, any values, [C,H,W] / [1,C,H,W] / [N,C,H,W]; y: [N,1,H,W] / [1,1,H,W] / [N,H,W] / [H,W] (a leading 1 is shared by the
    batch); lam: per-image (0-d / [N]), > 0 (checked where it is a host value; a device tensor is not read back); a new tensor.
    Under autograd, where any of bs, y, lam, mask requires a gradient, the backward is dpx_cs_backward (every b receives the gradient to
    v; lam's comes in lam's own shape); a call that needs no gradient saves nothing."""
    bs = [bs] if isinstance(bs, torch.Tensor) else list(bs)
    if not bs:
        raise be.DpxError("cs_xupdate: nb = 0 right-hand sides (at least one)")
    for b in bs:
        if not isinstance(b, torch.Tensor):
            raise be.DpxError(f"cs_xupdate: expected a torch.Tensor, got {type(b)}")
        if b.is_complex() or b.dtype != torch.float32:
            raise be.DpxError(f"cs_xupdate: expected real float32 right-hand sides, got {b.dtype}")
        if b.shape != bs[0].shape:
            raise be.DpxError(f"cs_xupdate: right-hand sides of shapes {tuple(bs[0].shape)} and {tuple(b.shape)}")
    shape = _shape4(bs[0])
    if min(shape) < 1:
        raise be.DpxError(f"cs_xupdate: empty iterate {shape}")
    if isinstance(num_psi, bool) or int(num_psi) != num_psi or num_psi < 1:
        raise be.DpxError(f"cs_xupdate: num_psi {num_psi} (an integer >= 1)")
    host_lam = lam if not isinstance(lam, torch.Tensor) else (lam.detach() if lam.device.type == "cpu" else None)
    if host_lam is not None and bool((torch.as_tensor(host_lam) <= 0).any()):
        raise be.DpxError("cs_xupdate: lam must be > 0")
    y3, mask4 = _cs_operands(shape, y, mask)
    needs_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in bs + [y, mask, lam])
    bs = [require(b.contiguous(), what="cs_xupdate right-hand side") for b in bs]
    lam_vec = as_batch_vec(lam, shape[0], bs[0].device)             # (held until the call returns)
    if needs_grad:
        return _CSXUpdateFn.apply(y, mask, lam if isinstance(lam, torch.Tensor) else None, y3, mask4, lam_vec, int(num_psi), *bs)
    return _cs_forward([b.detach() for b in bs], y3, mask4, lam_vec, int(num_psi))


# ----------------------------------------------------------------------------------------------
# DOE wave-optics model: height map -> psf (dpx_doe_psf / dpx_doe_psf_backward, csrc/dpx_doe.hip + the transform kernels of dpx_fft.hip)
# ----------------------------------------------------------------------------------------------
_doe_contexts = {}


def _three_doubles(v, what):
    """the three wavelengths' constants as host doubles: a float32 tensor's values widened exactly"""
    vals = [float(x) for x in (v.detach().double().reshape(-1).tolist() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64).reshape(-1))]
    if len(vals) != 3:
        raise NotImplementedError(f"DOE model: {len(vals)} {what} (three wavelengths are built: the reference's propagator is written for three)")
    return (c_double * 3)(*vals)


class DoeContext:
    """what the DOE kernels need besides the height map, per (geometry, optics, device): the propagator's transfer function H
    ([1, 3, M, M] complex64 with the inverse transforms' 1 / M^2 folded in, dpx_doe_propagator_init), the twiddle table of the M-point
    transforms, the optical constants as host doubles, and the scratch workspace of calls that need no gradient"""

    def __init__(self, R, P, distance, interval, wave_lengths, refractive_idcs, device):
        self.R, self.P, self.M = int(R), int(P), int(R) + 2 * (int(R) // 4)
        self.device = torch.device(device)
        self.wl, self.ri = _three_doubles(wave_lengths, "wave lengths"), _three_doubles(refractive_idcs, "refractive indices")
        self.distance, self.interval = float(distance), float(interval)
        L = be.lib()
        if self.R < 4 or self.P < 1 or self.R % self.P:
            raise NotImplementedError(f"DOE model: a wavefront of {R} samples and a patch of {P} (the patch size must divide the wave resolution)")
        if not L.query("dpx_doe_ws_bytes", self.R, self.P, 0):
            raise NotImplementedError(f"DOE model: wave resolution {R} -> patch {P}: a padded row of {self.M} samples (times the {self.R // self.P} rows "
                                      "of a block) is beyond the LDS-resident transforms")
        self.table = fft_table(self.M, self.M, self.device)
        nb = L.query("dpx_doe_propagator_bytes", self.R)
        self.H = _bytes(nb, self.device)[:nb].view(torch.complex64).view(1, 3, self.M, self.M)
        L.call("dpx_doe_propagator_init", ptr(self.H), self.R, c_double(self.distance), c_double(self.interval), self.wl, be.stream())
        self.cols_per_wg = 0            # 0 = the library's choice (tools/bench_doe.py times the others)
        self.last_ws_bytes = 0          # workspace of the most recent dpx_doe_psf call (a call that needs no gradient keeps no field)

    def ws_bytes(self, keep_field):
        return be.lib().query("dpx_doe_ws_bytes", self.R, self.P, int(bool(keep_field)))


def doe_context(R, P, distance, interval, wave_lengths, refractive_idcs, device):
    wl, ri = _three_doubles(wave_lengths, "wave lengths"), _three_doubles(refractive_idcs, "refractive indices")
    key = (int(R), int(P), float(distance), float(interval), tuple(wl), tuple(ri), str(torch.device(device)))
    c = _doe_contexts.get(key)
    if c is None:
        c = _doe_contexts[key] = DoeContext(R, P, distance, interval, wave_lengths, refractive_idcs, device)
    return c


class DoeOptions:
    """the hybrid model's generalisation of the DOE kernels (``dpx_doe_opts``): u_c = a exp(i (k_c (s + eps)^2 + phi_c)) with an optional
    fp32 plane phi [1, 3, R, R], the aperture kind (0 circular, 1 half-circular) and the normalisation (0: one sum over the three
    channels, 1: one per channel).  ``None`` in its place is the base model, which runs the kernels it always ran."""

    def __init__(self, eps=0.0, phi=None, aperture_kind=0, norm_mode=0):
        self.eps, self.phi, self.aperture_kind, self.norm_mode = float(eps), phi, int(aperture_kind), int(norm_mode)

    def block(self, doe, gs=None, g_field=None):
        phi = self.phi
        if phi is not None:
            if not isinstance(phi, torch.Tensor) or phi.dtype != torch.float32 or tuple(phi.shape) != (1, 3, doe.R, doe.R):
                raise ValueError(f"DOE model: the phase plane must be a float32 tensor of shape {(1, 3, doe.R, doe.R)}")
            require(phi, what="DOE model phase plane")
        addr = lambda t: None if t is None else t.data_ptr()
        return be.DoeOpts(self.eps, self.aperture_kind, self.norm_mode, 0, addr(phi), addr(gs), addr(g_field))


def _doe_forward(doe, s, profile, keep_field, opt=None):
    """one dpx_doe_psf call on checked operands: (psf [1, 3, P, P], the workspace -- the caller's to keep when it holds the field)"""
    L = be.lib()
    nb = doe.ws_bytes(keep_field)
    ws = _bytes(nb, doe.device) if keep_field else workspace("doe", nb, doe.device)
    psf = torch.empty(1, 3, doe.P, doe.P, dtype=torch.float32, device=doe.device)
    if opt is None and not (keep_field and profile is not None):
        L.call("dpx_doe_psf", ptr(s), ptr(profile), doe.wl, doe.ri, ptr(psf), ptr(doe.H), ptr(doe.table), doe.R, doe.P, int(keep_field),
               doe.cols_per_wg, ptr(ws), be.stream())
    else:
        block = (opt or DoeOptions()).block(doe)
        L.call("dpx_doe_psf_ex", ptr(s), ptr(profile), doe.wl, doe.ri, ptr(psf), ptr(doe.H), ptr(doe.table), doe.R, doe.P, int(keep_field),
               doe.cols_per_wg, ctypes.byref(block), ptr(ws), be.stream())
    doe.last_ws_bytes = nb
    return psf, ws


class _DoePsfFn(torch.autograd.Function):
    """ops.doe_psf under autograd: the forward keeps the propagated field in a workspace of its own, dpx_doe_psf_backward reads it"""

    @staticmethod
    def forward(ctx, s, doe, opt):
        sd = s.detach()
        psf, ws = _doe_forward(doe, sd, None, True, opt)
        ctx.doe, ctx.ws, ctx.opt = doe, ws, opt
        ctx.save_for_backward(sd, psf)
        return psf

    @staticmethod
    def backward(ctx, g):
        s, psf = ctx.saved_tensors
        doe = ctx.doe
        g = require(g.contiguous(), what="doe_psf cotangent")
        gs = torch.empty_like(s)
        if ctx.opt is None:
            be.lib().call("dpx_doe_psf_backward", ptr(g), ptr(psf), ptr(s), doe.wl, doe.ri, ptr(gs), ptr(doe.H), ptr(doe.table), doe.R, doe.P,
                          doe.cols_per_wg, ptr(ctx.ws), be.stream())
        else:
            block = ctx.opt.block(doe, gs=gs)
            be.lib().call("dpx_doe_psf_backward_ex", ptr(g), ptr(psf), ptr(s), doe.wl, doe.ri, ptr(doe.H), ptr(doe.table), doe.R, doe.P,
                          doe.cols_per_wg, ctypes.byref(block), ptr(ctx.ws), be.stream())
        return gs, None, None


class _DoePsfProfileFn(torch.autograd.Function):
    """ops.doe_psf_of_profile under autograd: the backward pass stores the cotangent of the field in front of the propagator, times the
    aperture -- the gradient to the profile, dL/dRe + i dL/dIm"""

    @staticmethod
    def forward(ctx, prof, doe, opt):
        pd = prof.detach()
        psf, ws = _doe_forward(doe, None, pd, True, opt)
        ctx.doe, ctx.ws, ctx.opt = doe, ws, opt
        ctx.save_for_backward(psf)
        return psf

    @staticmethod
    def backward(ctx, g):
        (psf,) = ctx.saved_tensors
        doe = ctx.doe
        g = require(g.contiguous(), what="doe_psf cotangent")
        gp = torch.empty(1, 3, doe.R, doe.R, dtype=torch.complex64, device=doe.device)
        block = (ctx.opt or DoeOptions()).block(doe, g_field=gp)
        be.lib().call("dpx_doe_psf_backward_ex", ptr(g), ptr(psf), None, None, None, ptr(doe.H), ptr(doe.table), doe.R, doe.P, doe.cols_per_wg,
                      ctypes.byref(block), ptr(ctx.ws), be.stream())
        return gp, None, None


def _doe_check(t, doe, channels, dtype, what):
    if not isinstance(t, torch.Tensor):
        raise be.DpxError(f"{what}: expected a torch.Tensor, got {type(t)}")
    if t.dtype != dtype:
        raise NotImplementedError(f"{what}: {t.dtype} ({dtype} is built; no float64 or bf16 form of the DOE kernels)")
    if tuple(t.shape) != (1, channels, doe.R, doe.R):
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected {(1, channels, doe.R, doe.R)}")
    return require(t.contiguous(), dtype=dtype, what=what)


def doe_psf(doe, s, opt=None):
    """psf [1, 3, P, P] of the height map s^2 for s = height_map_sqrt [1, 1, R, R] fp32 (RGBCollimator.get_psf of the reference): three
    transform launches + one normalising launch; differentiable in s (dpx_doe_psf_backward).  A call that needs no gradient keeps no
    field.  opt: a DoeOptions (the hybrid model); None = the base model."""
    s = _doe_check(s, doe, 1, torch.float32, "doe_psf height_map_sqrt")
    if torch.is_grad_enabled() and s.requires_grad:
        return _DoePsfFn.apply(s, doe, opt)
    return _doe_forward(doe, s.detach(), None, False, opt)[0]


def doe_psf_from_profile(doe, phase_profile):
    """the base model's psf from an explicit complex64 phase profile [1, 3, R, R] (multiplied by the aperture); forward only --
    doe_psf_of_profile is the differentiable form"""
    if isinstance(phase_profile, torch.Tensor) and phase_profile.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("doe_psf_from_profile: forward only; the gradient with respect to an explicit phase_profile is "
                                  "doe_psf_of_profile's (RGBCollimator.get_psf(phase_profile) goes through it)")
    return doe_psf_of_profile(doe, phase_profile)


def doe_psf_of_profile(doe, phase_profile, opt=None):
    """the psf from an explicit complex64 phase profile [1, 3, R, R] (multiplied by the aperture); differentiable in the profile
    (dpx_doe_psf_backward_ex with g_field).  opt: a DoeOptions (the hybrid model); None = the base model."""
    prof = _doe_check(phase_profile, doe, 3, torch.complex64, "doe_psf phase_profile")
    if torch.is_grad_enabled() and prof.requires_grad:
        return _DoePsfProfileFn.apply(prof, doe, opt)
    return _doe_forward(doe, None, prof.detach(), False, opt)[0]


def _doe_propagate(doe, field, backward):
    out = torch.empty_like(field)
    L = be.lib()
    ws = workspace("doe", L.query("dpx_doe_ws_bytes", doe.R, doe.R, 0), doe.device)
    L.call("dpx_doe_propagate_backward" if backward else "dpx_doe_propagate", ptr(field), ptr(out), ptr(doe.H), ptr(doe.table), doe.R,
           doe.cols_per_wg, ptr(ws), be.stream())
    return out


class _DoePropagateFn(torch.autograd.Function):
    """ops.doe_fresnel under autograd: the operator is linear, its backward is its adjoint on the cotangent (dpx_doe_propagate_backward)"""

    @staticmethod
    def forward(ctx, field, doe):
        ctx.doe = doe
        return _doe_propagate(doe, field.detach(), False)

    @staticmethod
    def backward(ctx, g):
        g = require(g.contiguous(), dtype=torch.complex64, what="doe_propagate cotangent")
        return _doe_propagate(ctx.doe, g, True), None


def doe_propagate(doe, field):
    """crop(ifft2(fft2(zero-pad(field)) . H)) of a complex64 field [1, 3, R, R]; forward only -- doe_fresnel is the differentiable form"""
    if isinstance(field, torch.Tensor) and field.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("doe_propagate: forward only; the gradient with respect to an explicit field is doe_fresnel's "
                                  "(FresnelPropagator.forward goes through it)")
    return doe_fresnel(doe, field)


def doe_fresnel(doe, field):
    """crop(ifft2(fft2(zero-pad(field)) . H)) of a complex64 field [1, 3, R, R] (FresnelPropagator.forward of the reference);
    differentiable in the field (dpx_doe_propagate_backward)"""
    field = _doe_check(field, doe, 3, torch.complex64, "doe_propagate field")
    if torch.is_grad_enabled() and field.requires_grad:
        return _DoePropagateFn.apply(field, doe)
    return _doe_propagate(doe, field.detach(), False)


class _DoePhaseFn(torch.autograd.Function):
    """ops.doe_phase under autograd: dpx_doe_phase_backward recomputes the profile"""

    @staticmethod
    def forward(ctx, x, squared, eps, offset, wl, ri):
        xd = x.detach()
        ctx.args = (squared, eps, offset, wl, ri)
        ctx.save_for_backward(xd)
        return _doe_phase(xd, squared, eps, offset, wl, ri)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        squared, eps, offset, wl, ri = ctx.args
        g = require(g.contiguous(), dtype=torch.complex64, what="doe_phase cotangent")
        gx = torch.empty_like(x)
        be.lib().call("dpx_doe_phase_backward", ptr(g), ptr(x), int(squared), c_float(eps), ptr(offset), wl, ri, ptr(gx), x.numel(), be.stream())
        return gx, None, None, None, None, None


def _doe_phase(x, squared, eps, offset, wl, ri):
    out = torch.empty(1, 3, int(x.shape[-2]), int(x.shape[-1]), dtype=torch.complex64, device=x.device)
    if eps == 0.0 and offset is None:
        be.lib().call("dpx_doe_phase", ptr(x), int(squared), wl, ri, ptr(out), x.numel(), be.stream())
    else:
        be.lib().call("dpx_doe_phase_ex", ptr(x), int(squared), c_float(eps), ptr(offset), wl, ri, ptr(out), x.numel(), be.stream())
    return out


def doe_phase(x, squared, wave_lengths, refractive_idcs, eps=0.0, offset=None):
    """exp(i (k_c h + offset_c)) as complex64 [1, 3, H, W] for h = (x + eps)^2 (squared) or x, x fp32 with H W elements ([H, W] ..
    [1, 1, H, W]); offset: an optional fp32 plane [1, 3, H, W].  Differentiable in x (dpx_doe_phase_backward)."""
    if not isinstance(x, torch.Tensor):
        raise be.DpxError(f"doe_phase: expected a torch.Tensor, got {type(x)}")
    if x.dtype != torch.float32:
        raise NotImplementedError(f"doe_phase: {x.dtype} (float32 is built)")
    if x.ndim < 2 or x.numel() != int(x.shape[-2]) * int(x.shape[-1]) or x.numel() < 1:
        raise ValueError(f"doe_phase: a height map of shape {tuple(x.shape)} (one plane: [H, W] .. [1, 1, H, W])")
    wl, ri = _three_doubles(wave_lengths, "wave lengths"), _three_doubles(refractive_idcs, "refractive indices")
    if offset is not None:
        if not isinstance(offset, torch.Tensor) or offset.dtype != torch.float32 or tuple(offset.shape) != (1, 3, int(x.shape[-2]), int(x.shape[-1])):
            raise ValueError(f"doe_phase: the phase offset must be a float32 tensor of shape {(1, 3, int(x.shape[-2]), int(x.shape[-1]))}")
        offset = require(offset.detach().to(x.device).contiguous(), what="doe_phase offset")
    xc = require(x.contiguous(), what="doe_phase height map")
    if torch.is_grad_enabled() and xc.requires_grad:
        return _DoePhaseFn.apply(xc, bool(squared), float(eps), offset, wl, ri)
    return _doe_phase(xc.detach(), bool(squared), float(eps), offset, wl, ri)
