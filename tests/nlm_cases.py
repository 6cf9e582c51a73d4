"""patch_nlm cases shared by the GPU tests (-m gpu, real MI355X) and the emulated-kernel tests (CPU, the same kernel sources under the
SIMT emulator).  Every case runs the drop-in API on `device` against the reference's stored outputs (tests/golden/g40_patch_nlm.npz,
make_golden_nlm.py) or against `nlm_f64`, a float64 NumPy restatement of the reference's formula (proxfn/nlm/nlm.py).

Gates: the operator within rel-L2 1e-6 of the reference's fp32 and float64 outputs (achieved 1.5e-7 .. 3.6e-7; sigma = 0 is exact); a
5-iteration solve within 1e-5 of the reference's fp32 iterate (or 2x the reference's own fp32-vs-float64 distance + 1e-5, were that
larger: it is 2.2e-6 / 1.1e-6 here; achieved 1.2e-6 .. 3.1e-6), its float64 iterate within 0.3 x that (achieved 3.1e-7 .. 2.2e-6)
and the split variable v within half of it (achieved 6e-7 .. 8.5e-7).
"""
import numpy as np
import torch

import dprox as dp
from dprox import _ops as ops
from conftest import assert_close, load_golden, record, rel_l2

TOL = 1e-5
TOL_OP = 1e-6
# the kernel sums the 121 weighted shifts one after the other in fp32 (fixed order, bit-reproducible): its largest single-pixel error
# against float64 is 1.1e-6 on the 33 x 47 fixture (rel-L2 2.7e-7), so the max-abs bar of the float64 comparisons is 2 x TOL_OP
MAXABS_OP = 2.0


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def nlm_f64(v, sigma, search=11, patch=5):
    """the reference's NonLocalMeansFast in float64, written from its formula: luminance (C = 3) or the plane (C = 1), circular shifts"""
    v = np.asarray(v, np.float64)
    B, C, H, W = v.shape
    y = 0.299 * v[:, 0] + 0.587 * v[:, 1] + 0.114 * v[:, 2] if C == 3 else v[:, 0]
    rs, rp = search // 2, patch // 2
    num, den = np.zeros_like(v), np.zeros((B, H, W))
    h = (np.maximum(2 * np.asarray(sigma, np.float64).reshape(B), 0) + 1e-6)[:, None, None]
    for dx in range(-rs, rs + 1):
        for dy in range(-rs, rs + 1):
            d2 = (y - np.roll(y, (dy, dx), axis=(1, 2))) ** 2
            D = sum(np.roll(d2, (oy, ox), axis=(1, 2)) for oy in range(-rp, rp + 1) for ox in range(-rp, rp + 1))
            w = np.exp(-np.sqrt(D) / h)
            num += w[:, None] * np.roll(v, (dy, dx), axis=(2, 3))
            den += w
    return np.clip(num / den[:, None], 0, 1)


def case_op(device, key):
    """ops.nlm on a golden input: `op` (2 x 3 x 33 x 47, per-image sigma), `wrap` (1 x 3 x 7 x 9), `wrap0` (the same at sigma = 0)"""
    g = load_golden("g40_patch_nlm")
    src = "op" if key == "op" else "wrap"
    sigma = g[f"{src}_sigma"] if key != "wrap0" else np.zeros(1, np.float32)
    out = ops.nlm(T(g[f"{src}_v"], device), T(sigma, device)).cpu().numpy()
    if key == "wrap0":                       # sigma = 0: only the zero shift (and exact patch copies) has weight -- exact in every arithmetic
        for ref in ("_out", "_out_f64"):
            assert np.array_equal(out, g[key + ref].astype(np.float32)), ref
            record(f"nlm {key} vs reference{ref} (exact)", rel_l2(out, g[key + ref]), 0.0)
        return out
    assert_close(out, g[f"{key}_out"], TOL_OP, f"nlm {key} vs reference fp32", maxabs_mult=MAXABS_OP)
    assert_close(out, g[f"{key}_out_f64"], TOL_OP, f"nlm {key} vs reference float64", maxabs_mult=MAXABS_OP)
    return out


def case_prox(device):
    """patch_nlm.prox at lam = sigma^2 (ProxFn.prox -> _prox: sigma = sqrt(lam)) equals ops.nlm at sqrt(lam), and `c * patch_nlm`
    denoises at sqrt(c lam)"""
    g = load_golden("g40_patch_nlm")
    v = T(g["op_v"], device)
    lam = T(g["op_sigma"], device) ** 2
    x = dp.Variable()
    fn = dp.patch_nlm(x)
    assert torch.equal(fn.prox(v, lam).cpu(), ops.nlm(v, lam.sqrt()).cpu())
    fn2 = 0.5 * dp.patch_nlm(x)
    assert torch.equal(fn2.prox(v, lam).cpu(), ops.nlm(v, (lam * 0.5).sqrt()).cpu())


def case_restatement(device, shape, search=11, patch=5, seed=0, tol=TOL_OP):
    """ops.nlm against nlm_f64 on random noisy input (C = 1 and non-default windows: shapes the reference cannot run or has no fixture of)"""
    rng = np.random.RandomState(seed)
    v = (0.5 + 0.2 * rng.randn(*shape)).astype(np.float32)
    sigma = (0.03 + 0.1 * rng.rand(shape[0])).astype(np.float32)
    out = ops.nlm(T(v, device), T(sigma, device), search, patch).cpu().numpy()
    ref = nlm_f64(v, sigma, search, patch)
    assert_close(out, ref, tol, f"nlm {shape} windows ({search}, {patch}) vs float64 restatement", maxabs_mult=MAXABS_OP)
    return out


def admm_problem(g, device, tag):
    x = dp.Variable()
    b = T(g["b"], device)
    prior = dp.patch_nlm(x)
    fns = dp.sum_squares(dp.conv(x, g["psf"]) - b)
    lams = {}
    if tag == "nn":
        prior = 0.5 * prior
        nn = dp.nonneg(x)
        fns = fns + prior + nn
        lams[nn] = 0.0
    else:
        fns = fns + prior
    lams[prior] = T(g["lams"], device)
    return fns, lams, b


def case_admm(device, tag, fused):
    """the reference's 5-iteration ADMM on sum_squares(conv(x, psf) - b) + [0.5 *] patch_nlm(x) [+ nonneg(x)] through the fused plan or
    the generic splitting"""
    g = load_golden("g40_patch_nlm")
    fns, lams, b = admm_problem(g, device, tag)
    s = dp.compile(fns, method="admm", device=device)
    s.use_fused = fused
    with torch.no_grad():
        st = s.solve(x0=b, rhos=T(g["rhos"], device), lams=lams, max_iter=5, return_full_states=True)
    assert s.last_path == ("fused" if fused else "generic")
    ref_gap = float(g[f"{tag}_ref_f32_vs_f64"])
    tol = TOL if ref_gap <= TOL else 2 * ref_gap + TOL
    x = st[0].cpu().numpy()
    assert_close(x, g[f"{tag}_x"], tol, f"{tag} x vs reference fp32")
    r64 = rel_l2(x, g[f"{tag}_x_f64"])
    record(f"{tag} x vs reference float64", r64, 0.3 * tol)
    assert r64 <= 0.3 * tol, r64
    for name, got, bar in (("v0", st[1][0], tol / 2), ("u0", st[2][0], tol)):
        err = np.linalg.norm((got.cpu().numpy().astype(np.float64) - g[f"{tag}_{name}"]).ravel()) / np.linalg.norm(g[f"{tag}_x"].ravel())
        record(f"{tag} {name} (on the iterate's scale)", err, bar)
        assert err <= bar, (name, err)
    return st
