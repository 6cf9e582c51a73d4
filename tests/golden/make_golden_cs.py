#!/usr/bin/env python
"""Golden vectors of the compress_sensing data term -- runs ONLY in the build container (needs the reference checkout).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt), imports the REFERENCE's
``compress_sensing`` (dprox/proxfn/fast/cs.py) and subclasses it with a constructor that runs: the reference's own calls
``self.to_parameter``, which does not exist, and hands ``y`` to ``ext_sum_squares`` as ``eps``.  The subclass calls
``ext_sum_squares.__init__(self, linop)``, sets ``.mask.value`` and ``.y.value``, calls the reference's ``_reload`` and keeps ``I`` from
the third argument ``ext_sum_squares.solve`` passes to ``_prox``; every number below comes out of the reference's ``_reload`` / ``_prox``
/ ADMM loop.  ``_reload`` casts the mask to float32, so for the float64 runs the subclass replaces ``phi``, ``A`` and ``At`` by the same
three expressions on the float64 mask.

  p_*        _prox(v, lam, I) in float32 (`x32`) and float64 (`x64`); per-image lam; 0/1 masks with about half ones, p_row real-valued
               p_one     1 x 1 x 3 x 5      C = 1, less than a wave                                  I = 1, 2, 3
               p_hsi     2 x 31 x 17 x 19   shared mask [1,C,H,W], per-image y                       I = 1, 2, 3
               p_hsi_sy  the same with one y [1,1,H,W] shared by both images                         I = 2
               p_wide    1 x 33 x 5 x 67    C just past the register chunk, W past a wave and odd    I = 1, 2, 3
               p_row     3 x 4 x 1 x 130    H = 1, per-image mask [N,C,H,W], real-valued mask        I = 1, 2, 3
  g_*        the reference's autograd of sum(w x) to v, y, lam, mask, float32 and float64: p_hsi and p_hsi_sy at I = 2, p_row at I = 3
  admm_tv3d  compress_sensing(x, mask, y) + deep_prior(x, denoiser=TVDenoiser(5, True)): the reference's ADMM, 8 iterations on a smooth
             1 x 31 x 24 x 20 cube with a random 0/1 mask, x0 = y mask, rhos = 0.05, lams = {prior: 0.02}: x, v, u in float32, x in float64
             and the reference's own float32-vs-float64 distance
  admm_two   the same + nonneg(x): the solver itself runs the x-update at I = 2

Float64 outputs are incompressible, so the arrays are spread over four files, each below the 1 MiB a committed file may have --
g46_cs.npz (p_one, p_wide, p_row, g_p_row), g46_cs_hsi.npz, g46_cs_hsi_grad.npz, g46_cs_admm.npz -- and a float32 result `<key>32` is
stored losslessly as `<key>bits`, the int32 difference between its bit pattern and that of its float64 twin rounded to float32
(tests/cs_cases.py:golden adds it back).

    python tests/golden/make_golden_cs.py
"""
import os
import runpy
import types

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp, synthetic = G["np"], G["torch"], G["dp"], G["synthetic"]
T, T64, save, reference_in_float64 = G["T"], G["T64"], G["save"], G["reference_in_float64"]
from dprox.proxfn import ext_sum_squares  # noqa: E402   (the REFERENCE's)
from dprox.proxfn.fast.cs import compress_sensing  # noqa: E402
from dprox.proxfn.pnp.denoisers.wrapper import TVDenoiser  # noqa: E402

assert dp.__file__.startswith(G["REF"]), dp.__file__

LAMS = {1: [0.05], 2: [0.05, 1.7], 3: [0.05, 1.7, 0.4]}


class repaired(compress_sensing):
    """the reference's term behind a constructor that runs"""

    def __init__(self, linop, mask, y):
        ext_sum_squares.__init__(self, linop)
        self.mask, self.y = types.SimpleNamespace(value=mask), types.SimpleNamespace(value=y)
        self._reload(None)
        if mask.dtype == torch.float64:                    # (_reload has cast the mask to float32)
            self.phi = torch.sum(mask ** 2, dim=1, keepdim=True)
            self.A = lambda x: torch.sum(x * mask, dim=1, keepdim=True)
            self.At = lambda x: x * mask

    def _prox(self, v, lam, I=1):
        self.I = I
        return compress_sensing._prox(self, v, lam)


def bits(r32, r64):
    return np.asarray(r32).view(np.int32) - np.asarray(r64).astype(np.float32).view(np.int32)


def prox_inputs(name, seed):
    rng = np.random.RandomState(seed)
    N, C, H, W = {"p_one": (1, 1, 3, 5), "p_hsi": (2, 31, 17, 19), "p_wide": (1, 33, 5, 67), "p_row": (3, 4, 1, 130)}[name]
    v = rng.randn(N, C, H, W).astype(np.float32)
    if name == "p_row":
        mask = rng.randn(N, C, H, W).astype(np.float32)
    else:
        mask = (rng.rand(1, C, H, W) < 0.5).astype(np.float32)
    y = (rng.randn(N, 1, H, W) * np.sqrt(C / 2.0)).astype(np.float32)
    return v, mask, y, np.asarray(LAMS[N], np.float32)


def run_prox(v, mask, y, lam, I, f64, w=None):
    """_prox at I; with w also the reference's autograd of sum(w x)"""
    cast = T64 if f64 else T
    vt, mt, yt, lt = cast(v), cast(mask), cast(y), cast(lam)
    if w is not None:
        for t in (vt, mt, yt, lt):
            t.requires_grad_(True)
    x = repaired(dp.Variable(), mt, yt)._prox(vt, lt.view(-1, 1, 1, 1), I)
    assert x.dtype == (torch.float64 if f64 else torch.float32) and tuple(x.shape) == v.shape
    if w is None:
        return x.detach().numpy()
    (x * cast(w)).sum().backward()
    return x.detach().numpy(), {"gv": vt.grad.numpy(), "gy": yt.grad.numpy(), "glam": lt.grad.numpy(), "gmask": mt.grad.numpy()}


def prox_cases(out, tag, v, mask, y, lam, Is):
    out[f"{tag}_v"], out[f"{tag}_mask"], out[f"{tag}_y"], out[f"{tag}_lam"] = v, mask, y, lam
    for I in Is:
        with torch.no_grad():
            x32, x64 = run_prox(v, mask, y, lam, I, False), run_prox(v, mask, y, lam, I, True)
        # the reading of I: x solves (A^T A + I lam) x = A^T y + lam v
        m64, lam4 = mask.astype(np.float64), lam.astype(np.float64).reshape(-1, 1, 1, 1)
        res = m64 * (m64 * x64).sum(1, keepdims=True) + I * lam4 * x64 - (m64 * y.astype(np.float64) + lam4 * v.astype(np.float64))
        assert np.abs(res).max() < 1e-12 * max(1.0, np.abs(x64).max()), (tag, I, np.abs(res).max())
        out[f"{tag}_I{I}_x64"], out[f"{tag}_I{I}_xbits"] = x64, bits(x32, x64)
        print(f"   {tag} I={I}: the reference's fp32 vs float64 prox: rel-L2 {np.linalg.norm(x32 - x64) / np.linalg.norm(x64):.2e}")


def grad_case(out, tag, v, mask, y, lam, I, seed):
    w = np.random.RandomState(seed).randn(*v.shape).astype(np.float32)
    _, g32 = run_prox(v, mask, y, lam, I, False, w)
    _, g64 = run_prox(v, mask, y, lam, I, True, w)
    out[f"g_{tag}_w"], out[f"g_{tag}_I"] = w, np.int32(I)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64 and g32[k].shape == g64[k].shape
        out[f"g_{tag}_{k}64"], out[f"g_{tag}_{k}bits"] = g64[k], bits(g32[k], g64[k])
        print(f"   g_{tag} {k}: the reference's fp32 vs float64 gradient: rel-L2 {np.linalg.norm(g32[k] - g64[k]) / np.linalg.norm(g64[k]):.2e}")


def admm(mask, y, two, f64):
    cast = T64 if f64 else T
    mt, yt = cast(mask), cast(y)
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=TVDenoiser(5, True))
    fns, lams = repaired(x, mt, yt) + prior, {prior: 0.02}
    if two:
        nn = dp.nonneg(x)
        fns, lams = fns + nn, {prior: 0.02, nn: 0.02}      # (the loop looks every Psi term's lam up; nonneg's prox does not read it)
    with torch.no_grad():
        st = dp.Problem(fns).solve(method="admm", device="cpu", x0=(yt * mt).clone(), rhos=0.05, lams=lams, max_iter=8, return_full_states=True)
    assert st[0].dtype == (torch.float64 if f64 else torch.float32)
    return st


def g46_cs():
    small, hsi, hsi_grad, traj = {}, {}, {}, {}
    for seed, name in enumerate(("p_one", "p_wide", "p_row")):
        prox_cases(small, name, *prox_inputs(name, 460 + seed), (1, 2, 3))
    grad_case(small, "p_row", *prox_inputs("p_row", 462), 3, 470)
    v, mask, y, lam = prox_inputs("p_hsi", 463)
    prox_cases(hsi, "p_hsi", v, mask, y, lam, (1, 2, 3))
    prox_cases(hsi, "p_hsi_sy", v, mask, y[:1], lam, (2,))
    for k in ("v", "mask", "lam"):
        del hsi[f"p_hsi_sy_{k}"]                               # (p_hsi's)
    grad_case(hsi_grad, "p_hsi", v, mask, y, lam, 2, 471)
    grad_case(hsi_grad, "p_hsi_sy", v, mask, y[:1], lam, 2, 471)
    del hsi_grad["g_p_hsi_sy_w"]                               # (g_p_hsi_w)
    save("g46_cs", **small)
    save("g46_cs_hsi", **hsi)
    save("g46_cs_hsi_grad", **hsi_grad)

    rng = np.random.RandomState(464)
    gt = synthetic.synth(rng, 1, 31, 24, 20).astype(np.float32)
    mask = (rng.rand(1, 31, 24, 20) < 0.5).astype(np.float32)
    y = (gt * mask).sum(1, keepdims=True).astype(np.float32)
    traj["admm_mask"], traj["admm_y"] = mask, y
    for tag, two in (("admm_tv3d", False), ("admm_two", True)):
        st = admm(mask, y, two, False)
        with reference_in_float64():
            st64 = admm(mask, y, two, True)
        traj[f"{tag}_x"] = st[0]
        for i in range(len(st[1])):
            traj[f"{tag}_v{i}"], traj[f"{tag}_u{i}"] = st[1][i], st[2][i]
        traj[f"{tag}_x_f64"] = st64[0]
        rel = float((st[0].double() - st64[0]).norm() / st64[0].norm())
        traj[f"{tag}_ref_f32_vs_f64"] = np.float64(rel)
        print(f"   {tag}: the reference's fp32 vs float64 iterate: rel-L2 {rel:.2e}")
    save("g46_cs_admm", **traj)


if __name__ == "__main__":
    g46_cs()
