#!/usr/bin/env python
"""Golden vectors of the TV denoiser's gradient -- runs ONLY in the build container (needs the reference checkout).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt) and stores what the reference's
TV_denoising / TV_denoising3d (proxfn/pnp/denoisers/models/TV_denoising.py) give under torch autograd, in float32 and in float64, on
[C, H, W] volumes with a 0-d `sigma` tensor that requires grad:

  case  volume      form  iters
  a     3 x 21 x 30  2-D   5
  b     3 x 21 x 30  3-D   5
  (c)   1 x 19 x 23  3-D   5     no fixture: the reference returns an EMPTY tensor when a differenced axis has length 1 (its dual of that axis
                                 has no rows and the broadcast against it empties x0; asserted below) -- tests/tv_bwd_cases.py runs this
                                 shape against the float64 restatement instead
  d     31 x 40 x 40 3-D   5     (D0 tiled, S = 2: a chain of three launches)
  e     3 x 21 x 70  2-D   7     (two launches, D2 no multiple of 4)

  g44_tv_bwd_<case>.npz        v, sigma, the seeded cotangent g, out_f64, out_bits, the shares of clipped / inside dual updates, the margin
  g44_tv_bwd_<case>_grad.npz   gv_f64, gv_bits (d <g, out> / d v), gsigma_f32, gsigma_f64 (d <g, out> / d sigma)

  g44_tv_bwd_admm.npz          end to end: 3 iterations of the reference's ADMM on sum_squares(conv(x, psf) - b) + deep_prior(x, TVDenoiser(5)) at
                               1 x 3 x 32 x 32, loss = MSE to the ground truth: x, the loss and its gradients to the per-step sigma schedule and
                               to b in fp32 and (reference_in_float64) float64, and the reference's own fp32-vs-float64 distance of each; the
                               same three conditions below on the dual updates of all three prox calls, at a margin of 1e-5 theta

(`<key>_bits`: the fp32 result stored losslessly as the int32 difference between its bit pattern and that of its float64 twin rounded to
fp32, as make_golden_tv.py does; tests/tv_bwd_cases.py:fixture adds it back.  v and g are multiples of 2^-12 and 2^-6: they compress.)

TV is piecewise linear: a clip state that flips between the float32 and the float64 run changes the gradient by a jump.  For every case
the generator therefore walks seeds until, at every step but the unused last one, (1) both runs have identical clip states, (2) no |w|
lies within 1e-4 theta of theta in either run, (3) at least 5 % of the dual updates are clipped and at least 5 % inside -- and asserts all
three on what it stores.  The states are read by wrapping the reference module's own `clip` while it runs (nothing of it is restated).

    python tests/golden/make_golden_tv_bwd.py          # writes tests/golden/g44_tv_bwd_*.npz
"""
import os
import runpy

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp, save = G["np"], G["torch"], G["dp"], G["save"]
from dprox.proxfn.pnp.denoisers.models import TV_denoising as ref_tv  # noqa: E402   (the REFERENCE's module)

assert dp.__file__.startswith(G["REF"]), dp.__file__

CASES = {"a": ((3, 21, 30), False, 5, 0.05), "b": ((3, 21, 30), True, 5, 0.05),
         "d": ((31, 40, 40), True, 5, 0.05), "e": ((3, 21, 70), False, 7, 0.05)}
MARGIN, SHARE = 1e-4, 0.05


def volume(shape, seed):
    """A cartoon: blocks of 1 x 7 x 9 voxels at levels out of {0, 1/4, .., 1} plus noise of 0.01, on a grid of 2^-12; the cotangent on a
    grid of 2^-6.  Condition (2) cannot hold for hundreds of thousands of dual updates whose arguments spread evenly around theta (the
    closest of n of them lies about theta / n away); here they fall into two groups -- far above theta across a block edge (a jump of
    1/4 gives 2 theta at sigma = 0.05), far below inside a block -- with a gap around theta that the iterations do not close."""
    rng = np.random.RandomState(seed)
    nb = [s // b + 1 for s, b in zip(shape, (1, 7, 9))]
    levels = rng.randint(0, 5, nb) / 4.0
    cartoon = np.kron(levels, np.ones((1, 7, 9)))[:shape[0], :shape[1], :shape[2]]
    v = np.round((cartoon + 0.01 * rng.randn(*shape)) * 4096) / 4096
    g = np.round(rng.randn(*shape) * 64) / 64
    return v.astype(np.float32), g.astype(np.float32)


def run(v, g, sigma, use_3d, iters, dtype):
    """(out, d<g, out>/dv, d<g, out>/dsigma, [(state array, margin)] per clip call but the last iteration's) of the reference in `dtype`"""
    seen = []
    real = ref_tv.clip

    def spy(x, thres):
        w, th = x.detach().double(), float(thres.detach())
        seen.append((np.sign(w.numpy()) * (np.abs(w.numpy()) > th), float((w.abs() - th).abs().min() / th) if w.numel() else np.inf))
        return real(x, thres)

    ref_tv.clip = spy
    try:
        vt = torch.from_numpy(v).to(dtype).requires_grad_(True)
        st = torch.tensor(sigma, dtype=dtype, requires_grad=True)
        out = (ref_tv.TV_denoising3d if use_3d else ref_tv.TV_denoising)(vt, st, iters)
        (out * torch.from_numpy(g).to(dtype)).sum().backward()
    finally:
        ref_tv.clip = real
    assert out.dtype == dtype and vt.grad.dtype == dtype
    k = 3 if use_3d else 2
    assert len(seen) == k * iters
    return out.detach(), vt.grad, st.grad, seen[:k * (iters - 1)]


def g44_tv_bwd():
    assert ref_tv.TV_denoising3d(torch.rand(1, 19, 23), torch.tensor(0.05), 5).numel() == 0, "the reference now handles an axis of length 1: add case c"
    for tag, (shape, use_3d, iters, sigma) in CASES.items():
        sigma = float(np.float32(sigma))
        for seed in range(4400, 4500):
            v, g = volume(shape, seed)
            o32, gv32, gs32, s32 = run(v, g, sigma, use_3d, iters, torch.float32)
            o64, gv64, gs64, s64 = run(v, g, sigma, use_3d, iters, torch.float64)
            same = all(np.array_equal(a[0], b[0]) for a, b in zip(s32, s64))
            margin = min(m for _, m in s32 + s64)
            n = sum(a[0].size for a in s64)
            clipped = sum(int((a[0] != 0).sum()) for a in s64) / max(n, 1)
            if same and margin >= MARGIN and clipped >= SHARE and 1 - clipped >= SHARE:
                break
        else:
            raise AssertionError(f"case {tag}: no seed satisfies the conditions")
        assert same and margin >= MARGIN and SHARE <= clipped <= 1 - SHARE, (tag, same, margin, clipped)
        bits = lambda r32, r64: r32.numpy().view(np.int32) - r64.numpy().astype(np.float32).view(np.int32)
        save(f"g44_tv_bwd_{tag}", v=v, sigma=np.float32(sigma), g=g, use_3d=np.array(use_3d), iters=np.array(iters), seed=np.array(seed),
             out_f64=o64, out_bits=bits(o32, o64), clipped=np.float64(clipped), margin=np.float64(margin))
        save(f"g44_tv_bwd_{tag}_grad", gv_f64=gv64, gv_bits=bits(gv32, gv64), gsigma_f32=gs32, gsigma_f64=gs64)
        rel = lambda a, b: float((a.double() - b).norm() / b.norm())
        print(f"   {tag}: seed {seed}, clipped {clipped:.3f}, margin {margin:.2e} theta; the reference's fp32 vs float64: out {rel(o32, o64):.2e}, "
              f"d/dv {rel(gv32, gv64):.2e}, d/dsigma {abs(float(gs32) - float(gs64)) / abs(float(gs64)):.2e}")


def admm_grads(b, gt, psf, rhos, sig, f64):
    """loss = mean((x_3 - gt)^2) of 3 ADMM iterations on sum_squares(conv(x, psf) - b) + deep_prior(x, TVDenoiser(5)) and its gradients to
    the per-step sigma schedule and to b; the clip calls are spied on as in `run`"""
    from dprox.proxfn.pnp.denoisers.wrapper import TVDenoiser
    dt = torch.float64 if f64 else torch.float32
    seen, real = [], ref_tv.clip

    def spy(x, thres):
        w, th = x.detach().double(), float(thres.detach())
        seen.append((np.sign(w.numpy()) * (np.abs(w.numpy()) > th), float((w.abs() - th).abs().min() / th)))
        return real(x, thres)

    ref_tv.clip = spy
    try:
        bt = torch.from_numpy(b).to(dt).requires_grad_(True)
        st = torch.from_numpy(sig).to(dt).requires_grad_(True)
        x = dp.Variable()
        prior = dp.deep_prior(x, denoiser=TVDenoiser(5, False))
        fns = dp.sum_squares(dp.conv(x, torch.from_numpy(psf).to(dt) if f64 else psf) - bt) + prior
        xo = dp.compile(fns, method="admm", device="cpu").solve(x0=bt.detach().clone(), rhos=torch.from_numpy(rhos), lams={prior: st}, max_iter=3)
        loss = ((xo - torch.from_numpy(gt).to(dt)) ** 2).mean()
        loss.backward()
    finally:
        ref_tv.clip = real
    assert xo.dtype == dt and st.grad.dtype == dt and bt.grad.dtype == dt
    used = [s for i, s in enumerate(seen) if i % 10 < 8]                         # (5 steps x 2 axes per prox; the last step's two are unused)
    return xo.detach(), loss.detach(), st.grad, bt.grad, used


def g44_tv_bwd_admm():
    """the end-to-end case: the same three conditions on every dual update of the three prox calls, at a margin of 1e-5 theta"""
    synthetic, reference_in_float64 = G["synthetic"], G["reference_in_float64"]
    rhos = np.array([0.2, 0.15, 0.1], np.float32)
    sig = np.array([0.05, 0.04, 0.03], np.float32)
    for seed in range(4450, 4550):
        gt, b, psf = synthetic.deconv_case(1, 3, 32, 32, seed=seed)
        r32 = admm_grads(b, gt, psf, rhos, sig, False)
        with reference_in_float64():
            r64 = admm_grads(b, gt, psf, rhos, sig, True)
        same = len(r32[4]) == len(r64[4]) == 24 and all(np.array_equal(a[0], c[0]) for a, c in zip(r32[4], r64[4]))
        margin = min(m for _, m in r32[4] + r64[4])
        clipped = sum(int((a[0] != 0).sum()) for a in r64[4]) / sum(a[0].size for a in r64[4])
        if same and margin >= 1e-5 and SHARE <= clipped <= 1 - SHARE:
            break
    else:
        raise AssertionError("end-to-end case: no seed satisfies the conditions")
    rel = lambda a, c: float((a.double() - c).norm() / c.norm())
    gaps = dict(x=rel(r32[0], r64[0]), g_sigma=rel(r32[2], r64[2]), g_b=rel(r32[3], r64[3]))
    save("g44_tv_bwd_admm", gt=gt, b=b, psf=psf, rhos=rhos, sigmas=sig, seed=np.array(seed), clipped=np.float64(clipped), margin=np.float64(margin),
         x=r32[0], loss=r32[1], g_sigma=r32[2], g_b=r32[3], x_f64=r64[0], loss_f64=r64[1], g_sigma_f64=r64[2], g_b_f64=r64[3],
         **{f"{k}_ref_f32_vs_f64": np.float64(v) for k, v in gaps.items()})
    print(f"   admm: seed {seed}, clipped {clipped:.3f}, margin {margin:.2e} theta; the reference's fp32 vs float64: {gaps}")


if __name__ == "__main__":
    g44_tv_bwd()
    g44_tv_bwd_admm()
