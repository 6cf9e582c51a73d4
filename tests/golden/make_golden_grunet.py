#!/usr/bin/env python
"""Golden vectors of the GRUNet denoiser prior -- runs ONLY in the build container (needs the reference checkout).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt) and runs the REFERENCE's own
modules on CPU, in float32 and -- ``module.double()`` on float64 inputs -- in float64: ``QRNNConv3D``, ``QRNNDeConv3D``,
``QRNNUpsampleConv3d``, ``BiQRNNConv3D``, ``BiQRNNDeConv3D`` (``bn=False``) for the layer cases, ``grunet_masked_nobn()`` behind
``GRUNetDenoiser._denoise`` for the network cases and the ADMM loop.  The cases, their inputs and the weights (drawn from seeds, never
stored) are those of tests/grunet_cases.py, imported from there.

  g47_grunet_layers*.npz  (the 2 x 18 x 34 and 2 x 10 x 18 cases in files of their own: _s3, _s3b)
                          l_<case>_o64 / _obits per layer case of grunet_cases.LAYERS, l_residual (two layers summed); l_saturated_s1_gmax,
                          the largest |gate| of the saturated case
  g47_grunet_net.npz      <case>_o64 / _obits per network case of grunet_cases.NETS, `range` (a 2 x 2 patch of 1e5), `admm` (x after 3
                          iterations of the reference's ADMM loop), and `keys`, the reference's state-dict keys in order

A float32 result is stored losslessly as `_obits`, the int32 difference between its bit pattern and that of its float64 twin rounded to
float32 (grunet_cases.golden adds it back).

    python tests/golden/make_golden_grunet.py
"""
import os
import runpy
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp = G["np"], G["torch"], G["dp"]
T, T64, save, reference_in_float64 = G["T"], G["T64"], G["save"], G["reference_in_float64"]
from dprox.proxfn.pnp.denoisers.base import Denoiser  # noqa: E402   (the REFERENCE's)
from dprox.proxfn.pnp.denoisers.models.qrnn import grunet_masked_nobn  # noqa: E402
from dprox.proxfn.pnp.denoisers.models.qrnn.layer import BiQRNNConv3D, BiQRNNDeConv3D, QRNNConv3D, QRNNDeConv3D, QRNNUpsampleConv3d  # noqa: E402
from dprox.proxfn.pnp.denoisers.wrapper import GRUNetDenoiser  # noqa: E402

assert dp.__file__.startswith(G["REF"]), dp.__file__
sys.path.insert(0, os.path.dirname(HERE))
import grunet_cases as GC  # noqa: E402   (module level: NumPy only)


def bits(r32, r64):
    return np.asarray(r32).view(np.int32) - np.asarray(r64).astype(np.float32).view(np.int32)


def both(out, key, run):
    """run(cast) in float32 and float64"""
    with torch.no_grad():
        o32, o64 = run(False).numpy(), run(True).numpy()
    assert o32.dtype == np.float32 and o64.dtype == np.float64 and o32.shape == o64.shape
    out[f"{key}_o64"], out[f"{key}_obits"] = o64, bits(o32, o64)
    print(f"   {key}: {o64.shape}, the reference's fp32 vs float64: rel-L2 {np.linalg.norm(o32 - o64) / np.linalg.norm(o64):.2e}")
    return o64


def make_layer(kind, cin, hidden, k):
    kw = dict(k=1, s=1, p=0) if k == 1 else {}
    if kind == "conv":
        return QRNNConv3D(cin, hidden, bn=False, **kw)
    if kind == "down":
        return QRNNConv3D(cin, hidden, k=3, s=(1, 2, 2), p=1, bn=False)
    if kind == "deconv":
        return QRNNDeConv3D(cin, hidden, bn=False, **kw)
    if kind == "up":
        return QRNNUpsampleConv3d(cin, hidden, bn=False)
    if kind == "bi":
        return BiQRNNConv3D(cin, hidden, bn=False)
    return BiQRNNDeConv3D(cin, hidden, bias=True, bn=False)


def load_layer(m, w, b):
    sd = m.state_dict()
    keys = list(sd)
    assert len(keys) == (2 if b is not None else 1) and tuple(sd[keys[0]].shape) == w.shape, (keys, w.shape)
    m.load_state_dict({keys[0]: T(w), **({keys[1]: T(b)} if b is not None else {})}, strict=True)
    return m


def layers():
    out = {}
    for name, (kind, cin, hidden, k, reverse, _) in GC.LAYERS.items():
        w, b = GC.layer_params(name)
        x = GC.layer_input(name)

        def run(f64):
            m = load_layer(make_layer(kind, cin, hidden, k), w, b)
            m, xt = (m.double(), T64(x)) if f64 else (m, T(x))
            return m(xt) if reverse is None else m(xt, reverse=reverse)

        both(out, f"l_{name}", run)
        if name.startswith("saturated"):
            m = load_layer(make_layer(kind, cin, hidden, k), w, b).double()
            out[f"l_{name}_gmax"] = np.float64(m.conv(T64(x)).abs().max())
            print(f"   l_{name}: largest |gate| {out[f'l_{name}_gmax']:.1f}")
    R = GC.RESIDUAL
    wa, wb, xa, xb = GC.residual_case()

    def run(f64):
        a = load_layer(QRNNConv3D(R["cin_a"], R["hidden"], bn=False), wa, None)
        b = load_layer(QRNNConv3D(R["cin_b"], R["hidden"], k=1, s=1, p=0, bn=False), wb, None)
        if f64:
            return a.double()(T64(xa)) + b.double()(T64(xb))
        return a(T(xa)) + b(T(xb))

    both(out, "l_residual", run)
    for f, pick in (("g47_grunet_layers", lambda k: "_s3" not in k), ("g47_grunet_layers_s3", lambda k: "_s3_" in k), ("g47_grunet_layers_s3b", lambda k: "_s3b_" in k)):
        save(f, **{k: v for k, v in out.items() if pick(k)})          # (float64 outputs are incompressible: every file below 1 MiB)


class Den(Denoiser):
    """the reference's GRUNetDenoiser without the checkpoint file: its own network, its own _denoise"""

    def __init__(self, model):
        super().__init__()
        self.model, self.use_noise_map = model, True

    def _denoise(self, x, sigma):
        return GRUNetDenoiser._denoise(self, x, sigma)


def network(f64):
    net = grunet_masked_nobn()
    sd = net.state_dict()
    w = GC.grunet_weights(GC.NET_SEED, [(k, tuple(v.shape)) for k, v in sd.items()])
    net.load_state_dict({k: T(v) for k, v in w.items()}, strict=True)
    assert len(sd) == 35 and sum(v.numel() for v in sd.values()) == 14278451
    return (net.double() if f64 else net).eval(), list(sd)


def nets():
    out = {}
    net32, keys = network(False)
    net64, _ = network(True)
    out["keys"] = np.asarray(keys)

    def denoise(x, sigma, f64):
        cast = T64 if f64 else T
        return Den(net64 if f64 else net32).denoise(cast(x), cast(sigma))

    for name in GC.NETS:
        x, sigma = GC.net_input(name)
        if len(sigma) > 1:                   # the reference takes one sigma per call: image by image
            run = lambda f64: torch.cat([denoise(x[i:i + 1], sigma[i:i + 1], f64) for i in range(len(sigma))])
        else:
            run = lambda f64: denoise(x, sigma, f64)
        o64 = both(out, name, run)
        res = o64 - x
        print(f"   {name}: |out - x| / |x| = {np.linalg.norm(res) / np.linalg.norm(x):.3f}")
    x, sigma = GC.range_input()
    both(out, "range", lambda f64: denoise(x, sigma, f64))

    b = GC.admm_input()

    def admm(f64):
        cast = T64 if f64 else T
        x = dp.Variable()
        reg = dp.deep_prior(x, denoiser=Den(net64 if f64 else net32))
        prob = dp.Problem(dp.sum_squares(x, cast(b)) + reg)
        if f64:
            with reference_in_float64():
                r = prob.solve(method="admm", device="cpu", x0=cast(b).clone(), rhos=0.5, lams={reg: 0.05}, max_iter=3)
        else:
            r = prob.solve(method="admm", device="cpu", x0=cast(b).clone(), rhos=0.5, lams={reg: 0.05}, max_iter=3)
        assert r.dtype == (torch.float64 if f64 else torch.float32), r.dtype
        return r

    both(out, "admm", admm)
    save("g47_grunet_net", **out)


if __name__ == "__main__":
    layers()
    nets()
