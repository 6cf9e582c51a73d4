#!/usr/bin/env python
"""The hybrid DOE model (dprox.contrib.optic.doe_hybrid, dpx_doe_psf_ex / dpx_doe_psf_backward_ex) at its default configuration:
1536 -> 512 (padded rows of 2304 samples, 3 x 3 blocks), half-circular aperture, lens phase plane, one normalisation per channel.

Prints ONE JSON line (kept as profiles/doe_hybrid_bench.json):
  * `hybrid`: ms per call of the C entry points on prepared arguments -- `forward` (no field kept), `forward_keep` + `backward` (a
    training step's pair) -- and the same pair through RGBCollimator.get_psf() and autograd (tools/bench_doe.py's windows: the median and
    the min .. max of `rounds` windows of `calls` back-to-back calls);
  * `base_same_R`: the base model (circular aperture, no lens plane, one normalisation) at the same sizes on this build -- what the extra
    phase plane and the three statistics cost;
  * per launch of the hybrid's forward + backward the kernel time, the bytes the algorithm needs in that launch and the fraction of the
    6.29 TB/s measured copy rate they amount to;
  * `torch`: the same arithmetic as torch ops on the device (torch.fft, avg_pool2d, autograd; float32 / complex64).

    python tools/bench_doe_hybrid.py [--calls 10] [--warmup 2] [--rounds 3]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_doe as bd  # noqa: E402
from dprox import _backend as be  # noqa: E402
from dprox.contrib import optic  # noqa: E402
from dprox.contrib.optic import doe_hybrid as hyb  # noqa: E402


def launch_bytes(R, P):
    """tools/bench_doe.py's bytes plus the lens phase plane phi [3][R][R] fp32 in the two launches that read it"""
    nb = bd.launch_bytes(R, P)
    phi = 4 * 3 * R * R
    nb["fwd"]["k_doe_rows_in"] += phi
    nb["bwd"]["k_doe_rows_grad"] += phi
    return nb


def raw_calls(m):
    """(forward without a field, forward keeping it, backward) of the hybrid model as calls of the C entry points"""
    L, p = be.lib(), be.ptr
    c = m._context()
    s = m.height_map.height_map_sqrt.detach()
    psf, g, gs = torch.empty(1, 3, c.P, c.P, device=s.device), torch.randn(1, 3, c.P, c.P, device=s.device), torch.empty_like(s)
    ws0 = torch.empty(c.ws_bytes(False), dtype=torch.uint8, device=s.device)
    ws1 = torch.empty(c.ws_bytes(True), dtype=torch.uint8, device=s.device)
    kind = hyb.APERTURE_KINDS[m.aperture_type]
    of = be.DoeOpts(hyb.EPS, kind, 1, 0, m.refractive_len.data_ptr(), None, None)
    ob = be.DoeOpts(hyb.EPS, kind, 1, 0, m.refractive_len.data_ptr(), gs.data_ptr(), None)
    fwd = lambda keep, ws: L.call("dpx_doe_psf_ex", p(s), None, c.wl, c.ri, p(psf), p(c.H), p(c.table), c.R, c.P, keep, c.cols_per_wg, ctypes.byref(of),
                                  p(ws), be.stream())
    bwd = lambda: L.call("dpx_doe_psf_backward_ex", p(g), p(psf), p(s), c.wl, c.ri, p(c.H), p(c.table), c.R, c.P, c.cols_per_wg, ctypes.byref(ob), p(ws1),
                         be.stream())
    return (lambda: fwd(0, ws0)), (lambda: fwd(1, ws1)), bwd, (psf, g, gs, ws0, ws1, of, ob)


def torch_model(m):
    """the same arithmetic as torch ops on the device, float32 / complex64: (psf of s)"""
    dev = m.height_map.height_map_sqrt.device
    c = m._context()
    R, P, p = c.R, c.P, c.R // 4
    H = (c.H * (c.M * c.M)).clone()
    ap, phi = m.aperture, m.refractive_len
    k = torch.tensor([2 * np.pi / c.wl[i] * (c.ri[i] - 1) for i in range(3)], dtype=torch.float32, device=dev).view(1, 3, 1, 1)

    def psf_of(s):
        u = ap * torch.exp(1j * (k * (s + 1e-7) ** 2 + phi))
        w = torch.fft.ifft2(torch.fft.fft2(torch.nn.functional.pad(u, [p, p, p, p])) * H)[:, :, p:p + R, p:p + R]
        q = torch.nn.functional.avg_pool2d(w.real ** 2 + w.imag ** 2, R // P, R // P)
        return q / q.sum(dim=[2, 3], keepdim=True)
    return psf_of


def timed(fwd, fwd_keep, bwd, a):
    row = {}
    for key, fn in (("forward", fwd), ("forward_keep", fwd_keep), ("backward", bwd)):
        ms, spread = bd.windows(fn, a.calls, a.warmup, a.rounds)
        row[key] = {"ms": ms, "ms_min_max": spread}
    row["forward_backward_ms"] = round(row["forward_keep"]["ms"] + row["backward"]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = hyb.DOEModelConfig()
    R, P = cfg.wave_resolution[0], cfg.patch_size
    res = {"metric": "doe_hybrid_psf", "device": torch.cuda.get_device_name(dev), "copy_rate_TBps": bd.COPY_RATE / 1e12, "case": f"{R}->{P}",
           "timing": f"median of {a.rounds} windows of {a.calls} back-to-back calls; (min, max) alongside; per-launch: median of 5 calls' kernel times"}
    m = hyb.build_doe_model(cfg).to(dev)
    c = m._context()
    res["M"] = c.M
    fwd, fwd_keep, bwd, hold = raw_calls(m)
    row = timed(fwd, fwd_keep, bwd, a)
    w = hold[1]

    def through_ops():
        m.height_map.height_map_sqrt.grad = None
        (m.get_psf() * w).sum().backward()
    ms, spread = bd.windows(through_ops, a.calls, a.warmup, a.rounds)
    row["ops_forward_backward_ms"] = {"ms": ms, "ms_min_max": spread}
    nb = launch_bytes(R, P)
    row["launches_forward"] = bd.per_launch(fwd_keep, nb["fwd"])
    row["launches_backward"] = bd.per_launch(bwd, nb["bwd"])
    res["hybrid"] = row
    psf_of = torch_model(m)
    s = m.height_map.height_map_sqrt
    with torch.no_grad():
        ms, spread = bd.windows(lambda: psf_of(s), a.calls, 1, a.rounds)
        diff = float((psf_of(s) - m.get_psf()).norm() / m.get_psf().norm())
    res["torch"] = {"forward": {"ms": ms, "ms_min_max": spread, "speedup": round(ms / row["forward"]["ms"], 2), "rel_l2_vs_ours": float(f"{diff:.3g}")}}

    def torch_fb():
        s.grad = None
        (psf_of(s) * w).sum().backward()
    ms, spread = bd.windows(torch_fb, a.calls, 1, a.rounds)
    res["torch"]["forward_backward"] = {"ms": ms, "ms_min_max": spread, "speedup": round(ms / row["forward_backward_ms"], 2)}
    s.grad = None
    del m, hold, fwd, fwd_keep, bwd, psf_of
    torch.cuda.empty_cache()
    base = optic.RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs, cfg.wave_lengths, P, cfg.sample_interval, (R, R)).to(dev)
    bf, bfk, bb, hold = bd.raw_calls(base)
    res["base_same_R"] = timed(bf, bfk, bb, a)
    res["hybrid_over_base"] = {k: round(res["hybrid"][k]["ms"] / res["base_same_R"][k]["ms"], 3) for k in ("forward", "forward_keep", "backward")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
