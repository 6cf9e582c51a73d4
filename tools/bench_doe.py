#!/usr/bin/env python
"""The DOE wave-optics model (dprox.contrib.optic, dpx_doe_psf / dpx_doe_psf_backward): height map -> PSF forward, and forward +
backward, at the default configuration (1496 -> 748, padded rows of 2244 samples) and at 748 -> 374 (1122 samples).

Prints ONE JSON line (kept as profiles/doe_bench.json):
  * per size the ms per call of the C entry points on prepared arguments (hip events around `calls` back-to-back calls, `warmup`
    calls excluded; the median and the min .. max of `rounds` windows): `forward` (no field kept), `forward_keep` + `backward`
    (a training step's pair), and `ops_forward_backward_ms`, the same pair through RGBCollimator.get_psf() and autograd;
  * per launch the kernel time of one forward + backward (dpx_timing_*: start / stop events on the kernel's own dispatch packet),
    the bytes the algorithm needs in that launch, computed from the shapes below, and the fraction of the 6.29 TB/s measured copy
    rate they amount to;
  * the column launch with ONE column per workgroup, with the widest tile a CU's LDS holds, and with the number the library ships;
  * the same arithmetic as torch ops on the device (torch.fft, avg_pool2d, autograd; float32 / complex64) as the comparison;
  * one leg timing a whole training step of tools/bench_train.py's workload (2 x 3 x 748 x 748, ADMM unrolled x 10, conv_doe data
    term + frozen FFDNet-colour prior, MSE, backward, AdamW) with the DOE model in front of the PSF, against the same step with a free
    PSF parameter.

    python tools/bench_doe.py [--calls 10] [--warmup 2] [--rounds 3] [--no-train] [--no-baseline]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dprox import _backend as be  # noqa: E402
from dprox.contrib import optic  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, the chip's measured copy rate
SIZES = [(1496, 748), (748, 374)]


def launch_bytes(R, P):
    """bytes the algorithm needs per launch: s and gs [R][R] fp32, Z [3][R][M] and H [3][M][M] complex64, w [3][R][R] complex64,
    q / psf / g [3][P][P] fp32"""
    M = R + 2 * (R // 4)
    s, Z, H, w, q = 4 * R * R, 8 * 3 * R * M, 8 * 3 * M * M, 8 * 3 * R * R, 4 * 3 * P * P
    return {"fwd": {"k_doe_rows_in": s + Z, "k_doe_cols": 2 * Z + H, "k_doe_rows_out": Z + q + w, "k_doe_normalise": 2 * q},
            "bwd": {"k_doe_dot": 2 * q, "k_doe_rows_in": w + q + Z, "k_doe_cols": 2 * Z + H, "k_doe_rows_grad": Z + s + s}}


def time_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def windows(fn, calls, warmup, rounds):
    ms = [time_ms(fn, calls, warmup if r == 0 else 1) for r in range(rounds)]
    return round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]


def raw_calls(m):
    """(forward without a field, forward keeping it, backward) as calls of the C entry points on prepared arguments"""
    L, p = be.lib(), be.ptr
    c = m._context()
    s = m.height_map.height_map_sqrt.detach()
    psf, g, gs = torch.empty(1, 3, c.P, c.P, device=s.device), torch.randn(1, 3, c.P, c.P, device=s.device), torch.empty_like(s)
    ws0 = torch.empty(c.ws_bytes(False), dtype=torch.uint8, device=s.device)
    ws1 = torch.empty(c.ws_bytes(True), dtype=torch.uint8, device=s.device)
    fwd = lambda keep, ws: L.call("dpx_doe_psf", p(s), None, c.wl, c.ri, p(psf), p(c.H), p(c.table), c.R, c.P, keep, c.cols_per_wg, p(ws), be.stream())
    bwd = lambda: L.call("dpx_doe_psf_backward", p(g), p(psf), p(s), c.wl, c.ri, p(gs), p(c.H), p(c.table), c.R, c.P, c.cols_per_wg, p(ws1), be.stream())
    return (lambda: fwd(0, ws0)), (lambda: fwd(1, ws1)), bwd, (psf, g, gs, ws0, ws1)


def kernel_times(fn):
    """{kernel: [ms per launch, in launch order collapsed by name]} of one call of fn (dpx_timing_*)"""
    L = be.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    L.call("dpx_timing_enable", 1)
    L.call("dpx_timing_report", buf, len(buf))
    fn()
    torch.cuda.synchronize()
    L.call("dpx_timing_report", buf, len(buf))
    L.call("dpx_timing_enable", 0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, tot = line.split()
        out[name] = (int(cnt), float(tot))
    return out


def per_launch(fn, nbytes, reps=5):
    """median kernel time per launch over `reps` timed calls, with the algorithmic bytes and the copy-rate fraction"""
    runs = [kernel_times(fn) for _ in range(reps + 1)][1:]
    out = {}
    for name, b in nbytes.items():
        ms = statistics.median(r[name][1] / r[name][0] for r in runs)
        out[name] = {"ms": round(ms, 4), "algorithmic_MB": round(b / 1e6, 1), "copy_rate_fraction": round(b / (ms * 1e-3) / COPY_RATE, 3) if ms > 0 else None}
    return out


def torch_model(m):
    """the same arithmetic as torch ops on the device, float32 / complex64: (psf of s)"""
    dev = m.height_map.height_map_sqrt.device
    c = m._context()
    R, P, p = c.R, c.P, c.R // 4
    H = (c.H * (c.M * c.M)).clone()
    ap = m.aperture
    k = torch.tensor([2 * np.pi / c.wl[i] * (c.ri[i] - 1) for i in range(3)], dtype=torch.float32, device=dev).view(1, 3, 1, 1)

    def psf_of(s):
        u = ap * torch.exp(1j * (k * s ** 2))
        w = torch.fft.ifft2(torch.fft.fft2(torch.nn.functional.pad(u, [p, p, p, p])) * H)[:, :, p:p + R, p:p + R]
        q = torch.nn.functional.avg_pool2d(w.real ** 2 + w.imag ** 2, R // P, R // P)
        return q / q.sum()
    return psf_of


def train_leg(steps, warmup, dev="cuda", R=1496, denoiser=None):
    """ms per training step of tools/bench_train.py's workload at 748 x 748 with (a) the free PSF parameter, (b) the DOE model in front
    (dev, R, denoiser: a smoke run on the SIMT emulator takes a small wavefront and a small network)"""
    import dprox as dp
    import synthetic
    from dprox.algo.training import TrainLoop
    from dprox.proxfn.pnp.denoisers import FFDNetColorDenoiser
    bs, size, iters = 2, R // 2, 10
    cfg = optic.DOEModelConfig()
    model = lambda: optic.RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs, cfg.wave_lengths, size, cfg.sample_interval, (R, R)).to(dev)
    out = {"workload": f"{bs}x3x{size}x{size}, ADMM unrolled x{iters}: sum_squares(conv_doe(x, PSF), b) + deep_prior(ffdnet_color, frozen), MSE, "
                       "backward, AdamW step"}
    for tag in ("free_psf_parameter", "doe_model"):
        rng = np.random.RandomState(2024)
        gt = torch.from_numpy((synthetic.synth_detail if size >= 256 else synthetic.synth)(rng, bs, 3, size, size)).to(dev)
        noise = torch.from_numpy((rng.randn(bs, 3, size, size) * 7.65 / 255).astype(np.float32)).to(dev)
        rhos, sig = dp.log_descent(49, 7.65, iters, sigma=7.65 / 255)
        if tag == "free_psf_parameter":
            class Free(torch.nn.Module):
                def __init__(self):
                    super().__init__()
                    self.psf = torch.nn.Parameter(torch.full((1, 3, size, size), 1.0 / (3 * size * size)))

                def get_psf(self):
                    p = self.psf.clamp_min(0)
                    return p / p.sum()
            m = Free().to(dev)
            with torch.no_grad():
                m.psf.copy_(model().get_psf())      # the same starting PSF in both legs
        else:
            m = model()
        m.rhos, m.lams = torch.nn.Parameter(rhos.float().to(dev)), torch.nn.Parameter(sig.float().to(dev))
        x, Pp, Bv = dp.Variable(), dp.Placeholder(), dp.Placeholder()
        reg = dp.deep_prior(x, denoiser=denoiser() if denoiser else FFDNetColorDenoiser(synthetic.ffdnet_weights(7)), trainable=False)
        solver = dp.compile(dp.sum_squares(dp.conv_doe(x, Pp, circular=True), Bv) + reg, method="admm", device=dev)
        solver = dp.specialize(solver, method="unroll", device=dev, max_iter=iters)
        loop = TrainLoop(torch.nn.ModuleList([m]), lr=1e-4, weight_decay=1e-3, savedir=os.path.join("/tmp", f"dpx_bench_doe_{os.getpid()}"))

        def step():
            psf = m.get_psf()
            Pp.value = psf
            inp = optic.img_psf_conv(gt, psf, circular=True) + noise
            Bv.value = inp
            pred = solver.solve(x0=inp.detach(), rhos=m.rhos, lams={reg: m.lams.sqrt()})
            return loop.step(gt, pred)
        for _ in range(warmup):
            l0, _ = step()
        ms, last = [], [l0]
        for _ in range(steps):
            ms.append(time_ms(lambda: last.__setitem__(0, step()[0]), 1, 0))
        leaf = m.psf if tag == "free_psf_parameter" else m.height_map.height_map_sqrt
        out[tag] = {"ms_per_step": round(statistics.median(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "steps": steps,
                    "loss_first": float(l0), "loss_last": float(last[0]), "grad_norm_of_the_optics_parameter": float(leaf.grad.norm())}
        del m, solver, loop
    out["doe_model_extra_ms_per_step"] = round(out["doe_model"]["ms_per_step"] - out["free_psf_parameter"]["ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=5)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = be.lib()
    res = {"metric": "doe_psf", "device": torch.cuda.get_device_name(dev), "copy_rate_TBps": COPY_RATE / 1e12,
           "timing": f"median of {a.rounds} windows of {a.calls} back-to-back calls; (min, max) alongside; per-launch: median of 5 calls' kernel times",
           "normalise": "a launch of its own (k_doe_normalise), not the tail of the last row workgroup", "cases": {}}
    for R, P in SIZES:
        cfg = optic.DOEModelConfig()
        m = optic.RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs, cfg.wave_lengths, P, cfg.sample_interval, (R, R)).to(dev)
        c = m._context()
        fwd, fwd_keep, bwd, hold = raw_calls(m)
        row = {"M": c.M, "cols_per_wg_shipped": L.query("dpx_doe_cols_per_wg", R, 0), "cols_per_wg_widest": L.query("dpx_doe_cols_per_wg", R, 1)}
        for key, fn in (("forward", fwd), ("forward_keep", fwd_keep), ("backward", bwd)):
            ms, spread = windows(fn, a.calls, a.warmup, a.rounds)
            row[key] = {"ms": ms, "ms_min_max": spread}
        row["forward_backward_ms"] = round(row["forward_keep"]["ms"] + row["backward"]["ms"], 4)
        w = hold[1]

        def through_ops():
            m.height_map.height_map_sqrt.grad = None
            (m.get_psf() * w).sum().backward()
        ms, spread = windows(through_ops, a.calls, a.warmup, a.rounds)
        row["ops_forward_backward_ms"] = {"ms": ms, "ms_min_max": spread}
        nb = launch_bytes(R, P)
        row["launches_forward"] = per_launch(fwd_keep, nb["fwd"])
        row["launches_backward"] = per_launch(bwd, nb["bwd"])
        cols = {}
        for label, ct in (("one", 1), ("widest", row["cols_per_wg_widest"]), ("shipped", 0)):
            c.cols_per_wg = ct
            ms, spread = windows(fwd, a.calls, 1, a.rounds)
            k = per_launch(fwd, {"k_doe_cols": nb["fwd"]["k_doe_cols"]})["k_doe_cols"]
            cols[label] = {"cols_per_wg": ct or row["cols_per_wg_shipped"], "forward_ms": ms, "forward_ms_min_max": spread, "k_doe_cols_ms": k["ms"],
                           "copy_rate_fraction": k["copy_rate_fraction"]}
        c.cols_per_wg = 0
        row["column_tile"] = cols
        if not a.no_baseline:
            psf_of = torch_model(m)
            s = m.height_map.height_map_sqrt
            with torch.no_grad():
                ms, spread = windows(lambda: psf_of(s), a.calls, 1, a.rounds)
                diff = float((psf_of(s) - m.get_psf()).norm() / m.get_psf().norm())
            row["torch_forward"] = {"ms": ms, "ms_min_max": spread, "speedup": round(ms / row["forward"]["ms"], 2), "rel_l2_vs_ours": float(f"{diff:.3g}")}

            def torch_fb():
                s.grad = None
                (psf_of(s) * w).sum().backward()
            ms, spread = windows(torch_fb, a.calls, 1, a.rounds)
            row["torch_forward_backward"] = {"ms": ms, "ms_min_max": spread, "speedup": round(ms / row["forward_backward_ms"], 2)}
            s.grad = None
        res["cases"][f"{R}->{P}"] = row
        del m, hold, fwd, fwd_keep, bwd
        torch.cuda.empty_cache()
    if not a.no_train:
        res["train_step"] = train_leg(a.train_steps, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
