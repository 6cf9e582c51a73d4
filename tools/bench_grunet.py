#!/usr/bin/env python
"""The GRUNet denoise (dpx_grunet_forward, csrc/dpx_qrnn3d.hip) at 1 x 31 x 512 x 512 -- the cube of the reference's hyperspectral examples --
and at 1 x 31 x 256 x 256, in the default split-f16 arithmetic (and split-bf16 with --modes f16x2,bf16x3).

Prints ONE JSON line (and, with --out, writes it to that file after every finished part): per shape the ms per call of the C entry point
on prepared arguments (hip events around `calls` back-to-back calls, `warmup` calls excluded; the median and the min .. max of `rounds`
windows), the fp32-equivalent TFLOP/s from the module's own MAC count (2 x grunet_macs_per_voxel x voxels), and per layer class -- the
library's per-kernel events (dpx_timing_enable) over one more call -- the ms of its convolutions and of its pooling passes, the class's
TFLOP/s, and the pooling passes' algorithmic bytes (gate channels read once, hidden channels written once; a bidirectional layer's
second walk is not counted) as a fraction of the 6.29 TB/s measured copy rate.  Baseline: the same arithmetic as torch ops on the device
(F.conv3d / F.conv_transpose3d, F.interpolate, the scan as a loop over the bands), on the module's own weights, timed the same way and
compared with ours on the residual.

    python tools/bench_grunet.py [--calls 5] [--warmup 2] [--rounds 3] [--baseline-calls 2] [--no-baseline] [--shapes 31x512x512,31x256x256]
                                 [--baseline-shapes 31x256x256]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "delta-prox_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dprox import _backend as be  # noqa: E402
from dprox import _ops as ops  # noqa: E402
from dprox.proxfn.pnp.denoisers import GRUNET_MODES, GRUnet, grunet_layer_table, grunet_macs_per_voxel  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, the chip's measured copy rate
SIGMA = 0.1
CLASSES = {"Conv1": "Conv1", "Down": "Down", "Conv2": "Conv2-5", "Conv3": "Conv2-5", "Conv4": "Conv2-5", "Conv5": "Conv2-5", "Up_conv": "Up_conv", "Up": "Up",
           "Conv": "Conv"}


def layer_class(key):
    head = key.split(".")[0]
    for prefix in ("Up_conv", "Down", "Up"):
        if head.startswith(prefix):
            return prefix
    return CLASSES[head]


def seeded(net, seed=470):
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if v.ndim > 1:
            fan = v.shape[1] * v[0, 0].numel()
        b = 1.0 / fan ** 0.5
        sd[k] = (torch.rand(v.shape, generator=gen) * 2 - 1) * b
    net.load_state_dict(sd, strict=True)
    return net


# ---- the baseline: the reference's arithmetic as torch ops --------------------------------------------------------------------------
def pool_torch(gates, C, direction):
    def scan(Z, Fg, rev):
        D, h, out = Z.shape[2], None, [None] * Z.shape[2]
        for s in range(D):
            d = D - 1 - s if rev else s
            z, f = Z[:, :, d], Fg[:, :, d]
            h = (1 - f) * z if h is None else f * h + (1 - f) * z
            out[d] = h
        return torch.stack(out, dim=2)
    Z = gates[:, :C].tanh()
    if direction == "bi":
        return scan(Z, gates[:, C:2 * C].sigmoid(), False) + scan(Z, gates[:, 2 * C:].sigmoid(), True)
    return scan(Z, gates[:, C:].sigmoid(), direction == "rev")


def layer_torch(x, w, bias, form, hidden, direction, tr):
    if form == "up":
        x = F.interpolate(x, scale_factor=(1, 2, 2), mode="trilinear", align_corners=True)
    pad = 0 if form == "k1" else 1
    if tr:
        gates = F.conv_transpose3d(x, w, bias, stride=1, padding=pad)
    else:
        gates = F.conv3d(x, w, bias, stride=(1, 2, 2) if form == "down" else 1, padding=pad)
    return pool_torch(gates, hidden, direction)


def forward_torch(net, x, sigma):
    T = {k: (net.ref_param(k), form, hidden, direction, tr) for k, form, _, hidden, direction, tr, _ in net.table}
    run = lambda key, t, bias=None: layer_torch(t, T[key][0], bias, *T[key][1:])
    block = lambda name, t, de: (run(f"{name}.conv2.conv.{de}.weight", run(f"{name}.conv1.conv.{de}.weight", t))
                                 + run(f"{name}.conv_residual.conv.{de}.weight", t))
    N, D, H, W = x.shape
    inp = torch.stack([x, sigma.view(N, 1, 1, 1).expand(N, D, H, W)], dim=1)
    e = [run("Conv1.conv.conv.weight", inp)]
    for l in range(1, 5):
        e.append(block(f"Conv{l + 1}", run(f"Down{l}.conv.conv.weight", e[-1]), "conv"))
    d = e[4]
    for l in (5, 4, 3, 2):
        d = block(f"Up_conv{l}", torch.cat((e[l - 2], run(f"Up{l}.conv.upsample_conv.conv3d.weight", d)), dim=1), "deconv")
    return run("Conv.conv.deconv.weight", d, net.ref_param("Conv.conv.deconv.bias"))[:, 0] + x


# ---- timing -------------------------------------------------------------------------------------------------------------------------
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
    return statistics.median(ms), [round(min(ms), 3), round(max(ms), 3)]


def per_class(fn, voxels):
    """one call under the library's per-kernel events -> {class: conv_ms, pool_ms, ...}"""
    L = be.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    L.call("dpx_timing_report", buf, len(buf))           # (drop what is there)
    L.call("dpx_timing_enable", 1)
    fn()
    torch.cuda.synchronize()
    L.call("dpx_timing_enable", 0)
    L.call("dpx_timing_report", buf, len(buf))
    rows = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        kernel, _, cls = name.partition(".")
        if kernel in ("k_conv3d_gates", "k_qrnn_pool") and cls:
            rows.setdefault(cls, {})["conv_ms" if kernel == "k_conv3d_gates" else "pool_ms"] = round(float(ms), 3)
            rows[cls]["conv_launches" if kernel == "k_conv3d_gates" else "pool_launches"] = int(cnt)
        elif kernel == "k_qrnn_to_c8":
            rows.setdefault("input", {})["pack_ms"] = round(float(ms), 3)
    macs, pool_bytes = {}, {}
    for key, form, cin, hidden, direction, _, level in grunet_layer_table(2):
        cls, gates, v = layer_class(key), hidden * (3 if direction == "bi" else 2), voxels / 4.0 ** level
        macs[cls] = macs.get(cls, 0.0) + (1 if form == "k1" else 27) * cin * gates * v
        # a block's conv_residual branch is pooled in its conv2's pass and writes nothing of its own
        pool_bytes[cls] = pool_bytes.get(cls, 0.0) + 4.0 * v * (gates + (0 if "conv_residual" in key else hidden))
    for cls, row in rows.items():
        if cls in macs:
            row["GMAC"] = round(macs[cls] / 1e9, 2)
            row["conv_TFLOPs_fp32_equivalent"] = round(2 * macs[cls] / (row["conv_ms"] * 1e-3) / 1e12, 1)
            row["pool_algorithmic_MB"] = round(pool_bytes[cls] / 1e6, 1)
            row["pool_copy_rate_fraction"] = round(pool_bytes[cls] / (row["pool_ms"] * 1e-3) / COPY_RATE, 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--modes", default="f16x2")
    ap.add_argument("--shapes", default="31x512x512,31x256x256")
    ap.add_argument("--baseline-shapes", default="31x256x256", help="the shapes whose torch baseline is timed: at 31x512x512 torch's own "
                    "3-D convolutions did not get through their first call inside 390 s on the box the committed numbers come from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    macs = grunet_macs_per_voxel(2)
    res = {"metric": "grunet_forward", "device": torch.cuda.get_device_name(dev), "copy_rate_TBps": COPY_RATE / 1e12, "macs_per_voxel": macs,
           "timing": f"median of {a.rounds} windows of {a.calls} back-to-back calls; (min, max) alongside; per class: the kernels' own events over one call",
           "yardsticks": {"ffdnet_split_f16_layers_TFLOPs_fp32_equivalent": 348, "three_product_split_f16_floor_ms_31x512x512": 7.5}, "cases": {}}

    def emit():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    net = seeded(GRUnet(in_ch=2)).to(dev).eval()
    L, ptr = be.lib(), be.ptr
    for shape in a.shapes.split(","):
        D, H, W = (int(s) for s in shape.split("x"))
        voxels = D * H * W
        x = torch.rand(1, D, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(D + H))
        sig = torch.full((1,), SIGMA, device=dev)
        y = torch.empty_like(x)
        ws = ops._bytes(L.query("dpx_grunet_ws_bytes", 1, D, H, W), dev)
        row = {"voxels": voxels, "GMAC": round(macs * voxels / 1e9, 1), "workspace_MB": round(ws.numel() / 1e6, 1)}
        for mode in a.modes.split(","):
            mid = GRUNET_MODES[mode]
            blob = net.packed(mid)
            fn = lambda: L.call("dpx_grunet_forward", ptr(x), ptr(sig), ptr(y), ptr(blob), 2, mid, 1, D, H, W, ptr(ws), be.stream())
            ms, spread = windows(fn, a.calls, a.warmup, a.rounds)
            row[mode] = {"ms": round(ms, 3), "ms_min_max": spread, "TFLOPs_fp32_equivalent": round(2 * macs * voxels / (ms * 1e-3) / 1e12, 1),
                         "per_class": per_class(fn, voxels)}
            assert not L.query("dpx_ffdnet_f16_overflow", 1)
            res["cases"][shape] = row
            emit()
        if not a.no_baseline and shape in a.baseline_shapes.split(","):
            with torch.no_grad():
                net.compute_mode = a.modes.split(",")[0]
                ours = net(x, sig)
                theirs = forward_torch(net, x, sig)
                row["residual_rel_l2_vs_torch"] = float(f"{((ours - theirs).norm() / (theirs - x).norm()).item():.3g}")
                del ours, theirs
                ms, spread = windows(lambda: forward_torch(net, x, sig), a.baseline_calls, 1, a.rounds)
            first = row[a.modes.split(",")[0]]
            row["torch"] = {"ms": round(ms, 3), "ms_min_max": spread, "TFLOPs": round(2 * macs * voxels / (ms * 1e-3) / 1e12, 1)}
            first["speedup_vs_torch"] = round(ms / first["ms"], 2)
            emit()
        del x, y, ws
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
