"""GRUNet cases shared by the GPU tests (-m gpu, real MI355X), the emulated-kernel tests (CPU, the same kernel source under the SIMT
emulator), the guarded-workspace tests and the fixture generator (tests/golden/make_golden_grunet.py, which imports this module next to
the REFERENCE's ``dprox`` -- so nothing at module level imports ours).

Weights are not stored (the network has 14 278 451 parameters): ``grunet_weights(seed, shapes)`` draws them, the generator and the tests
alike.  Fixtures (g47_grunet_layers*.npz, g47_grunet_net.npz) hold the inputs, the reference's float64 result `<key>_o64` and its float32
result as `<key>_obits`, the int32 distance of its bit pattern from that of the float64 one rounded to float32.

The bound (README "parity"; nothing chosen here): on the RESIDUAL ``out - input`` of the network (a layer has no skip: its output), the
relative l2 distance from the reference's float64 run is at most the reference's own float32 distance from it plus 1e-5, and the distance
from the reference's float32 run at most the sum of the two."""
import json
import os

import numpy as np

SLACK = 1e-5
ACHIEVED = {}          # case -> distances; written to the file DPX_GRUNET_PARITY_OUT names, if it is set (write_achieved)
NET_SEED = 470

# name -> (kind, cin, hidden, k, reverse, shape of x [N, cin, D, H, W]); kinds: the reference's layer classes
#   conv QRNNConv3D | down QRNNConv3D s=(1,2,2) | deconv QRNNDeConv3D | up QRNNUpsampleConv3d | bi BiQRNNConv3D | bide BiQRNNDeConv3D (bias)
# shapes: 3 x 6 x 10 (less than one 64-pixel wave tile), 1 x 4 x 4 (D = 1: every depth tap but the centre is padding), 2 x 18 x 34 (two cubes,
# 612 pixels: ten wave tiles, the last one ragged, rows crossing tile borders) and, where a float64 fixture of that size would not fit a
# committed file, 2 x 10 x 18 (two cubes, 180 pixels: three wave tiles, the last one ragged; upsampled 20 x 36: twelve)
S1, S2, S3, S3B = (1, 3, 6, 10), (1, 1, 4, 4), (2, 2, 18, 34), (2, 2, 10, 18)
LAYERS = {
    "k3_fwd_s1": ("conv", 8, 16, 3, False, S1), "k3_rev_s3": ("conv", 8, 16, 3, True, S3), "k3_fwd_s2": ("conv", 16, 32, 3, False, S2),
    "down_rev_s1": ("down", 8, 16, 3, True, S1), "down_fwd_s3b": ("down", 16, 32, 3, False, S3B), "down_rev_s2": ("down", 8, 16, 3, True, S2),
    "k1_fwd_s1": ("conv", 8, 16, 1, False, S1), "k1_rev_s3b": ("conv", 16, 32, 1, True, S3B),
    "deconv_fwd_s1": ("deconv", 16, 32, 3, False, S1), "deconv_rev_s2": ("deconv", 8, 16, 3, True, S2), "deconv_rev_s3b": ("deconv", 8, 16, 3, True, S3B),
    "deconv_k1_rev_s1": ("deconv", 16, 32, 1, True, S1), "deconv_k1_fwd_s2": ("deconv", 8, 16, 1, False, S2),
    "up_rev_s1": ("up", 8, 16, 3, True, S1), "up_fwd_s2": ("up", 16, 32, 3, False, S2), "up_fwd_s3b": ("up", 8, 16, 3, False, S3B),
    "bi_s1": ("bi", 2, 16, 3, None, S1), "bi_s3": ("bi", 2, 16, 3, None, S3), "bide_s1": ("bide", 16, 1, 3, None, S1), "bide_s2": ("bide", 16, 1, 3, None, S2),
    "saturated_s1": ("conv", 8, 16, 3, False, S1),           # weights x 100: gates of +-60 and more
}
SATURATED_GAIN = 100.0
# pool(conv k3 16 -> 32 on xa) + pool(conv k1 8 -> 32 on xb), forward, written to channels [8, 40) of a 48-channel destination
RESIDUAL = dict(cin_a=16, cin_b=8, hidden=32, shape=S1, out_channels=48, out_offset=8)
# name -> ([N, B, H, W], sigma per image)
NETS = {"n_3x16x16": ((1, 3, 16, 16), (0.1,)), "n_1x16x16": ((1, 1, 16, 16), (0.1,)), "n_5x16x32": ((1, 5, 16, 32), (0.1,)),
        "n_2x32x48": ((1, 2, 32, 48), (0.1,)), "n_b2_3x16x16": ((2, 3, 16, 16), (0.1, 0.3))}
FORM = {"conv": 0, "down": 1, "deconv": 0, "up": 3, "bi": 0, "bide": 0}


def grunet_weights(seed, shapes):
    """{key: float32 array}: np.random.RandomState(seed).uniform(-b, b) with b = 1 / sqrt(fan_in) per tensor, drawn in the order of
    ``shapes`` (a list of (key, shape) in state-dict order); fan_in = shape[1] * taps as torch counts it, a bias takes its weight's"""
    rng, out, fan = np.random.RandomState(seed), {}, 1
    for key, shape in shapes:
        if len(shape) > 1:
            fan = int(shape[1]) * int(np.prod(shape[2:]))
        b = 1.0 / np.sqrt(fan)
        out[key] = rng.uniform(-b, b, size=tuple(shape)).astype(np.float32)
    return out


def layer_weight_shape(kind, cin, hidden, k):
    gates = hidden * (3 if kind in ("bi", "bide") else 2)
    return (cin, gates, k, k, k) if kind in ("deconv", "bide") else (gates, cin, k, k, k)


def layer_params(name):
    """(weight, bias or None) of a layer case"""
    kind, cin, hidden, k, _, _ = LAYERS[name]
    seed = 4700 + sorted(LAYERS).index(name)
    shapes = [("w", layer_weight_shape(kind, cin, hidden, k))] + ([("b", (3 * hidden,))] if kind == "bide" else [])
    p = grunet_weights(seed, shapes)
    if name.startswith("saturated"):
        p["w"] = p["w"] * np.float32(SATURATED_GAIN)
    return p["w"], p.get("b")


def layer_input(name):
    _, cin, _, _, _, (N, D, H, W) = LAYERS[name]
    return np.random.RandomState(4800 + sorted(LAYERS).index(name)).randn(N, cin, D, H, W).astype(np.float32)


def residual_case():
    R = RESIDUAL
    N, D, H, W = R["shape"]
    p = grunet_weights(4790, [("wa", layer_weight_shape("conv", R["cin_a"], R["hidden"], 3)), ("wb", layer_weight_shape("conv", R["cin_b"], R["hidden"], 1))])
    rng = np.random.RandomState(4791)
    return p["wa"], p["wb"], rng.randn(N, R["cin_a"], D, H, W).astype(np.float32), rng.randn(N, R["cin_b"], D, H, W).astype(np.float32)


def net_input(name):
    shape, sigma = NETS[name]
    return np.random.RandomState(4900 + sorted(NETS).index(name)).rand(*shape).astype(np.float32), np.asarray(sigma, np.float32)


def range_input():
    """an ordinary 1 x 1 x 16 x 16 cube with a 2 x 2 patch of 1e5: outside the binary16 range"""
    x = np.random.RandomState(4950).rand(1, 1, 16, 16).astype(np.float32)
    x[0, 0, 3:5, 3:5] = 1e5
    return x, np.asarray([0.1], np.float32)


def admm_input():
    return np.random.RandomState(4960).rand(1, 3, 16, 16).astype(np.float32)


# ---- everything below runs against OUR package -------------------------------------------------------------------------------------
_golden = {}


def golden():
    if not _golden:
        from conftest import load_golden
        for f in ("g47_grunet_layers", "g47_grunet_layers_s3", "g47_grunet_layers_s3b", "g47_grunet_net"):
            _golden.update(load_golden(f))
        for k in [k for k in _golden if k.endswith("_obits")]:
            r64 = _golden[k[:-6] + "_o64"]
            _golden[k[:-6] + "_o32"] = (r64.astype(np.float32).view(np.int32) + _golden[k]).view(np.float32)
    return _golden


def T(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def check(name, ours, base=None, tag=""):
    """the module's bound for one comparison; base: what is subtracted first (the network's input); tag: suffix of the achieved-distance key"""
    from conftest import record, rel_l2
    g = golden()
    o64, o32 = g[f"{name}_o64"], g[f"{name}_o32"]
    ours = np.asarray(ours)
    assert ours.shape == o64.shape and ours.dtype == np.float32 and np.isfinite(ours).all(), (name, ours.shape, o64.shape)
    if base is not None:
        o64, o32, ours = o64 - base.astype(np.float64), o32.astype(np.float64) - base, ours.astype(np.float64) - base
    d64, theirs, d32 = rel_l2(ours, o64), rel_l2(o32, o64), rel_l2(ours, o32)
    ACHIEVED[name + tag] = dict(ours_vs_ref64=d64, ref32_vs_ref64=theirs, ours_vs_ref32=d32, bound=theirs + SLACK)
    record(f"grunet {name} vs the reference's float64 run", d64, theirs + SLACK)
    print(f"grunet {name}: |ours - ref64| {d64:.3e}; the reference's float32 run {theirs:.3e}; |ours - ref32| {d32:.3e}")
    assert d64 <= theirs + SLACK, (name, d64, theirs)
    assert d32 <= 2 * theirs + SLACK, (name, d32, theirs)         # (the sum of the two: (theirs + SLACK) + theirs)
    return d64


def pack_layer(L, w, b, form, cin, gates, tr, mode, device):
    from dprox import _backend as be, _ops as ops
    blob = ops._bytes(L.query("dpx_qrnn3d_packed_bytes", form, cin, gates, mode), device)
    wt, bt = T(w, device), (T(b, device) if b is not None else None)
    L.call("dpx_qrnn3d_pack", be.ptr(blob), be.ptr(wt), be.ptr(bt), form, cin, gates, int(tr), mode, be.stream())
    return blob


def run_layer(device, x, w, b, kind, hidden, k, reverse, mode=3, second=None, out_channels=None, out_offset=0, alloc=None):
    """dpx_qrnn3d_layer on one reference layer; second = (xr, wr) adds a k = 1 QRNNConv3D on xr; alloc: the workspace allocator"""
    import torch
    from dprox import _backend as be, _ops as ops
    L = be.lib()
    N, cin, D, H, W = x.shape
    form = 2 if k == 1 else FORM[kind]
    direction = 2 if reverse is None else int(bool(reverse))
    gates = hidden * (3 if direction == 2 else 2)
    blob = pack_layer(L, w, b, form, cin, gates, kind in ("deconv", "bide"), mode, device)
    xr, blob_r, cin_r = None, None, 0
    if second is not None:
        xr, cin_r = T(second[0], device), second[0].shape[1]
        blob_r = pack_layer(L, second[1], None, 2, cin_r, gates, False, mode, device)
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if form == 1 else ((2 * H, 2 * W) if form == 3 else (H, W))
    Ct = out_channels or hidden
    out = torch.full((N, Ct, D, Ho, Wo), -7.0, dtype=torch.float32, device=device)
    nbytes = L.query("dpx_qrnn3d_layer_ws_bytes", form, 2, N, cin, cin_r, hidden, direction, D, H, W)
    assert nbytes > 0
    ws = (alloc or ops._bytes)(nbytes, device)
    xt = T(x, device)
    L.call("dpx_qrnn3d_layer", be.ptr(xt), be.ptr(blob), be.ptr(xr), be.ptr(blob_r), be.ptr(out), form, 2, N, cin, cin_r, hidden, direction, D, H, W,
           Ct, out_offset, mode, be.ptr(ws), be.stream())
    return out, nbytes


def case_layer(device, name, mode=3, alloc=None):
    kind, cin, hidden, k, reverse, _ = LAYERS[name]
    w, b = layer_params(name)
    out, nbytes = run_layer(device, layer_input(name), w, b, kind, hidden, k, reverse, mode, alloc=alloc)
    check(f"l_{name}", out.cpu().numpy(), tag="" if mode == 3 else "_bf16x3")
    return nbytes


def case_saturated(device):
    from dprox import _backend as be
    g = golden()
    assert np.abs(g["l_saturated_s1_gmax"]) >= 60.0, "the fixture's gates do not reach +-60"
    case_layer(device, "saturated_s1")
    case_layer(device, "saturated_s1", mode=6)
    be.lib().query("dpx_ffdnet_f16_overflow", 1)


def case_residual_offset(device):
    R = RESIDUAL
    wa, wb, xa, xb = residual_case()
    out, _ = run_layer(device, xa, wa, None, "conv", R["hidden"], 3, False, second=(xb, wb), out_channels=R["out_channels"], out_offset=R["out_offset"])
    out = out.cpu().numpy()
    lo, hi = R["out_offset"], R["out_offset"] + R["hidden"]
    assert (out[:, :lo] == -7.0).all() and (out[:, hi:] == -7.0).all(), "channels outside the destination's slice were written"
    check("l_residual", np.ascontiguousarray(out[:, lo:hi]))


_nets = {}


def denoiser(device, mode="f16x2"):
    """GRUNetDenoiser on the seeded weights (one per device and mode, shared by the cases)"""
    import torch
    import dprox as dp
    key = (str(device), mode)
    if key not in _nets:
        den = dp.GRUNetDenoiser()
        sd = den.model.state_dict()
        w = grunet_weights(NET_SEED, [(k, tuple(v.shape)) for k, v in sd.items()])
        den.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        den = den.to(device).eval()
        den.model.compute_mode = mode
        _nets[key] = den
    return _nets[key]


def case_net(device, name):
    import torch
    x, sigma = net_input(name)
    den = denoiser(device)
    with torch.no_grad():
        y = den.denoise(T(x, device), T(sigma, device) if len(sigma) > 1 else torch.tensor(float(sigma[0])))
    assert den.model.compute_mode == "f16x2" and y.shape == x.shape
    check(name, y.cpu().numpy(), base=x)
    return y


def write_achieved():
    """the measured distances of the cases run so far -> the JSON file the environment variable DPX_GRUNET_PARITY_OUT names (how
    profiles/grunet_parity_achieved.json is produced from a GPU run); without the variable nothing is written"""
    path = os.environ.get("DPX_GRUNET_PARITY_OUT")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ACHIEVED, f, indent=1, sort_keys=True)


def case_registry(device, tmp_path):
    """deep_prior on an instance; the registry name without the checkpoint; a {'net': ...} checkpoint; the state-dict keys"""
    import pytest
    import torch
    import dprox as dp
    from dprox.proxfn.pnp import prior
    g = golden()
    den = denoiser(device)
    assert list(den.model.state_dict()) == [str(k) for k in g["keys"]]
    assert sum(v.numel() for v in den.model.state_dict().values()) == 14278451
    x, sigma = net_input("n_3x16x16")
    xt = T(x, device)
    with torch.no_grad():
        y = dp.deep_prior(dp.Variable(), denoiser=den).prox(xt, torch.tensor(float(sigma[0]), device=device))
    check("n_3x16x16", y.cpu().numpy(), base=x)
    old = prior.CACHE_DIR
    prior.CACHE_DIR = str(tmp_path)
    try:
        with pytest.raises(FileNotFoundError):
            dp.deep_prior(dp.Variable(), "grunet")
        os.makedirs(os.path.join(str(tmp_path), "pnp_denoisers"))
        torch.save({"net": {k: v.cpu() for k, v in den.model.state_dict().items()}, "epoch": 3}, os.path.join(str(tmp_path), "pnp_denoisers", "unet_qrnn3d.pth"))
        reg = dp.deep_prior(dp.Variable(), "grunet")
    finally:
        prior.CACHE_DIR = old
    assert isinstance(reg.denoiser, dp.GRUNetDenoiser)
    reg.denoiser.to(device)
    with torch.no_grad():
        assert torch.equal(reg.prox(xt, torch.tensor(float(sigma[0]), device=device)), y)
    for name, exc in (("qrnn3d", NotImplementedError), ("grunet_tv", NotImplementedError), ("nonesuch", ValueError)):
        with pytest.raises(exc):
            dp.deep_prior(dp.Variable(), name)
    with pytest.raises(NotImplementedError):
        dp.GRUNetTVDenoiser("x.pth")
    with pytest.raises(NotImplementedError):
        dp.QRNN3DDenoiser("x.pth")
    with pytest.raises(NotImplementedError, match="batch-norm"):
        dp.GRUnet(in_ch=2, bn=True)
    with pytest.raises(NotImplementedError, match="205"):
        dp.GRUnet(in_ch=2).load_reference_state_dict({f"k{i}": torch.zeros(1) for i in range(205)})


def case_scalar_sigma_batch(device):
    """one sigma for two cubes = two single calls, bit for bit"""
    import torch
    x, _ = net_input("n_b2_3x16x16")
    den, xt = denoiser(device), T(x, device)
    with torch.no_grad():
        both = den.denoise(xt, torch.tensor(0.2))
        one = [den.denoise(xt[i:i + 1].contiguous(), torch.tensor(0.2)) for i in range(2)]
    assert torch.equal(both, torch.cat(one))


def case_admm(device):
    import torch
    import dprox as dp
    b = T(admm_input(), device)
    x = dp.Variable()
    reg = dp.deep_prior(x, denoiser=denoiser(device))
    with torch.no_grad():
        out = dp.Problem(dp.sum_squares(x, b) + reg).solve(method="admm", device=device, x0=b.clone(), rhos=0.5, lams={reg: 0.05}, max_iter=3)
    check("admm", out.cpu().numpy(), base=admm_input())


def case_deterministic(device):
    import torch
    x, sigma = net_input("n_5x16x32")
    den = denoiser(device)
    with torch.no_grad():
        a = den.denoise(T(x, device), torch.tensor(float(sigma[0])))
        b = den.denoise(T(x, device), torch.tensor(float(sigma[0])))
    assert torch.equal(a, b)


def case_range(device):
    """a patch of 1e5 trips the binary16 range trap; denoise() reruns on split-bf16 and that result is the fixture's"""
    import warnings
    import torch
    import dprox as dp
    from dprox import _backend as be
    x, sigma = range_input()
    den = dp.GRUNetDenoiser()
    den.model.load_state_dict(denoiser(device).model.state_dict())
    den = den.to(device).eval()
    assert den.model.compute_mode == "f16x2"
    with torch.no_grad():
        den.model.f16_fallback = "raise"
        try:
            den.denoise(T(x, device), torch.tensor(float(sigma[0])))
        except be.F16RangeError:
            pass
        else:
            raise AssertionError("an input of 1e5 did not trip the binary16 range trap")
        den.model.f16_fallback = "bf16x3"
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            y = den.denoise(T(x, device), torch.tensor(float(sigma[0])))
    assert den.model.compute_mode == "bf16x3" and any(issubclass(i.category, RuntimeWarning) for i in w)
    check("range", y.cpu().numpy(), base=x, tag="_bf16x3")


def case_errors(device):
    import pytest
    import torch
    from dprox import _backend as be
    den = denoiser(device)
    s = torch.tensor(0.1)
    with torch.no_grad():
        with pytest.raises(ValueError, match="multiples of 16"):
            den.denoise(torch.zeros(1, 3, 24, 16, device=device), s)
        with pytest.raises(ValueError):
            den.denoise(torch.zeros(1, 0, 16, 16, device=device), s)
        with pytest.raises(ValueError, match="4-D"):
            den.model(torch.zeros(1, 1, 3, 16, 16, device=device), s)
    with pytest.raises(NotImplementedError, match="forward-only"):
        den.denoise(torch.zeros(1, 3, 16, 16, device=device, requires_grad=True), s)
    # the C ABI's own checks: DPX_ERR_ARG, nothing launched
    L, p = be.lib(), be.ptr
    x = torch.zeros(1, 3, 16, 16, device=device)
    y, sig = torch.empty_like(x), torch.full((1,), 0.1, device=device)
    blob = den.model.packed(3)
    ws = torch.zeros(L.query("dpx_grunet_ws_bytes", 1, 3, 16, 16), dtype=torch.uint8, device=device)
    assert L.query("dpx_grunet_ws_bytes", 1, 3, 24, 16) == 0 and L.query("dpx_grunet_ws_bytes", 1, 0, 16, 16) == 0
    assert L.query("dpx_grunet_packed_bytes", 2, 5) == 0 and L.query("dpx_qrnn3d_packed_bytes", 0, 8, 32, 4) == 0
    assert L.query("dpx_qrnn3d_layer_ws_bytes", 0, 0, 1, 8, 0, 16, 0, 0, 4, 4) == 0
    good = [p(x), p(sig), p(y), p(blob), 2, 3, 1, 3, 16, 16, p(ws), be.stream()]
    for idx, bad, msg in ((8, 24, "multiples of 16"), (9, 40, "multiples of 16"), (7, 0, "shape"), (5, 4, "mode"), (4, 3, "in_ch"), (0, None, "null"), (2, p(x), "in-place")):
        args = list(good)
        args[idx] = bad
        with pytest.raises(be.DpxError, match=msg):
            L.call("dpx_grunet_forward", *args)
    L.call("dpx_grunet_forward", *good)
