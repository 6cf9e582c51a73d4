"""compress_sensing cases shared by the GPU tests (-m gpu, real MI355X), the emulated-kernel tests (CPU, the same kernel source under the
SIMT emulator) and the host tests: ``ops.cs_xupdate`` / ``dp.compress_sensing`` against a float64 restatement written here and against
the reference's stored float32 and float64 runs (tests/golden/g46_cs*.npz, make_golden_cs.py).

Per pixel, channels c, I = num_psi:   s = sum m_c v_c,  phi = sum m_c^2,  d = phi + I lam,  r = (I y - s) / d,  x_c = (v_c + m_c r) / I;
for a cotangent g:  t = sum m_c g_c,  q = t / d,  gv_c = (g_c - m_c q) / I,  gy = q,  glam = -sum_hw q r,  gmask_c = (g_c r - q (v_c + 2 m_c r)) / I.

The elementwise bounds of ``case_prox`` (derived, u = float32 machine epsilon, every quantity of the right-hand sides taken from the
float64 restatement on the float32 inputs; `bounds` writes them out):
  a channel sum over C products          within (sqrt(C) + 4) u sum|terms|                           -> ds, dphi
  d = phi + I lam                        a product and a sum: dphi + 4 u (phi + I lam)               -> dd
  a = I y - s                            ds + 4 u (|I y| + |s|)                                       -> da
  r = a / d                              (da + |r| dd) / d + 4 u |r|                                  -> dr
  x_c = (v_c + m_c r) / I                4 u (|v_c| + |m_c r|) / I + |m_c| dr / I (+ dv_c / I)
  v_c = b_1 + .. + b_nb (summed in the kernel, or by the host first): 2 u per extra addend on sum_i |b_i,c| -> dv_c, which also enters ds
  through sum_c |m_c| dv_c.
Against the reference (round-off of two float32 programs, no number chosen in advance): the relative l2 distance from the reference's
float64 result is at most the distance of the reference's own float32 result from it, plus 1e-5 (README "parity"); gradients likewise,
each against the reference's float64 autograd.  glam, a sum over H W products q r, additionally stays within
(sqrt(H W) + 4) u sum|q r| of the restatement's value."""
import itertools
import json
import os

import numpy as np
import torch

import dprox as dp
from conftest import load_golden, record, rel_l2
from dprox import _ops as ops

SLACK = 1e-5
U = float(np.finfo(np.float32).eps)
PROX = {"p_one": (1, 2, 3), "p_hsi": (1, 2, 3), "p_hsi_sy": (2,), "p_wide": (1, 2, 3), "p_row": (1, 2, 3)}
GRADS = ("p_hsi", "p_hsi_sy", "p_row")
ADMM = ("admm_tv3d", "admm_two")
ACHIEVED = {}          # case -> distances; written to the file DPX_CS_PARITY_OUT names, if it is set (write_achieved)

_golden = {}


def golden():
    """the four fixture files as one dict; a float32 result stored as `<key>bits` (the int32 distance of its bit pattern from that of its
    float64 twin `<key>64` rounded to float32) comes back as `<key>32`"""
    if not _golden:
        for f in ("g46_cs", "g46_cs_hsi", "g46_cs_hsi_grad", "g46_cs_admm"):
            _golden.update(load_golden(f))
        for k in [k for k in _golden if k.endswith("bits")]:
            r64 = _golden[k[:-4] + "64"]
            _golden[k[:-4] + "32"] = (r64.astype(np.float32).view(np.int32) + _golden[k]).view(np.float32)
    return _golden


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def inputs(name):
    """(v, mask, y, lam) of a prox case, float32 NumPy"""
    g, base = golden(), "p_hsi" if name == "p_hsi_sy" else name
    return g[f"{base}_v"], g[f"{base}_mask"], g[f"{name}_y"], g[f"{base}_lam"]


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------
def restate(v, mask, y, lam, I):
    """both formula sets' forward half in float64 NumPy: v [N,C,H,W], mask [1|N,C,H,W], y [1|N,1,H,W], lam [N]"""
    v, m, y = np.asarray(v, np.float64), np.asarray(mask, np.float64), np.asarray(y, np.float64)
    lam = np.asarray(lam, np.float64).reshape(-1, 1, 1, 1)
    s = (m * v).sum(1, keepdims=True)
    phi = (m * m).sum(1, keepdims=True)
    d = phi + I * lam
    r = (I * y - s) / d
    return dict(s=s, phi=phi, d=d, r=r, x=(v + m * r) / I, m=m, v=v, y=y, lam=lam)


def restate_grad(g, v, mask, y, lam, I):
    """(gv, gy, glam, gmask, sum_hw |q r| per image) for the cotangent g; gy / gmask summed over the batch where y / mask is shared"""
    f, g = restate(v, mask, y, lam, I), np.asarray(g, np.float64)
    m, r = f["m"], f["r"]
    q = (m * g).sum(1, keepdims=True) / f["d"]
    gv = (g - m * q) / I
    gy = q if f["y"].shape[0] == g.shape[0] else q.sum(0, keepdims=True)
    gmask = (g * r - q * (f["v"] + 2 * m * r)) / I
    if m.shape[0] != g.shape[0]:
        gmask = gmask.sum(0, keepdims=True)
    return gv, gy, -(q * r).sum((1, 2, 3)), gmask, np.abs(q * r).sum((1, 2, 3))


def check_restatement():
    """the restatement is the reference's float64 arithmetic: every stored float64 output and gradient to 1e-12 relative"""
    g = golden()
    for name, Is in PROX.items():
        for I in Is:
            d = rel_l2(restate(*inputs(name), I)["x"], g[f"{name}_I{I}_x64"])
            assert d <= 1e-12, (name, I, d)
    for name in GRADS:
        I = int(g[f"g_{name}_I"])
        w = g["g_p_hsi_w" if name == "p_hsi_sy" else f"g_{name}_w"]
        gv, gy, glam, gmask, _ = restate_grad(w, *inputs(name), I)
        for k, ours in (("gv", gv), ("gy", gy), ("glam", glam), ("gmask", gmask)):
            ref = g[f"g_{name}_{k}64"]
            assert ours.shape == ref.shape, (name, k, ours.shape, ref.shape)
            d = rel_l2(ours, ref)
            assert d <= 1e-12, (name, k, d)


def bounds(f, I, bs=None):
    """the elementwise bound on x (module docstring) from the restatement `f`; bs: the float32 right-hand sides the device added up"""
    C = f["v"].shape[1]
    red = np.sqrt(C) + 4.0
    m, r = np.abs(f["m"]), np.abs(f["r"])
    dv = 0.0 if bs is None or len(bs) == 1 else 2 * U * (len(bs) - 1) * sum(np.abs(np.asarray(b, np.float64)) for b in bs)
    ds = red * U * np.abs(f["m"] * f["v"]).sum(1, keepdims=True) + (m * dv).sum(1, keepdims=True)
    dd = red * U * f["phi"] + 4 * U * (f["phi"] + I * f["lam"])
    da = ds + 4 * U * (np.abs(I * f["y"]) + np.abs(f["s"]))
    dr = (da + r * dd) / f["d"] + 4 * U * r
    return 4 * U * (np.abs(f["v"]) + m * r) / I + m * dr / I + dv / I


def _within(x, f, I, what, bs=None):
    err, tol = np.abs(x.astype(np.float64) - f["x"]), bounds(f, I, bs)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"{what}: largest elementwise error / bound {worst:.3f}")
    assert np.isfinite(x).all() and worst <= 1.0, (what, worst)
    return worst


def case_prox(device, name, I):
    g = golden()
    v, mask, y, lam = inputs(name)
    f = restate(v, mask, y, lam, I)
    vt, mt, yt, lt = T(v, device), T(mask, device), T(y, device), T(lam, device)
    x = ops.cs_xupdate([vt], yt, mt, lt, I)
    assert x.dtype == torch.float32 and x.shape == vt.shape and x.data_ptr() != vt.data_ptr() and not x.requires_grad
    xn = x.cpu().numpy()
    worst = _within(xn, f, I, f"cs prox {name} I={I}")
    x32, x64 = g[f"{name}_I{I}_x32"], g[f"{name}_I{I}_x64"]
    ours, theirs = rel_l2(xn, x64), rel_l2(x32, x64)
    ACHIEVED[f"{name}_I{I}"] = dict(ours_vs_ref64=ours, ref32_vs_ref64=theirs, bound=theirs + SLACK, worst_error_over_elementwise_bound=worst)
    record(f"cs prox {name} I={I} vs the reference's float64 run", ours, theirs + SLACK)
    print(f"cs prox {name} I={I}: |x - x64| {ours:.3e}; the reference's float32 run {theirs:.3e}")
    assert ours <= theirs + SLACK, (name, I, ours, theirs)
    # the same launch behind the term's own interface; the other spellings of mask and y
    term = dp.compress_sensing(dp.Variable(), mt, yt)
    assert torch.equal(term._prox(vt, lt, I), x) and torch.equal(term.solve([vt] + [torch.zeros_like(vt)] * (I - 1), lt), x)
    if I == 1:
        assert torch.equal(term.prox(vt, lt), x)
    if mask.shape[0] == 1:
        assert torch.equal(ops.cs_xupdate([vt], yt, mt[0], lt, I), x)
    assert torch.equal(ops.cs_xupdate([vt], yt[:, 0], mt, lt, I), x)
    if y.shape[0] == 1:
        assert torch.equal(ops.cs_xupdate([vt], yt[0, 0], mt, lt, I), x)
    if v.shape[0] == 1:
        assert torch.equal(ops.cs_xupdate([vt], yt, mt, float(lam[0]), I), x) and torch.equal(ops.cs_xupdate([vt], yt, mt, lt[0], I), x)
    return xn


def case_zero_mask_pixel(device):
    """a pixel whose mask is all zero returns v_c / I, whatever y says"""
    v, mask, y, lam = inputs("p_hsi")
    mask = mask.copy()
    mask[:, :, 3, 5] = 0.0
    for I in (1, 2):
        x = ops.cs_xupdate([T(v, device)], T(y, device), T(mask, device), T(lam, device), I).cpu().numpy()
        assert np.array_equal(x[:, :, 3, 5], v[:, :, 3, 5] / np.float32(I)), I


def case_sum_in_kernel(device):
    """three right-hand sides added inside the kernel, five with the host adding the first two: the restatement on their float64 sum"""
    _, mask, y, lam = inputs("p_hsi")
    rng = np.random.RandomState(46)
    for nb in (3, 5):
        bs = [rng.randn(2, 31, 17, 19).astype(np.float32) for _ in range(nb)]
        f = restate(sum(b.astype(np.float64) for b in bs), mask, y, lam, nb)
        x = ops.cs_xupdate([T(b, device) for b in bs], T(y, device), T(mask, device), T(lam, device), nb).cpu().numpy()
        ACHIEVED[f"sum_of_{nb}"] = dict(worst_error_over_elementwise_bound=_within(x, f, nb, f"cs x-update, {nb} right-hand sides", bs))


def case_vector_path(device):
    """planes of a multiple of four pixels move 16 bytes per lane (four pixels per thread): within the restatement's bounds, and the
    same bits as the one-pixel form, which the same data takes from buffers that start off a 16-byte boundary.  31 and 33 channels:
    either side of the register chunk; 1 x 1028: past one workgroup of four-pixel threads"""
    rng = np.random.RandomState(47)

    def off(a):
        t = torch.empty(a.size + 1, dtype=torch.float32, device=device)
        t[1:] = T(a, device).reshape(-1)
        assert t[1:].data_ptr() % 16 == 4
        return t[1:].view(a.shape)

    for (N, C, H, W), Nm, I in (((2, 31, 16, 20), 1, 2), ((1, 33, 4, 8), 1, 1), ((3, 5, 2, 2), 3, 3), ((1, 8, 1, 1028), 1, 1)):
        bs = [rng.randn(N, C, H, W).astype(np.float32) for _ in range(I)]
        mask, y = rng.randn(Nm, C, H, W).astype(np.float32), rng.randn(N, 1, H, W).astype(np.float32)
        lam = (0.05 + rng.rand(N)).astype(np.float32)
        f = restate(sum(b.astype(np.float64) for b in bs), mask, y, lam, I)
        x = ops.cs_xupdate([T(b, device) for b in bs], T(y, device), T(mask, device), T(lam, device), I)
        assert x.data_ptr() % 16 == 0
        _within(x.cpu().numpy(), f, I, f"cs x-update, 16-byte path {(N, C, H, W)}", bs)
        assert torch.equal(ops.cs_xupdate([off(b) for b in bs], off(y), off(mask), T(lam, device), I), x), (N, C, H, W)


def _differentiate(device, name, need=(True, True, True, True)):
    """the gradients ops.cs_xupdate's autograd node returns for sum(w x), those of (v, y, lam, mask) that `need` asks for"""
    g = golden()
    v, mask, y, lam = inputs(name)
    w, I = g["g_p_hsi_w" if name == "p_hsi_sy" else f"g_{name}_w"], int(g[f"g_{name}_I"])
    ts = [T(a, device).requires_grad_(n) for a, n in zip((v, y, lam, mask), need)]
    x = ops.cs_xupdate([ts[0]], ts[1], ts[3], ts[2], I)
    assert x.requires_grad
    x.backward(T(w, device))
    for t, n in zip(ts, need):
        assert (t.grad is not None) == n and (not n or (t.grad.shape == t.shape and t.grad.device == t.device))
    return [t.grad for t in ts]


def case_grad(device, name, subsets=True):
    g = golden()
    v, mask, y, lam = inputs(name)
    w, I = g["g_p_hsi_w" if name == "p_hsi_sy" else f"g_{name}_w"], int(g[f"g_{name}_I"])
    full = _differentiate(device, name)
    out = {}
    for k, ours in zip(("gv", "gy", "glam", "gmask"), full):
        ref32, ref64 = g[f"g_{name}_{k}32"], g[f"g_{name}_{k}64"]
        ours = ours.cpu().numpy()
        assert ours.shape == ref64.shape, (k, ours.shape, ref64.shape)
        d, theirs = rel_l2(ours, ref64), rel_l2(ref32, ref64)
        out[k] = dict(ours_vs_ref64=d, ref32_vs_ref64=theirs, bound=theirs + SLACK)
        record(f"cs gradient {name} {k} vs the reference's float64 autograd", d, theirs + SLACK)
        print(f"cs gradient {name} {k}: |ours - ref64| {d:.3e}; the reference's float32 autograd {theirs:.3e}")
        assert np.isfinite(ours).all() and d <= theirs + SLACK, (name, k, d, theirs)
    _, _, glam64, _, sum_qr = restate_grad(w, v, mask, y, lam, I)
    H, W = v.shape[2:]
    err, tol = np.abs(full[2].cpu().numpy().astype(np.float64) - glam64), (np.sqrt(H * W) + 4.0) * U * sum_qr
    out["glam"]["worst_error_over_reduction_bound"] = float((err / tol).max())
    print(f"cs gradient {name} glam: error / reduction bound {err / tol}")
    assert np.all(err <= tol), (name, err, tol)
    ACHIEVED[f"grad_{name}"] = out
    if subsets:                # null outputs in every combination autograd can ask for: the requested gradients keep their bits
        for need in itertools.product((False, True), repeat=4):
            if any(need) and not all(need):
                for k, a, b, n in zip(("gv", "gy", "glam", "gmask"), _differentiate(device, name, need), full, need):
                    assert not n or torch.equal(a, b), (name, need, k)
    return full


def case_grad_shared_lam_and_two_inputs(device):
    """one lam for N images receives the sum in its own (0-d) shape, as _TVDenoiseFn does; every right-hand side receives gv"""
    g = golden()
    v, mask, y, _ = inputs("p_hsi")
    w = T(g["g_p_hsi_w"], device)
    lam = torch.tensor(0.3, device=device, requires_grad=True)
    b1, b2 = T(v, device).requires_grad_(True), T(v[::-1].copy(), device).requires_grad_(True)
    ops.cs_xupdate([b1, b2], T(y, device), T(mask, device), lam, 2).backward(w)
    gv, _, glam, _, _ = restate_grad(g["g_p_hsi_w"], v.astype(np.float64) + v[::-1], mask, y, [0.3, 0.3], 2)
    assert lam.grad.shape == () and torch.equal(b1.grad, b2.grad)
    assert rel_l2(b1.grad.cpu().numpy(), gv) <= SLACK
    assert abs(float(lam.grad) - glam.sum()) <= SLACK * np.abs(glam).sum()          # (on the scale of the per-image gradients it adds up)


def case_no_grad_saves_nothing(device):
    v, mask, y, lam = (T(a, device) for a in inputs("p_one"))
    assert ops.cs_xupdate([v], y, mask, lam, 1).grad_fn is None
    with torch.no_grad():
        assert ops.cs_xupdate([v.clone().requires_grad_(True)], y, mask, lam, 1).grad_fn is None


def _solve(device, name, placeholders):
    g = golden()
    mask, y = T(g["admm_mask"], device), T(g["admm_y"], device)
    x = dp.Variable()
    if placeholders:
        mp, yp = dp.Placeholder(), dp.Placeholder()
        mp.value, yp.value = mask, y
        term = dp.compress_sensing(x, mp, yp)
    else:
        term = dp.compress_sensing(x, mask, y)
    prior = dp.deep_prior(x, denoiser=dp.TVDenoiser(5, True))
    fns, lams = term + prior, {prior: 0.02}
    if name == "admm_two":
        nn = dp.nonneg(x)
        fns, lams = fns + nn, {prior: 0.02, nn: 0.02}
    prob = dp.Problem(fns)
    with torch.no_grad():
        st = prob.solve(method="admm", device=device, x0=(y * mask), rhos=0.05, lams=lams, max_iter=8, return_full_states=True)
    assert prob.solver.last_path == "generic", prob.solver.last_path
    assert prob.solver.least_square is term
    return st


def case_admm(device, name):
    g = golden()
    st = _solve(device, name, False)
    psi = 2 if name == "admm_two" else 1
    assert len(st[1]) == psi and len(st[2]) == psi
    out = {}
    for key, got in [("x", st[0])] + [(f"v{i}", st[1][i]) for i in range(psi)] + [(f"u{i}", st[2][i]) for i in range(psi)]:
        ref = g[f"{name}_{key}"]
        # (a dual that is exactly zero in the reference -- nonneg's, inactive -- has no relative scale: the iterate's)
        d = rel_l2(got.cpu().numpy(), ref) if np.linalg.norm(ref) > 0 else float(np.linalg.norm(got.cpu().numpy()) / np.linalg.norm(g[f"{name}_x"]))
        out[key] = d
        record(f"cs {name}: {key} at iteration 8 vs the reference's float32 state", d, SLACK)
        print(f"cs {name}: {key} rel-L2 {d:.3e}")
        assert d <= SLACK, (name, key, d)
    d64, theirs = rel_l2(st[0].cpu().numpy(), g[f"{name}_x_f64"]), float(g[f"{name}_ref_f32_vs_f64"])
    assert abs(theirs - rel_l2(g[f"{name}_x"], g[f"{name}_x_f64"])) <= 1e-12
    out.update(x_vs_ref64=d64, ref32_vs_ref64=theirs, bound=theirs + SLACK)
    record(f"cs {name}: x vs the reference's float64 run", d64, theirs + SLACK)
    assert d64 <= theirs + SLACK, (name, d64, theirs)
    ACHIEVED[name] = out
    ph = _solve(device, name, True)
    for a, b in zip([st[0]] + list(st[1]) + list(st[2]), [ph[0]] + list(ph[1]) + list(ph[2])):
        assert torch.equal(a, b), "a Placeholder for mask and y changes the bits"
    return st


def case_deterministic(device):
    x0 = case_prox(device, "p_hsi", 2)
    x1 = case_prox(device, "p_hsi", 2)
    assert np.array_equal(x0, x1)
    for name in ("p_hsi", "p_hsi_sy"):
        a, b = _differentiate(device, name), _differentiate(device, name)
        assert all(torch.equal(s, t) for s, t in zip(a, b)), name


def case_argument_errors(device):
    """dpx_cs_xupdate's and dpx_cs_backward's own argument checks surface as DpxError"""
    import ctypes
    from dprox import _backend as be
    L, p = be.lib(), be.ptr
    v, mask, y, lam = (T(a, device) for a in inputs("p_one"))
    x, y3 = torch.empty_like(v), y.reshape(1, 3, 5)
    pb = (ctypes.c_void_p * 1)(v.data_ptr())
    ws = torch.zeros(L.query("dpx_cs_bwd_ws_bytes", 1, 1, 3, 5), dtype=torch.uint8, device=device)
    assert L.query("dpx_cs_bwd_ws_bytes", 1, 1, 3, 5) == 256 + 8 and L.query("dpx_cs_bwd_ws_bytes", 0, 1, 3, 5) == 0
    assert L.query("dpx_cs_bwd_ws_bytes", 3, 31, 17, 19) == 256 + 3 * 2 * 8
    fwd = [pb, 1, p(y3), p(mask), p(lam), 1, p(x), 1, 1, 3, 5, 1, 1, be.stream()]
    glam = torch.empty(1, device=device)
    bwd = [p(v), p(v), p(y3), p(mask), p(lam), 1, p(x), None, p(glam), None, 1, 1, 3, 5, 1, 1, p(ws), be.stream()]
    for name, good, cases in (("dpx_cs_xupdate", fwd, ((1, 0, "nb"), (1, 5, "nb"), (2, None, "null"), (3, None, "null"), (4, None, "null"), (6, None, "null"),
                                                      (6, p(v), "in-place"), (5, 0, "num_psi"), (7, 0, "shape"), (11, 2, "mask_batch"), (12, 3, "y_batch"))),
                              ("dpx_cs_backward", bwd, ((0, None, "null"), (1, None, "null"), (6, p(v), "in-place"), (16, None, "workspace"), (5, 0, "num_psi"),
                                                        (13, 0, "shape"), (14, 2, "mask_batch")))):
        for idx, bad, msg in cases:
            args = list(good)
            args[idx] = bad
            try:
                L.call(name, *args)
            except be.DpxError as e:
                assert msg in str(e), (name, msg, str(e))
            else:
                raise AssertionError(f"{name} accepted argument {idx} = {bad}")
    L.call("dpx_cs_backward", *bwd[:8], None, None, *bwd[10:16], None, be.stream())          # no gradient of lam: no workspace needed


def write_achieved():
    """the measured distances of the cases run so far -> the JSON file the environment variable DPX_CS_PARITY_OUT names (how
    profiles/cs_parity_achieved.json is produced from a GPU run); without the variable nothing is written"""
    path = os.environ.get("DPX_CS_PARITY_OUT")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ACHIEVED, f, indent=1, sort_keys=True)
