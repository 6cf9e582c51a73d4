"""CPU-only (SIMT emulator): which engine a fused solve gets, pinned by the C entry points it drives.

``last_path`` says only "fused"; here every ``be.Library.call`` / ``.query`` of a solve is recorded -- the entry point's name, its
scalar integer and float arguments as they are, its pointer arguments as "ptr" / "null" -- and compared with the sequences of
tests/golden/fused_call_sequences.json, recorded with this same recorder (``record_all``) from the commit BEFORE FusedADMM._run chose
its engine in one place: the refactor moved no launch.  One entry point is left out of the comparison, not of the record:
``dpx_admm_iter_supported``, the question "does the two-kernel iteration take this plane and these terms".  It launches nothing, and
asking it once per solve instead of up to three times is what that refactor was for.  The engine's name (``solver.last_engine``,
fused.ENGINES) is asserted next to the sequence.

Every case starts from empty host-side caches (tables, workspaces, schedule tables, chain buffers: a cached object elides its C call),
so a sequence does not depend on which cases ran before."""
import contextlib
import ctypes
import json
import os

import pytest
import torch

import emul_util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_call_sequences.json")
PURE_QUERIES = ("dpx_admm_iter_supported",)
POW2 = 256          # the smallest plane dpx_admm_iter_supported accepts (test_the_power_of_two_plane_is_the_smallest_one asks it)
REFUSED = (24, 20)


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


def _reduce(a):
    """an argument of a C call as the fixture keeps it: scalars by value, anything that is an address as null / non-null"""
    if a is None:
        return "null"
    if isinstance(a, (bool, int)):
        return int(a)
    if isinstance(a, float):
        return a
    if isinstance(a, (bytes, str)):
        return a.decode() if isinstance(a, bytes) else a
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, ctypes._SimpleCData):
        return _reduce(a.value)
    return "ptr" if a else "null"              # ctypes arrays, structures, pointers


@contextlib.contextmanager
def recorded(log):
    from dprox import _backend as be
    call, query = be.Library.call, be.Library.query

    def wrap(real):
        def f(self, name, *args):
            log.append([name] + [_reduce(a) for a in args])
            return real(self, name, *args)
        return f
    be.Library.call, be.Library.query = wrap(call), wrap(query)
    try:
        yield log
    finally:
        be.Library.call, be.Library.query = call, query


def _clear_host_caches():
    from dprox import _ops
    from dprox.algo import fused
    _ops.clear_caches()
    for cache in (fused._sched_cache, fused._chain_tab_cache, fused._chain_spec_bytes):
        cache.clear()


def _tv_problem(B, H, W, seed=5):
    """sum_squares(conv(x, psf) - b) + norm1(grad_H x) + norm1(grad_W x), one channel"""
    import dprox as dp
    import synthetic
    _, b0, psf = synthetic.deconv_case(B, 1, H, W, seed=seed)
    b = torch.from_numpy(b0)
    x = dp.Variable()
    return dp.sum_squares(dp.conv(x, psf) - b) + dp.norm1(dp.grad(x, dim=0)) + dp.norm1(dp.grad(x, dim=1)), b, x


def _solve(method, H, W, T, B=1, **kw):
    import dprox as dp
    fns, b, _ = _tv_problem(B, H, W)
    s = dp.compile(fns, method=method, device="cpu")
    return s, s.solve(x0=b.clone(), rhos=torch.linspace(0.4, 0.2, max(T, 1)), lams=0.01, max_iter=T, return_full_states=True, **kw)


def _iters_on_written_state(H, W, T, B=1, callback=None):
    """ADMM.iters on a state the caller has written to: not fresh, the general seed pass"""
    import dprox as dp
    fns, b, _ = _tv_problem(B, H, W)
    s = dp.compile(fns, method="admm", device="cpu")
    x0 = b.clone()
    _, rhos, lams, _ = s.defaults(x0, torch.linspace(0.4, 0.2, T), 0.01, T)
    st = s.initialize(x0)
    st[2][0].add_(0.0)
    return s, s.iters(st, rhos, lams, T, callback=callback)


def _two_chains(H, W, T):
    old = os.environ.get("DPX_CHAINS")
    os.environ["DPX_CHAINS"] = "2"                  # (sub_batch_chains(2, 1, 256, 256) = 2 with it; unforced, two chains take 96 planes of 256^2)
    try:
        from dprox.algo import fused
        assert fused.sub_batch_chains(2, 1, H, W) == 2
        return _iters_on_written_state(H, W, T, B=2)
    finally:
        if old is None:
            os.environ.pop("DPX_CHAINS")
        else:
            os.environ["DPX_CHAINS"] = old


def _staged(merge):
    from dprox.algo import fused
    old = fused.FusedADMM.merge_z_rhs
    fused.FusedADMM.merge_z_rhs = merge
    try:
        return _solve("admm", *REFUSED, 3)
    finally:
        fused.FusedADMM.merge_z_rhs = old


def _prior(denoiser):
    import dprox as dp
    import synthetic
    H, W = REFUSED
    _, b0, psf = synthetic.deconv_case(1, 1, H, W, seed=9)
    b = torch.from_numpy(b0)
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=denoiser)
    with torch.no_grad():
        s = dp.compile(dp.sum_squares(dp.conv(x, psf) - b) + prior, method="admm", device="cpu")
        return s, s.solve(x0=b.clone(), rhos=torch.tensor([0.5, 0.3]), lams={prior: torch.tensor([0.08, 0.05])}, max_iter=2, return_full_states=True)


def _ffdnet():
    import synthetic
    from dprox.proxfn.pnp.denoisers import FFDNet, FFDNetDenoiser
    den = FFDNetDenoiser()
    den.model = FFDNet(in_nc=1, out_nc=1, nc=16, nb=3, act_mode="R").load_layers(synthetic.ffdnet_weights(3, 1, 1, 16, 3))      # (seeded)
    return _prior(den)


def _tv_prior():
    import dprox as dp
    return _prior(dp.TVDenoiser(5))


def _rho_grad_on_a_lazy_state():
    import dprox as dp
    fns, b, _ = _tv_problem(1, POW2, POW2)
    s = dp.compile(fns, method="admm", device="cpu")
    rhos = torch.tensor([0.4, 0.3], requires_grad=True)
    return s, s.solve(x0=b.clone(), rhos=rhos, lams=0.01, max_iter=2, return_full_states=True)


# name -> (the solve, the engine FusedADMM.route / run_stencil names for it; None: nothing to run)
CASES = {
    "admm_solve_lazy_pow2":        (lambda: _solve("admm", POW2, POW2, 3), "two_kernel"),
    "admm_iters_written_pow2":     (lambda: _iters_on_written_state(POW2, POW2, 3), "two_kernel"),
    "admm_iters_callback_pow2":    (lambda: _iters_on_written_state(POW2, POW2, 3, callback=lambda **k: None), "two_kernel"),
    "admm_iters_two_chains_pow2":  (lambda: _two_chains(POW2, POW2, 3), "chains"),
    "admm_refused_merged":         (lambda: _staged(True), "staged"),
    "admm_refused_unmerged":       (lambda: _staged(False), "staged"),
    "hqs_pow2":                    (lambda: _solve("hqs", POW2, POW2, 3), "two_kernel"),
    "hqs_refused":                 (lambda: _solve("hqs", *REFUSED, 3), "staged"),
    "vxu_pow2_T3":                 (lambda: _solve("admm_vxu", POW2, POW2, 3), "vxu_two_kernel"),
    "vxu_pow2_T2":                 (lambda: _solve("admm_vxu", POW2, POW2, 2), "vxu_staged"),
    "vxu_refused":                 (lambda: _solve("admm_vxu", *REFUSED, 3), "vxu_staged"),
    "ffdnet_prior_no_grad":        (_ffdnet, "pnp_one_call"),
    "tv_denoiser_prior":           (_tv_prior, "staged"),
    "rho_grad_lazy_pow2":          (_rho_grad_on_a_lazy_state, "autograd"),
    "ladmm_refused":               (lambda: _solve("ladmm", *REFUSED, 3), "stencil_ladmm"),
    "pc_refused":                  (lambda: _solve("pc", *REFUSED, 3), "stencil_pc"),
    "admm_max_iter_0_pow2":        (lambda: _solve("admm", POW2, POW2, 0), None),
}


def _flat(state):
    out = []
    for part in (state if isinstance(state, (list, tuple)) else [state]):
        out += _flat(part) if isinstance(part, (list, tuple)) else [part.detach().clone()]
    return out


def record_case(name):
    """(the solver, the recorded sequence, the returned state as a flat list of tensors) of one case, from empty host-side caches"""
    _clear_host_caches()
    with recorded([]) as log:
        solver, state = CASES[name][0]()
    return solver, log, _flat(state)


def record_all():
    """{case: sequence}: what tests/golden/fused_call_sequences.json holds (run against the commit whose dispatch is the reference)"""
    emul_util.use_emulator()
    return {name: record_case(name)[1] for name in CASES}


def _launching(seq):
    return [c for c in seq if c[0] not in PURE_QUERIES]


def test_the_power_of_two_plane_is_the_smallest_one():
    from dprox import _backend as be
    from dprox import _ops as ops
    terms = (ops.Term * 2)()
    terms[0].linop, terms[0].prox = be.LIN_GRAD_H, be.PROX_NORM1
    terms[1].linop, terms[1].prox = be.LIN_GRAD_W, be.PROX_NORM1
    sizes = [n for n in range(8, POW2 + 1, 8) if ops.iter_supported(n, n, terms, 2)]
    assert sizes == [POW2], sizes
    assert not ops.iter_supported(*REFUSED, terms, 2)


@pytest.mark.parametrize("name", list(CASES))
def test_engine_and_call_sequence(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    solver, seq, _ = record_case(name)
    assert solver.last_path in ("fused", "unrolled"), solver.last_path
    assert solver.last_engine == CASES[name][1], (name, solver.last_engine)
    got, want = _launching(json.loads(json.dumps(seq))), _launching(golden[name])
    assert [c[0] for c in got] == [c[0] for c in want], name          # (the names first: the readable failure)
    assert got == want, name
