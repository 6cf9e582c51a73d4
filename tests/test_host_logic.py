"""CPU-only: host-side logic of the drop-in layer (no kernel launches) + the C-ABI library loads and
exports every symbol include/dpx.h declares."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import dprox as dp
from conftest import ROOT, load_golden
from dprox import _backend as be
from dprox.algo.driver import Algorithm
from dprox.utils import to_ndarray, to_torch_tensor


def test_c_abi_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "dpx.h")).read()
    declared = set(re.findall(r"\b(dpx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(be.SIGNATURES), declared ^ set(be.SIGNATURES)
    if not os.path.exists(be.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = be.Library(be.LIB_PATH)          # AttributeError if a symbol is missing
    assert lib.query("dpx_version") >= 100
    assert lib.query("dpx_fft_table_bytes", 1024, 1024) == 2048 * 8
    assert lib.query("dpx_spectrum_bytes", 24, 1024, 1024) == 2 * (24 * 1024 * 512 + 24 * 1024) * 8  # 2 x (half spectrum + Nyquist side)
    assert lib.query("dpx_spectrum_bytes", 1, 15, 21) == 2 * 15 * 11 * 8


def test_no_shipped_kernel_uses_scratch_memory():
    """tools/spill_check.py over the compiler's resource remarks of every kernel of the library (kept by __graft_entry__.build()): a spilled
    register in any instantiation fails the suite"""
    import __graft_entry__
    __graft_entry__.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_check
    rows = spill_check.kernels()
    assert len(rows) > 300, len(rows)
    for fam in ("k_iter_rows_par", "k_iter_rows_seq", "k_conv3x3_bf16", "k_conv3x3_wino", "k_cols_p2", "k_bwd_rows"):
        assert any(fam in r[1] for r in rows), fam
    assert spill_check.main() == 0


def test_build_time_switches_of_the_kernels_are_the_listed_ones():
    """The DPX_* macros that a preprocessor conditional of csrc tests are the emulator build, the trace builds and the two switches
    whose value differs from file to file (set in front of the #include).  A switch nothing sets is a constant: an experiment that adds one adds it here."""
    allowed = {"DPX_EMULATED", "DPX_PAR_TRACE", "DPX_WC_TRACE", "DPX_WN_TRACE", "DPX_PK_ASM", "DPX_FFT_BASEOFF"}
    csrc = os.path.join(ROOT, "delta-prox_amd", "csrc")
    files = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    assert len(files) > 30, files
    tested = {}
    for f in files:
        text = open(os.path.join(csrc, f)).read().replace("\\\n", " ")
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b.*$", text, re.M):
            for m in re.findall(r"\bDPX_\w+", line):
                tested.setdefault(m, f)
    assert set(tested) == allowed, {m: f for m, f in tested.items() if m not in allowed} or allowed - set(tested)


def test_streaming_row_kernel_always_has_a_band_partition():
    """dpx_admm_iter_supported answers for a plane size without knowing the plane count, so the streaming row kernel (the only row
    kernel of 768-wide planes) must find a band partition for EVERY count: planes x bands fill whole workgroups of 4 waves, bands are
    at least one row long -- also for odd and large plane counts and with sub-batch chains sharing the GPU (round-4 advisor finding:
    P x share > 1024 with P not a multiple of 4 had no partition and the solve raised)."""
    lib = be.Library(be.LIB_PATH)
    for W, per_block in ((768, 4), (1024, 4), (512, 8), (256, 16)):
        for share in (1, 2, 3):
            lib.call("dpx_admm_iter_share", share)
            try:
                for H in (256, 768, 1024):
                    for P in list(range(1, 70)) + [255, 257, 1023, 1025, 1027, 2049, 4097]:
                        nb = lib.query("dpx_admm_iter_bands", P, H, W)
                        assert nb >= 1 and nb <= H and (P * nb) % per_block == 0, (W, share, H, P, nb)
            finally:
                lib.call("dpx_admm_iter_share", 1)
    assert lib.query("dpx_admm_iter_bands", 3, 1024, 1000) == 0


def test_tuning_registry_is_documented_and_round_trips():
    """every knob of the library's registry is in include/dpx.h's table, and dpx_tune_set / dpx_tune_get round-trip"""
    hdr = open(os.path.join(ROOT, "include", "dpx.h")).read()
    lib = be.Library(be.LIB_PATH)
    import ctypes
    n = lib.query("dpx_tune_count")
    names = [lib.query("dpx_tune_name", i).decode() for i in range(n)]
    assert n >= 20 and lib.query("dpx_tune_name", n) is None
    table = hdr[hdr.index("tuning knobs"):hdr.index("int dpx_tune_count")]
    for name in names:
        assert re.search(r"\b" + name + r"\b", table), f"knob {name} is not documented in include/dpx.h"
        v = ctypes.c_int(-7)
        lib.call("dpx_tune_get", name.encode(), ctypes.byref(v))
        old = v.value
        lib.call("dpx_tune_set", name.encode(), 5)
        lib.call("dpx_tune_get", name.encode(), ctypes.byref(v))
        assert v.value == 5
        lib.call("dpx_tune_set", name.encode(), old)
    assert lib.query("dpx_tune_set", b"no_such_knob", 1) < 0 and b"no_such_knob" in lib.cdll.dpx_last_error()
    # no getenv outside the registry (and the collective library's path): a knob a test cannot reach in-process is a regression
    csrc = os.path.join(ROOT, "delta-prox_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(csrc, f)).read()
            hits = [ln for ln in src.splitlines() if "getenv(" in ln]
            assert all("kKnobs[i].env" in ln or "DPX_RCCL_LIB" in ln for ln in hits), (f, hits)


def _strip_comments_and_strings(src):
    """comments blanked and string / character literals emptied, line structure kept"""
    pat = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', re.S)
    return pat.sub(lambda m: m.group(0)[0] * 2 if m.group(0)[0] in "\"'" else re.sub(r"[^\n]", " ", m.group(0)), src)


def _declarations(text):
    """(line, name, statement) of every body-less function declaration at namespace scope of stripped source: a statement that starts in
    column 0, has a parameter list closed by `);` and no `{`.  One-line `namespace x { ...; }` blocks count as their statements."""
    text = re.sub(r"^namespace\b[^{\n]*\{([^{}\n]*)\}[ \t]*$", lambda m: "\n".join(s.strip() + ";" for s in m.group(1).split(";") if s.strip()),
                  text, flags=re.M)               # (only ever met on lines the test then rejects, so the shifted line numbers do not matter)
    for m in re.finditer(r"^(?![#}\s])([^;{}=]*?\([^;{}]*\))\s*;", text, re.M):
        stmt = " ".join(m.group(1).split())
        depth, i = 0, len(stmt) - 1
        while i >= 0:                             # the parenthesis that opens the parameter list
            depth += (stmt[i] == ")") - (stmt[i] == "(")
            if depth == 0:
                break
            i -= 1
        head = re.search(r"([A-Za-z_]\w*)\s*$", stmt[:i])
        if not head or stmt.startswith(("typedef ", "using ")) or len(re.findall(r"[A-Za-z_]\w*", stmt[:i])) < 2:
            continue                              # function-pointer / vector typedefs, static_assert(...), a macro call
        yield text.count("\n", 0, m.start()) + 1, head.group(1), stmt, m.end()


def _defined_at(name, text):
    return re.findall(r"^(?![#}\s])[^;{}=()]*\b(?:dpx::)?%s\s*\([^;{}]*\)\s*\{" % re.escape(name), text, re.M)


def _cross_file_declaration_faults(csrc):
    """what test_cross_file_internals_are_declared_once_in_dpx_internal_h rejects in a csrc/ directory, one line each"""
    hips = {f: _strip_comments_and_strings(open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}
    faults = []
    for f, text in hips.items():
        for line, name, stmt, end in _declarations(text):
            forward = ("__global__" in stmt or stmt.startswith("template")) and _defined_at(name, text[end:])
            if not forward:
                faults.append(f"{f}:{line}: prototype of {name} outside dpx_internal.h: {stmt[:100]}")
        for m in re.finditer(r"\bextern\b(?!\s*\"\"|\s+__shared__)", text):
            line = text.count("\n", 0, m.start()) + 1
            faults.append(f"{f}:{line}: extern: {text.splitlines()[line - 1].strip()[:100]}")
    hdr = os.path.join(csrc, "dpx_internal.h")
    if not os.path.exists(hdr):
        return faults + ["dpx_internal.h is missing"]
    if '#include "dpx_internal.h"' not in open(os.path.join(csrc, "dpx_common.h")).read():
        faults.append("dpx_common.h does not include dpx_internal.h")
    names = [name for _, name, _, _ in _declarations(_strip_comments_and_strings(open(hdr).read()))]
    if len(names) < 20 or len(set(names)) != len(names):
        faults.append(f"dpx_internal.h: {len(names)} declarations, {len(set(names))} names")
    for name in names:
        defs = [(f, d) for f, text in hips.items() for d in _defined_at(name, text)]
        users = [f for f, text in hips.items() if re.search(r"\b%s\s*\(" % re.escape(name), text)]
        if len(defs) != 1 or defs[0][1].startswith("static"):
            faults.append(f"dpx_internal.h: {name} has {len(defs)} non-static definitions in csrc/*.hip: {[f for f, _ in defs]}")
        elif len(users) < 2:
            faults.append(f"dpx_internal.h: {name} is used by {defs[0][0]} alone: make it static there")
    return faults


def test_cross_file_internals_are_declared_once_in_dpx_internal_h():
    """A function of one .hip file that another one calls is declared in csrc/dpx_internal.h (which dpx_common.h includes, so the defining
    file sees it too and the compiler checks the definition against it) and nowhere else: no .hip file holds a body-less declaration at
    namespace scope -- except a forward declaration of a kernel or a template it defines further down -- or an `extern` other than
    extern "C" / extern __shared__, and every name the header declares has exactly one definition and a user in another file."""
    probe = _strip_comments_and_strings(
        'namespace dpx {\nint far_away(const float* x, int n,\n            bool flag = false);   // dpx_other.hip\n'
        'template <int N> __global__ void k_later(float* p);\n__global__ void k_never(float* p);\nstatic int g = f(3);\n'
        'typedef void (*Fn)(int);\nint here(int n) { return n; }\ntemplate <int N> __global__ void k_later(float* p) { p[0] = N; }\n}\n'
        'namespace dpx { int g_a = 0; bool one_liner(int H); }\n')
    found = [(name, ("__global__" in stmt or stmt.startswith("template")) and bool(_defined_at(name, probe[end:])))
             for _, name, stmt, end in _declarations(probe)]
    assert found == [("far_away", False), ("k_later", True), ("k_never", False), ("one_liner", False)], found
    faults = _cross_file_declaration_faults(os.path.join(ROOT, "delta-prox_amd", "csrc"))
    assert not faults, "\n".join(faults)


# Full-wave butterflies left open-coded: replacing the loop by the call changes the kernel's assembly (instruction order, or the count),
# and these kernels are on benchmarked paths (profiles/reduce_helpers_isa.txt).  file -> (loop headers, reason)
_BUTTERFLY_LOOPS_KEPT = {
    "dpx_reduce_dev.h": (2, "wave_sum and wave_max themselves"),
    "dpx_fft.hip": (4, "k_crows_real_out and k_crows_real_out_w<5>, <6>: same instructions in another order at both sites of each kernel"),
    "dpx_bwd_rows_par.hip": (1, "k_bwd_rows_par reduces two doubles in one loop to keep register pressure down: all 24 instantiations change"),
    "dpx_conv_bf16.hip": (1, "k_bx_absmax: fmaxf butterfly, 204 -> 213 instructions with wave_max's comparison form"),
}
_REDUCE_NAMES = r"\w*(?:wave_sum|wave_max|block_sum|block_reduce|st_agent|al16|aligned16)\w*"


def _reduce_helper_faults(csrc):
    """what test_reduction_helpers_are_written_once_in_dpx_reduce_dev_h rejects in a csrc/ directory, one line each"""
    faults = []
    if not os.path.exists(os.path.join(csrc, "dpx_reduce_dev.h")):
        faults.append("dpx_reduce_dev.h is missing")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        text = _strip_comments_and_strings(open(os.path.join(csrc, f)).read())
        line = lambda m: text.count("\n", 0, m.start()) + 1
        if f != "dpx_reduce_dev.h":
            # a function definition (a type or a declarator in front of the name, a parameter list, a body), a lambda, a function-like macro
            for m in re.finditer(r"(\w+|[>*&])\s+(%s)\s*\([^;{}()]*(?:\([^()]*\)[^;{}()]*)*\)\s*(?:const\s*)?\{" % _REDUCE_NAMES, text):
                if m.group(1) not in ("return", "else", "case", "new", "throw"):
                    faults.append(f"{f}:{line(m)}: defines {m.group(2)}")
            for m in re.finditer(r"\b(%s)\s*=\s*\[[^\]\n]*\]\s*\(" % _REDUCE_NAMES, text):
                faults.append(f"{f}:{line(m)}: defines the lambda {m.group(1)}")
            for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(%s)\(" % _REDUCE_NAMES, text, re.M):
                faults.append(f"{f}:{line(m)}: defines the macro {m.group(1)}")
        loops = list(re.finditer(r"\bfor\s*\(\s*int\s+o\s*=\s*32\s*;\s*o\s*>\s*0\s*;\s*o\s*>>=\s*1\s*\)", text))
        kept = _BUTTERFLY_LOOPS_KEPT.get(f, (0, ""))[0]
        if len(loops) != kept:
            faults += [f"{f}:{line(m)}: open-coded full-wave butterfly ({len(loops)} in the file, {kept} listed)" for m in loops] or \
                      [f"{f}: no open-coded butterfly left, {kept} listed"]
    return faults


def test_reduction_helpers_are_written_once_in_dpx_reduce_dev_h():
    """The wave butterflies, the block-level sum, the write-through store of the last-workgroup hand-over and the 16-byte alignment test
    live in csrc/dpx_reduce_dev.h and nowhere else: no other file of csrc/ defines a function, lambda or macro whose name contains
    wave_sum, wave_max, block_sum, block_reduce, st_agent, al16 or aligned16, and the butterfly's loop header appears only in that header
    and at the sites _BUTTERFLY_LOOPS_KEPT lists with their reason (exactly as many as listed: a site that goes is taken off the list)."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:              # the checker finds each kind of copy, and only those
        open(os.path.join(d, "dpx_reduce_dev.h"), "w").write(
            "template <class T> T wave_sum(T v) {\n  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);\n  for (int o = 32; o > 0; o >>= 1) v = v;\n}\n")
        open(os.path.join(d, "dpx_probe.hip"), "w").write(
            "// float my_wave_sum(float v) { in a comment }\n"
            "__device__ __forceinline__ float my_wave_sum(float v) {\n  for (int o = 32;  o > 0; o >>= 1) v += __shfl_xor(v, o);\n  return v;\n}\n"
            "template <class T, bool MAX> __device__ T block_reduce_t(T v, T* sh) { return v; }\n"
            "static bool mr_al16(const void* p) { return (size_t)p % 16 == 0; }\n"
            "void user(float* p) {\n  auto wave_sum_d = [](double v) { return v; };\n  const bool al16 = aligned16({p});\n"
            "  if (aligned16({p}) && wave_sum(p[0]) > 0) { p[0] = block_sum(p[0], p); }\n  for (int o = 32; o >= KV; o >>= 1) p[o] = 0;\n}\n"
            "#define st_agent_all(p) (p)\n")
        got = _reduce_helper_faults(d)
    assert [g.split(": ", 1)[1].split(" (")[0] for g in got] == [
        "defines my_wave_sum", "defines block_reduce_t", "defines mr_al16", "defines the lambda wave_sum_d", "defines the macro st_agent_all",
        "open-coded full-wave butterfly"], got
    faults = _reduce_helper_faults(os.path.join(ROOT, "delta-prox_amd", "csrc"))
    assert not faults, "\n".join(faults)


def test_wheel_builds_and_imports_without_path_edits(tmp_path):
    """packaging (pyproject.toml + setup.py): `pip wheel` runs the HIP build hook, the wheel holds the package `dprox` with
    dprox/lib/libdpx_hip.so inside, and a fresh interpreter imports it from the unpacked wheel alone (no sys.path edits, no repo)"""
    import shutil
    import subprocess
    import sys
    import zipfile
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    wh = tmp_path / "wh"
    r = subprocess.run([sys.executable, "-m", "pip", "wheel", "--no-build-isolation", "--no-deps", "-q", "-w", str(wh), ROOT],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=1500)
    for junk in ("build", "UNKNOWN.egg-info", os.path.join("delta-prox_amd", "dprox_mi355x.egg-info")):
        shutil.rmtree(os.path.join(ROOT, junk), ignore_errors=True)
    assert r.returncode == 0, r.stderr[-2000:]
    wheels = list(wh.glob("dprox_mi355x-*.whl"))
    assert len(wheels) == 1, list(wh.iterdir())
    site = tmp_path / "site"
    with zipfile.ZipFile(wheels[0]) as z:
        names = z.namelist()
        z.extractall(site)
    assert "dprox/lib/libdpx_hip.so" in names and "dprox/_backend.py" in names and not any(n.startswith(("oracle", "tests")) for n in names)
    code = ("import dprox, dprox._backend as be; L = be.lib(); "
            "assert L.path.endswith('dprox/lib/libdpx_hip.so') and '/site/' in L.path, L.path; "
            "assert dprox.__file__.startswith(%r), dprox.__file__; print(L.query('dpx_version'))" % str(site))
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "DPX_LIB")}
    env["PYTHONPATH"] = str(site)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=600)
    assert r.returncode == 0 and int(r.stdout.strip()) >= 101, (r.stdout, r.stderr[-2000:])


def test_to_torch_tensor_and_ndarray():
    a = np.zeros((5, 7, 3), np.float32)
    assert tuple(to_torch_tensor(a, batch=True).shape) == (1, 3, 5, 7)          # HWC -> NCHW
    assert tuple(to_torch_tensor(np.zeros((5, 7, 1)), batch=True).shape) == (1, 1, 5, 7)
    assert tuple(to_torch_tensor(np.zeros((5, 7, 2)), batch=True).shape) == (1, 5, 7, 2)   # C not in {1,3}: untouched
    assert tuple(to_torch_tensor(np.zeros((5, 7)), batch=True).shape) == (1, 5, 7)
    t = dp.tensor(np.zeros((5, 7, 3)))
    assert to_torch_tensor(t, batch=True) is t                                  # tagged tensors are never re-batchified
    assert to_ndarray(torch.zeros(1, 3, 4, 5), debatch=True).shape == (4, 5, 3)
    assert to_ndarray(np.zeros((2, 2), np.float64)).dtype == np.float32


def test_partition_and_defaults():
    x = dp.Variable()
    data = dp.sum_squares(dp.conv(x, np.ones((3, 3, 1)) / 9) - torch.zeros(1, 1, 8, 8))
    r0, r1, nn = dp.norm1(dp.grad(x, dim=0)), 2.0 * dp.norm1(dp.grad(x, dim=1)), dp.nonneg(x)
    fns = data + r0 + r1 + nn
    assert isinstance(fns, list) and len(fns) == 4 and r1.alpha == 2.0
    psi, omega = dp.ADMM.partition(fns)
    assert omega == [data] and psi == [r0, r1, nn]

    class weighted(dp.sum_squares):          # subclasses of sum_squares stay in Psi (exact-type test, admm.py:33)
        pass
    psi, omega = dp.ADMM.partition([weighted(x), data])
    assert len(omega) == 1 and omega[0] is data
    with pytest.raises(ValueError):
        dp.ProximalGradientDescent.partition([data])
    with pytest.raises(ValueError):
        dp.ProximalGradientDescent.partition([r0, nn])
    psi, omega = dp.ProximalGradientDescent.partition([nn, data])
    assert omega == [data] and psi == [nn]

    solver = dp.ADMM(*dp.ADMM.partition(fns))
    _, rhos, lams, T = solver.defaults(None, None, None, 24)
    assert T == 24 and torch.equal(rhos, torch.full((24,), 1.0)) and set(lams) == {r0, r1, nn}
    assert all(torch.allclose(v, torch.full((24,), 0.02)) for v in lams.values())
    _, rhos, lams, _ = solver.defaults(None, 0.3, {r0: 0.1, r1: torch.arange(5.0)}, 5)
    assert torch.allclose(lams[r0], torch.full((5,), 0.1)) and torch.equal(lams[r1], torch.arange(5.0))
    assert solver.least_square.freq_diagonalizable and not solver.least_square.diagonalizable
    assert solver.nparams == 4 and solver.state_split == [1, [3], [3]]


def test_errors_and_quirks():
    x = dp.Variable()
    with pytest.raises(ValueError):
        dp.grad(x, dim=3)
    with pytest.raises(TypeError):
        x * np.ones(3)
    with pytest.raises(KeyError):
        dp.compile([dp.nonneg(x)], method="nope", device="cuda")
    if not be.host_mode():
        with pytest.raises(be.DpxError):
            dp.compile([dp.nonneg(x), dp.sum_squares(x)], method="admm", device="cpu")   # no CPU path
    with pytest.raises(NotImplementedError):
        dp.specialize(None, method="deq")
    ph = dp.Placeholder()
    seen = []
    ph.change(seen.append)
    ph.value = torch.ones(2)
    ph.value = torch.nn.Parameter(torch.zeros(2))       # the reference silently skips watchers here
    assert len(seen) == 2
    e = 2 * x - 3.0
    assert type(e).__name__ == "sum" and len(e.input_nodes) == 2 and e.variables == [x]
    assert (x + 1 + 2).__class__.__name__ == "sum" and len((x + 1 + 2).input_nodes) == 3   # sums are flattened


def test_log_descent_matches_reference_tables():
    g = load_golden("g12_log_descent")
    r, s = dp.log_descent(35, 5, 30)
    assert np.array_equal(r.numpy(), g["rhos_35_5_30"]) and np.array_equal(s.numpy(), g["sigmas_35_5_30"])
    r, s = dp.log_descent(upper=30, lower=10, iter=8, sqrt=True, lam=0.1, w=0.7)
    assert np.array_equal(r.numpy(), g["rhos_30_10_8_sqrt"]) and np.array_equal(s.numpy(), g["sigmas_30_10_8_sqrt"])


def test_denoiser_state_dicts_follow_the_nn_module_protocol():
    """checkpoints keep the reference's keys through nn.Module's own recursion: a parent's state_dict() holds every denoiser
    weight under its reference name, round-trips through load_state_dict(), and the reference's solver-level layout
    (psi_fns.<i>.denoiser.model.<key>) loads -- reference network_ffdnet.py:43-47, network_unet.py:67-104, models/unet/unet.py:34-46"""
    import synthetic
    from dprox.proxfn.pnp.denoisers import DRUNetDenoiser, FFDNetColorDenoiser, IRCNN, UNetDenoiser

    class Parent(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ffd = FFDNetColorDenoiser(synthetic.ffdnet_weights(7))
            self.dru = DRUNetDenoiser(1, synthetic.drunet_weights(22, 2, 1))
            self.unet = UNetDenoiser(synthetic.unet_weights(41))
            self.irc = IRCNN(1, 1, 64)

    a, b = Parent(), Parent()
    sd = a.state_dict()
    assert "ffd.model.model.0.weight" in sd and "ffd.model.model.22.bias" in sd
    assert "dru.model.m_down1.0.res.0.weight" in sd and "unet.model.up1.conv.conv-0.conv2d.weight" in sd and "irc.model.12.bias" in sd
    assert len([k for k in sd if k.startswith("ffd.")]) == 24 and len([k for k in sd if k.startswith("unet.")]) == 56
    for p in b.parameters():
        p.data.zero_()
    res = b.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in b.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # strict loading reports foreign / missing keys like any nn.Module
    bad = dict(sd)
    bad["ffd.model.model.99.weight"] = torch.zeros(1)
    del bad["unet.model.outc.conv.bias"]
    with pytest.raises(RuntimeError) as e:
        b.load_state_dict(bad)
    assert "model.99.weight" in str(e.value) and "outc.conv.bias" in str(e.value)
    # a reference-format solver checkpoint (weights of the prior inside the solver's psi_fns) loads into the compiled solver
    x = dp.Variable()
    prior = dp.deep_prior(x, denoiser=FFDNetColorDenoiser(None))
    solver = dp.compile(dp.sum_squares(x - torch.zeros(1, 3, 8, 8)) + prior, method="admm", device="cuda" if torch.cuda.is_available() else "cpu") \
        if (torch.cuda.is_available() or be.host_mode()) else None
    if solver is not None:
        ref_ckpt = {f"psi_fns.0.denoiser.model.{k}": torch.as_tensor(v) for k, v in a.ffd.model.state_dict().items()}
        out = solver.load_state_dict(ref_ckpt, strict=False)
        assert not [k for k in out.unexpected_keys if "denoiser" in k]
        assert torch.equal(solver.psi_fns[0].denoiser.model.weights[3].cpu(), a.ffd.model.weights[3])


def test_train_loop_repeats_a_step_whose_split_f16_backward_left_the_range(tmp_path):
    """dp.train's epoch loop: a backward pass that trips the range trap of the split-f16 FFDNet arithmetic raises F16RangeError out of
    loss.backward() (be.note_f16_backward: the networks concerned have fallen back to split-bf16 by then) -- the batch is run again, once;
    a second failure is not swallowed"""
    from dprox.algo.training import TrainLoop
    m = torch.nn.Linear(4, 4)
    loop = TrainLoop(m, savedir=str(tmp_path))
    x = torch.randn(3, 4)
    calls = {"step_fn": 0, "fail": 1}
    real_step = loop.step

    def step_fn(batch):
        calls["step_fn"] += 1
        return batch, batch, m(batch)

    def flaky_step(gt, pred):
        if calls["fail"] > 0:
            calls["fail"] -= 1
            raise be.F16RangeError("backward: test")
        return real_step(gt, pred)

    loop.step = flaky_step
    with pytest.warns(RuntimeWarning, match="repeating the step"):
        rec = loop.run_epoch(step_fn, [x, x])
    assert calls["step_fn"] == 3 and rec["steps"] == 2 and loop.gstep == 2
    calls["fail"] = 2
    with pytest.raises(be.F16RangeError), pytest.warns(RuntimeWarning):
        loop.run_epoch(step_fn, [x])


def test_product_does_not_import_the_oracle():
    import subprocess
    import sys
    code = ("import sys; sys.path[:0]=[%r, %r]; import dprox, dprox.algo.fused, dprox.proxfn.pnp; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle leaked into the product'"
            % (ROOT, os.path.join(ROOT, "delta-prox_amd")))
    subprocess.run([sys.executable, "-c", code], check=True)
    src = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "delta-prox_amd", "dprox")):
        src += [open(os.path.join(dirpath, f)).read() for f in files if f.endswith(".py")]
    assert not any(re.search(r"^\s*(import|from)\s+oracle", s, re.M) for s in src)


def test_bench_dump_outputs_writes_the_same_sample_of_every_state_array(tmp_path):
    """bench.py --dump-outputs: x and every v_i / u_i of the state as float32 <name>.npy, the same seeded entries of each in every run,
    within the 64 MB the option allows for the headline's five arrays"""
    import bench
    x = torch.randn(2, 3, 1024, 1024, generator=torch.Generator().manual_seed(0))
    state = (x, [x + 1, x + 2], [x + 3, x + 4])
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), state)
    names = ["x", "v0", "v1", "u0", "u1"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    idx = np.sort(np.random.default_rng(0).choice(x.numel(), bench.DUMP_SAMPLES, replace=False))
    for i, n in enumerate(names):
        got = np.load(tmp_path / "a" / (n + ".npy"))
        assert got.dtype == np.float32 and got.shape == (bench.DUMP_SAMPLES,)
        np.testing.assert_array_equal(got, np.load(tmp_path / "b" / (n + ".npy")))
        np.testing.assert_array_equal(got, (x + i).numpy().ravel()[idx])
    assert len(names) * bench.DUMP_SAMPLES * 4 <= 64e6
