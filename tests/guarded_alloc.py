"""TEST INFRASTRUCTURE: exact-size, poisoned, guarded buffers for every allocation the host layer sizes from a ``*_bytes`` /
``*_floats`` query of the C ABI.

The product hides two kinds of bug from the parity cases: its workspace cache only grows (a small case gets the buffer of a
larger one), and the allocator behind ``torch.empty`` rounds sizes up and hands back a kernel's previous, finite output.  Inside
``with guarded(monkeypatch) as g:`` the two allocation functions of ``dprox._ops`` are substituted:

* ``ops._bytes(n, device, zero=False)`` takes one uint8 arena of ``G + n + G`` bytes (``n`` after the product's own
  ``max(n, 16)``) and returns the view ``arena[G:G + n]``.  The back guard starts at byte ``n`` exactly; ``G`` = 64 KiB, a multiple
  of 512, so the payload keeps the start alignment of an allocation of its own.  Both guards hold a fixed byte pattern (never 0,
  never 0xFF); the payload is filled with 0xFF -- NaN as float16 / bfloat16 / float32 / float64, -1 as an integer -- or with zeros
  for ``zero=True``.  A read of workspace that was never written therefore surfaces as NaN in the case's own comparison.
* ``ops.workspace(tag, nbytes, device)`` reuses nothing: every request is a fresh guarded buffer of exactly ``nbytes``.
* ``Library.query`` is wrapped: every ``*_bytes`` / ``*_floats`` name (``is_size_query``: the ``*_bytes_bf16`` ones too) is
  recorded (``g.seen``), and each guarded buffer remembers the most recent such query with its arguments.
* every arena is kept in a registry until ``check()``, so freed memory is not recycled under a later buffer;
  ``ops.clear_caches()`` runs on entry and on exit, so no guarded view outlives the context.

``g.check()`` synchronises the device, compares every guard with the pattern on the device, and fails the calling test with one
line per damaged buffer: the recorded query and its arguments, ``n``, which guard, the offset of the first damaged byte and the
number of damaged bytes.

What this does NOT catch -- a stated condition, not a measurement: a stray write further than 64 KiB from the buffer lands
outside the arena and is not seen; reads beyond the payload are seen only through the guard pattern's effect on the result.
Outputs and iterates (``torch.empty_like`` and friends) are not guarded: only query-sized buffers are.

``shrink={"dpx_x_bytes": k}`` hands out a payload ``k`` bytes shorter than requested for buffers sized by that query (the back
guard moves in with it: an access of the last ``k`` bytes lands in the arena's own guard) -- the self-test that a wrong
``*_bytes`` formula is reported.
"""
import contextlib
import os
import time

import torch

G = 64 << 10
POISON = 0xFF
_patterns = {}
STATS = []            # one dict per finished guarded(...) context: label, seconds, buffers, hits, queries


def is_size_query(name):
    """dpx_*_bytes / dpx_*_floats, and the bf16-history variants whose names go on (dpx_admm_unrolled_hist_bytes_bf16)"""
    return "_bytes" in name or "_floats" in name


def _pattern(device):
    """G bytes, every value in 2 .. 252, period 251 (a prime: no power-of-two stride of a kernel maps onto itself)"""
    key = str(device)
    if key not in _patterns:
        _patterns[key] = (torch.arange(G, dtype=torch.int32) % 251 + 2).to(torch.uint8).to(device)
    return _patterns[key]


class Guard:
    def __init__(self, shrink=None, label=""):
        self.shrink = dict(shrink or {})
        self.label = label
        self.seen = set()              # names of the *_bytes / *_floats queries asked so far
        self.last = (None, ())         # the most recent of them, with its arguments
        self.live = []                 # (arena, n, query name, query args) not yet checked
        self.buffers = 0
        self.hits = []

    # ---- the substitutes ----------------------------------------------------------------------------------------------------
    def bytes(self, n, device, zero=False):
        name, args = self.last
        n = max(int(n), 16)
        n = max(n - int(self.shrink.get(name, 0)), 0)
        arena = torch.empty(G + n + G, dtype=torch.uint8, device=device)
        pat = _pattern(arena.device)
        arena[:G].copy_(pat)
        arena[G + n:].copy_(pat)
        payload = arena[G:G + n]
        payload.zero_() if zero else payload.fill_(POISON)
        self.live.append((arena, n, name, args))
        self.buffers += 1
        return payload

    def workspace(self, tag, nbytes, device):
        return self.bytes(nbytes, device)

    def note_query(self, name, args):
        if is_size_query(name):
            self.seen.add(name)
            self.last = (name, tuple(args))

    # ---- the check ----------------------------------------------------------------------------------------------------------
    def damage(self):
        """[(query, args, n, 'front' | 'back', offset of the first damaged byte in that guard, damaged bytes)] of the buffers handed
        out since the last call; releases them"""
        live, self.live = self.live, []
        if any(a.is_cuda for a, *_ in live):
            torch.cuda.synchronize()
        out = []
        if not live:
            return out
        counts = torch.stack([torch.stack([(a[:G] != _pattern(a.device)).sum(), (a[G + n:] != _pattern(a.device)).sum()]) for a, n, *_ in live]).cpu()
        for (a, n, name, args), (front, back) in zip(live, counts.tolist()):
            for side, cnt, guard in (("front", front, a[:G]), ("back", back, a[G + n:])):
                if cnt:
                    first = int((guard != _pattern(a.device)).nonzero()[0])
                    out.append((name, args, n, side, first, int(cnt)))
        return out

    def check(self):
        hits = self.damage()
        self.hits += hits
        if hits:
            lines = [f"{name}{args}: n = {n}, {side} guard damaged from offset {first}, {cnt} byte(s)" for name, args, n, side, first, cnt in hits]
            raise AssertionError("guarded workspace(s) written out of bounds:\n  " + "\n  ".join(lines))


@contextlib.contextmanager
def guarded(monkeypatch, shrink=None, label=""):
    from dprox import _backend as be
    from dprox import _ops as ops
    g = Guard(shrink, label)
    real_query = be.Library.query

    def query(self, name, *args):
        g.note_query(name, args)
        return real_query(self, name, *args)

    t0 = time.perf_counter()
    ops.clear_caches()
    with monkeypatch.context() as m:
        m.setattr(be.Library, "query", query)
        m.setattr(ops, "_bytes", g.bytes)
        m.setattr(ops, "workspace", g.workspace)
        try:
            yield g
        finally:
            ops.clear_caches()
            g.live = []
            STATS.append({"label": label, "seconds": time.perf_counter() - t0, "buffers": g.buffers, "hits": len(g.hits), "queries": sorted(g.seen)})


def run(monkeypatch, label, fn, *args, **kwargs):
    """``fn(*args, **kwargs)`` on guarded workspaces, then the check; returns the Guard (its ``seen`` feeds a coverage test)"""
    with guarded(monkeypatch, label=label) as g:
        fn(*args, **kwargs)
        g.check()
    return g


def report(allow=()):
    """the text committed as profiles/guarded_alloc.txt: per guarded run its wall time, buffers, guard hits and (indented, without
    the dpx_ prefix) the size queries it asked; then the union of the queries and the coverage test's allow-list"""
    lines = [f"{'run':<64} {'seconds':>8} {'buffers':>8} {'hits':>5}"]
    seen = set()
    for s in STATS:
        lines.append(f"{s['label']:<64} {s['seconds']:8.2f} {s['buffers']:8d} {s['hits']:5d}")
        lines.append("    " + " ".join(q[4:] for q in s["queries"]))
        seen.update(s["queries"])
    lines.append(f"queries seen ({len(seen)}): " + " ".join(sorted(seen)))
    lines.append("allow-list: " + (" ".join(sorted(allow)) if allow else "(empty)"))
    return "\n".join(lines) + "\n"


def write_report(allow=()):
    """with DPX_GUARDED_REPORT set, ``report()`` is written to the file it names (the judged copy is profiles/guarded_alloc.txt)"""
    path = os.environ.get("DPX_GUARDED_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(report(allow))
