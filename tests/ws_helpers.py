"""The memory-contract harness (not a test module; tests/test_memory_contract.py, DESIGN.md "Memory contract").

Every workspace, engine state, packed buffer and output of piccolo_amd/ops.py is a torch.empty: ops._bytes(n) for the byte buffers, torch.empty
for the typed outputs.  poisoned(fill_word) replaces both names of that module: every such allocation then sits between two guards of
GUARD bytes of 0xC3, its interior holds fill_word repeated, and a ledger remembers it.  A result that depends on memory the library never
wrote changes with the fill word; a write outside the queried bytes damages a guard.

Three fill words, because each hides what another shows:
    0x00000000  0.0 / 0 / u64 0: a missing z-buffer initialisation (depth 0 occludes everything); hides a missing zero-init
    0xFFFFFFFF  NaN / -1 / the z-buffers' "empty" word: a missing zero-init of sums, counters, tickets, border texels; hides a missing
                "empty" fill and vanishes wherever a comparison masks NaN
    0x3F800000  1.0 / 1065353216: finite, survives fminf / fmaxf and comparison masks; changes sums, counts and colours visibly
No structure meant to be trusted is ever planted: the fills are these words and nothing else."""
import collections
import contextlib
import struct
import sys

import torch

GUARD = 4096                 # keeps the view 512-aligned like the caching allocator's own blocks; catches overruns of up to a page
GUARD_BYTE = 0xC3
FILL_WORDS = (0x00000000, 0xFFFFFFFF, 0x3F800000)

# base: the flat uint8 buffer, guards included; n: the interior's bytes; caller: (co_name, f_lineno) of the frame that asked;
# kind: "bytes" (ops._bytes) or "empty" (ops.torch.empty)
Entry = collections.namedtuple("Entry", "base n caller kind")
Run = collections.namedtuple("Run", "result callers")

_LEDGER = None               # the active context's ledger


def _signed(word):
    return struct.unpack("<i", struct.pack("<I", word))[0]


def _guarded(n, word, dev, caller, kind, ledger):
    """a flat uint8 buffer of GUARD + n + GUARD bytes on dev, guards and interior filled, recorded -> the interior view"""
    base = torch.empty(GUARD + n + GUARD, dtype=torch.uint8, device=dev)
    base[:GUARD] = GUARD_BYTE
    base[GUARD + n:] = GUARD_BYTE
    inner = base[GUARD:GUARD + n]
    full = n // 4 * 4
    if full:
        inner[:full].view(torch.int32).fill_(_signed(word))
    if n > full:
        inner[full:] = torch.tensor(list(struct.pack("<I", word))[:n - full], dtype=torch.uint8, device=dev)
    ledger.append(Entry(base, n, caller, kind))
    return inner


class _TorchProxy:
    """forwards every attribute to torch, except `empty`"""

    def __init__(self, word, device, ledger):
        self.__dict__.update(_word=word, _device=device, _ledger=ledger)

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        dev = torch.device(device) if device is not None else torch.device("cpu")
        if dev.type != ("cuda" if self._device is None else self._device.type):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        dtype = dtype or torch.get_default_dtype()
        numel = 1
        for s in size:
            numel *= int(s)
        nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        f = sys._getframe(1)
        inner = _guarded(nbytes, self._word, dev, (f.f_code.co_name, f.f_lineno), "empty", self._ledger)
        return inner.view(dtype).reshape(tuple(int(s) for s in size))


def clear_caches():
    """the pack cache (cached engines among its entries), the colour templates, the candidate grids and the pack kernels' scratch flags"""
    from piccolo_amd import color_utils, omniloc, ops, utils
    omniloc._cache.clear()
    color_utils._templates.clear()
    utils._ROT_GRIDS.clear()
    utils._INIT_KEYS.clear()
    ops._SCRATCH_FLAGS.clear()


@contextlib.contextmanager
def poisoned(fill_word, device=None, refuse_above=None, refuse_in=None):
    """Replaces ops._bytes and ops.torch while active (module docstring) -> the ledger, a list of Entry.  device: where the guarded buffers
    live and which torch.empty results are guarded — None: the GPU; "cpu" for the harness's own tests.  refuse_above: _bytes raises
    torch.cuda.OutOfMemoryError for more bytes than that, unrecorded, when the function refuse_in asks (None: whoever asks) — how
    tests/test_hist_fallbacks.py reaches the allocation ladder's last resort without provoking an allocation failure."""
    global _LEDGER
    from piccolo_amd import ops
    assert 0 <= fill_word <= 0xFFFFFFFF
    dev = None if device is None else torch.device(device)
    ledger = []
    real_bytes, real_torch = ops._bytes, ops.torch

    def _bytes(nbytes):
        f = sys._getframe(1)
        if refuse_above is not None and nbytes > refuse_above and refuse_in in (None, f.f_code.co_name):
            raise torch.cuda.OutOfMemoryError("memory contract: no more than %d bytes" % refuse_above)
        return _guarded(max(int(nbytes), 16), fill_word, dev if dev is not None else ops.device(), (f.f_code.co_name, f.f_lineno), "bytes", ledger)

    clear_caches()
    outer, _LEDGER = _LEDGER, ledger
    ops._bytes, ops.torch = _bytes, _TorchProxy(fill_word, dev, ledger)
    try:
        yield ledger
    finally:
        ops._bytes, ops.torch = real_bytes, real_torch
        _LEDGER = outer
        clear_caches()


def check_guards(ledger=None):
    """every head and tail guard byte of every ledger entry is still 0xC3; a failure names the caller and the first damaged offset
    (relative to the interior: negative in the head guard, >= n in the tail guard)"""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    ledger = _LEDGER if ledger is None else ledger
    assert ledger is not None, "check_guards outside poisoned()"
    if not ledger:
        return
    flags = torch.stack([((e.base[:GUARD] != GUARD_BYTE).any() | (e.base[GUARD + e.n:] != GUARD_BYTE).any()).cpu() for e in ledger])
    if not bool(flags.any()):
        return
    e = ledger[int(flags.nonzero()[0])]
    bad = torch.cat([e.base[:GUARD], e.base[GUARD + e.n:]]) != GUARD_BYTE
    at = int(bad.nonzero()[0])
    offset = at - GUARD if at < GUARD else e.n + at - GUARD
    raise AssertionError("guard damaged: %s of %s:%d (%d bytes) wrote at offset %d" % (e.kind, e.caller[0], e.caller[1], e.n, offset))


def same_bits(a, b):
    """equal as bits (view as uint8, torch.equal), so that a NaN equals the same NaN; shapes and dtypes must agree.  None, numbers and
    nested lists / tuples compare entry by entry."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if not torch.is_tensor(a) or not torch.is_tensor(b):
        if torch.is_tensor(a) or torch.is_tensor(b):
            return False
        if isinstance(a, (int, float)) and isinstance(b, (int, float)):
            return struct.pack("<d", float(a)) == struct.pack("<d", float(b))
        return type(a) is type(b) and a == b
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8).cpu(), b.contiguous().reshape(-1).view(torch.uint8).cpu())


def flat(obj, prefix="", out=None):
    """a nested dict / list / tuple / attribute bag of tensors (None, numbers, strings) -> a flat dict of its leaves, keyed by their path"""
    out = {} if out is None else out
    if not torch.is_tensor(obj) and hasattr(obj, "__dict__"):
        obj = vars(obj)
    if isinstance(obj, dict):
        for k, v in obj.items():
            flat(v, "%s%s." % (prefix, k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            flat(v, "%s%d." % (prefix, i), out)
    else:
        out[prefix[:-1]] = obj.detach().clone() if torch.is_tensor(obj) else obj
    return out


def differences(ref, got):
    """the keys at which two flat result dicts differ (a missing key differs)"""
    return sorted(k for k in set(ref) | set(got) if k not in ref or k not in got or not same_bits(ref[k], got[k]))


def poisoned_runs(scenario, device=None, **kw):
    """scenario() under each fill word -> {word: Run(its flat result, its ledger's (kind, caller) list)}; the guards are checked after each"""
    runs = {}
    for word in FILL_WORDS:
        with poisoned(word, device, **kw) as ledger:
            result = scenario()
            check_guards(ledger)
            runs[word] = Run(result, [(e.kind, e.caller) for e in ledger])
    return runs


def assert_contract(ref, runs):
    """what every scenario asserts: the unpatched result and the three poisoned ones are bit-identical key by key, every ledger is
    non-empty, and the ledgers have the same length and callers"""
    for word, run in runs.items():
        diff = differences(ref, run.result)
        assert not diff, "fill word 0x%08X changes %s" % (word, diff)
        assert run.callers, "fill word 0x%08X: nothing was allocated through ops" % word
    first = runs[FILL_WORDS[0]].callers
    for word, run in runs.items():
        assert run.callers == first, "fill word 0x%08X: %d allocations, 0x%08X has %d (or other callers)" % (word, len(run.callers), FILL_WORDS[0],
                                                                                                         len(first))


def bytes_sites(path=None):
    """the `_bytes(` call sites of piccolo_amd/ops.py by an ast walk: a list of (enclosing function's name, line), one per call"""
    import ast
    import os
    if path is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "piccolo_amd", "ops.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    sites = []

    def walk(node, name):
        for child in ast.iter_child_nodes(node):
            inner = child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else "<lambda>" if isinstance(child, ast.Lambda) else name
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Name) and child.func.id == "_bytes":
                sites.append((name, child.lineno))
            walk(child, inner)

    walk(tree, "<module>")
    return sites
