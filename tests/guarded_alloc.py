"""TEST INFRASTRUCTURE ONLY: every buffer the package hands to a kernel, poisoned and fenced.

Inside `guarded(fill)` the four calls the Python layer allocates outputs, gradients and workspaces with - `torch.empty`, `torch.empty_like`,
`torch.zeros`, `torch.Tensor.new_empty` - return the middle of a larger uint8 allocation whose every byte is `fill`: a guard band of G bytes
on each side of the payload (`zeros` then zeroes its payload).  What that shows that a fresh or a recycled block hides:

  1. an element a launch never writes keeps the fill (0xFF: NaN in f32 / f64 / bf16 / f16, -1 in integers; 0x7B: 1.3e36 in f32 and bf16,
     61 280 in f16) instead of the previous call's correct value, or `malloc`'s zero on the host build;
  2. a write outside the payload lands in a guard band, which is compared byte for byte with the fill when the context ends;
  3. a kernel that reads an output, an accumulator or a workspace before it initialised it computes with the fill - and two runs under two
     fills then differ, whatever the dtype.

G is a multiple of 256 bytes, so a payload is aligned as the allocator's own blocks are and every kernel takes the path it takes in the product.

What is guarded: allocations made from the package's own frames (module `kornia_amd.*`) of memory a kernel may be handed.  On a HIP device
that is decided by the device of the allocation (its `device` argument, or the template's): host memory passes through.  On the host build of
the kernels (tests/emu/mode.py) "cuda" is host memory and a device says nothing, so every allocation of the package is guarded but the call
sites listed in `HOST_STAGING`, each with the reason no kernel reads it; enter `emulated_device()` first, this context second.  What passes
through unchanged on both: the tests' own allocations (and torch's, and the oracle's) and calls with `pin_memory`, `out=`, `memory_format=`,
a layout or `requires_grad`.

The same context replaces `kornia_amd._native.lib` by a proxy that records which `km_*` entry points were called (`Guard.called`)."""
from __future__ import annotations

import contextlib
import linecache
import sys

import torch

G = 64 * 1024

# Host staging the package allocates and no kernel ever reads: what the host build passes through (on a device their memory is host memory and
# passes anyway).  (file, the statement that allocates): reason.  Matched by the text of the calling line, so an entry follows its statement
# when lines move and covers nothing else in the file.
HOST_STAGING = {
    # draws.py:34 - the (pinned) host buffer a call's random draws are written to by torch's CPU generator; it crosses to the device as
    # ONE copy (`.to(device)`) and the kernels read that copy (on the host build the copy is a clone, tests/emu/mode.py).  It must stay an
    # allocation of its own: draws.py:87 and `device_views` find a parameter's place as `data_ptr() - (start of its storage)`, and a
    # payload in the middle of a guarded buffer would put every such offset one guard band too low - the views would then show the band.
    ("kornia_amd/augmentation/draws.py", "self.buf = torch.empty("): "host side of the draws: filled by the CPU generator, copied to the device, never passed to a kernel",
    # draws.py:87 - a 0-element tensor that is at once `.set_()` onto an existing host storage: no memory of its own.
    ("kornia_amd/augmentation/draws.py", "return torch.empty(0, dtype=torch.float32).set_(store)"): "empty(0) re-pointed at an existing host storage with set_()",
}


class GuardBandOverwritten(AssertionError):
    pass


class _Recorder:
    """`kornia_amd._native.lib()` with the names of the `km_*` attributes that were fetched (every call site fetches at the call)."""

    def __init__(self, handle, called: set):
        object.__setattr__(self, "_h", handle)
        object.__setattr__(self, "_called", called)

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        if name.startswith("km_"):
            self._called.add(name)
        return fn

    def __setattr__(self, name, value):
        setattr(self._h, name, value)


class Guard:
    def __init__(self, fill: int):
        self.fill = int(fill)
        self.word = int.from_bytes(bytes([self.fill]) * 8, "little", signed=True)
        self.records = []  # (raw uint8 tensor, payload bytes, "file:line", shape, dtype, zeroed)
        self.called: set = set()

    # ---- allocation -------------------------------------------------------------------------------------------------------------------
    def alloc(self, shape, dtype, device, zero: bool, site: str, strides=None) -> torch.Tensor:
        """A guarded tensor of `shape` (contiguous, or with the given strides of a dense layout)."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = n * item
        # (the buffer is filled and its bands compared as 64-bit words: 8 K elements a band, below the size at which torch splits a host op
        # over its thread pool - the worker processes of a parallel CPU run would fight for the cores)
        raw = _REAL["empty"](G + ((nbytes + 7) & ~7) + G, dtype=torch.uint8, device=device)
        raw.view(torch.int64).fill_(self.word)
        if zero and nbytes:
            raw[G:G + nbytes].zero_()
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.append(acc)
                acc *= max(s, 1)
            strides = tuple(reversed(strides))
        assert n == 0 or 1 + sum((d - 1) * st for d, st in zip(shape, strides)) == n, f"{site}: strides {strides} of shape {shape} are not a dense layout"
        # (set_ on the storage, not a view: a view returned from an autograd Function's forward would forbid the caller's in-place ops)
        out = _REAL["empty"](0, dtype=dtype, device=raw.device).set_(raw.untyped_storage(), G // item, shape, tuple(strides))
        self.records.append((raw, nbytes, site, shape, dtype, bool(zero)))
        return out

    def zero_initialised(self, file: str, shape, since: int = 0) -> bool:
        """was a buffer of `shape` allocated from `file` (records since index `since`) handed out zeroed?  What the package itself does where
        a kernel accumulates into the buffer instead of writing every element."""
        return any(z for _, _, site, sh, _, z in self.records[since:] if site.split(":")[0].endswith(file) and sh == tuple(shape))

    def _differs(self, raw, nbytes):
        """0-dim bool tensor: some byte outside the payload is not the fill"""
        end = G + ((nbytes + 7) & ~7)
        bad = raw[:G].view(torch.int64).ne(self.word).any() | raw[end:].view(torch.int64).ne(self.word).any()
        return bad | raw[G + nbytes:end].ne(self.fill).any() if end != G + nbytes else bad

    # ---- the check --------------------------------------------------------------------------------------------------------------------
    def check(self) -> None:
        """Every guard band is still the fill, byte for byte (one comparison per allocation, one read-back per device)."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if not self.records:
            return
        bad = [self._differs(raw, nbytes) for raw, nbytes, *_ in self.records]
        by_device = {}
        for b in bad:
            by_device.setdefault(b.device, []).append(b)
        if not any(bool(torch.stack(v).any()) for v in by_device.values()):
            return
        for (raw, nbytes, site, shape, dtype, _), b in zip(self.records, bad):
            if bool(b):
                lo, hi = raw[:G].ne(self.fill).cpu(), raw[G + nbytes:].ne(self.fill).cpu()
                if lo.any():
                    off = int(lo.nonzero()[-1]) - G  # (the byte nearest the payload)
                else:
                    off = nbytes + int(hi.nonzero()[0])
                raise GuardBandOverwritten(f"write outside the buffer allocated at {site} (shape {shape}, {dtype}, {nbytes} bytes): "
                                           f"first overwritten byte at offset {off} from the start of the payload")


_ACTIVE: list = []


def current() -> Guard:
    """the innermost active guard: for a test that calls the C ABI itself and wants its own buffers fenced (`current().alloc(...)`)"""
    return _ACTIVE[-1]


_REAL = {"empty": torch.empty, "empty_like": torch.empty_like, "zeros": torch.zeros}
_PASS_KW = ("pin_memory", "out", "memory_format", "layout", "requires_grad", "names")


def _passes(kw) -> bool:
    return any(kw.get(k) is not None and kw.get(k) is not False for k in _PASS_KW)


def _guarded_caller(frame) -> str | None:
    """"file:line" when the calling frame is the package's - and, on the host build, no host-staging site -, else None"""
    if not frame.f_globals.get("__name__", "").startswith("kornia_amd."):
        return None
    path, line = frame.f_code.co_filename.replace(chr(92), "/"), frame.f_lineno
    if not torch.cuda.is_available():
        text = linecache.getline(path, line).strip()
        if any(path.endswith(p) and text.startswith(stmt) for p, stmt in HOST_STAGING):
            return None
    return f"{path[path.rfind('kornia_amd/'):]}:{line}"


def _is_device(device) -> bool:
    """may a kernel be handed memory of `device` (None: torch's default, the host)?  On the host build the caller alone decides."""
    if not torch.cuda.is_available():
        return True
    return device is not None and torch.device(device).type == "cuda"


def _shape_of(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(args[0])
    return tuple(args)


@contextlib.contextmanager
def guarded(fill: int = 0xFF):
    """Patch the four allocation calls and `kornia_amd._native.lib`; restore them and check every guard band on exit (the bands are checked
    on an error inside the context too - a stray write may be its cause - but the error itself wins)."""
    from kornia_amd import _native as N

    g = Guard(fill)

    def _factory(real, zero):
        def patched(*args, **kw):
            site = _guarded_caller(sys._getframe(1))
            if site is None or _passes(kw) or "size" in kw or not _is_device(kw.get("device")):
                return real(*args, **kw)
            return g.alloc(_shape_of(args), kw.get("dtype") or torch.get_default_dtype(), kw.get("device") or "cpu", zero, site)
        return patched

    def empty_like(t, **kw):
        site = _guarded_caller(sys._getframe(1))
        if site is None or _passes(kw) or t.layout != torch.strided or not _is_device(kw.get("device") or t.device):
            return _REAL["empty_like"](t, **kw)
        # (the strides torch itself gives the result - a permuted template keeps its order, a sliced one comes out dense -, asked of a meta tensor)
        like = _REAL["empty_like"](t, device="meta", dtype=kw.get("dtype"))
        return g.alloc(t.shape, like.dtype, kw.get("device") or t.device, False, site, like.stride())

    real_new_empty = torch.Tensor.new_empty
    own_new_empty = "new_empty" in torch.Tensor.__dict__

    def new_empty(self, *args, **kw):
        site = _guarded_caller(sys._getframe(1))
        if site is None or _passes(kw) or "size" in kw or not _is_device(kw.get("device") or self.device):
            return real_new_empty(self, *args, **kw)
        return g.alloc(_shape_of(args), kw.get("dtype") or self.dtype, kw.get("device") or self.device, False, site)

    real_lib = N.lib
    outer = (torch.empty, torch.zeros, torch.empty_like)  # (another guard's, when nested: put back as found)
    N.lib = lambda: _Recorder(real_lib(), g.called)
    torch.empty, torch.zeros, torch.empty_like = _factory(_REAL["empty"], False), _factory(_REAL["zeros"], True), empty_like
    torch.Tensor.new_empty = new_empty
    _ACTIVE.append(g)
    ok = False
    try:
        yield g
        ok = True
    finally:
        _ACTIVE.pop()
        torch.empty, torch.zeros, torch.empty_like = outer
        if own_new_empty:
            torch.Tensor.new_empty = real_new_empty
        else:
            del torch.Tensor.new_empty
        N.lib = real_lib
        try:
            g.check()
        except GuardBandOverwritten:
            if ok:
                raise
            import traceback
            traceback.print_exc()  # (the test's own error is raised; the stray write is reported beside it)
        finally:
            g.records.clear()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


@contextlib.contextmanager
def unchanged(*tensors):
    """The arguments (None passes) hold the same bits on exit as on entry: a kernel's inputs - source, grad_out, matrix, taps, saved
    tensors - are read-only."""
    before = [None if t is None else _bits(t).clone() for t in tensors]
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    for i, (t, b) in enumerate(zip(tensors, before)):
        if t is not None:
            now = _bits(t)
            if not torch.equal(now, b):
                first = int((now != b).nonzero()[0])
                raise AssertionError(f"input {i} (shape {tuple(t.shape)}, {t.dtype}) was written to: first changed byte at offset {first}")


def same_bits(a, b) -> bool:
    """bit-for-bit equal, whatever the dtype (NaN payloads included)"""
    if a is None or b is None:
        return a is b
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))
