"""Guarded allocations: every tensor a wrapper allocates sits between two bands of 0xFF bytes that must still be 0xFF afterwards.

``guarded()`` replaces torch.empty, empty_like, zeros, zeros_like, full and ones -- the constructors through which diff_sal_amd/ops.py
and autograd_ops.py allocate every output and workspace -- and puts them back on exit, also after an exception.  A call whose result
would be a contiguous tensor of at least one element on the guarded device type ("cuda"; "cpu" for tests/test_guard_host.py) is served
from one larger uint8 allocation

    [ slack < 256 B | front guard | payload | back guard ]

whose every byte is 0xFF (the payload too for ``empty*``; the filling constructors then write theirs).  0xFF bytes are a NaN in
fp32, fp64, bf16 and fp16 and -1 / 255 in the integer types, so an element the kernel never writes is a NaN as well.  The payload
starts at a multiple of 256 bytes (what the caching allocator gives, and what float4 / buffer-descriptor code may assume); the back
guard starts at the payload's last byte + 1 with no padding, so an overrun of a single byte lands in it.  Every other call (CPU
tensor, pinned memory, a ``memory_format`` / ``out`` / ``layout`` argument, a non-contiguous ``empty_like`` source, no element)
passes through to the original and is counted as unguarded; those on the guarded device type are listed with their call site.

Guard size, each side: max(64 KiB, 256 x bytes of one row of the last dimension), at most 4 MiB, rounded up to 256 B.
  * An overrun that continues where the buffer ends -- one element, one float4, one row or one tile too many -- starts in the
    first bytes of the back guard (the last bytes of the front one for an underrun) whatever the guard's size: any size finds it.
  * A strided overrun skips bytes: a tile that stores r rows too many, each a part of a row of the last dimension, touches
    payload_end + j * row_bytes + column offset for j < r.  256 rows is the tallest tile of the library (the 256 x 96 tile of
    gemm16_dma / conv16_dma), so 256 rows of the last dimension hold every row such a tile can add; the same holds for a halo
    load some rows in front.
  * 64 KiB is the floor so that narrow tensors (a [M, 4] fp32 row is 16 B) still see a stray access tens of thousands of elements
    away, 4 MiB the cap so that the widest rows (a 1 M-element reduction scratch) do not multiply the memory of a case.
An access further away than the guard is not seen, nor is one that lands in a guard and writes 0xFF.

What is and is not detected
  * a write outside a guarded output or workspace, within the guard's reach: ``check()`` names the allocation, side and offsets;
  * a read outside a guarded input (``put``) or workspace that reaches an output, even multiplied by zero: the NaN shows against
    the test's reference;
  * NOT an over-read whose value is masked off or otherwise dropped afterwards (a select, a buffer-descriptor load the kernel
    then ignores): nothing of it is left to observe;
  * NOT an access to memory the shim did not allocate (a tensor made by .clone(), .to(), torch.cat or a Tensor.new_* method).
"""
import contextlib
import os
import sys

import torch

KIB = 1024
GUARD_MIN = 64 * KIB
GUARD_MAX = 4 * KIB * KIB
GUARD_ROWS = 256
ALIGN = 256
FILL = 0xFF
NAMES = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones")
SITE_FILES = ("ops.py", "autograd_ops.py")

_ACTIVE = [None]


def guard_bytes(shape, itemsize):
    """max(64 KiB, 256 rows of the last dimension), capped at 4 MiB, rounded up to 256 B (derivation: module docstring)."""
    row = (shape[-1] if len(shape) else 1) * itemsize
    g = min(max(GUARD_MIN, GUARD_ROWS * row), GUARD_MAX)
    return (g + ALIGN - 1) // ALIGN * ALIGN


class GuardError(AssertionError):
    pass


class _Buffer:
    __slots__ = ("order", "raw", "start", "nbytes", "guard", "shape", "dtype", "site", "kind")

    def describe(self):
        return f"allocation #{self.order} ({self.kind}) {tuple(self.shape)} {self.dtype} asked for at {self.site}"


def _site():
    """file:line of the nearest caller in ops.py / autograd_ops.py, else of the nearest caller outside this file."""
    f = sys._getframe(2)
    first = None
    while f is not None:
        name = f.f_code.co_filename
        if name != __file__:
            if first is None:
                first = f"{os.path.basename(name)}:{f.f_lineno}"
            if os.path.basename(name) in SITE_FILES:
                return f"{os.path.basename(name)}:{f.f_lineno} ({f.f_code.co_name})"
        f = f.f_back
    return first or "?"


class Guard:
    """What ``guarded()`` yields: ``put``, ``owns``, ``check`` and the counters."""

    def __init__(self, device_type="cuda"):
        self.device_type = device_type
        self.buffers = []
        self.guarded = 0            # constructor calls served from a guarded buffer
        self.puts = 0               # inputs uploaded through put()
        self.unguarded = 0          # constructor calls passed through, any device
        self.unguarded_device = []  # those of them on the guarded device type: "call site: what"
        self.bytes = 0              # bytes allocated for guarded buffers, guards included
        self._orig = {}
        self._ptrs = {}
        self._inside = False

    # ---- allocation --------------------------------------------------------------------------------------------------------------
    def _alloc(self, shape, dtype, device, kind, fill_payload=True):
        itemsize = dtype.itemsize
        numel = 1
        for s in shape:
            numel *= int(s)
        nbytes = numel * itemsize
        g = guard_bytes(shape, itemsize)
        raw = self._orig["empty"]((ALIGN + 2 * g + nbytes,), dtype=torch.uint8, device=device)
        slack = -raw.data_ptr() % ALIGN
        raw = raw[:slack + 2 * g + nbytes]          # the back guard is the buffer's end
        b = _Buffer()
        b.order, b.raw, b.start, b.nbytes, b.guard = len(self.buffers), raw, slack + g, nbytes, g
        b.shape, b.dtype, b.site, b.kind = tuple(int(s) for s in shape), dtype, _site(), kind
        if fill_payload:
            raw.fill_(FILL)
        else:
            raw[:b.start].fill_(FILL)
            raw[b.start + nbytes:].fill_(FILL)
        self.buffers.append(b)
        self._ptrs[raw.untyped_storage().data_ptr()] = b
        self.bytes += raw.numel()
        return raw[b.start:b.start + nbytes].view(dtype).view(b.shape)

    def _shim(self, name):
        orig = self._orig[name]
        like = name.endswith("_like")

        def shim(*args, **kwargs):
            if self._inside:                # torch's own Python code (meta kernels) asking for a tensor on behalf of a call below
                return orig(*args, **kwargs)
            self._inside = True
            try:
                return serve(*args, **kwargs)
            finally:
                self._inside = False

        def serve(*args, **kwargs):
            meta = None
            plain = not any(kwargs.get(k) is not None for k in ("memory_format", "out", "layout", "names")) and not kwargs.get("pin_memory")
            device = kwargs.get("device")
            if device is None:
                device = args[0].device if like else torch.get_default_device()
            device = torch.device(device)
            if plain and device.type == self.device_type:
                kw = {k: v for k, v in kwargs.items() if k not in ("requires_grad", "pin_memory")}
                kw["device"] = "meta"
                meta = orig(*args, **kw)
                if meta.numel() == 0 or not meta.is_contiguous():
                    meta = None
            if meta is None:
                self.unguarded += 1
                if device.type == self.device_type:
                    self.unguarded_device.append(f"{_site_of_shim()}: torch.{name} passed through unguarded")
                return orig(*args, **kwargs)
            self.guarded += 1
            out = self._alloc(meta.shape, meta.dtype, device, "torch." + name, fill_payload=name.startswith("empty"))
            if name.startswith("zeros"):
                out.zero_()
            elif name == "ones":
                out.fill_(1)
            elif name == "full":
                out.fill_(args[1] if len(args) > 1 else kwargs["fill_value"])
            if kwargs.get("requires_grad"):
                out.requires_grad_(True)
            return out

        shim.__name__ = name
        return shim

    def put(self, t, device=None):
        """A copy of the CPU or device tensor ``t`` (None stays None) in a guarded buffer on the guarded device type, same shape and
        dtype, contiguous: the upload function that tests hand to their case bodies, so that every input is surrounded by NaN.  An
        out-of-range read that reaches an output, even multiplied by zero, then shows as NaN against the reference; an over-read
        that is masked off afterwards is not detected."""
        if t is None:
            return None
        if device is None:
            device = t.device if t.device.type == self.device_type else torch.device(self.device_type)
        self.puts += 1
        out = self._alloc(t.shape, t.dtype, device, "put")
        if t.numel():
            out.copy_(t)
        return out

    def owns(self, t):
        """True if ``t``'s storage is one of the registered buffers (a view of a guarded tensor counts)."""
        return torch.is_tensor(t) and t.untyped_storage().data_ptr() in self._ptrs

    # ---- the check ---------------------------------------------------------------------------------------------------------------
    def check(self):
        """Both guards of every registered buffer must be all 0xFF; compared on the device, one synchronisation when all is well."""
        if not self.buffers:
            return
        flags = []
        for b in self.buffers:
            flags.append((b.raw[b.start - b.guard:b.start] != FILL).any())
            flags.append((b.raw[b.start + b.nbytes:] != FILL).any())
        by_device = {}
        for f in flags:
            by_device.setdefault(f.device, []).append(f)
        if not any(bool(torch.stack(fs).any()) for fs in by_device.values()):
            return
        lines = []
        for b, front, back in zip(self.buffers, flags[0::2], flags[1::2]):
            for side, hit in (("front", front), ("back", back)):
                if not bool(hit):
                    continue
                lo, hi = (b.start - b.guard, b.start) if side == "front" else (b.start + b.nbytes, b.start + b.nbytes + b.guard)
                band = b.raw[lo:hi]
                at = (band != FILL).nonzero().flatten()
                base = -b.guard if side == "front" else 0
                found = " ".join(f"{int(v):02x}" for v in band[at[:8]].cpu())
                what = ("bytes in front of the payload's first byte (-1 = the byte just in front)" if side == "front"
                        else "bytes behind the payload's last byte (0 = the byte just behind)")
                lines.append(f"{b.describe()}: {side} guard changed, {at.numel()} bytes, offsets {base + int(at[0])} .. {base + int(at[-1])} "
                             f"{what}; payload {b.nbytes} B, guard {b.guard} B; first bytes found: {found}")
        raise GuardError("guard bytes were overwritten:\n  " + "\n  ".join(lines))

    def release(self):
        self.buffers.clear()
        self._ptrs.clear()


def _site_of_shim():
    f = sys._getframe(2)
    while f is not None:
        if f.f_code.co_filename != __file__:
            return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})"
        f = f.f_back
    return "?"


@contextlib.contextmanager
def guarded(device_type="cuda"):
    """The six constructors replaced while active (not re-entrant); ``check()`` runs on a normal exit, and the buffers are released."""
    if _ACTIVE[0] is not None:
        raise RuntimeError("guarded() is already active: nesting is refused")
    g = Guard(device_type)
    g._orig = {n: getattr(torch, n) for n in NAMES}
    _ACTIVE[0] = g
    try:
        for n in NAMES:
            setattr(torch, n, g._shim(n))
        yield g
        g.check()
    finally:
        for n, f in g._orig.items():
            setattr(torch, n, f)
        _ACTIVE[0] = None
        g.release()

