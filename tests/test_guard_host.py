"""tests/_guard.py on the CPU: the same shim with the device test switched to CPU tensors (``guarded("cpu")``), so that what
tests/test_gpu_guard_bands.py relies on -- placement, fill, detection with the right side and offset, restoration -- is proved
without a GPU."""
import re

import pytest
import torch

from tests import _guard as G

DTYPES = (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int32, torch.uint8)
ORIGINALS = {n: getattr(torch, n) for n in G.NAMES}


def buffer_of(g, t):
    return g._ptrs[t.untyped_storage().data_ptr()]


def originals_are_back():
    return all(getattr(torch, n) is ORIGINALS[n] for n in G.NAMES)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_payload_is_aligned_contiguous_and_filled(dtype):
    with G.guarded("cpu") as g:
        t = torch.empty((3, 5, 7), dtype=dtype)
        assert g.owns(t) and (g.guarded, g.unguarded, g.unguarded_device) == (1, 0, [])
        assert t.shape == (3, 5, 7) and t.dtype == dtype and t.is_contiguous()
        assert t.data_ptr() % 256 == 0
        if dtype.is_floating_point:
            assert torch.isnan(t).all()
        else:
            assert (t == (-1 if dtype == torch.int32 else 255)).all()
        b = buffer_of(g, t)
        assert (b.raw == 0xFF).all() and g.bytes == b.raw.numel() >= 2 * b.guard + 105 * dtype.itemsize
        assert t.data_ptr() == b.raw.data_ptr() + b.start and b.nbytes == 105 * dtype.itemsize
    assert originals_are_back()


def test_back_guard_starts_at_the_payloads_last_byte_plus_one():
    """37 bytes and 3 x 2 bytes: no multiple of 16, and no padding between the payload and the guard."""
    with G.guarded("cpu") as g:
        for t in (torch.empty(37, dtype=torch.uint8), torch.empty((3,), dtype=torch.bfloat16)):
            b = buffer_of(g, t)
            nbytes = t.numel() * t.element_size()
            assert b.nbytes == nbytes and nbytes % 16 != 0
            t.view(torch.uint8).fill_(0)
            zero = (b.raw == 0).nonzero().flatten()
            assert zero[0] == b.start and zero[-1] == b.start + nbytes - 1 and zero.numel() == nbytes
            assert b.raw.numel() - (b.start + nbytes) == b.guard and b.start >= b.guard
            g.check()
            b.raw[b.start + nbytes] = 0
            with pytest.raises(G.GuardError, match=r"back guard changed, 1 bytes, offsets 0 \.\. 0 "):
                g.check()
            b.raw[b.start + nbytes] = 0xFF


def test_filling_constructors_and_like_give_the_requested_contents():
    src = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    with G.guarded("cpu") as g:
        e = torch.empty_like(src)
        assert e.shape == src.shape and e.dtype == src.dtype and torch.isnan(e).all() and g.owns(e)
        e16 = torch.empty_like(src, dtype=torch.float16)
        assert e16.dtype == torch.float16 and g.owns(e16)
        z = torch.zeros(2, 3)
        assert z.dtype == torch.float32 and (z == 0).all() and g.owns(z)
        zl = torch.zeros_like(src)
        assert zl.dtype == torch.float64 and (zl == 0).all() and g.owns(zl)
        f = torch.full((2, 5), 2.5, dtype=torch.float64)
        assert (f == 2.5).all() and g.owns(f)
        fi = torch.full((4,), 7)
        assert fi.dtype == torch.int64 and (fi == 7).all() and g.owns(fi)
        o = torch.ones((3,), dtype=torch.int32)
        assert (o == 1).all() and g.owns(o)
        r = torch.zeros((2,), requires_grad=True)
        assert r.requires_grad and g.owns(r)
        for t in (z, zl, f, fi, o, r):
            b = buffer_of(g, t)
            assert (b.raw[:b.start] == 0xFF).all() and (b.raw[b.start + b.nbytes:] == 0xFF).all()
        assert g.guarded == 8 and g.unguarded == 0


def test_put_surrounds_an_input_with_nan():
    src = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    with G.guarded("cpu") as g:
        t = g.put(src)
        assert torch.equal(t, src) and t.data_ptr() != src.data_ptr() and g.owns(t) and not g.owns(src)
        assert g.owns(t[1:]) and g.put(None) is None
        nc = g.put(src.t())
        assert torch.equal(nc, src.t()) and nc.is_contiguous()
        assert (g.puts, g.guarded) == (2, 0)
        b = buffer_of(g, t)
        around = b.raw[b.start - 4:b.start].view(torch.float32), b.raw[b.start + b.nbytes:b.start + b.nbytes + 4].view(torch.float32)
        assert torch.isnan(around[0]).all() and torch.isnan(around[1]).all()


def test_other_calls_pass_through_and_are_counted():
    with G.guarded("cpu") as g:
        assert not g.owns(torch.empty(0))                                                   # no element
        assert not g.owns(torch.empty((2, 3, 4, 5), memory_format=torch.channels_last))     # a memory_format argument
        assert not g.owns(torch.empty_like(torch.zeros(3, 4).t()))                          # non-contiguous source (zeros: guarded)
        assert not g.owns(torch.empty(3, device="meta"))                                    # another device
        assert g.unguarded == 4 and g.guarded == 1
        assert len(g.unguarded_device) == 3 and all("test_guard_host.py" in s for s in g.unguarded_device)
    with G.guarded("cuda") as g:                                                            # CPU tensors while the GPU is guarded
        assert not g.owns(torch.zeros(3)) and g.unguarded == 1 and g.unguarded_device == []


WHERE = [("front", "first"), ("front", "last"), ("back", "first"), ("back", "last")]


@pytest.mark.parametrize("side,which", WHERE, ids=[f"{s}-{w}" for s, w in WHERE])
def test_one_changed_guard_byte_is_reported_with_side_and_offset(side, which):
    with pytest.raises(G.GuardError) as err:
        with G.guarded("cpu") as g:
            torch.zeros(5)
            t = torch.empty((7, 3), dtype=torch.float16)
            b = buffer_of(g, t)
            off = {"first": 0, "last": b.guard - 1}[which] + (-b.guard if side == "front" else 0)
            pos = (b.start if side == "front" else b.start + b.nbytes) + off
            b.raw[pos] = 0x3C
    msg = str(err.value)
    assert re.search(rf"allocation #1 \(torch\.empty\) \(7, 3\) torch\.float16 asked for at test_guard_host\.py:\d+: {side} guard changed, "
                     rf"1 bytes, offsets {off} \.\. {off} ", msg), msg
    assert "first bytes found: 3c" in msg and "allocation #0" not in msg
    assert originals_are_back()


def test_the_call_site_in_ops_is_named():
    """The stack at allocation time is searched for diff_sal_amd's ops.py / autograd_ops.py; compile() gives a frame of that name."""
    ns = {}
    exec(compile("import torch\ndef wrapper():\n    return torch.empty((4,))\n", "/somewhere/diff_sal_amd/ops.py", "exec"), ns)
    with G.guarded("cpu") as g:
        assert buffer_of(g, ns["wrapper"]()).site == "ops.py:3 (wrapper)"


def test_writing_every_payload_byte_does_not_fail():
    with G.guarded("cpu") as g:
        for dtype in DTYPES:
            t = torch.empty((5, 13), dtype=dtype)
            t.view(torch.uint8).fill_(0x5A)
            t.view(torch.uint8).fill_(0xFF)
            t.view(torch.uint8).fill_(0)
        g.check()


def test_originals_are_back_after_an_exception():
    with pytest.raises(KeyError):
        with G.guarded("cpu"):
            assert not originals_are_back()
            raise KeyError("x")
    assert originals_are_back()
    with G.guarded("cpu"):
        pass
    assert originals_are_back()


def test_nesting_is_refused():
    with G.guarded("cpu"):
        with pytest.raises(RuntimeError, match="nesting is refused"):
            with G.guarded("cpu"):
                pass
        assert not originals_are_back()         # the outer one is still active
    assert originals_are_back()


@pytest.mark.parametrize("shape,dtype,want", [
    ((1,), torch.float32, 64 * 1024),                       # the floor
    ((), torch.float64, 64 * 1024),
    ((1, 1536), torch.float32, 256 * 1536 * 4),             # 256 rows of 6 KiB = 1.5 MiB
    ((3, 100), torch.bfloat16, 64 * 1024),                  # 256 rows of 200 B < the floor
    ((3, 129), torch.bfloat16, 66048),                      # 256 rows of 258 B, just above the floor
    ((2, 5000), torch.float32, 4 * 1024 * 1024),            # above the cap (256 rows = 5 MB)
    ((1 << 21,), torch.uint8, 4 * 1024 * 1024),
])
def test_guard_size_rule(shape, dtype, want):
    assert G.guard_bytes(shape, dtype.itemsize) == want and want % 256 == 0
    if shape and shape[-1] * dtype.itemsize * (shape[0] if len(shape) > 1 else 1) < (1 << 20):
        with G.guarded("cpu") as g:
            assert buffer_of(g, torch.empty(shape, dtype=dtype)).guard == want
