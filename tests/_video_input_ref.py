"""NumPy restatement of Pillow's 8-bit ``Image.resize`` (ImagingResample) and the seeded inputs of the video front end's tests.
Test infrastructure only: written from the algorithm's description, independently of diff_sal_amd/video_input.py, and held to
the recorded Pillow outputs of tests/golden/video_input.npz (tools/gen_video_input_golden.py) and, where Pillow is installed, to
Pillow itself (tests/test_video_input_host.py).

The algorithm.  Per axis, for ``n_in -> n_out`` samples and a filter of support ``s0`` (1 bilinear; 2 bicubic, Keys a = -0.5):
``scale = n_in / n_out``, ``fs = max(scale, 1)``, ``s = s0 fs``; output ``o`` is centred on ``c = (o + 0.5) scale``, reads source
indices ``xmin = max(trunc(c - s + 0.5), 0)`` up to (not including) ``min(trunc(c + s + 0.5), n_in)`` with the weights
``filter((i - c + 0.5) / fs)`` normalised to sum 1, all float64; each weight times 2^22 is rounded half away from zero to an
integer.  A pass is ``clip((2^21 + sum pixel * weight) >> 22, 0, 255)`` in int32; the horizontal pass comes first and its result
is a uint8 image; a pass whose axis keeps its size is skipped."""
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "video_input.npz")
BITS = 22


def _tri(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _keys(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


FILTERS = {"bilinear": (_tri, 1.0), "bicubic": (_keys, 2.0)}


def coefficients(n_in, n_out, filt):
    """(bounds int64 [n_out, 2], weights float64 [n_out, ksize] (normalised, zero past the count), integer weights int64)"""
    fn, s0 = FILTERS[filt]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    s = s0 * fs
    ksize = int(np.ceil(s)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int64)
    w = np.zeros((n_out, ksize), dtype=np.float64)
    for o in range(n_out):
        c = (o + 0.5) * scale
        lo = max(int(c - s + 0.5), 0)
        hi = min(int(c + s + 0.5), n_in)
        row = fn((np.arange(lo, hi) - c + 0.5) * (1.0 / fs))
        tot = 0.0
        for v in row:      # a running sum in index order, as a C loop adds them
            tot += float(v)
        if tot != 0.0:
            row = row / tot
        bounds[o] = (lo, hi - lo)
        w[o, :hi - lo] = row
    scaled = w * float(1 << BITS)
    ik = np.where(scaled < 0, np.trunc(scaled - 0.5), np.trunc(scaled + 0.5)).astype(np.int64)
    return bounds, w, ik


def _pass(img, axis, bounds, ik):
    """one resample pass of uint8 ``img`` along ``axis``"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for o, (lo, cnt) in enumerate(bounds):
        acc = (1 << (BITS - 1)) + np.tensordot(ik[o, :cnt], src[lo:lo + cnt], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31, "the int32 accumulator would wrap"
        out[o] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size, filt):
    """``Image.resize((w, h), filt)`` of uint8 ``img`` [..., H, W, C] (or [H, W] with ``img.ndim == 2``), ``size = (h, w)``."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return resize(img[..., None], size, filt)[..., 0]
    h, w = size
    H, W = img.shape[-3], img.shape[-2]
    if W != w:
        b, _, ik = coefficients(W, w, filt)
        img = _pass(img, img.ndim - 2, b, ik)
    if H != h:
        b, _, ik = coefficients(H, h, filt)
        img = _pass(img, img.ndim - 3, b, ik)
    return img.copy()


def chain(img, size, pre_size=None, pre_filter="bicubic", filt="bilinear"):
    if pre_size is not None:
        img = resize(img, pre_size, pre_filter)
    return resize(img, size, filt)


# ---- seeded inputs (rebuilt at test time, never stored) ----------------------------------------------------------------

def noise(shape, seed):
    """uniform random bytes"""
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=shape, dtype=np.uint8)


def blocks(shape, seed, cell=5):
    """hard 0 / 255 blocks of ``cell`` pixels: the bicubic lobes leave 0 .. 255 at every edge, so the clip is exercised"""
    n, h, w, c = shape
    g = np.random.Generator(np.random.PCG64(seed)).integers(0, 2, size=(n, -(-h // cell), -(-w // cell), c), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(g, cell, axis=1), cell, axis=2)[:, :h, :w] * np.uint8(255))


# name: (generator, seed, input shape [N, H, W, C], output (h, w), filter)
CASES = {
    "down_bilinear": (noise, 11, (1, 97, 131, 3), (11, 20), "bilinear"),
    "down_bicubic": (noise, 11, (1, 97, 131, 3), (11, 20), "bicubic"),
    "down_blocks_bicubic": (blocks, 12, (1, 97, 131, 3), (11, 20), "bicubic"),
    "up_bilinear": (noise, 13, (1, 11, 20, 3), (37, 53), "bilinear"),
    "up_bicubic": (noise, 13, (1, 11, 20, 3), (37, 53), "bicubic"),
    "up_blocks_bicubic": (blocks, 14, (1, 11, 20, 3), (37, 53), "bicubic"),
    "x_only": (noise, 15, (1, 40, 64, 3), (40, 24), "bilinear"),
    "y_only": (noise, 15, (1, 40, 64, 3), (16, 64), "bicubic"),
    "gray": (noise, 16, (1, 97, 131, 1), (24, 40), "bilinear"),
    "three_frames": (noise, 17, (3, 37, 53, 3), (11, 20), "bicubic"),
    "bands": (blocks, 18, (1, 200, 64, 3), (77, 32), "bicubic"),
}
# the protocol chain: 360 x 640 -> 240 x 320 bicubic (pil_loader) -> 224 x 384 bilinear (Scale), two frames
PROTOCOL = ("protocol", 19, (2, 360, 640, 3), (240, 320), (224, 384))
PROTOCOL_STRIDE = (7, 11)      # the fixture keeps out[:, ::7, ::11] and the row / column sums of the whole result


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def case_input(name):
    gen, seed, shape, _, _ = CASES[name]
    return gen(shape, seed)


def protocol_input():
    """frame 0 random bytes, frame 1 blocks"""
    _, seed, shape, _, _ = PROTOCOL
    return np.concatenate([noise((1,) + shape[1:], seed), blocks((1,) + shape[1:], seed + 1, cell=9)], axis=0)


def protocol_digest(out):
    """what the fixture keeps of the protocol-size result [2, 224, 384, 3]"""
    sy, sx = PROTOCOL_STRIDE
    o = out.astype(np.int64)
    return {"sample": np.ascontiguousarray(out[:, ::sy, ::sx]), "row_sums": o.sum(axis=2), "col_sums": o.sum(axis=1)}


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
