"""The frame and map files of the visual sets, decoded on the device (csrc/png_decode.hip, arithmetic in include/diffsal.h "PNG
decode").  For DHF1K, UCF-Sports and Hollywood-2 the reference reads every frame ``'%d.png'`` with
``Image.open(f).convert('RGB')`` (R/datasets/dhf1k_data.py:78, R/datasets/ucf_dataset.py:68, R/datasets/holly2wood_dataset.py:72) and
every annotation map ``'%04d.png'`` with ``.convert('L')`` (R/datasets/meta_data.py:49-57), on the host, inflating and unfiltering
each file on one thread; R/compute_metrics.py:9-14 reads the ``maps`` and ``fixation`` files back the same way.

* ``decode`` / ``decode_files`` give those uint8 frames from the files' bytes, bit-equal to Pillow 12.2, in the layouts
  ``video_input.transform_frames``, ``target_maps`` and ``postprocess.from_uint8`` take.  The host walks the chunk headers
  (``parse_file``, ``pack``); inflate, the filters, sample unpacking, the palette and the conversion to ``RGB`` / ``L`` run on the
  device, and no pixel exists on the host.

The other direction, the reference's export for these sets (csrc/png_encode.hip, arithmetic in include/diffsal.h "PNG export"):
R/diffusion_trainer.py:898-935 (``save_img``) writes every prediction as ``<video>/<frame>.png``.

* ``encode`` gives the complete 8-bit greyscale files of a batch in device memory, ``save_predictions`` writes them; only finished
  file bytes travel to the host.  The files are not Pillow's bytes: they are valid PNGs that every decoder reads back to exactly the
  input pixels, and their bytes are a function of the pixels alone (tests/_png_encode_ref.py restates them).
  ``postprocess.save_predictions`` is the host path through Pillow, unchanged and still the default there.

GPU only: CPU tensors raise.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _image_files, ops

Tensor = torch.Tensor

# the per-file record the kernels read: csrc/png_decode_core.h's FileDesc
FILE_DTYPE = np.dtype([("off", "<u4"), ("len", "<u4"), ("pad", "<u4", (2,)), ("pal", "u1", (768,))])
assert FILE_DTYPE.itemsize == 784
STATUS_BITS = {1: "an invalid block type", 2: "a stored block whose length check fails", 4: "an invalid or over-subscribed set of code lengths",
               8: "an invalid literal/length or distance symbol", 16: "a distance that reaches before the start of the output",
               32: "the stream's bits ran out", 64: "the stream ended with fewer bytes than the image needs",
               128: "the stream carries more bytes than the image needs", 256: "a filter type above 4", 512: "an Adler-32 mismatch"}
MAX_WIDTH = 8192
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


class _Refused(ValueError):
    pass


def _bytes_of(f, i: int) -> np.ndarray:
    if isinstance(f, np.ndarray):
        if f.dtype != np.uint8 or f.ndim != 1:
            raise ValueError(f"png.decode: file {i}: a numpy array must be one-dimensional uint8, got {f.dtype} {f.shape}")
        return np.ascontiguousarray(f)
    if not isinstance(f, (bytes, bytearray, memoryview)):
        raise ValueError(f"png.decode: file {i}: expected bytes, bytearray, memoryview or a uint8 numpy array, got {type(f).__name__}")
    return np.frombuffer(f, dtype=np.uint8)


def _chunks(a: np.ndarray):
    """the chunks of file bytes ``a`` behind the signature: yields (type, payload start, payload stop); stops behind IEND or at the
    file's end (Pillow does not need IEND either)"""
    at, n = 8, a.size
    while at < n:
        if at + 8 > n:
            raise _Refused(f"a chunk header at byte {at} runs past the file's end")
        length = int.from_bytes(a[at:at + 4].tobytes(), "big")
        kind = a[at + 4:at + 8].tobytes()
        if at + 12 + length > n:      # the payload and the CRC behind it
            raise _Refused(f"the length {length} of chunk {kind!r} at byte {at} runs past the file's end")
        yield kind, at + 8, at + 8 + length
        if kind == b"IEND":
            return
        at += 12 + length


def parse_file(data) -> dict:
    """Walks the chunks of one complete PNG file (bytes-like or a uint8 array) and returns what the device decode needs: ``H``,
    ``W``, ``color_type``, ``bit_depth``, ``stream`` (the IDAT payloads joined end to end: one zlib stream, uint8) and ``palette``
    (uint8 ``[768]``, PLTE zero-padded).  Host work on the chunk headers only; chunk CRCs are not verified (Pillow does not verify
    IDAT's either).  Raises ValueError with the reason for anything the decode does not take (see ``decode``)."""
    try:
        return _parse(_bytes_of(data, 0))
    except _Refused as e:
        raise ValueError(f"png.parse_file: {e}") from None


def _parse(a: np.ndarray) -> dict:
    if a.size < 8 or a[:8].tobytes() != _SIGNATURE:
        raise _Refused("no PNG signature: not a PNG file")
    head, palette, parts = None, None, []
    for k, (kind, lo, hi) in enumerate(_chunks(a)):
        if kind == b"IHDR":
            if head is not None:
                raise _Refused("a second IHDR chunk")
            if hi - lo < 13:
                raise _Refused(f"an IHDR chunk of {hi - lo} bytes (13)")
            p = a[lo:hi].tobytes()
            head = (int.from_bytes(p[0:4], "big"), int.from_bytes(p[4:8], "big")) + tuple(p[8:13])
        elif head is None:
            raise _Refused(f"chunk {kind!r} in front of IHDR: IHDR is missing")
        elif kind == b"PLTE":
            palette = np.zeros(768, dtype=np.uint8)
            n = min(hi - lo, 768) // 3 * 3
            palette[:n] = a[lo:lo + n]
        elif kind == b"IDAT":
            parts.append(a[lo:hi])
    if head is None:
        raise _Refused("IHDR is missing")
    W, H, depth, ctype, comp, filt, lace = head
    if ctype not in _DEPTHS or depth not in _DEPTHS[ctype]:
        raise _Refused(f"bit depth {depth} with colour type {ctype}: a pair the standard does not allow")
    if depth == 16:
        raise _Refused("16-bit samples: decode this file with Pillow")
    if lace != 0:
        raise _Refused(f"interlace method {lace}: decode an interlaced file with Pillow")
    if comp != 0 or filt != 0:
        raise _Refused(f"compression method {comp}, filter method {filt}: both are 0 in every PNG")
    if W == 0 or H == 0:
        raise _Refused(f"a size of {W} x {H}")
    if W > MAX_WIDTH or H > 65535:
        raise _Refused(f"{W} x {H}: at most {MAX_WIDTH} x 65535")
    if ctype == 3 and palette is None:
        raise _Refused("a palette file without PLTE")
    if not parts:
        raise _Refused("no IDAT chunk")
    stream = np.concatenate(parts) if len(parts) > 1 else parts[0]
    if stream.size < 2:
        raise _Refused("a zlib stream without its header")
    cmf, flg = int(stream[0]), int(stream[1])
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31:
        raise _Refused(f"zlib header {cmf:#04x} {flg:#04x}: not deflate with a window of at most 32 K")
    if flg & 0x20:
        raise _Refused("a zlib stream with a preset dictionary (FDICT)")
    return dict(H=H, W=W, color_type=ctype, bit_depth=depth, stream=stream, palette=np.zeros(768, dtype=np.uint8) if palette is None else palette)


def pack(files: Sequence) -> dict:
    """The host side of ``decode``: parses every file and lays out the one buffer that travels to the device, uint8 ``host`` = the
    files' zlib streams, each starting at a multiple of 16 and zero-padded, up to ``desc_at`` | ``N`` FILE_DTYPE records.  Also
    returns ``N`` and the shared geometry ``H``, ``W``, ``color_type``, ``bit_depth``.  Raises ValueError naming the file's position
    and the reason."""
    files, parsed = _image_files.parse_files(
        files, "png", lambda f, i: _parse(_bytes_of(f, i)), _Refused, ("H", "W", "color_type", "bit_depth"),
        lambda a, b: f"{b['W']} x {b['H']}, colour type {b['color_type']}, {b['bit_depth']} bits where file 0 has "
                     f"{a['W']} x {a['H']}, {a['color_type']}, {a['bit_depth']}: the files of a call share size, colour type and depth")
    N, g = len(files), parsed[0]
    sizes = np.array([p["stream"].size for p in parsed], dtype=np.int64)
    padded = (sizes + 15) & ~15
    starts = np.concatenate([[0], np.cumsum(padded)[:-1]])
    desc_at = int(padded.sum())
    if desc_at >= 2 ** 31 - 16:
        raise ValueError(f"png.decode: {desc_at} bytes of streams in one call (below 2^31: split the call)")
    host = np.zeros(desc_at + N * FILE_DTYPE.itemsize, dtype=np.uint8)      # one host buffer, one copy
    desc = host[desc_at:].view(FILE_DTYPE)
    for i, p in enumerate(parsed):
        host[starts[i]:starts[i] + sizes[i]] = p["stream"]
        desc["off"][i], desc["len"][i], desc["pal"][i] = starts[i], sizes[i], p["palette"]
    return dict(host=host, N=N, desc_at=desc_at, H=g["H"], W=g["W"], color_type=g["color_type"], bit_depth=g["bit_depth"])


def decode(files: Sequence, mode: str = "RGB", device=None, strict: bool = True):
    """What ``np.asarray(Image.open(f).convert(mode))`` returns for every PNG file of ``files`` (``bytes`` / ``bytearray`` /
    ``memoryview`` / uint8 numpy array, one complete file each), decoded on the device: uint8 ``[N, H, W, 3]`` for ``mode="RGB"``,
    ``[N, H, W]`` for ``"L"`` -- the layouts ``video_input.transform_frames`` and ``target_maps`` take -- bit-equal to Pillow.

    The host walks the chunk headers only: the IDAT payloads of every file, joined, and one descriptor per file travel in one
    copy, and no pixel exists on the host.  All files of a call share width, height, colour type and bit depth (a video's frames
    do); the palette is per file.  Taken: non-interlaced files of bit depth 8 with colour type 0, 2, 3, 4, 6 (Pillow's ``L``,
    ``RGB``, ``P``, ``LA``, ``RGBA``) and of depth 1, 2, 4 with colour type 0 or 3, up to 8192 pixels wide.  Alpha is dropped,
    ``tRNS`` is ignored, ``L`` of colour is ``(19595 R + 38470 G + 7471 B + 0x8000) >> 16``, as Pillow does.  Everything else
    (16-bit, interlaced, a damaged chunk structure or zlib header) raises ValueError naming the file's position and the reason before
    anything is launched; decode such files with Pillow.  Chunk CRCs are not verified; the stream's Adler-32 is, on the device.

    Damage inside the compressed data shows only on the device, as a non-zero int32 status per file (``STATUS_BITS``).
    ``strict=True`` reads the status back (one synchronisation) and raises ValueError naming the files; ``strict=False`` returns
    ``(frames, status)`` without synchronising.  A stream that ends with fewer bytes than the image needs is an error here (status
    64); this is stricter than Pillow, which returns such a file silently with the missing rows left blank.  A stream that carries
    more (128) still delivers its pixels.  With any other bit the file's pixels are unspecified; the other files of the batch are
    unaffected.  One file is one wave's work: the parallelism is across files."""
    def run(packed, records, tail, p):
        return ops.png_decode(packed, records, p["N"], p["H"], p["W"], p["color_type"], p["bit_depth"], mode == "L")

    return _image_files.decode(files, mode, device, strict, codec="png", pack=pack, file_dtype=FILE_DTYPE, status_bits=STATUS_BITS,
                               noun="stream", run=run)


decode_files = _image_files.file_decoder(decode)


def decode_groups(files: Sequence, mode: str = "RGB", device=None):
    """``decode`` for files that do not share one geometry (a shuffled training batch holds frames of several videos): the chunk
    headers are parsed, the files grouped by (height, width, colour type, bit depth) and every group decoded in one ``decode``
    call.  Returns ``(groups, where)``: the uint8 tensor of every group, in order of first appearance, and per file its
    ``(group, position)``.  One read-back of all the files' status, as ``decode(strict=True)``."""
    def geometry(f, i):
        p = _parse(_bytes_of(f, i))
        return p["H"], p["W"], p["color_type"], p["bit_depth"]

    return _image_files.decode_groups(files, mode, device, codec="png", geometry=geometry, refused=_Refused, decode=decode,
                                      status_bits=STATUS_BITS, noun="stream")


# ---- export: 8-bit maps -> complete .png files (csrc/png_encode.hip, include/diffsal.h "PNG export") ----
def _limit(shape):
    if shape[0] > 65535 or shape[1] > 65535 or shape[2] > MAX_WIDTH:
        return f"{shape}: at most 65535 maps of at most 65535 rows and {MAX_WIDTH} columns (what decode takes)"


def capacity(h: int, w: int) -> int:
    """The bytes no file of an ``h x w`` map exceeds: the width of ``encode``'s rows, a multiple of 16."""
    return ops.png_capacity(h, w)


def encode(u8: Tensor):
    """The ``.png`` file of every map of ``u8`` (uint8 ``[B, H, W]`` or ``[B, 1, H, W]``): ``(data uint8 [B, cap], lengths int32
    [B])`` on the device, map ``b``'s file being ``data[b, :lengths[b]]`` (zeros behind it).  8-bit greyscale, one IDAT; a decoder
    reads back exactly ``u8``.  No host copy, no synchronisation: capturable."""
    return ops.png_encode(_image_files._maps(u8, "png", _limit))


def save_predictions(pred: Tensor, video_ids: Sequence, frame_ids: Sequence, root: str):
    """The reference's ``save_img`` for the visual sets: ``<root>/<video id>/<frame id>.png`` holding
    ``encode(postprocess.to_uint8(pred))``'s bytes.  One host copy of ``lengths``, then one of the used part of ``data``: nothing
    else leaves the device.  The pixels a decoder reads from these files are those of ``postprocess.save_predictions``'s files;
    the bytes are not.  Returns the paths written."""
    from . import postprocess

    u8 = postprocess.to_uint8(pred)
    video_ids, frame_ids = _image_files.checked_ids(u8.shape[0], video_ids, frame_ids, "png")
    rows, lengths = _image_files.host_rows(*encode(u8))
    return _image_files.write_files(rows, lengths, _image_files.prediction_paths(root, video_ids, frame_ids, "{}.png"))
