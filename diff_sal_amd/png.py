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

import os
from typing import Sequence

import numpy as np
import torch

from . import ops

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
    files = list(files)
    if not files:
        raise ValueError("png.decode: an empty list of files")
    parsed = []
    for i, f in enumerate(files):
        try:
            parsed.append(_parse(_bytes_of(f, i)))
        except _Refused as e:
            raise ValueError(f"png.decode: file {i}: {e}") from None
        a, b = parsed[0], parsed[-1]
        if any(a[k] != b[k] for k in ("H", "W", "color_type", "bit_depth")):
            raise ValueError(f"png.decode: file {i}: {b['W']} x {b['H']}, colour type {b['color_type']}, {b['bit_depth']} bits where file 0 has "
                             f"{a['W']} x {a['H']}, {a['color_type']}, {a['bit_depth']}: the files of a call share size, colour type and depth")
    N, g = len(files), parsed[0]
    if N > 65535:
        raise ValueError(f"png.decode: {N} files in one call (at most 65535)")
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
    if mode not in ("RGB", "L"):
        raise ValueError(f"png.decode: mode must be 'RGB' or 'L', got {mode!r}")
    dev = torch.device("cuda" if device is None else device)
    files = files if isinstance(files, Tensor) else list(files)
    if dev.type != "cuda" or isinstance(files, Tensor) or any(isinstance(f, Tensor) for f in files):
        raise RuntimeError(f"diff_sal_amd png runs on the GPU only (no CPU fallback); decode takes the files' bytes and a GPU device, got "
                           f"{'a tensor' if dev.type == 'cuda' else dev}")
    p = pack(files)
    buf = torch.from_numpy(p["host"]).to(dev)
    N, desc_at = p["N"], p["desc_at"]
    frames, status = ops.png_decode(buf[:desc_at], buf[desc_at:].view(N, FILE_DTYPE.itemsize), N, p["H"], p["W"], p["color_type"], p["bit_depth"],
                                    mode == "L")
    if not strict:
        return frames, status
    bad = status.cpu().numpy()
    if bad.any():
        names = "; ".join(f"file {i}: " + ", ".join(t for b, t in STATUS_BITS.items() if bad[i] & b) for i in np.flatnonzero(bad)[:8])
        raise ValueError(f"png.decode: {int((bad != 0).sum())} of {N} files are damaged inside their stream ({names})")
    return frames


def decode_files(paths: Sequence, mode: str = "RGB", device=None, strict: bool = True):
    """``decode`` of the files at ``paths``."""
    data = []
    for p in paths:
        with open(p, "rb") as f:
            data.append(f.read())
    return decode(data, mode=mode, device=device, strict=strict)


# ---- export: 8-bit maps -> complete .png files (csrc/png_encode.hip, include/diffsal.h "PNG export") ----
def _maps(u8: Tensor, what: str = "u8") -> Tensor:
    """[B, 1, H, W] or [B, H, W] uint8 GPU tensor -> contiguous [B, H, W]"""
    if not isinstance(u8, Tensor) or not u8.is_cuda:
        raise RuntimeError(f"diff_sal_amd png runs on the GPU only (no CPU fallback); {what} is on "
                           f"{getattr(u8, 'device', type(u8).__name__)}")
    if u8.dtype != torch.uint8:
        raise ValueError(f"png: {what} must be uint8 (postprocess.to_uint8 gives it), got {u8.dtype}")
    if u8.dim() == 4 and u8.shape[1] == 1:
        u8 = u8[:, 0]
    if u8.dim() != 3 or u8.numel() == 0:
        raise ValueError(f"png: {what} must be a non-empty [B, 1, H, W] or [B, H, W], got {tuple(u8.shape)}")
    if u8.shape[0] > 65535 or u8.shape[1] > 65535 or u8.shape[2] > MAX_WIDTH:
        raise ValueError(f"png: {tuple(u8.shape)}: at most 65535 maps of at most 65535 rows and {MAX_WIDTH} columns (what decode takes)")
    return u8.contiguous()


def capacity(h: int, w: int) -> int:
    """The bytes no file of an ``h x w`` map exceeds: the width of ``encode``'s rows, a multiple of 16."""
    return ops.png_capacity(h, w)


def encode(u8: Tensor):
    """The ``.png`` file of every map of ``u8`` (uint8 ``[B, H, W]`` or ``[B, 1, H, W]``): ``(data uint8 [B, cap], lengths int32
    [B])`` on the device, map ``b``'s file being ``data[b, :lengths[b]]`` (zeros behind it).  8-bit greyscale, one IDAT; a decoder
    reads back exactly ``u8``.  No host copy, no synchronisation: capturable."""
    return ops.png_encode(_maps(u8))


def save_predictions(pred: Tensor, video_ids: Sequence, frame_ids: Sequence, root: str):
    """The reference's ``save_img`` for the visual sets: ``<root>/<video id>/<frame id>.png`` holding
    ``encode(postprocess.to_uint8(pred))``'s bytes.  One host copy of ``lengths``, then one of the used part of ``data``: nothing
    else leaves the device.  The pixels a decoder reads from these files are those of ``postprocess.save_predictions``'s files;
    the bytes are not.  Returns the paths written."""
    from . import postprocess

    u8 = postprocess.to_uint8(pred)
    frame_ids = [int(f) for f in (frame_ids.reshape(-1).tolist() if isinstance(frame_ids, Tensor) else frame_ids)]
    video_ids = list(video_ids)
    if not (u8.shape[0] == len(video_ids) == len(frame_ids)):
        raise ValueError(f"postprocess: {u8.shape[0]} predictions, {len(video_ids)} video ids, {len(frame_ids)} frame ids")
    data, lengths = encode(u8)
    n = lengths.cpu().numpy()
    host = data[:, :int(n.max())].cpu().numpy()      # the rows cut at the longest file: a few per cent of their capacity
    paths = []
    for row, length, vid, fid in zip(host, n, video_ids, frame_ids):
        d = os.path.join(root, str(vid))
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"{fid}.png")
        with open(path, "wb") as f:
            f.write(row[:int(length)].tobytes())
        paths.append(path)
    return paths
