"""The reference's export for the audio-visual sets, on the device: 8-bit maps to the ``.jpg`` files it writes and to the pixels it
reads back from them (csrc/jpeg_export.hip, arithmetic in include/diffsal.h "JPEG export").  For AVAD, Coutrot, DIEM, ETMD and
SumMe R/diffusion_trainer.py:898-935 (``save_img(..., av_data=True)``) does not write a PNG but ``pred_sal_%06d.jpg`` with
``cv2.imwrite``, and the benchmark scores what a decoder makes of that file:

* ``encode`` gives the complete files of a batch in device memory, ``save_predictions`` writes them; only finished file bytes
  travel to the host;
* ``roundtrip`` gives the decoded pixels in one launch, without the entropy coder: what scoring needs
  (``postprocess.protocol_metrics(..., quantize="jpeg")``);
* ``quant_table`` is libjpeg's table for a quality, on the host.

The file is 8-bit greyscale, baseline, libjpeg's slow-integer DCT, the standard tables unoptimised, quality 95 by default: every
step is integer arithmetic, so the result is a matter of bits, not of tolerance.  The tests hold the files and the decoded pixels
to Pillow 12.2 (libjpeg-turbo) byte for byte.  One thing could not be run where this module was written and rests on reading the
sources:

* OpenCV itself.  The claim is that ``cv2.imwrite(path, u8)`` of a 2-D uint8 array sets quality 95, no optimised tables, no
  progressive mode and libjpeg's defaults otherwise into the same libjpeg-turbo, and so writes the same scan and tables as Pillow's
  ``save(f, "JPEG", quality=95)``, and that ``cv2.imread`` decodes with libjpeg's default slow-integer inverse DCT.

The other direction, for the data sets' own files (csrc/jpeg_decode.hip, arithmetic in include/diffsal.h "JPEG decode"):
R/datasets/saliency_db.py:29-44 decodes every ``img_%05d.jpg`` with ``Image.open(f).convert('RGB')`` and every ``eyeMap_%05d.jpg``
with ``.convert('L')``, on the host, once per clip that holds the frame.

* ``decode`` / ``decode_files`` give those uint8 frames from the files' bytes, bit-equal to Pillow (libjpeg-turbo's defaults: the
  slow-integer inverse DCT shared with the export's read-back, fancy chroma up-sampling, its YCbCr -> RGB; Pillow's ``L``), in the
  layouts ``video_input.transform_frames`` and ``target_maps`` take.  The host walks the marker segments (``parse_file``, ``pack``);
  the entropy decode, the transform, the up-sampling and the colour conversion run on the device, and no pixel exists on the host.

GPU only: CPU tensors raise.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _image_files, ops

Tensor = torch.Tensor

# ITU-T T.81 Annex K.1, luminance, natural order
_BASE_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
           103, 99)


def _quality(quality) -> int:
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"jpeg: quality must be an integer in 1..100, got {quality!r}")
    return q


def quant_table(quality: int = 95) -> np.ndarray:
    """libjpeg's quantisation table for ``quality`` (``jpeg_quality_scaling``, baseline): int64 ``[64]`` in natural order."""
    q = _quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(_BASE_Q, dtype=np.int64) * s + 50) // 100, 1, 255)


def _limit(shape):
    if max(shape[1:]) > 65535:
        return f"{shape[1:]}: a JPEG axis holds at most 65535 pixels"


def capacity(h: int, w: int) -> int:
    """The bytes no file of an ``h x w`` image exceeds: the width of ``encode``'s rows."""
    return ops.jpeg_capacity(h, w)


def encode(u8: Tensor, quality: int = 95, return_decoded: bool = False):
    """The ``.jpg`` file of every image of ``u8`` (uint8 ``[B, H, W]``): ``(data uint8 [B, cap], lengths int32 [B])`` on the device,
    image ``b``'s file being ``data[b, :lengths[b]]`` (the bytes behind it are undefined).  ``return_decoded=True`` adds what a
    decoder reads back from those files, uint8 ``[B, H, W]``.  No host copy, no synchronisation: capturable."""
    q = _quality(quality)
    data, lengths, recon = ops.jpeg_encode(_image_files._maps(u8, "jpeg", _limit), q, want_recon=bool(return_decoded))
    return (data, lengths, recon) if return_decoded else (data, lengths)


def roundtrip(u8: Tensor, quality: int = 95) -> Tensor:
    """What a decoder reads back from ``encode(u8, quality)``'s files, uint8 ``[B, H, W]``, without making them: one launch."""
    return ops.jpeg_roundtrip(_image_files._maps(u8, "jpeg", _limit), _quality(quality))


# ---- decode: the data sets' frame files -> the uint8 frames Pillow returns (csrc/jpeg_decode.hip, include/diffsal.h "JPEG decode") ----
# the per-file record the kernels read: csrc/jpeg_decode_core.h's FileDesc
FILE_DTYPE = np.dtype([("scan_off", "<u4"), ("scan_len", "<u4"), ("restart", "<u4"), ("seg0", "<u4"), ("nseg", "<u4"), ("pad", "<u4", (3,)),
                       ("comp", "u1", (4, 4)), ("qt", "u1", (4, 64)), ("hbits", "u1", (4, 16)), ("hvals", "u1", (4, 256))])
assert FILE_DTYPE.itemsize == 1392
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                    42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                    63])
_NOT_BASELINE = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
                 0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic", 0xCA: "arithmetic progressive",
                 0xCB: "arithmetic lossless", 0xCD: "arithmetic differential", 0xCE: "arithmetic differential progressive",
                 0xCF: "arithmetic differential lossless"}
STATUS_BITS = {1: "a bit pattern no Huffman code matches", 2: "a run past coefficient 63", 4: "a segment ended before its MCUs"}


class _Refused(ValueError):
    pass


def _marker_segments(a: np.ndarray, at: int):
    """Marker segments of file bytes ``a`` from offset ``at``: yields (marker, payload start, payload stop); stops behind SOS or EOI."""
    n = a.size
    while True:
        if at + 2 > n:
            raise _Refused("the file ends inside a marker segment")
        if a[at] != 0xFF:
            raise _Refused(f"byte {at}: {int(a[at]):#04x} where a marker should start")
        while at + 1 < n and a[at + 1] == 0xFF:      # fill bytes
            at += 1
        if at + 2 > n:
            raise _Refused("the file ends inside a marker segment")
        m = int(a[at + 1])
        if m == 0xD9:
            yield m, at + 2, at + 2
            return
        if m == 0x01 or 0xD0 <= m <= 0xD8:      # no payload
            at += 2
            continue
        if at + 4 > n:
            raise _Refused("the file ends inside a marker segment")
        length = (int(a[at + 2]) << 8) | int(a[at + 3])
        if length < 2 or at + 2 + length > n:
            raise _Refused("the file ends inside a marker segment")
        yield m, at + 4, at + 2 + length
        if m == 0xDA:
            return
        at += 2 + length


def parse_file(data) -> dict:
    """Walks the marker segments of one complete JPEG file (bytes-like) and returns what the device decode needs: ``H``, ``W``,
    ``ncomp``, the luma sampling ``hs``, ``vs``, ``desc`` (one FILE_DTYPE record; ``seg0`` is left 0, offsets count from the file's
    first byte) and ``segments`` int32 ``[n, 3]``: (begin, end, first MCU) of every restart interval, the RSTn markers and fill bytes
    left out.  Host work on the headers only; the scan is searched for markers with NumPy.  Raises ValueError with the reason for
    anything the decode does not take (see ``decode``)."""
    return _parse(data, None)[0]


def _parse(data, same_header):
    """``parse_file`` and the header it read, ``(bytes in front of the scan, what they hold)``.  A video's frames usually carry the
    same header byte for byte; when ``data`` starts with ``same_header``'s bytes, what they hold is taken from there."""
    a = np.frombuffer(data, dtype=np.uint8)
    if same_header is not None and a.size > len(same_header[0]) and a[:len(same_header[0])].tobytes() == same_header[0]:
        head = same_header
    else:
        head = _parse_header(a)
        head = (a[:head[2]].tobytes(), head)
    d, frame, scan_at = head[1]
    return _parse_scan(a, d.copy(), frame, scan_at), head


def _parse_header(a: np.ndarray):
    """the marker segments up to and including SOS: (FILE_DTYPE record, (H, W, components, hs, vs, [(id, h, v, tq)]), scan start)"""
    if a.size < 4 or a[0] != 0xFF or a[1] != 0xD8:
        raise _Refused("no SOI marker: not a JPEG file")
    d = np.zeros((), dtype=FILE_DTYPE)
    have_q, have_h = set(), set()
    frame, jfif, adobe, scan_at = None, False, None, None
    for m, lo, hi in _marker_segments(a, 2):
        p = a[lo:hi]
        if m == 0xE0 and p.size >= 5 and p[:5].tobytes() == b"JFIF\0":
            jfif = True
        elif m == 0xEE and p.size >= 12 and p[:5].tobytes() == b"Adobe":
            adobe = int(p[11])
        elif m == 0xDB:
            k = 0
            while k < p.size:
                if p[k] >> 4:
                    raise _Refused("a 16-bit quantisation table (DQT)")
                if (p[k] & 15) > 3 or k + 65 > p.size:
                    raise _Refused("a malformed DQT segment")
                d["qt"][p[k] & 15][_ZIGZAG] = p[k + 1:k + 65]
                have_q.add(int(p[k] & 15))
                k += 65
        elif m == 0xC4:
            k = 0
            while k < p.size:
                cls, tid = int(p[k]) >> 4, int(p[k]) & 15
                if cls > 1 or tid > 1 or k + 17 > p.size:
                    raise _Refused("a malformed DHT segment (baseline has DC / AC tables 0 and 1)")
                total = int(p[k + 1:k + 17].sum())
                if total > 256 or k + 17 + total > p.size:
                    raise _Refused("a malformed DHT segment")
                d["hbits"][2 * cls + tid] = p[k + 1:k + 17]
                d["hvals"][2 * cls + tid] = 0
                d["hvals"][2 * cls + tid][:total] = p[k + 17:k + 17 + total]
                have_h.add(2 * cls + tid)
                k += 17 + total
        elif m in _NOT_BASELINE:
            raise _Refused(f"a {_NOT_BASELINE[m]} frame (SOF{m - 0xC0}): baseline sequential (SOF0) only")
        elif m == 0xDC:
            raise _Refused("a DNL marker")
        elif m == 0xC0:
            if frame is not None or p.size < 6 or p.size != 6 + 3 * int(p[5]):
                raise _Refused("a malformed or repeated SOF0 segment")
            if p[0] != 8:
                raise _Refused(f"sample precision {int(p[0])}: 8 only")
            H, W, nc = (int(p[1]) << 8) | int(p[2]), (int(p[3]) << 8) | int(p[4]), int(p[5])
            if H == 0:
                raise _Refused("height 0 (to be set by a DNL marker)")
            if W == 0:
                raise _Refused("width 0")
            if nc not in (1, 3):
                raise _Refused(f"{nc} components: 1, or 3 read as YCbCr")
            comps = [(int(p[6 + 3 * c]), int(p[7 + 3 * c]) >> 4, int(p[7 + 3 * c]) & 15, int(p[8 + 3 * c])) for c in range(nc)]
            if any(tq > 3 for _, _, _, tq in comps):
                raise _Refused("a quantisation table selector above 3")
            hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)      # one component is never interleaved: its factors are idle
            if nc == 3 and ((hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comps[1:])):
                raise _Refused("sampling factors " + " ".join(f"{c[1]}x{c[2]}" for c in comps) + ": luma 1x1, 2x1 or 2x2 with chroma 1x1")
            frame = (H, W, nc, hs, vs, comps)
        elif m == 0xDD:
            if p.size != 2:
                raise _Refused("a malformed DRI segment")
            d["restart"] = (int(p[0]) << 8) | int(p[1])
        elif m == 0xDA:
            if frame is None:
                raise _Refused("SOS in front of SOF0")
            H, W, nc, hs, vs, comps = frame
            if p.size < 1 or int(p[0]) != nc or p.size != 4 + 2 * nc:
                raise _Refused("more than one scan: the first does not hold all components")
            for c in range(nc):
                if int(p[1 + 2 * c]) != comps[c][0]:
                    raise _Refused("the scan's components are not the frame's, in order")
                td, ta = int(p[2 + 2 * c]) >> 4, int(p[2 + 2 * c]) & 15
                if td > 1 or ta > 1:
                    raise _Refused("a Huffman table selector above 1")
                if comps[c][3] not in have_q or td not in have_h or 2 + ta not in have_h:
                    raise _Refused(f"component {c} selects a table the file does not define")
                d["comp"][c] = (comps[c][3], td, ta, 0)
            if (int(p[-3]), int(p[-2]), int(p[-1])) != (0, 63, 0):
                raise _Refused("a scan of part of the coefficients (not baseline)")
            scan_at = hi
        elif m == 0xD9:
            break
    if scan_at is None:
        raise _Refused("no SOS marker: the file holds no scan")
    H, W, nc, hs, vs, comps = frame
    if nc == 3:
        if adobe == 0:
            raise _Refused("an Adobe APP14 segment with transform 0: the components are RGB, not YCbCr")
        if adobe is None and not jfif and bytes(c[0] for c in comps) == b"RGB":
            raise _Refused("component ids R, G, B without JFIF: libjpeg reads them as RGB, not YCbCr")
    return d, frame, scan_at


def _parse_scan(a: np.ndarray, d, frame, scan_at: int) -> dict:
    """the scan's restart segments and what follows the scan; fills the record's scan_off, scan_len and nseg"""
    H, W, nc, hs, vs, comps = frame
    # the scan: up to the first marker that is no RSTn; FF 00 is data, FF FF is fill
    scan = a[scan_at:]
    ff_all = np.flatnonzero(scan == 0xFF)      # the one pass over the scan's bytes; everything below works on these few positions
    ff = ff_all[:-1] if ff_all.size and ff_all[-1] == scan.size - 1 else ff_all
    nxt = scan[ff + 1]
    marks = ff[(nxt != 0) & (nxt != 0xFF)]
    codes = scan[marks + 1]
    other = np.flatnonzero((codes < 0xD0) | (codes > 0xD7))
    if other.size:
        end, rst = int(marks[other[0]]), marks[:other[0]]
    else:
        end, rst = int(scan.size), marks      # no EOI: the file was cut inside its scan, the device will say so
    begin = np.concatenate([[0], rst + 2]).astype(np.int64)
    stop = np.concatenate([rst, [end]]).astype(np.int64)
    if ff_all.size:      # a segment ends in front of the fill bytes before its marker: back to the start of the run of FF that ends at stop - 1
        runs = np.concatenate([[0], np.flatnonzero(np.diff(ff_all) != 1) + 1])      # index in ff_all of every run's first FF
        at = np.searchsorted(ff_all, stop) - 1      # the last FF in front of stop
        fill = (at >= 0) & (ff_all[np.maximum(at, 0)] == stop - 1)
        first = ff_all[runs[np.searchsorted(runs, np.maximum(at, 0), side="right") - 1]]
        stop = np.maximum(begin, np.where(fill, first, stop))
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    ri = int(d["restart"])
    want = -(-mcus // ri) if ri else 1
    if begin.size != want:
        raise _Refused(f"{begin.size} restart segments in the scan where {mcus} MCUs at interval {ri} make {want}")
    if other.size:      # what follows the scan
        for m, lo, hi in _marker_segments(a, scan_at + end):
            if m == 0xDA:
                raise _Refused("more than one scan")
            if m == 0xDC:
                raise _Refused("a DNL marker")
            if m in _NOT_BASELINE or m == 0xC0:
                raise _Refused("a second frame")
    d["scan_off"], d["scan_len"], d["nseg"] = scan_at, end, begin.size
    seg = np.stack([begin + scan_at, stop + scan_at, np.arange(begin.size, dtype=np.int64) * ri], axis=1)
    return dict(H=H, W=W, ncomp=nc, hs=hs, vs=vs, desc=d, segments=seg.astype(np.int32))


def decode(files: Sequence, mode: str = "RGB", device=None, strict: bool = True):
    """What ``np.asarray(Image.open(f).convert(mode))`` returns for every JPEG file of ``files`` (``bytes`` / ``bytearray`` /
    ``memoryview``, one complete file each), decoded on the device: uint8 ``[N, H, W, 3]`` for ``mode="RGB"``, ``[N, H, W]`` for
    ``"L"`` -- the layouts ``video_input.transform_frames`` and ``target_maps`` take -- bit-equal to Pillow (libjpeg-turbo defaults).

    The host walks the marker segments only: the files, their descriptors and the table of restart segments travel in one copy, and
    no pixel exists on the host.  All files of a call share width, height, component count and sampling factors (a video's frames
    do); quantisation tables, Huffman tables and the restart interval are per file.  Taken: baseline sequential (SOF0), 8-bit, one
    component or three read as YCbCr, luma sampling 1x1, 2x1 or 2x2 with chroma 1x1, one interleaved scan, 8-bit DQT, DRI / RSTn, fill
    bytes, any APPn / COM.  Everything else raises ValueError naming the file's position and the reason before anything is launched.

    Damage inside the entropy-coded data shows only on the device, as a non-zero int32 status per file (``STATUS_BITS``).
    ``strict=True`` reads the status back (one synchronisation) and raises ValueError naming the files; ``strict=False`` returns
    ``(frames, status)`` without synchronising.  The pixels of a file with non-zero status are unspecified (libjpeg's error recovery
    is not reproduced); the other files of the batch are unaffected.  One file without restart markers is one lane's serial work:
    the parallelism is across files and restart intervals."""
    def run(packed, records, tail, p):
        return ops.jpeg_decode(packed, records, tail.view(torch.int32).view(p["nseg"], 4), p["max_file_seg"], p["N"], p["H"], p["W"],
                               p["ncomp"], p["hs"], p["vs"], mode == "L")

    return _image_files.decode(files, mode, device, strict, codec="jpeg", pack=pack, file_dtype=FILE_DTYPE, status_bits=STATUS_BITS,
                               noun="scan", run=run)


def pack(files: Sequence) -> dict:
    """The host side of ``decode``: parses every file and lays out the one buffer that travels to the device, uint8 ``host`` =
    the files back to back, zero-padded to ``desc_at`` (a multiple of 16) | ``N`` FILE_DTYPE records up to ``seg_at`` | ``nseg``
    int32 rows (file, begin, end, first MCU).  Also returns ``N``, ``nseg``, ``max_file_seg`` and the shared geometry ``H``, ``W``,
    ``ncomp``, ``hs``, ``vs``.  Raises ValueError naming the file's position and the reason."""
    head = [None]      # the header the file before carried

    def parse(f, i):
        if not isinstance(f, (bytes, bytearray, memoryview)):
            raise _Refused(f"expected bytes, bytearray or memoryview, got {type(f).__name__}")
        one, head[0] = _parse(f, head[0])
        return one

    files, parsed = _image_files.parse_files(
        files, "jpeg", parse, _Refused, ("H", "W", "ncomp", "hs", "vs"),
        lambda a, b: f"{b['W']} x {b['H']}, {b['ncomp']} components, luma {b['hs']}x{b['vs']} where file 0 has "
                     f"{a['W']} x {a['H']}, {a['ncomp']}, {a['hs']}x{a['vs']}: the files of a call share size and sampling")
    N, g = len(files), parsed[0]
    sizes = np.array([len(memoryview(f).cast("B")) for f in files], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    nbytes = (int(sizes.sum()) + 15) & ~15
    nseg = sum(p["segments"].shape[0] for p in parsed)
    if nbytes >= 2 ** 31:
        raise ValueError(f"jpeg.decode: {nbytes} bytes of files in one call (below 2^31: split the call)")
    # one host buffer, one copy: the files, the descriptors, the segment table
    desc_at, seg_at = nbytes, nbytes + N * FILE_DTYPE.itemsize
    host = np.zeros(seg_at + 16 * nseg, dtype=np.uint8)
    desc = host[desc_at:seg_at].view(FILE_DTYPE)
    seg = host[seg_at:].view(np.int32).reshape(nseg, 4)
    row = 0
    for i, (f, p) in enumerate(zip(files, parsed)):
        host[starts[i]:starts[i] + sizes[i]] = np.frombuffer(f, dtype=np.uint8)
        n = p["segments"].shape[0]
        desc[i] = p["desc"]
        desc["scan_off"][i] += starts[i]
        desc["seg0"][i] = row
        seg[row:row + n, 0] = i
        seg[row:row + n, 1:3] = p["segments"][:, :2] + starts[i]
        seg[row:row + n, 3] = p["segments"][:, 2]
        row += n
    return dict(host=host, N=N, nseg=nseg, desc_at=desc_at, seg_at=seg_at, max_file_seg=max(p["segments"].shape[0] for p in parsed),
                H=g["H"], W=g["W"], ncomp=g["ncomp"], hs=g["hs"], vs=g["vs"])


decode_files = _image_files.file_decoder(decode)


def decode_groups(files: Sequence, mode: str = "RGB", device=None):
    """``decode`` for files that do not share one geometry (a shuffled training batch holds frames of several videos): the headers
    are parsed, the files grouped by (height, width, components, luma sampling) and every group decoded in one ``decode`` call.
    Returns ``(groups, where)``: the uint8 tensor of every group, in order of first appearance, and per file its
    ``(group, position)``.  One read-back of all the files' status, as ``decode(strict=True)``."""
    def geometry(f, i):
        if not isinstance(f, (bytes, bytearray, memoryview)):
            raise _Refused(f"expected bytes, bytearray or memoryview, got {type(f).__name__}")
        return _parse_header(np.frombuffer(f, dtype=np.uint8))[1][:5]

    return _image_files.decode_groups(files, mode, device, codec="jpeg", geometry=geometry, refused=_Refused, decode=decode,
                                      status_bits=STATUS_BITS, noun="scan")


def save_predictions(pred: Tensor, video_ids: Sequence, frame_ids: Sequence, root: str, quality: int = 95):
    """The reference's ``save_img`` for the audio-visual sets: ``<root>/<video id>/pred_sal_{frame id:06d}.jpg`` holding
    ``encode(postprocess.to_uint8(pred))``'s bytes.  One host copy of ``lengths``, then one of the used part of ``data``: nothing else leaves the device.  The
    reference also renames the data set's folder inside the video id (``"AVAD/..."`` -> ``"avad/..."``); that is left to the caller,
    who passes the ids as the folders should be named.  Returns the paths written."""
    from . import postprocess

    q = _quality(quality)
    u8 = postprocess.to_uint8(pred)
    video_ids, frame_ids = _image_files.checked_ids(u8.shape[0], video_ids, frame_ids, "jpeg")
    rows, lengths = _image_files.host_rows(*encode(u8, q))
    return _image_files.write_files(rows, lengths, _image_files.prediction_paths(root, video_ids, frame_ids, "pred_sal_{:06d}.jpg"))
