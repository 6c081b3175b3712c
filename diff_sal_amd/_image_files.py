"""The host path the image file codecs share (``jpeg``, ``png``; ``postprocess`` for an export's ids and paths): the check of an export's
maps, the driver of a batched decode and its damage report, the head of ``pack``, the ids, paths and file writes of ``save_predictions``.
Per codec stay: what a file is (``parse_file``), the buffer that travels (``pack``), the size limits, the call into ``ops`` and every
sentence that names the format.  Plain functions: the codec's name and nouns come in as arguments."""
import os
from typing import Callable, Sequence

import numpy as np
import torch
from torch import Tensor


def _maps(u8: Tensor, codec: str, limit: Callable, what: str = "u8") -> Tensor:
    """[B, 1, H, W] or [B, H, W] uint8 GPU tensor -> contiguous [B, H, W]; ``limit(shape)``: the codec's sentence about a size it does not take"""
    if not isinstance(u8, Tensor) or not u8.is_cuda:
        raise RuntimeError(f"diff_sal_amd {codec} runs on the GPU only (no CPU fallback); {what} is on "
                           f"{getattr(u8, 'device', type(u8).__name__)}")
    if u8.dtype != torch.uint8:
        raise ValueError(f"{codec}: {what} must be uint8 (postprocess.to_uint8 gives it), got {u8.dtype}")
    if u8.dim() == 4 and u8.shape[1] == 1:
        u8 = u8[:, 0]
    if u8.dim() != 3 or u8.numel() == 0:
        raise ValueError(f"{codec}: {what} must be a non-empty [B, 1, H, W] or [B, H, W], got {tuple(u8.shape)}")
    refused = limit(tuple(u8.shape))
    if refused:
        raise ValueError(f"{codec}: {refused}")
    return u8.contiguous()


def damage_message(status: np.ndarray, status_bits: dict, codec: str, noun: str) -> str:
    """what ``decode(strict=True)`` raises for a per-file ``status`` with non-zero entries: their count, and the bits of the first 8"""
    names = "; ".join(f"file {i}: " + ", ".join(t for b, t in status_bits.items() if status[i] & b) for i in np.flatnonzero(status)[:8])
    return f"{codec}.decode: {int((status != 0).sum())} of {status.size} files are damaged inside their {noun} ({names})"


def decode(files: Sequence, mode: str, device, strict: bool, *, codec: str, pack: Callable, file_dtype: np.dtype, status_bits: dict,
           noun: str, run: Callable):
    """``jpeg.decode`` / ``png.decode`` around the codec's launch: ``pack(files)``'s buffer travels in one copy and is cut at its
    ``desc_at`` and behind the ``N`` records of ``file_dtype``; ``run(packed, records, tail, p)`` gives ``(frames, status)``."""
    if mode not in ("RGB", "L"):
        raise ValueError(f"{codec}.decode: mode must be 'RGB' or 'L', got {mode!r}")
    dev = torch.device("cuda" if device is None else device)
    files = files if isinstance(files, Tensor) else list(files)
    if dev.type != "cuda" or isinstance(files, Tensor) or any(isinstance(f, Tensor) for f in files):
        raise RuntimeError(f"diff_sal_amd {codec} runs on the GPU only (no CPU fallback); decode takes the files' bytes and a GPU device, got "
                           f"{'a tensor' if dev.type == 'cuda' else dev}")
    p = pack(files)
    buf = torch.from_numpy(p["host"]).to(dev)
    desc_at, tail_at = p["desc_at"], p["desc_at"] + p["N"] * file_dtype.itemsize
    frames, status = run(buf[:desc_at], buf[desc_at:tail_at].view(p["N"], file_dtype.itemsize), buf[tail_at:], p)
    if not strict:
        return frames, status
    bad = status.cpu().numpy()
    if bad.any():
        raise ValueError(damage_message(bad, status_bits, codec, noun))
    return frames


MAX_READ_THREADS = 16


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def read_files(paths: Sequence, threads: int = 1) -> list:
    """the bytes of the files at ``paths``, in their order; ``threads`` above 1 reads them from that many host threads (at most
    ``MAX_READ_THREADS``, and no more than there are files): a read releases the interpreter lock, so a video's files arrive together"""
    paths = list(paths)
    n = min(int(threads), MAX_READ_THREADS, len(paths))
    if n <= 1:
        return [_read(p) for p in paths]
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=n) as pool:
        return list(pool.map(_read, paths))


def file_decoder(decode: Callable) -> Callable:
    def decode_files(paths: Sequence, mode: str = "RGB", device=None, strict: bool = True):
        """``decode`` of the files at ``paths``."""
        return decode(read_files(paths), mode=mode, device=device, strict=strict)
    return decode_files


def parse_files(files: Sequence, codec: str, parse: Callable, refused: type, keys: Sequence[str], mismatch: Callable):
    """The head of a codec's ``pack`` -> (the files as a list, ``parse(f, i)`` of each).  A ``refused`` from ``parse`` becomes a ValueError
    naming the file's position; where a file differs from file 0 in one of ``keys``, ``mismatch(file 0's, its)`` is the sentence."""
    files = list(files)
    if not files:
        raise ValueError(f"{codec}.decode: an empty list of files")
    parsed = []
    for i, f in enumerate(files):
        try:
            parsed.append(parse(f, i))
        except refused as e:
            raise ValueError(f"{codec}.decode: file {i}: {e}") from None
        if any(parsed[0][k] != parsed[i][k] for k in keys):
            raise ValueError(f"{codec}.decode: file {i}: {mismatch(parsed[0], parsed[i])}")
    if len(files) > 65535:
        raise ValueError(f"{codec}.decode: {len(files)} files in one call (at most 65535)")
    return files, parsed


def decode_groups(files: Sequence, mode: str, device, *, codec: str, geometry: Callable, refused: type, decode: Callable,
                  status_bits: dict, noun: str):
    """``jpeg.decode_groups`` / ``png.decode_groups``: files of several geometries through the codec's ``decode``, which takes one
    geometry per call.  ``geometry(f, i)`` reads file ``i``'s header and gives what the files of a call must share; the files are
    grouped by it (groups in order of first appearance, a group's files in list order) and every group is one ``decode`` call, so
    the calls number the distinct geometries, not the files.  Returns ``(groups, where)``: the decoded tensor of every group and,
    per file, ``(group, position in it)``.  The per-file status of all calls is read back once; damage raises as ``decode`` does,
    naming the files by their positions in ``files``."""
    files = list(files)
    if not files:
        raise ValueError(f"{codec}.decode_groups: an empty list of files")
    index, members, where = {}, [], []
    for i, f in enumerate(files):
        try:
            key = geometry(f, i)
        except refused as e:
            raise ValueError(f"{codec}.decode_groups: file {i}: {e}") from None
        g = index.setdefault(key, len(index))
        if g == len(members):
            members.append([])
        where.append((g, len(members[g])))
        members[g].append(f)
    groups, status = [], []
    for m in members:
        frames, st = decode(m, mode, device, False)
        groups.append(frames)
        status.append(st)
    per_group = [s.cpu().numpy() for s in ([torch.cat(status)] if len(status) > 1 else status)][0]
    if per_group.any():
        first = np.concatenate([[0], np.cumsum([len(m) for m in members])])
        in_order = np.array([per_group[first[g] + k] for g, k in where])
        raise ValueError(damage_message(in_order, status_bits, codec, noun))
    return groups, where


def checked_ids(n: int, video_ids: Sequence, frame_ids, module: str):
    """``save_predictions``' ids for ``n`` predictions -> (video ids as a list, frame ids as Python ints; a tensor is flattened)"""
    frame_ids = [int(f) for f in (frame_ids.reshape(-1).tolist() if isinstance(frame_ids, Tensor) else frame_ids)]
    video_ids = list(video_ids)
    if not (n == len(video_ids) == len(frame_ids)):
        raise ValueError(f"{module}: {n} predictions, {len(video_ids)} video ids, {len(frame_ids)} frame ids")
    return video_ids, frame_ids


def prediction_paths(root: str, video_ids: Sequence, frame_ids: Sequence[int], name: str):
    """``<root>/<video id>/<name.format(frame id)>`` of every prediction"""
    return [os.path.join(root, str(vid), name.format(fid)) for vid, fid in zip(video_ids, frame_ids)]


def host_rows(data: Tensor, lengths: Tensor):
    """an encode's ``(data, lengths)`` on the host, in two copies: the lengths, then the rows cut at the longest file (a few per cent of them)"""
    n = lengths.cpu().numpy()
    return data[:, :int(n.max())].cpu().numpy(), n


def write_files(rows: np.ndarray, lengths: Sequence[int], paths: Sequence[str]):
    """writes ``rows[i, :lengths[i]]`` to ``paths[i]``, creating its directory; returns the paths as a list"""
    paths = list(paths)
    for row, length, path in zip(rows, lengths, paths):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "wb") as f:
            f.write(row[:int(length)].tobytes())
    return paths
