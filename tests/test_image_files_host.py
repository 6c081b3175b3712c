"""The host path the image file codecs share (diff_sal_amd/_image_files.py), off the GPU: the file writes, the id check and the
damage report of a batched decode."""
import os
import re

import numpy as np
import pytest
import torch

from diff_sal_amd import _image_files, jpeg


def test_write_files_cuts_every_row_and_creates_the_directories(tmp_path):
    rows = np.arange(24, dtype=np.uint8).reshape(3, 8)
    lengths = (8, 3, 5)
    paths = [str(tmp_path / "a" / "x.bin"), str(tmp_path / "b" / "y.bin"), str(tmp_path / "a" / "z.bin")]
    assert not os.path.exists(tmp_path / "a") and not os.path.exists(tmp_path / "b")
    assert _image_files.write_files(rows, lengths, paths) == paths
    for row, length, path in zip(rows, lengths, paths):
        with open(path, "rb") as f:
            assert f.read() == row[:length].tobytes()


def test_checked_ids_counts_and_flattens():
    with pytest.raises(ValueError, match="3 predictions, 2 video ids, 3 frame ids"):
        _image_files.checked_ids(3, ["v", "w"], [1, 2, 3], "png")
    video_ids, frame_ids = _image_files.checked_ids(3, ("v", "v", "w"), torch.tensor([[7], [8], [9]], dtype=torch.int64), "png")
    assert video_ids == ["v", "v", "w"]
    assert frame_ids == [7, 8, 9] and all(type(f) is int for f in frame_ids)


def test_damage_message_names_the_bits_and_at_most_eight_files():
    bits = jpeg.STATUS_BITS
    text = _image_files.damage_message(np.array([0, 5, 0, 2], dtype=np.int32), bits, "jpeg", "scan")
    assert text.startswith("jpeg.decode: 2 of 4 files are damaged inside their scan (file 1: ")
    assert f"file 1: {bits[1]}, {bits[4]}; file 3: {bits[2]})" in text
    assert bits[2] not in text.split("file 3: ")[0]
    status = np.array([1, 0, 2, 4, 1, 2, 0, 4, 1, 2, 4, 1], dtype=np.int32)
    text = _image_files.damage_message(status, bits, "jpeg", "scan")
    assert text.startswith("jpeg.decode: 10 of 12 files are damaged inside their scan (file 0: ")
    assert [int(i) for i in re.findall(r"file (\d+): ", text)] == [0, 2, 3, 4, 5, 7, 8, 9]
