"""Writes tests/golden/video_input.npz: what Pillow's ``Image.resize`` gives for the seeded uint8 inputs of
tests/_video_input_ref.py, recorded with the calls the reference makes: ``img.resize((320, 240))`` with no filter argument
(R/datasets/saliency_db.py:35), ``img.resize(size, Image.BILINEAR)`` (``Scale``, R/datasets/spatial_transforms.py:156) and, for the
single-channel case, an image made by ``Image.fromarray(..., 'L')``.  Small cases are stored in full; of the protocol-size chain
(360 x 640 -> 240 x 320 -> 224 x 384, two frames) a strided sample and the row and column sums.  The Pillow version is stored
beside the arrays.  Expected outputs only: the inputs are rebuilt from their seeds at test time (a CRC of each is kept, so that a
platform that rebuilds another input is noticed).

    python tools/gen_video_input_golden.py

Needs numpy and Pillow; no GPU.  No test runs this tool."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _video_input_ref as ref  # noqa: E402

PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def to_image(a):
    """one frame [H, W, C] as the PIL image the reference would hold after convert('RGB' | 'L')"""
    return Image.fromarray(a[..., 0], "L") if a.shape[-1] == 1 else Image.fromarray(a, "RGB")


def from_image(img, channels):
    a = np.asarray(img)
    return a[..., None] if channels == 1 else a


def main():
    blob = {"pillow_version": np.array(PIL.__version__)}
    for name, (_, _, shape, (h, w), filt) in ref.CASES.items():
        x = ref.case_input(name)
        out = np.stack([from_image(to_image(f).resize((w, h), PIL_FILTERS[filt]), shape[3]) for f in x])
        assert out.shape == (shape[0], h, w, shape[3]) and out.dtype == np.uint8
        blob[f"{name}/out"] = out
        blob[f"crc/{name}"] = np.array(ref.crc(x), dtype=np.int64)
        same = np.array_equal(out, ref.resize(x, (h, w), filt))
        print(name, shape, "->", out.shape, filt, "restatement equal:", same, "| 0s", int((out == 0).sum()), "255s", int((out == 255).sum()))
    _, _, shape, (ph, pw), (h, w) = ref.PROTOCOL
    x = ref.protocol_input()
    blob["crc/protocol"] = np.array(ref.crc(x), dtype=np.int64)
    mids, outs = [], []
    for f in x:
        img = to_image(f)
        mid = img.resize((pw, ph))                                  # the loader's call: Pillow's default filter
        assert np.array_equal(np.asarray(mid), np.asarray(img.resize((pw, ph), Image.BICUBIC))), "the default filter is not bicubic here"
        mids.append(np.asarray(mid))
        outs.append(np.asarray(mid.resize((w, h), Image.BILINEAR)))      # Scale
    mid, out = np.stack(mids), np.stack(outs)
    for k, v in ref.protocol_digest(out).items():
        blob[f"protocol/{k}"] = v
    blob["protocol/mid_row_sums"] = mid.astype(np.int64).sum(axis=2)
    print("protocol", x.shape, "->", mid.shape, "->", out.shape, "restatement equal:",
          np.array_equal(out, ref.chain(x, (h, w), (ph, pw))))
    path = ref.GOLDEN
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
