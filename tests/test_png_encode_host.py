"""The PNG export off the GPU: the files of the NumPy restatement (tests/_png_encode_ref.py) checked from the outside -- a plain
chunk walk with zlib's CRC-32, zlib's inflate (which verifies the Adler-32), the decode's own restatement, the host parser and, where
PIL imports, Pillow -- against the fixtures (tools/gen_png_encode_golden.py -> tests/golden/png_encode.npz); the coverage the
fixture's case set was built for; the capacity; the GPU-only guard.  Every comparison is exact."""
import io
import zlib

import numpy as np
import pytest
import torch

from diff_sal_amd import ops, png
from tests import _png_decode_ref as dec
from tests import _png_encode_ref as ref

CASES, COUNTERS = ref.load_cases()
SHAPES = {(1, 1), (1, 5), (300, 1), (7, 13), (17, 33), (2, 8192), (16, 16), (33, 48), (120, 160), (128, 127), (113, 144), (130, 130),
          (1, 2471), (1, 3568), (1, 8190), (64, 70)}
SMOOTH = ("64x70_blobs_a", "64x70_blobs_b")


def walk(data: bytes):
    """[(type, payload)] by a plain walk; every chunk's CRC-32 is checked against zlib's"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], "big")
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(payload) == n and int.from_bytes(data[at + 8 + n:at + 12 + n], "big") == zlib.crc32(kind + payload), (kind, at)
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture(name):
    c = CASES[name]
    assert ref.encode(c["img"]) == c["file"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_from_the_outside(name):
    c = CASES[name]
    data, img = c["file"], c["img"]
    H, W = img.shape
    chunks = walk(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 0, 0, 0, 0]) and chunks[2][1] == b""
    idat = chunks[1][1]
    assert idat[:2] == b"\x78\x01" and len(data) == 57 + len(idat) <= png.capacity(H, W)
    raw = zlib.decompress(idat)      # also the Adler-32
    assert len(raw) == H * (W + 1)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, W + 1)
    assert rows[:, 0].max() <= 4
    stream, filters = ref.filtered(img)
    assert stream.tobytes() == raw and np.array_equal(filters, rows[:, 0])
    rgb, lum, status = dec.decode(data)      # the device decode's restatement: its inflate follows zlib's acceptance rules
    assert status == 0 and np.array_equal(lum, img) and np.array_equal(rgb, np.repeat(img[:, :, None], 3, axis=2))
    p = png.parse_file(data)
    assert (p["H"], p["W"], p["color_type"], p["bit_depth"]) == (H, W, 0, 8) and p["stream"].tobytes() == idat


def test_live_pillow_reads_the_input_back():
    Image = pytest.importorskip("PIL.Image")
    for name, c in CASES.items():
        im = Image.open(io.BytesIO(c["file"]))
        assert im.mode == "L" and np.array_equal(np.asarray(im), c["img"]), name


def test_fixture_cases_cover_the_coder():
    k = ref.new_counters()
    for c in CASES.values():
        ref.encode(c["img"], k)
    assert {n: int(v) for n, v in k.items()} == COUNTERS      # what the generator recorded
    for name in ref.COUNTERS:
        assert k[name] > 0, name
    assert {c["img"].shape for c in CASES.values()} == SHAPES
    one = lambda name: (lambda q: (ref.encode(CASES[name]["img"], q), q)[1])(ref.new_counters())      # noqa: E731
    assert one("1x3568_limit15")["limit15"] == 1 and one("1x8190_limit7")["limit7"] == 1
    assert one("130x130_zeros")["previous_segment"] == 1 and one("128x127_smooth")["full_segment"] == 1
    assert one("113x144_smooth")["segment_of_1"] == 1 and one("113x144_zeros")["segment_of_1"] == 1
    q = one("33x48_noise")
    assert q["match258"] == q["remainder1"] == q["remainder2"] == 0
    # the rows of runs: exactly these counts of positions that equal the byte in front of them occur
    raw = np.frombuffer(zlib.decompress(walk(CASES["1x2471_runs"]["file"])[1][1]), dtype=np.uint8)
    eq = np.concatenate([[False], raw[1:] == raw[:-1], [False]])
    edges = np.flatnonzero(np.diff(eq.astype(np.int8)))
    assert {2, 3, 257, 258, 259, 260, 261, 516, 517} <= set((edges[1::2] - edges[0::2]).tolist())


def test_lengths_are_complete_and_limited():
    """the code construction on its own: Kraft sum exactly 1, the limit held, at least two symbols"""
    rng = np.random.RandomState(5)
    fib = [1, 1, 1]
    while len(fib) < 24:
        fib.append(sum(fib[:-1]) + 1)
    for counts, limit in ((fib + [0] * 262, 15), (fib[:12] + [0] * 7, 7), ([0] * 19, 7), ([0, 0, 0, 5] + [0] * 15, 7), ([7] * 19, 7),
                          (rng.randint(0, 50, 286).tolist(), 15), ((rng.randint(0, 3, 286) * rng.randint(0, 9000, 286)).tolist(), 15)):
        lens, _ = ref.limited_lengths(counts, limit)
        used = [v for v in lens if v]
        assert len(used) >= 2 and max(used) <= limit and sum(1 << (limit - v) for v in used) == 1 << limit
        assert all(lens[i] for i in range(len(counts)) if counts[i])
        order = sorted((i for i in range(len(counts)) if lens[i]), key=lambda i: (counts[i], i))
        assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]))      # the rarer, the longer


def test_capacity():
    for H, W in sorted(SHAPES) + [(224, 384), (360, 640), (65535, 8192), (1, 16383 // 2)]:
        cap = png.capacity(H, W)
        assert cap == ref.capacity(H, W) == ops.png_capacity(H, W) and cap % 16 == 0 and cap < 2 ** 31
    for bad in ((0, 5), (5, 0), (65536, 5), (5, 8193)):
        with pytest.raises(ValueError, match="png_capacity"):
            png.capacity(*bad)


@pytest.mark.parametrize("name", SMOOTH)
def test_smaller_than_huffman_only(name):
    c = CASES[name]
    stream, _ = ref.filtered(c["img"])
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    only = z.compress(stream.tobytes()) + z.flush()
    assert len(walk(c["file"])[1][1]) < len(only)


def test_cpu_tensors_raise(tmp_path):
    u8 = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda: png.encode(u8), lambda: png.encode(u8.numpy()),
                 lambda: png.save_predictions(torch.zeros(1, 1, 8, 8), ["a"], [1], str(tmp_path))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(RuntimeError, match="png runs on the GPU only"):
        png.encode(u8)
    assert not list(tmp_path.iterdir())
