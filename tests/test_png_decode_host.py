"""The PNG decode off the GPU: the NumPy restatement (tests/_png_decode_ref.py) against the fixtures recorded from Pillow
(tools/gen_png_decode_golden.py -> tests/golden/png_decode.npz) and, where PIL imports, a live Pillow against the same fixtures; the
coverage the fixture's case set was built for; the host parser's descriptors for every case; every refusal the parser can be brought
to; the restatement's status for each damaged copy; the GPU-only guard.  Every comparison is exact."""
import io
import zlib

import numpy as np
import pytest
import torch

from diff_sal_amd import png
from tests import _png_decode_ref as ref

CASES, COUNTERS, DAMAGED = ref.load_cases()
SHAPES = {(1, 1), (1, 5), (2, 3), (7, 13), (9, 5), (16, 16), (17, 33), (40, 3), (33, 48), (65, 70), (130, 9), (120, 160)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture(name):
    c = CASES[name]
    rgb, lum, status = ref.decode(c["file"])
    assert status == 0
    assert np.array_equal(rgb, c["rgb"]) and np.array_equal(lum, c["l"]), name
    assert c["rgb"].shape == (c["H"], c["W"], 3) and c["l"].shape == (c["H"], c["W"])


def test_live_pillow_agrees_with_the_fixture():
    Image = pytest.importorskip("PIL.Image")
    for name, c in CASES.items():
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(c["file"])).convert("RGB")), c["rgb"]), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(c["file"])).convert("L")), c["l"]), name


def test_fixture_cases_cover_the_decoder():
    k = ref.new_counters()
    for c in CASES.values():
        ref.decode(c["file"], k)
    assert {n: int(v) for n, v in k.items()} == COUNTERS      # what the generator recorded
    for name in ref.COUNTERS:
        assert k[name] > 0, name
    assert k["max_distance"] == 32768
    assert {(c["H"], c["W"]) for c in CASES.values()} == SHAPES
    assert {(c["color_type"], c["bit_depth"]) for c in CASES.values()} == {(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8),
                                                                         (4, 8), (6, 8)}
    # two stored blocks in one file; IDAT chunks of 1, 5 and 4096 bytes; tRNS on types 0, 2, 3; a 5-entry PLTE
    two = ref.new_counters()
    ref.decode(CASES["120x160_hand_rgba_stored2"]["file"], two)
    assert two["stored"] == 2
    sizes = {n: [len(p) for kind, p in ref.chunks(c["file"]) if kind == b"IDAT"] for n, c in CASES.items()}
    for name, step in (("9x5_hand_rgb_idat1", 1), ("17x33_hand_rgb_idat5", 5), ("65x70_hand_rgba_cycle_idat4096", 4096)):
        assert len(sizes[name]) > 2 and set(sizes[name][:-1]) == {step}
    kinds = {n: [kind for kind, _ in ref.chunks(c["file"])] for n, c in CASES.items()}
    assert {CASES[n]["color_type"] for n in CASES if b"tRNS" in kinds[n] and "hand" in n} == {0, 2, 3}
    assert any(len(p) == 15 for kind, p in ref.chunks(CASES["17x33_hand_pal8_plte5"]["file"]) if kind == b"PLTE")
    assert set(DAMAGED) == {"cut", "zeroed", "adler", "far", "type3", "short", "long"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parser_descriptors(name):
    c = CASES[name]
    p = png.parse_file(c["file"])
    assert [p[k] for k in ("H", "W", "color_type", "bit_depth")] == [c[k] for k in ("H", "W", "color_type", "bit_depth")]
    idat = b"".join(payload for kind, payload in ref.chunks(c["file"]) if kind == b"IDAT")
    assert p["stream"].tobytes() == idat
    plte = b"".join(payload for kind, payload in ref.chunks(c["file"]) if kind == b"PLTE")
    assert p["palette"].tobytes() == (plte + bytes(768))[:768]      # zero-padded
    for as_type in (bytes, bytearray, memoryview, lambda b: np.frombuffer(b, dtype=np.uint8)):
        assert png.parse_file(as_type(c["file"]))["stream"].tobytes() == idat


def test_pack_lays_out_streams_and_records():
    group = max(ref.groups(CASES).values(), key=len)
    files = [CASES[n]["file"] for n in group]
    p = png.pack(files)
    assert p["N"] == len(files) and p["desc_at"] % 16 == 0 and p["host"].size == p["desc_at"] + 784 * len(files)
    desc = p["host"][p["desc_at"]:].view(png.FILE_DTYPE)
    end = 0
    for i, f in enumerate(files):
        one = png.parse_file(f)
        off, n = int(desc["off"][i]), int(desc["len"][i])
        assert off % 16 == 0 and off >= end and p["host"][off:off + n].tobytes() == one["stream"].tobytes()
        assert not p["host"][end:off].any()
        assert np.array_equal(desc["pal"][i], one["palette"])
        end = off + n
    assert end <= p["desc_at"] and not p["host"][end:p["desc_at"]].any()
    with pytest.raises(ValueError, match=r"file 1: 3 x 2, colour type 2, 8 bits where file 0 has"):
        png.pack([files[0], CASES[next(n for n in sorted(CASES) if n.startswith("2x3_pil_RGB_"))]["file"]])


def _chunk(kind, payload):
    return len(payload).to_bytes(4, "big") + kind + payload + zlib.crc32(kind + payload).to_bytes(4, "big")


def _file(ihdr=None, plte=None, idat=(b"\x78\x9c\x63\x00\x00\x00\x01\x00\x01",), head=True, extra_ihdr=False):
    ihdr = (2).to_bytes(4, "big") + (2).to_bytes(4, "big") + bytes([8, 0, 0, 0, 0]) if ihdr is None else ihdr
    out = b"\x89PNG\r\n\x1a\n" + (_chunk(b"IHDR", ihdr) if head else b"") + (_chunk(b"IHDR", ihdr) if extra_ihdr else b"")
    if plte is not None:
        out += _chunk(b"PLTE", plte)
    for p in idat:
        out += _chunk(b"IDAT", p)
    return out + _chunk(b"IEND", b"")


def _ihdr(w=2, h=2, depth=8, ctype=0, comp=0, filt=0, lace=0):
    return w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([depth, ctype, comp, filt, lace])


REFUSALS = [
    ("signature", b"\x89PNX" + _file()[4:], "no PNG signature"),
    ("no_ihdr", _file(head=False), "IHDR is missing"),
    ("short_ihdr", _file(ihdr=_ihdr()[:12]), r"an IHDR chunk of 12 bytes"),
    ("two_ihdr", _file(extra_ihdr=True), "a second IHDR"),
    ("depth16", _file(ihdr=_ihdr(depth=16)), "16-bit samples: decode this file with Pillow"),
    ("interlaced", _file(ihdr=_ihdr(lace=1)), "interlace method 1: decode an interlaced file with Pillow"),
    ("compression", _file(ihdr=_ihdr(comp=1)), "compression method 1, filter method 0"),
    ("filter_method", _file(ihdr=_ihdr(filt=1)), "compression method 0, filter method 1"),
    ("rgb_4bit", _file(ihdr=_ihdr(depth=4, ctype=2)), "bit depth 4 with colour type 2: a pair the standard does not allow"),
    ("pal_16bit", _file(ihdr=_ihdr(depth=16, ctype=3)), "bit depth 16 with colour type 3"),
    ("type5", _file(ihdr=_ihdr(ctype=5)), "colour type 5"),
    ("no_plte", _file(ihdr=_ihdr(ctype=3)), "a palette file without PLTE"),
    ("no_idat", _file(idat=()), "no IDAT chunk"),
    ("length", b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", _ihdr()) + (10 ** 6).to_bytes(4, "big") + b"IDAT" + bytes(18), r"the length 1000000 of chunk b'IDAT' at byte \d+ runs past the file's end"),
    ("header_cut", _file()[:-7], "a chunk header at byte"),
    ("not_deflate", _file(idat=(b"\x79\x9c" + bytes(8),)), "zlib header 0x79 0x9c: not deflate"),
    ("window", _file(idat=(b"\x88\x1c" + bytes(8),)), "zlib header 0x88 0x1c: not deflate with a window of at most 32 K"),
    ("check", _file(idat=(b"\x78\x9d" + bytes(8),)), "zlib header 0x78 0x9d"),
    ("fdict", _file(idat=(b"\x78\xbb" + bytes(8),)), "preset dictionary"),
    ("too_wide", _file(ihdr=_ihdr(w=8193)), "8193 x 2: at most 8192 x 65535"),
]


@pytest.mark.parametrize("name,data,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_file_and_the_reason(name, data, message):
    good = CASES["2x3_hand_grey1"]["file"]
    with pytest.raises(ValueError, match="png.parse_file: .*" + message):
        png.parse_file(data)
    with pytest.raises(ValueError, match=r"png.decode: file 1: .*" + message):      # raised on the host, before anything is launched
        png.pack([good, data])


def test_the_parser_takes_the_unpatched_file():
    p = png.parse_file(_file())
    assert (p["H"], p["W"], p["color_type"], p["bit_depth"]) == (2, 2, 0, 8)
    assert png.parse_file(_file(idat=(b"\x78", b"\x9c\x63\x00", b"", b"\x00\x00\x01\x00\x01")))["stream"].tobytes() == b"\x78\x9c\x63\x00\x00\x00\x01\x00\x01"


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_restatement_flags_every_damaged_copy(name):
    data, base, bit = DAMAGED[name]
    p = png.parse_file(data)      # the damage is inside the stream: the parser takes the file
    c = CASES[base]
    assert (p["H"], p["W"], p["color_type"], p["bit_depth"]) == (c["H"], c["W"], c["color_type"], c["bit_depth"])
    rgb, lum, status = ref.decode(data)
    assert status != 0 and status & bit == bit and all(b in png.STATUS_BITS for b in (1 << k for k in range(10)) if status & b)
    if name == "long":      # the pixels are still delivered
        Image = pytest.importorskip("PIL.Image")
        assert status == ref.LONG and np.array_equal(rgb, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


def test_status_bits_are_the_headers():
    from diff_sal_amd import _cdecl, build
    consts = _cdecl.parse(open(build.HEADER).read()).constants
    bits = {v for k, v in consts.items() if k.startswith("DIFFSAL_PNG_")}
    assert bits == set(png.STATUS_BITS) == {1 << k for k in range(10)}
    assert (ref.BAD_BLOCK, ref.BAD_ADLER) == (consts["DIFFSAL_PNG_BAD_BLOCK"], consts["DIFFSAL_PNG_BAD_ADLER"])


def test_gpu_only_guard_and_argument_errors():
    good = CASES["2x3_hand_grey1"]["file"]
    for call in (lambda: png.decode([good], device="cpu"), lambda: png.decode(torch.zeros(4, dtype=torch.uint8)),
                 lambda: png.decode([torch.zeros(4, dtype=torch.uint8)])):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(ValueError, match="empty list"):
        png.pack([])
    with pytest.raises(ValueError, match="mode must be 'RGB' or 'L'"):
        png.decode([good], mode="P")
    with pytest.raises(ValueError, match="file 0: expected bytes"):
        png.pack(["name.png"])
