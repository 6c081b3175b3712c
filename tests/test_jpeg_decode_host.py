"""The JPEG decode off the GPU: the NumPy restatement (tests/_jpeg_decode_ref.py) against the fixtures recorded from Pillow
(tools/gen_jpeg_decode_golden.py -> tests/golden/jpeg_decode.npz) and, where PIL imports, a live Pillow against the same fixtures; the
coverage the fixture's case set was built for; the host parser's descriptors for every case; every refusal the parser can be brought
to; the GPU-only guard.  Every comparison is exact."""
import io

import numpy as np
import pytest
import torch

from diff_sal_amd import jpeg
from tests import _jpeg_decode_ref as ref

CASES, COUNTERS, DAMAGED = ref.load_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture(name):
    c = CASES[name]
    assert np.array_equal(ref.decode(c["file"], "RGB"), c["rgb"]), name
    assert np.array_equal(ref.decode(c["file"], "L"), c["l"]), name
    assert c["rgb"].shape == (c["H"], c["W"], 3) and c["l"].shape == (c["H"], c["W"])


def test_fixture_cases_cover_the_decoder():
    k = ref.new_counters()
    for c in CASES.values():
        ref.decode(c["file"], "RGB", k)
    assert {n: int(v) for n, v in k.items()} == COUNTERS      # what the generator recorded
    for name, v in k.items():
        assert v > 0, name
    shapes = {(c["H"], c["W"]) for c in CASES.values()}
    assert {(1, 1), (2, 3), (1, 4), (1, 5), (3, 6), (5, 4), (2, 7), (9, 5), (8, 8), (16, 16), (17, 33), (31, 18), (37, 53), (40, 3), (33, 48),
            (120, 160)} <= shapes
    assert {(c["ncomp"], c["hs"], c["vs"]) for c in CASES.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {c["restart"] for c in CASES.values()} >= {0, 1, 2, 3}
    # an MCU count that is no multiple of the interval, and more than eight restart markers in one file
    assert any(c["restart"] > 1 and (-(-c["W"] // (8 * c["hs"])) * -(-c["H"] // (8 * c["vs"]))) % c["restart"] for c in CASES.values())
    assert any(c["nseg"] > 9 for c in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_parser_descriptors(name):
    c = CASES[name]
    p = jpeg.parse_file(c["file"])
    assert [p[k] for k in ("H", "W", "ncomp", "hs", "vs")] == [c[k] for k in ("H", "W", "ncomp", "hs", "vs")]
    hd = ref.walk(c["file"])
    d = p["desc"]
    assert int(d["restart"]) == c["restart"] == hd["restart"] and int(d["nseg"]) == c["nseg"] == p["segments"].shape[0]
    for i, (cid, dc, ac) in enumerate(hd["scan"]):
        assert d["comp"][i].tolist() == [hd["comps"][i][3], dc, ac, 0], i
        assert np.array_equal(d["qt"][hd["comps"][i][3]], hd["qt"][hd["comps"][i][3]])
        for cls, tid in ((0, dc), (1, ac)):      # counts and symbols as DHT carries them
            codes = hd["huff"][(cls, tid)]
            counts = [sum(1 for length, _ in codes if length == n) for n in range(1, 17)]
            assert d["hbits"][2 * cls + tid].tolist() == counts
            assert d["hvals"][2 * cls + tid][:len(codes)].tolist() == [codes[key] for key in sorted(codes)]
    segs, end = ref.segments(c["file"], hd["scan_at"])
    assert int(d["scan_off"]) == hd["scan_at"] and int(d["scan_off"]) + int(d["scan_len"]) == end
    mcus = -(-c["W"] // (8 * c["hs"])) * -(-c["H"] // (8 * c["vs"]))
    assert c["nseg"] == (-(-mcus // c["restart"]) if c["restart"] else 1)
    for s, (b, e) in enumerate(segs):
        assert p["segments"][s].tolist() == [b, e, s * c["restart"]], s
        assert c["file"][e:e + 1] == b"\xFF" and (s == len(segs) - 1 or 0xD0 + s % 8 == c["file"][e + 1])


def _save(img, **kw):
    Image = pytest.importorskip("PIL.Image")
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", **kw)
    return f.getvalue()


def _refused(files, text, **kw):
    with pytest.raises(ValueError, match=text):
        jpeg.decode(files, **kw)


def _patch(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


def test_refusals_from_patched_bytes():
    good = CASES["16x16_420_base"]["file"]
    other = CASES["8x8_420_smooth"]["file"]
    sof, dqt, sos = good.index(b"\xFF\xC0"), good.index(b"\xFF\xDB"), good.index(b"\xFF\xDA")
    _refused([], "empty list")
    _refused([good, other], "file 1: 8 x 8.*share size and sampling")
    _refused([good, CASES["16x16_444_saturated"]["file"]], "file 1: .*share size and sampling")
    _refused([good, _patch(good, sof + 4, [12])], "file 1: sample precision 12")
    _refused([_patch(good, dqt + 4, [0x10])], "file 0: a 16-bit quantisation table")
    _refused([good, good[:sof + 6]], "file 1: the file ends inside a marker segment")
    _refused([good[:sos]], "file 0: the file ends inside a marker segment")
    _refused([good[:sos] + b"\xFF\xD9"], "file 0: no SOS marker")
    _refused([b"\x89PNG\r\n\x1a\n"], "file 0: no SOI")
    _refused([_patch(good, sof + 1, [0xC2])], "file 0: a progressive frame")
    _refused([_patch(good, sof + 1, [0xC1])], "extended sequential")
    _refused([_patch(good, sof + 1, [0xC9])], "arithmetic")
    _refused([_patch(good, sof + 1, [0xC3])], "lossless")
    _refused([_patch(good, sof + 5, [0, 0])], "height 0")
    _refused([_patch(good, sof + 11, [0x12])], "sampling factors 1x2 1x1 1x1")
    _refused([_patch(good, sof + 14, [0x21])], "sampling factors")
    _refused([_patch(good, sof + 12, [3])], "component 0 selects a table the file does not define")
    grey = CASES["16x16_grey_noise"]["file"]      # defines DC 0 and AC 0 alone
    _refused([_patch(grey, grey.index(b"\xFF\xDA") + 6, [0x11])], "component 0 selects a table")
    _refused([_patch(good, sos + 4, [1])], "more than one scan")
    _refused([good[:-2] + good[sos:]], "more than one scan")
    _refused([good[:-2] + b"\xFF\xDC\x00\x04\x00\x10\xFF\xD9"], "a DNL marker")
    # a wrong count of restart segments: a marker taken out of a file with restart markers, one put into a file without
    rst = CASES["37x53_420rst_noise"]["file"]
    assert CASES["37x53_420rst_noise"]["nseg"] > 1
    at = rst.index(b"\xFF\xD0", rst.index(b"\xFF\xDA"))
    _refused([rst[:at] + rst[at + 2:]], "restart segments in the scan")
    _refused([good[:sos + 30] + b"\xFF\xD0" + good[sos + 30:]], "1 MCUs at interval 0|restart segments in the scan")
    # an Adobe APP14 segment with transform 0, and component ids R G B without JFIF
    adobe = b"\xFF\xEE\x00\x0EAdobe\x00\x64\x00\x00\x00\x00\x00"
    _refused([good[:2] + adobe + good[2:]], "Adobe APP14 segment with transform 0")
    rgb_ids = _patch(_patch(_patch(good, sof + 10, [ord("R")]), sof + 13, [ord("G")]), sof + 16, [ord("B")])
    rgb_ids = _patch(_patch(_patch(rgb_ids, sos + 5, [ord("R")]), sos + 7, [ord("G")]), sos + 9, [ord("B")])
    app0 = rgb_ids.index(b"\xFF\xE0")
    _refused([rgb_ids[:app0] + rgb_ids[app0 + 18:]], "component ids R, G, B without JFIF")
    for bad in ("rgb", "YCbCr", None):
        _refused([good], "mode", mode=bad)
    _refused(["not bytes"], "file 0: expected bytes")


def test_refusals_from_pillow_files():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(16, 24, 3), dtype=np.uint8)
    _refused([_save(img, progressive=True)], "file 0: a progressive frame")
    Image = pytest.importorskip("PIL.Image")
    f = io.BytesIO()
    Image.frombytes("CMYK", (24, 16), np.dstack([img, img[..., :1]]).tobytes()).save(f, "JPEG")
    _refused([f.getvalue()], "file 0: 4 components")
    _refused([_save(img, subsampling=0), _save(img, subsampling=2)], "file 1: .*luma 2x2 where file 0 has .*1x1")


def test_a_cut_scan_and_fill_bytes_pass_the_parser():
    """damage inside the entropy-coded data is the device's to report: the parser takes the three damaged fixtures"""
    for name, data in DAMAGED.items():
        p = jpeg.parse_file(data)
        assert (p["H"], p["W"], p["hs"], p["vs"]) == (16, 16, 2, 2) and p["segments"].shape == (1, 3), name
        b, e, _ = p["segments"][0].tolist()
        assert int(p["desc"]["scan_off"]) == b <= e <= len(data)
    b, e, _ = jpeg.parse_file(DAMAGED["ff"])["segments"][0].tolist()
    assert b == e      # fill only
    good = CASES["16x16_420_base"]["file"]
    filled = good[:-2] + b"\xFF\xFF\xFF" + good[-2:]      # fill bytes in front of EOI, and in front of a marker of the header
    sof = good.index(b"\xFF\xC0")
    filled = filled[:sof] + b"\xFF\xFF" + filled[sof:]
    assert jpeg.parse_file(filled)["segments"][0, 1] - 2 == jpeg.parse_file(good)["segments"][0, 1]


@pytest.mark.parametrize("name", ["37x53_420_noise", "17x33_422_noise", "2x3_420opt_noise", "120x160_422rows_smooth", "37x53_grey_noise"])
def test_installed_pillow_still_reads_the_fixture_pixels(name):
    Image = pytest.importorskip("PIL.Image")
    c = CASES[name]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(c["file"])).convert("RGB")), c["rgb"])
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(c["file"])).convert("L")), c["l"])


def test_cpu_devices_and_tensors_raise():
    good = CASES["8x8_420_smooth"]["file"]
    for call in (lambda: jpeg.decode([good], device="cpu"), lambda: jpeg.decode([good], device=torch.device("cpu")),
                 lambda: jpeg.decode(torch.zeros(4, dtype=torch.uint8)), lambda: jpeg.decode([torch.zeros(4, dtype=torch.uint8)])):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
