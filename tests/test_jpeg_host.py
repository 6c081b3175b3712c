"""The JPEG export off the GPU: the NumPy restatement (tests/_jpeg_ref.py) against the fixtures recorded from Pillow
(tools/gen_jpeg_golden.py -> tests/golden/jpeg_export.npz) and, where PIL imports, against a live Pillow; the host-side quantisation
table; the coverage the fixture's case set was built for; the GPU-only guard.  Every comparison is exact."""
import io

import numpy as np
import pytest
import torch

from diff_sal_amd import jpeg
from tests import _jpeg_ref as ref

CASES, BIG, COUNTERS = ref.load_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture(name):
    c = CASES[name]
    for q, want in c["q"].items():
        assert ref.encode(c["u8"], q) == want["file"], (name, q)
        assert np.array_equal(ref.decode(c["u8"], q), want["decoded"]), (name, q)


def test_restatement_reproduces_the_full_size_case():
    big = ref.big_input()
    assert big.shape == ref.BIG_SHAPE and big.dtype == np.uint8
    for b, img in enumerate(big):
        data = ref.encode(img, BIG["quality"])
        assert len(data) == BIG["lengths"][b] and ref.sha256(data) == BIG["sha256"][b], b
        assert np.array_equal(ref.decode(img, BIG["quality"])[BIG["rows"]][:, BIG["cols"]], BIG["decoded"][b]), b


@pytest.mark.parametrize("name", ["r13x21", "bw24x32"])
def test_restatement_reproduces_a_live_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    c = CASES[name]
    for q in c["q"]:
        f = io.BytesIO()
        Image.fromarray(c["u8"]).save(f, "JPEG", quality=q)
        assert ref.encode(c["u8"], q) == f.getvalue(), (name, q)
        assert np.array_equal(ref.decode(c["u8"], q), np.asarray(Image.open(io.BytesIO(f.getvalue())))), (name, q)


def test_quant_table_is_the_fixture_files_dqt_payload():
    seen = set()
    for c in CASES.values():
        for q, want in c["q"].items():
            data = want["file"]
            at = data.index(b"\xFF\xDB")
            assert data[at + 2:at + 5] == b"\x00\x43\x00"      # 67 bytes: 8-bit table 0
            payload = np.frombuffer(data[at + 5:at + 69], dtype=np.uint8).astype(np.int64)      # zig-zag order
            table = jpeg.quant_table(q)
            assert table.shape == (64,) and np.array_equal(table[ref.ZIGZAG], payload), q
            assert np.array_equal(table, ref.quant_table(q))
            seen.add(q)
    assert seen == set(ref.QUALITIES)
    assert jpeg.quant_table().tolist()[:8] == [2, 1, 1, 2, 2, 4, 5, 6]      # quality 95
    for bad in (0, 101, 95.5):
        with pytest.raises(ValueError, match="quality"):
            jpeg.quant_table(bad)


def test_fixture_cases_cover_the_coder():
    k = ref.new_counters()
    for c in CASES.values():
        for q in c["q"]:
            ref.encode(c["u8"], q, k)
    for img in ref.big_input():
        ref.encode(img, BIG["quality"], k)
    assert k == COUNTERS      # what the generator recorded
    assert k["zrl"] >= 1 and k["no_eob"] >= 1 and k["stuffed_ff"] >= 1 and k["padded_last_ff"] >= 1
    assert k["max_dc_cat"] == 11 and k["max_ac_cat"] == 10
    assert k["dc_neg"] >= 1 and k["dc_pos"] >= 1 and k["all_eob_images"] >= 1
    shapes = {c["u8"].shape for c in CASES.values()}
    assert {(1, 1), (3, 17), (8, 8), (13, 21), (16, 24), (37, 50), (24, 32)} <= shapes
    blocks = [((h + 7) // 8) * ((w + 7) // 8) for h, w in shapes]
    assert any(n > 2 * 256 and n % 2 == 1 for n in blocks)      # more than two chunks of the offset scan's workgroup, odd
    both = [n for n, c in CASES.items() if set(c["q"]) == set(ref.QUALITIES)]
    assert len(both) >= 2


def test_cpu_tensors_raise():
    u8 = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda: jpeg.encode(u8), lambda: jpeg.roundtrip(u8),
                 lambda: jpeg.save_predictions(torch.zeros(1, 1, 8, 8), ["a"], [1], "unused")):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
