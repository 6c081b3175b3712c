"""The video front end without a GPU: the NumPy restatement of Pillow's 8-bit resample (tests/_video_input_ref.py) against the
outputs recorded from Pillow (tools/gen_video_input_golden.py) and, where Pillow is installed, against Pillow itself; the
package's host-side tables and index arithmetic against the restatement, against torch's own CPU operators and against
hand-worked lists; and the argument checks of the C ABI, which precede any launch.

Every comparison is exact: the resample is integer arithmetic on float64-built coefficients, and the look-up tables are the
reference's own float32 operations on 256 inputs."""
import ctypes

import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, ops, video_input as vi
from tests import _video_input_ref as ref

GOLD = ref.load_golden()


def test_inputs_are_the_ones_the_fixture_was_recorded_from():
    for name in ref.CASES:
        assert ref.crc(ref.case_input(name)) == int(GOLD[f"crc/{name}"]), name
    assert ref.crc(ref.protocol_input()) == int(GOLD["crc/protocol"])
    b = ref.case_input("bands")
    assert set(np.unique(b)) == {0, 255}


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_restatement_equals_the_pillow_fixture(name):
    _, _, shape, size, filt = ref.CASES[name]
    out = ref.resize(ref.case_input(name), size, filt)
    want = GOLD[f"{name}/out"]
    assert out.shape == want.shape == (shape[0],) + size + (shape[3],)
    assert np.array_equal(out, want)


def test_the_clip_is_exercised_by_the_block_images():
    """the bicubic lobes overshoot at a 0 / 255 edge: without the clip to 0 .. 255 these outputs would wrap"""
    for name in ("up_blocks_bicubic", "bands"):
        out = GOLD[f"{name}/out"]
        assert (out == 0).sum() > 100 and (out == 255).sum() > 100
        assert ((out > 0) & (out < 255)).any()


def test_restatement_equals_the_fixture_on_the_protocol_chain():
    _, _, _, pre, size = ref.PROTOCOL
    x = ref.protocol_input()
    mid = ref.resize(x, pre, "bicubic")
    assert np.array_equal(mid.astype(np.int64).sum(axis=2), GOLD["protocol/mid_row_sums"])
    out = ref.resize(mid, size, "bilinear")
    assert out.shape == (2,) + size + (3,)
    for k, v in ref.protocol_digest(out).items():
        assert np.array_equal(v, GOLD[f"protocol/{k}"]), k
    assert np.array_equal(out, ref.chain(x, size, pre))


def test_restatement_equals_pillow_itself():
    Image = pytest.importorskip("PIL.Image")
    flt = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
    for name, (_, _, shape, (h, w), filt) in ref.CASES.items():
        x = ref.case_input(name)
        for f, want in zip(x, ref.resize(x, (h, w), filt)):
            img = Image.fromarray(f[..., 0], "L") if shape[3] == 1 else Image.fromarray(f, "RGB")
            got = np.asarray(img.resize((w, h), flt[filt]))
            assert np.array_equal(got if shape[3] == 3 else got[..., None], want), name
    f = ref.case_input("down_bicubic")[0]
    img = Image.fromarray(f, "RGB")
    assert np.array_equal(np.asarray(img.resize((20, 11))), ref.resize(f, (11, 20), "bicubic"))       # the default filter is bicubic
    assert np.array_equal(np.asarray(img.resize((131, 97), Image.BICUBIC)), f)                        # equal sizes: a copy


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("sizes", [(640, 320), (360, 240), (320, 384), (240, 224), (1920, 320), (1080, 240), (131, 20), (97, 11),
                                   (20, 53), (11, 37), (200, 77), (7, 1), (1, 5)])
def test_resample_table_equals_the_restatement(sizes, filt):
    n_in, n_out = sizes
    bounds, kk = vi.resample_table(n_in, n_out, filt)
    rb, rw, rk = ref.coefficients(n_in, n_out, filt)
    assert bounds.dtype == kk.dtype == np.int32 and bounds.shape == (n_out, 2)
    assert kk.shape == rk.shape == (n_out, _lib.load().diffsal_resample_ksize(n_in, n_out, vi.FILTERS[filt]))
    assert np.array_equal(bounds, rb) and np.array_equal(kk, rk)
    # the bounds are clamped to the source at both edges, rise with the output index and every count fits the row
    assert bounds[0, 0] == 0 and bounds[-1, 0] + bounds[-1, 1] == n_in
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all() and bounds[:, 1].max() <= kk.shape[1]
    # weights past the count are zero, and a row sums to 2^22 within one unit per tap (each weight is rounded on its own)
    for o in range(n_out):
        assert not kk[o, bounds[o, 1]:].any()
    assert (np.abs(kk.astype(np.int64).sum(axis=1) - (1 << 22)) <= bounds[:, 1]).all()
    assert np.abs(rw.sum(axis=1) - 1.0).max() < 1e-12
    assert np.abs(kk).max() < 2 ** 23      # what the kernel's 24-bit multiply relies on


def test_resample_table_rejects_bad_arguments():
    with pytest.raises(ValueError):
        vi.resample_table(10, 5, "lanczos")
    with pytest.raises(ValueError):
        vi.resample_table(0, 5, "bilinear")
    with pytest.raises(ValueError):
        vi.resample_table(10, 0, "bilinear")


def test_normalize_table_is_the_reference_s_cpu_arithmetic():
    # the audio-visual datasets: ToTensor(norm_value=1), Normalize(mean, std) of R/cfgs/dataset.json, python-float operands
    mean, std = [114.7748, 107.7354, 99.475], [38.7568578, 37.88248729, 40.02898126]
    img = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).repeat(3, 1, 1)
    want = img.float().div(1)
    for t, m, s in zip(want, mean, std):
        t.sub_(m).div_(s)
    got = vi.normalize_table()
    assert got.dtype == torch.float32 and got.shape == (3, 256) and not got.is_cuda
    assert torch.equal(got, want.view(3, 256)) and torch.equal(got, vi.normalize_table(1, mean, std))
    # meta_data.py / dhf1k_data.py: torchvision's ToTensor (/ 255) and Normalize (tensor operands) with the ImageNet statistics
    m = torch.as_tensor([0.485, 0.456, 0.406], dtype=torch.float32)[:, None, None]
    s = torch.as_tensor([0.229, 0.224, 0.225], dtype=torch.float32)[:, None, None]
    want = img.to(torch.float32).div(255).sub_(m).div_(s)
    assert torch.equal(vi.normalize_table(255, vi.IMAGENET_MEAN, vi.IMAGENET_STD), want.view(3, 256))
    assert torch.equal(vi.target_table(), torch.arange(256, dtype=torch.uint8).float().div(255)[None])
    with pytest.raises(ValueError):
        vi.normalize_table(1, [1.0, 2.0], [1.0, 2.0, 3.0])


def test_index_helpers_on_hand_worked_lists():
    # TemporalCenterCrop(16) of 40 indices: centre 20, begin 12
    assert vi.center_crop_indices(list(range(1, 41)), 16) == list(range(13, 29))
    # fewer than `size` indices: the walk over the growing list cycles through it
    assert vi.center_crop_indices([7, 8, 9], 8) == [7, 8, 9, 7, 8, 9, 7, 8]
    assert vi.center_crop_indices([5], 4) == [5, 5, 5, 5]
    # 5 indices, size 4: centre 2, begin 0, end 4
    assert vi.center_crop_indices([1, 2, 3, 4, 5], 4) == [1, 2, 3, 4]
    src = [1, 2, 3]
    vi.center_crop_indices(src, 8)
    assert src == [1, 2, 3]                                   # the caller's list is left alone
    # the median of an even-length list is a half: rounded up, where round() would go to the even neighbour
    assert vi.median_index([1, 2, 3, 4]) == 3 and vi.median_index([3, 4, 5, 6]) == 5 and round(2.5) == 2
    assert vi.median_index(list(range(13, 29))) == 21         # (20 + 21) / 2 = 20.5
    assert vi.median_index([1, 2, 3]) == 2 and vi.median_index([4, 9, 4]) == 4
    assert vi.median_index([7, 8, 9, 7, 8, 9, 7, 8]) == 8     # the loop-padded list is sorted first: (8 + 8) / 2
    assert vi.dhf1k_indices(0, 1, 4) == [1, 2, 3, 4]
    assert vi.dhf1k_indices(10, 2, 16) == [11 + 2 * i for i in range(16)]
    assert vi.dhf1k_indices(10, 2, 32) == [11 + 2 * i for i in range(16)]      # capped at 16 frames


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.diffsal_last_error()      # noqa: E731
    ks = lambda a, b, f: lib.diffsal_resample_ksize(a, b, f)      # noqa: E731
    assert ks(640, 320, 1) == 9 and ks(640, 320, 0) == 5 and ks(20, 53, 1) == 5 and ks(20, 53, 0) == 3 and ks(1920, 320, 1) == 25
    assert ks(640, 320, 2) == 0 and ks(0, 320, 0) == 0

    def call(N=1, H0=97, W0=131, C=3, H1=11, W1=20, filt=1, xks=None, yks=None, form=0, band=0, ws_bytes=0):
        xks = ks(W0, W1, filt) if xks is None else xks
        yks = ks(H0, H1, filt) if yks is None else yks
        return lib.diffsal_resample_u8(None, N, H0, W0, C, H1, W1, filt, None, None, xks, None, None, yks, form, band, None, None, ws_bytes,
                                       None)

    assert call(C=2) == -4 and b"channels" in err()
    assert call(C=4) == -4
    assert call(filt=2) == -4 and b"filter" in err()
    assert call(filt=-1) == -4
    assert call(H1=0) == -1 and call(W0=0) == -1 and call(N=0) == -1 and b"bad shape" in err()
    assert call(xks=7) == -1 and b"coefficients per output column" in err()
    assert call(yks=3) == -1 and b"coefficients per output row" in err()
    assert call(form=3) == -4 and b"form" in err()
    assert call(band=33) == -4 and b"band_rows" in err()
    # the two-pass form keeps the horizontally resampled image [N][H0][W1][C] in the workspace
    need = lib.diffsal_resample_u8_ws_bytes(2, 97, 131, 3, 11, 20, 1, ops.RESAMPLE_TWO_PASS)
    assert need == 2 * 97 * 20 * 3
    assert call(N=2, form=ops.RESAMPLE_TWO_PASS, ws_bytes=need - 1) == -4 and b"workspace too small" in err()
    assert lib.diffsal_resample_u8_ws_bytes(2, 97, 131, 3, 11, 20, 1, ops.RESAMPLE_FUSED) == 0
    assert lib.diffsal_resample_u8_ws_bytes(2, 97, 131, 3, 11, 20, 1, ops.RESAMPLE_AUTO) == 0        # a band fits: the fused form
    assert lib.diffsal_resample_u8_ws_bytes(2, 240, 320, 3, 224, 384, 0, ops.RESAMPLE_AUTO) == 2 * 240 * 384 * 3      # near-unity scale: two passes
    assert lib.diffsal_resample_u8_ws_bytes(2, 360, 640, 3, 240, 320, 1, ops.RESAMPLE_AUTO) == 0
    assert lib.diffsal_resample_u8_ws_bytes(2, 40, 64, 3, 40, 24, 0, ops.RESAMPLE_TWO_PASS) == 0     # a single pass has no intermediate
    assert lib.diffsal_resample_u8_ws_bytes(2, 97, 131, 2, 11, 20, 1, ops.RESAMPLE_TWO_PASS) == 0    # bad C
    # every other argument in order: only the pointers are missing
    assert call() == -4 and b"null argument" in err()
    # a source row too wide for even a one-row band: the fused form refuses, the automatic one asks for the two-pass workspace
    assert lib.diffsal_resample_u8_band_rows(8000, 16000, 3, 240, 320, 1) == 0
    assert call(H0=8000, W0=16000, H1=240, W1=320, form=ops.RESAMPLE_FUSED) == -1 and b"does not fit" in err()
    assert lib.diffsal_resample_u8_ws_bytes(1, 8000, 16000, 3, 240, 320, 1, ops.RESAMPLE_AUTO) == 8000 * 320 * 3
    assert call(H0=8000, W0=16000, H1=240, W1=320, form=ops.RESAMPLE_AUTO) == -4 and b"workspace too small" in err()
    # band heights: within the limits, and a prime number of output rows leaves a part-filled last band
    for args in ((360, 640, 3, 240, 320, 1), (240, 320, 3, 224, 384, 0), (1080, 1920, 3, 240, 320, 1), (200, 64, 3, 77, 32, 1)):
        assert 1 <= lib.diffsal_resample_u8_band_rows(*args) <= 32
    assert 77 % lib.diffsal_resample_u8_band_rows(200, 64, 3, 77, 32, 1) != 0
    assert lib.diffsal_resample_u8_band_rows(40, 64, 3, 40, 24, 0) == 0      # one pass

    def gather(N=4, h=5, w=7, C=3, B=2, T=2):
        return lib.diffsal_clip_gather_u8(None, N, h, w, C, None, B, T, None, None, None)

    assert gather(C=2) == -4 and b"channels" in err()
    assert gather(h=0) == -1 and gather(B=0) == -1
    assert gather(B=3) == -1 and b"without an index table" in err()
    assert gather() == -4 and b"null argument" in err()
    assert isinstance(ctypes.c_int(gather()).value, int)


def test_python_argument_checks():
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        vi.resize_u8(x, (4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        vi.clip_rgb(x, [[0]], (4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        vi.gather_clips(x, [[0]])
    with pytest.raises(RuntimeError, match="GPU only"):
        vi.target_maps(x[..., 0], (4, 4))
    with pytest.raises(ValueError):
        vi.resize_u8(x, (4, 4), "lanczos")
    with pytest.raises(ValueError):
        vi.resize_u8(x, (4, 0))
    with pytest.raises(ValueError):
        vi.resize_u8(x, (4, 4), fused="yes")
