"""The JPEG decode on the GPU (csrc/jpeg_decode.hip through diff_sal_amd.jpeg.decode) against the fixtures recorded from Pillow
(tools/gen_jpeg_decode_golden.py): every case alone and in one call with the cases of its shape group, both modes; the export's own
files against ``roundtrip``; the video front end on decoded frames; sentinels around the output and the workspace; three damaged
files (each decoded first by tools/jpeg_decode_host_check.cpp under a sanitizer) next to intact ones; the GPU-only guard.  Every
comparison is exact: the decode is integer arithmetic."""
import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, jpeg, ops, video_input
from tests import _jpeg_decode_ref as ref
from tests import _jpeg_ref as export_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES, _, DAMAGED = ref.load_cases()
GROUPS = ref.groups(CASES)


@pytest.mark.parametrize("key", sorted(GROUPS), ids=lambda k: "{}x{}_c{}_{}x{}".format(*k))
def test_decode_is_the_fixture_alone_and_in_its_group(key):
    names = GROUPS[key]
    for mode, field in (("RGB", "rgb"), ("L", "l")):
        want = np.stack([CASES[n][field] for n in names])
        both = jpeg.decode([CASES[n]["file"] for n in names], mode=mode)
        assert both.dtype == torch.uint8 and both.is_cuda and tuple(both.shape) == want.shape
        assert np.array_equal(both.cpu().numpy(), want), (names, mode)
        for i, n in enumerate(names):      # batch independence: alone, the same bits
            alone = jpeg.decode([bytearray(CASES[n]["file"])], mode=mode)
            assert torch.equal(alone[0], both[i]), (n, mode)


@pytest.mark.parametrize("shape,quality", [((13, 21), 95), ((40, 72), 30)])
def test_decode_of_the_exports_files_is_roundtrip(shape, quality):
    rng = np.random.default_rng(shape[0])
    u8 = torch.from_numpy(rng.integers(0, 256, size=(3,) + shape, dtype=np.uint8)).to(DEV)
    data, lengths = jpeg.encode(u8, quality)
    data, lengths = data.cpu().numpy(), lengths.cpu().numpy()
    files = [data[b, :n].tobytes() for b, n in enumerate(lengths)]
    got = jpeg.decode(files, mode="L")
    assert torch.equal(got, jpeg.roundtrip(u8, quality))
    assert np.array_equal(got[0].cpu().numpy(), export_ref.decode(u8[0].cpu().numpy(), quality))
    rgb = jpeg.decode(files, mode="RGB")      # one component: R = G = B = y
    assert torch.equal(rgb, got[..., None].expand(-1, -1, -1, 3))


def test_video_front_end_on_decoded_frames(tmp_path):
    names = GROUPS[(37, 53, 3, 2, 2)]
    paths = []
    for i, n in enumerate(names):
        paths.append(tmp_path / f"img_{i + 1:05d}.jpg")
        paths[-1].write_bytes(CASES[n]["file"])
    frames = jpeg.decode_files(paths)
    pillow = torch.from_numpy(np.stack([CASES[n]["rgb"] for n in names])).to(DEV)
    kw = dict(size=(28, 48), pre_size=(30, 40))
    assert torch.equal(video_input.transform_frames(frames, **kw), video_input.transform_frames(pillow, **kw))
    maps = jpeg.decode([CASES[n]["file"] for n in names], mode="L")
    pillow_l = torch.from_numpy(np.stack([CASES[n]["l"] for n in names])).to(DEV)
    assert torch.equal(video_input.target_maps(maps, size=(28, 48)), video_input.target_maps(pillow_l, size=(28, 48)))


def _raw_decode(p, buf, mode_l, out, status, ws, nws):
    N, nseg = p["N"], p["nseg"]
    _lib.check(_lib.load().diffsal_jpeg_decode(buf.data_ptr(), p["desc_at"], buf[p["desc_at"]:].data_ptr(), buf[p["seg_at"]:].data_ptr(), nseg,
                                               p["max_file_seg"], N, p["H"], p["W"], p["ncomp"], p["hs"], p["vs"], mode_l, out.data_ptr(),
                                               status.data_ptr(), ws.data_ptr(), nws, ops._stream()), "jpeg_decode")


@pytest.mark.parametrize("key,mode_l", [((37, 53, 3, 2, 2), 0), ((33, 48, 3, 2, 1), 0), ((33, 48, 3, 2, 1), 1), ((17, 33, 1, 1, 1), 1),
                                        ((120, 160, 3, 2, 1), 0)])
def test_sentinels_around_the_output_and_the_workspace(key, mode_l):
    """The output inside a larger allocation filled with a sentinel, the workspace of exactly the reported size likewise: both
    sentinels intact, the pixels the fixture's, twice into the same (then dirty) workspace.  33 x 48 takes the 16-byte stores."""
    lib = _lib.load()
    names = GROUPS[key]
    p = jpeg.pack([CASES[n]["file"] for n in names])
    buf = torch.from_numpy(p["host"]).to(DEV)
    N, H, W = p["N"], p["H"], p["W"]
    nws = lib.diffsal_jpeg_decode_ws_bytes(N, H, W, p["ncomp"], p["hs"], p["vs"])
    assert nws > 0 and nws % 16 == 0
    n_out, guard = N * H * W * (1 if mode_l else 3), 256
    big = torch.full((guard + n_out + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((guard + nws + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.full((N + 2,), -7, dtype=torch.int32, device=DEV)
    want = np.stack([CASES[n]["l" if mode_l else "rgb"] for n in names]).ravel()
    for _ in range(2):
        _raw_decode(p, buf, mode_l, big[guard:], status[1:], ws[guard:], nws)
        assert np.array_equal(big[guard:guard + n_out].cpu().numpy(), want)
        assert bool((big[:guard] == 0xA5).all()) and bool((big[guard + n_out:] == 0xA5).all())
        assert bool((ws[:guard] == 0x5A).all()) and bool((ws[guard + nws:] == 0x5A).all())
        assert status.tolist() == [-7] + [0] * N + [-7]


def test_damaged_files_next_to_intact_ones():
    good, other = CASES["16x16_420_base"], CASES["16x16_420_noise"]
    files = [good["file"], DAMAGED["cut"], other["file"], DAMAGED["zeroed"], DAMAGED["ff"]]
    for mode, field in (("RGB", "rgb"), ("L", "l")):
        frames, status = jpeg.decode(files, mode=mode, strict=False)
        status = status.cpu().tolist()
        assert status[0] == 0 and status[2] == 0 and all(status[i] != 0 for i in (1, 3, 4)), status
        assert all(0 < status[i] < 8 for i in (1, 3, 4))
        assert np.array_equal(frames[0].cpu().numpy(), good[field]) and np.array_equal(frames[2].cpu().numpy(), other[field])
    with pytest.raises(ValueError, match=r"3 of 5 files are damaged inside their scan \(file 1: .*file 3: .*file 4: "):
        jpeg.decode(files)
    assert torch.equal(jpeg.decode([good["file"], other["file"]], strict=True), frames.new_tensor(np.stack([good["rgb"], other["rgb"]])))


def test_argument_errors():
    good = CASES["16x16_420_base"]["file"]
    for call in (lambda: jpeg.decode([good], device="cpu"), lambda: jpeg.decode(torch.zeros(4, dtype=torch.uint8)),
                 lambda: jpeg.decode([torch.zeros(4, dtype=torch.uint8, device=DEV)])):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(ValueError, match="empty list"):
        jpeg.decode([])
    # the C entry point checks for itself, before any launch
    lib = _lib.load()
    p = jpeg.pack([good])
    buf = torch.from_numpy(p["host"]).to(DEV)
    nws = lib.diffsal_jpeg_decode_ws_bytes(1, 16, 16, 3, 2, 2)
    out = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(nws + 16, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_decode(p, buf, 0, out, status, ws, nws - 16)
    with pytest.raises(RuntimeError, match="misaligned"):
        _raw_decode(p, buf, 0, out, status, ws[1:], nws)
    with pytest.raises(RuntimeError, match="mode_l"):
        _raw_decode(p, buf, 2, out, status, ws, nws)
    with pytest.raises(RuntimeError, match="luma sampling"):
        _raw_decode(dict(p, hs=1, vs=2), buf, 0, out, status, ws, nws)
    for bad in ((0, 16, 16, 3, 2, 2), (1, 0, 16, 3, 2, 2), (1, 16, 65536, 3, 2, 2), (1, 16, 16, 2, 1, 1), (1, 16, 16, 1, 2, 2), (1, 16, 16, 3, 1, 2)):
        assert lib.diffsal_jpeg_decode_ws_bytes(*bad) == 0
