"""The PNG decode on the GPU (csrc/png_decode.hip through diff_sal_amd.png.decode) against the fixtures recorded from Pillow
(tools/gen_png_decode_golden.py): every case alone and in one call with the cases of its shape group, both modes; sentinels around
the output, the workspace and the status; damaged files (each decoded first by tools/png_decode_host_check.cpp under a sanitizer)
next to intact ones; the video front end and the protocol's read-back on decoded frames; the C entry point's own argument errors;
graph capture.  Every comparison is exact: the decode is integer arithmetic.

``16x16_hand_rgb_overlap`` (matches with distance < length at 1, 2, 3), ``120x160_hand_rgb_far`` (a match at distance 32768) and the
fixed-code files Pillow writes for flat content are the regression guard of the wave's match copy: with the table build compiled
as an out-of-line device function these files lost the bytes that lanes 0-31 copy (csrc/png_decode_core.h, at PNG_DEV).  They are
decoded by ``test_decode_is_the_fixture_alone_and_in_its_group[16x16]`` and ``[120x160]`` and named again in
``test_the_match_copy_guard_files_are_in_the_fixture``."""
import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, ops, png, postprocess, video_input
from tests import _png_decode_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES, _, DAMAGED = ref.load_cases()
GROUPS = ref.groups(CASES)
SHAPES = sorted({k[:2] for k in GROUPS})


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_decode_is_the_fixture_alone_and_in_its_group(shape):
    for key in sorted(k for k in GROUPS if k[:2] == shape):
        names = GROUPS[key]
        for mode, field in (("RGB", "rgb"), ("L", "l")):
            want = np.stack([CASES[n][field] for n in names])
            both = png.decode([CASES[n]["file"] for n in names], mode=mode)
            assert both.dtype == torch.uint8 and both.is_cuda and tuple(both.shape) == want.shape
            assert np.array_equal(both.cpu().numpy(), want), (names, mode)
            for i, n in enumerate(names):      # batch independence: alone, the same bits
                alone = png.decode([bytearray(CASES[n]["file"])], mode=mode)
                assert torch.equal(alone[0], both[i]), (n, mode)


def test_the_match_copy_guard_files_are_in_the_fixture():
    for name in ("16x16_hand_rgb_overlap", "120x160_hand_rgb_far"):
        c = CASES[name]
        for mode, field in (("RGB", "rgb"), ("L", "l")):
            assert np.array_equal(png.decode([c["file"]], mode=mode)[0].cpu().numpy(), c[field]), (name, mode)


def _raw_decode(p, buf, mode_l, out_t, status_t, ws_t, nws, **over):
    """the C entry point on tensors; ``over`` replaces single arguments (a pointer as an integer or None)"""
    a = dict(N=p["N"], H=p["H"], W=p["W"], color_type=p["color_type"], bit_depth=p["bit_depth"], bytes=buf.data_ptr(), nbytes=p["desc_at"],
             files=buf[p["desc_at"]:].data_ptr(), out=out_t.data_ptr(), status=status_t.data_ptr(), ws=ws_t.data_ptr())
    a.update(over)
    _lib.check(_lib.load().diffsal_png_decode(a["bytes"], a["nbytes"], a["files"], a["N"], a["H"], a["W"], a["color_type"], a["bit_depth"], mode_l,
                                              a["out"], a["status"], a["ws"], nws, ops._stream()), "png_decode")


@pytest.mark.parametrize("key,mode_l", [((17, 33, 3, 4), 0), ((17, 33, 3, 4), 1), ((33, 48, 2, 8), 0), ((33, 48, 2, 8), 1), ((65, 70, 6, 8), 0),
                                        ((130, 9, 0, 8), 1), ((130, 9, 0, 8), 0), ((120, 160, 2, 8), 0), ((120, 160, 6, 8), 1)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sentinels_around_the_output_the_workspace_and_the_status(key, mode_l):
    """The output inside a larger allocation filled with a sentinel, the workspace of exactly the reported size likewise: the
    sentinels intact, the pixels the fixture's, twice into the same (then dirty) workspace."""
    lib = _lib.load()
    names = GROUPS[key]
    p = png.pack([CASES[n]["file"] for n in names])
    buf = torch.from_numpy(p["host"]).to(DEV)
    N, H, W = p["N"], p["H"], p["W"]
    nws = lib.diffsal_png_decode_ws_bytes(N, H, W, p["color_type"], p["bit_depth"])
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
    base = DAMAGED["cut"][1]
    good = CASES[base]
    others = [n for n in GROUPS[(good["H"], good["W"], good["color_type"], good["bit_depth"])] if n != base]
    order = ["cut", "zeroed", "adler", "far", "type3", "short", "long"]
    files, intact = [], {}
    for i, name in enumerate(order):      # intact, damaged, intact, damaged, ...
        n = ([base] + others)[i % (1 + len(others))]
        intact[len(files)] = CASES[n]
        files += [CASES[n]["file"], DAMAGED[name][0]]
    for mode, field in (("RGB", "rgb"), ("L", "l")):
        frames, status = png.decode(files, mode=mode, strict=False)
        status = status.cpu().tolist()
        for at, c in intact.items():
            assert status[at] == 0 and np.array_equal(frames[at].cpu().numpy(), c[field]), at
        for i, name in enumerate(order):
            got, bit = status[2 * i + 1], DAMAGED[name][2]
            assert got != 0 and got & bit == bit and 0 < got < 1024, (name, got, bit)
            assert got == ref.decode(DAMAGED[name][0])[2], name      # the restatement stops where the device stops
        # a stream that is one row long still delivers its pixels
        rgb, lum, _ = ref.decode(DAMAGED["long"][0])
        assert np.array_equal(frames[2 * order.index("long") + 1].cpu().numpy(), rgb if mode == "RGB" else lum)
    with pytest.raises(ValueError, match=r"7 of 14 files are damaged inside their stream \(file 1: the stream's bits ran out.*file 3: .*"
                                         r"file 5: an Adler-32 mismatch; file 7: a distance that reaches before the start of the output.*"
                                         r"file 9: an invalid block type.*file 11: the stream ended with fewer bytes than the image needs; "
                                         r"file 13: the stream carries more bytes than the image needs"):
        png.decode(files)
    two = png.decode([good["file"], CASES[others[0]]["file"]], strict=True)
    assert np.array_equal(two.cpu().numpy(), np.stack([good["rgb"], CASES[others[0]]["rgb"]]))


def test_video_front_end_on_decoded_frames(tmp_path):
    names = GROUPS[(33, 48, 2, 8)]
    paths = []
    for i, n in enumerate(names):
        paths.append(tmp_path / f"{i + 1}.png")
        paths[-1].write_bytes(CASES[n]["file"])
    frames = png.decode_files(paths)
    pillow = torch.from_numpy(np.stack([CASES[n]["rgb"] for n in names])).to(DEV)
    kw = dict(size=(28, 48), pre_size=(30, 40))
    assert torch.equal(video_input.transform_frames(frames, **kw), video_input.transform_frames(pillow, **kw))
    maps = png.decode([CASES[n]["file"] for n in GROUPS[(33, 48, 0, 8)]], mode="L")
    pillow_l = torch.from_numpy(np.stack([CASES[n]["l"] for n in GROUPS[(33, 48, 0, 8)]])).to(DEV)
    assert torch.equal(video_input.target_maps(maps, size=(28, 48)), video_input.target_maps(pillow_l, size=(28, 48)))


def test_read_back_of_maps_is_byte_over_255():
    names = GROUPS[(65, 70, 0, 8)]
    maps = png.decode([CASES[n]["file"] for n in names], mode="L")
    want = np.stack([CASES[n]["l"] for n in names]).astype(np.float32) / np.float32(255)
    assert np.array_equal(postprocess.from_uint8(maps).cpu().numpy(), want)


def test_saved_predictions_read_back_are_to_uint8s_bytes(tmp_path):
    pytest.importorskip("PIL.Image")
    g = torch.Generator(device="cpu").manual_seed(3)
    pred = torch.rand((3, 1, 36, 52), generator=g).to(DEV)
    paths = postprocess.save_predictions(pred, ["v1", "v1", "v2"], [1, 2, 1], str(tmp_path))
    got = png.decode_files(paths, mode="L")
    assert torch.equal(got, postprocess.to_uint8(pred))


def test_the_entry_point_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    names = GROUPS[(16, 16, 2, 8)][:1]
    p = png.pack([CASES[n]["file"] for n in names])
    buf = torch.from_numpy(p["host"]).to(DEV)
    nws = lib.diffsal_png_decode_ws_bytes(1, 16, 16, 2, 8)
    out = torch.full((16 * 16 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(nws + 16, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    for over, message, small in ((dict(N=0), "N=0", 0), (dict(H=0), "0 x 16", 0), (dict(W=8193), "16 x 8193", 0), (dict(W=-1), "16 x -1", 0),
                                 (dict(color_type=2, bit_depth=4), "colour type 2 at 4 bits", 0), (dict(color_type=5), "colour type 5", 0),
                                 (dict(bit_depth=16), "at 16 bits", 0), ({}, "workspace too small", 16), (dict(bytes=None), "null", 0),
                                 (dict(files=None), "null", 0), (dict(out=None), "null", 0), (dict(status=None), "null", 0),
                                 (dict(ws=None), "null", 0), (dict(nbytes=p["desc_at"] - 1), "multiple of 16", 0),
                                 (dict(ws=ws[1:].data_ptr()), "misaligned", 0)):
        with pytest.raises(RuntimeError, match=message):
            _raw_decode(p, buf, 0, out, status, ws, nws - small, **over)
    with pytest.raises(RuntimeError, match="mode_l"):
        _raw_decode(p, buf, 2, out, status, ws, nws)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and status.tolist() == [-7]      # nothing was launched
    for bad in ((0, 16, 16, 2, 8), (1, 0, 16, 2, 8), (1, 16, 8193, 2, 8), (65536, 16, 16, 2, 8), (1, 65536, 16, 2, 8), (1, 16, 16, 2, 4),
                (1, 16, 16, 4, 2), (1, 16, 16, 6, 1), (1, 16, 16, 1, 8), (1, 16, 16, 0, 16), (1, 16, 16, 0, 3)):
        assert lib.diffsal_png_decode_ws_bytes(*bad) == 0, bad
    _raw_decode(p, buf, 0, out, status, ws, nws)
    assert np.array_equal(out.cpu().numpy(), CASES[names[0]]["rgb"].ravel()) and status.tolist() == [0]


def test_a_captured_call_replays_to_the_same_pixels():
    names = GROUPS[(33, 48, 2, 8)]
    p = png.pack([CASES[n]["file"] for n in names])
    buf = torch.from_numpy(p["host"]).to(DEV)
    N, at = p["N"], p["desc_at"]
    args = (buf[:at], buf[at:].view(N, png.FILE_DTYPE.itemsize), N, p["H"], p["W"], p["color_type"], p["bit_depth"], False)
    warm, _ = ops.png_decode(*args)
    want = np.stack([CASES[n]["rgb"] for n in names])
    assert np.array_equal(warm.cpu().numpy(), want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frames, status = ops.png_decode(*args)
    frames.zero_()
    status.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), want) and status.tolist() == [0] * N
