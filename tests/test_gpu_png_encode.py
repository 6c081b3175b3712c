"""The PNG export on the GPU (csrc/png_encode.hip through diff_sal_amd.png.encode) against the files of the NumPy restatement
(tools/gen_png_encode_golden.py -> tests/golden/png_encode.npz): every case alone and in one call with the cases of its shape; the
round trip through the device's own decode; full-size maps read back by Pillow and by the decode; dirty buffers of exactly the
reported sizes with guards behind them; repeatability; graph capture; save_predictions; the entry point's argument checks.  Every
comparison is exact."""
import io

import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, ops, png, postprocess
from tests import _png_encode_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES, _ = ref.load_cases()
SHAPES = sorted({c["img"].shape for c in CASES.values()})


def _files(data, lengths):
    n = lengths.cpu().numpy()
    host = data.cpu().numpy()
    return [host[b, :int(n[b])].tobytes() for b in range(len(n))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_files_are_the_fixture_alone_and_with_the_cases_of_their_shape(shape):
    names = sorted(n for n, c in CASES.items() if c["img"].shape == shape)
    batch = torch.from_numpy(np.stack([CASES[n]["img"] for n in names])).to(DEV)
    data, lengths = png.encode(batch)
    assert data.dtype == torch.uint8 and lengths.dtype == torch.int32 and data.is_cuda and lengths.is_cuda
    assert tuple(data.shape) == (len(names), png.capacity(*shape)) and tuple(lengths.shape) == (len(names),)
    together = _files(data, lengths)
    for i, n in enumerate(names):
        assert together[i] == CASES[n]["file"], n
        alone = _files(*png.encode(batch[i:i + 1].unsqueeze(1)))      # [1, 1, H, W]: batch independence, the same bytes
        assert alone == [CASES[n]["file"]], n
    # the round trip stays on the device until the comparison
    back = png.decode(together, mode="L")
    assert torch.equal(back, batch)


def test_full_size_maps_read_back_by_pillow_and_by_the_decode():
    Image = pytest.importorskip("PIL.Image")
    maps = np.stack([ref.saliency_like(40 + k, 224, 384, noise=(0, 0, 6, 0)[k]) for k in range(4)])
    batch = torch.from_numpy(maps).to(DEV)
    data, lengths = png.encode(batch)
    assert int(lengths.max()) <= png.capacity(224, 384) and int(lengths.min()) > 57
    files = _files(data, lengths)
    for k, f in enumerate(files):
        im = Image.open(io.BytesIO(f))
        assert im.mode == "L" and np.array_equal(np.asarray(im), maps[k]), k
    assert torch.equal(png.decode(files, mode="L"), batch)
    assert files[0] == ref.encode(maps[0])      # six segments


def _raw_encode(u8, data, lengths, ws, nws, /, **over):
    """the C entry point on tensors; ``over`` replaces single arguments (a pointer as an integer or None)"""
    B, H, W = u8.shape
    a = dict(u8=u8.data_ptr(), B=B, H=H, W=W, data=data.data_ptr(), cap=png.capacity(H, W), lengths=lengths.data_ptr(), ws=ws.data_ptr(), nws=nws)
    a.update(over)
    _lib.check(_lib.load().diffsal_png_encode(a["u8"], a["B"], a["H"], a["W"], a["data"], a["cap"], a["lengths"], a["ws"], a["nws"], ops._stream()),
               "png_encode")


@pytest.mark.parametrize("shape", [(1, 1), (17, 33), (113, 144), (130, 130), (120, 160), (2, 8192)], ids=lambda s: "{}x{}".format(*s))
def test_dirty_buffers_of_the_reported_sizes_with_guards_behind(shape):
    lib = _lib.load()
    names = sorted(n for n, c in CASES.items() if c["img"].shape == shape)
    batch = torch.from_numpy(np.stack([CASES[n]["img"] for n in names])).to(DEV)
    B, (H, W) = len(names), shape
    cap, nws, guard = png.capacity(H, W), lib.diffsal_png_encode_ws_bytes(B, H, W), 256
    assert nws > 0 and nws % 16 == 0 and cap % 16 == 0
    clean, clean_len = png.encode(batch)
    data = torch.full((guard + B * cap + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((guard + nws + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((4 + B + 4,), -1515870811, dtype=torch.int32, device=DEV)      # 0xA5A5A5A5
    for _ in range(2):      # the second time into the workspace the first left behind
        _raw_encode(batch, data[guard:], lengths[4:], ws[guard:], nws)
        got = data[guard:guard + B * cap].view(B, cap)
        assert torch.equal(lengths[4:4 + B], clean_len)
        assert _files(got, lengths[4:4 + B]) == [CASES[n]["file"] for n in names] == _files(clean, clean_len)
        assert bool((data[:guard] == 0xA5).all()) and bool((data[guard + B * cap:] == 0xA5).all())
        assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + nws:] == 0xA5).all())
        assert bool((lengths[:4] == -1515870811).all()) and bool((lengths[4 + B:] == -1515870811).all())


def test_two_runs_give_the_same_bytes():
    batch = torch.from_numpy(np.stack([ref.saliency_like(50 + k, 120, 160, noise=4 * k) for k in range(3)])).to(DEV)
    a, na = png.encode(batch)
    b, nb = png.encode(batch)
    assert torch.equal(na, nb) and torch.equal(a, b)      # whole rows: zeros behind the files


def test_a_captured_call_replays_on_new_pixels():
    first = np.stack([ref.saliency_like(60 + k, 64, 70) for k in range(2)])
    second = np.stack([ref.saliency_like(70 + k, 64, 70, noise=8) for k in range(2)])
    u8 = torch.from_numpy(first).to(DEV)
    warm = _files(*png.encode(u8))
    assert warm == [ref.encode(m) for m in first]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        data, lengths = png.encode(u8)
    u8.copy_(torch.from_numpy(second).to(DEV))
    data.fill_(0xA5)
    lengths.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert _files(data, lengths) == [ref.encode(m) for m in second]


def test_save_predictions(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    g = torch.Generator(device="cpu").manual_seed(3)
    pred = torch.rand((3, 1, 36, 52), generator=g).to(DEV)
    paths = png.save_predictions(pred, ["v1", "v1", "v2"], torch.tensor([1, 2, 1]), str(tmp_path))
    assert [str(p) for p in paths] == [str(tmp_path / "v1" / "1.png"), str(tmp_path / "v1" / "2.png"), str(tmp_path / "v2" / "1.png")]
    want = postprocess.to_uint8(pred)
    pillow = np.stack([np.asarray(Image.open(p)) for p in paths])
    assert np.array_equal(pillow, want.cpu().numpy())
    assert torch.equal(png.decode_files(paths, mode="L"), want)
    with pytest.raises(ValueError, match="3 predictions, 2 video ids, 3 frame ids"):
        png.save_predictions(pred, ["v1", "v2"], [1, 2, 3], str(tmp_path / "none"))
    assert not (tmp_path / "none").exists()


def test_argument_errors_of_the_python_entry():
    with pytest.raises(ValueError, match="uint8"):
        png.encode(torch.zeros(1, 8, 8, device=DEV))
    for shape in ((8, 8), (1, 2, 8, 8), (0, 8, 8)):
        with pytest.raises(ValueError, match=r"\[B, 1, H, W\] or \[B, H, W\]"):
            png.encode(torch.zeros(shape, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="8192 columns"):
        png.encode(torch.zeros((1, 1, 8193), dtype=torch.uint8, device=DEV))


def test_the_entry_point_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    u8 = torch.from_numpy(CASES["17x33_smooth"]["img"][None]).to(DEV)
    cap, nws = png.capacity(17, 33), lib.diffsal_png_encode_ws_bytes(1, 17, 33)
    data = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((nws + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    for over, message in ((dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(H=0), "0 x 33"), (dict(H=65536), "65536 x 33"), (dict(W=0), "17 x 0"),
                          (dict(W=8193), "17 x 8193"), (dict(u8=None), "null"), (dict(data=None), "null"), (dict(lengths=None), "null"),
                          (dict(ws=None), "null"), (dict(cap=cap - 16), "cap"), (dict(cap=cap + 8), "multiple of 16"),
                          (dict(nws=nws - 16), "workspace too small"), (dict(ws=ws[1:].data_ptr()), "misaligned"),
                          (dict(data=data[4:].data_ptr()), "misaligned"), (dict(lengths=lengths.data_ptr() + 2), "misaligned")):
        with pytest.raises(RuntimeError, match=message):
            _raw_encode(u8, data, lengths, ws, nws, **over)
    torch.cuda.synchronize()
    assert bool((data == 0xA5).all()) and bool((ws == 0xA5).all()) and lengths.tolist() == [-7, -7]      # nothing was launched
    for bad in ((0, 17, 33), (1, 0, 33), (1, 17, 0), (65536, 17, 33), (1, 65536, 33), (1, 17, 8193)):
        assert lib.diffsal_png_encode_ws_bytes(*bad) == 0, bad
    assert lib.diffsal_png_encode_capacity(0, 33) == 0 and lib.diffsal_png_encode_capacity(17, 8193) == 0
    _raw_encode(u8, data, lengths, ws, nws)
    assert _files(data[:cap].view(1, cap), lengths[:1]) == [CASES["17x33_smooth"]["file"]] and lengths.tolist()[1] == -7
