"""The JPEG export on the GPU (csrc/jpeg_export.hip through diff_sal_amd.jpeg): the files and the read-back pixels against the
fixtures recorded from Pillow (tools/gen_jpeg_golden.py) and against the NumPy restatement on every pixel, a live Pillow decode of the
device's bytes, batch independence, determinism on a dirty workspace, guard words behind the output and the workspace, graph capture,
the files on disk, protocol_metrics(quantize="jpeg") against its composition, argument errors.  Every comparison is exact: the
export is integer arithmetic."""
import io
import os

import numpy as np
import pytest
import torch

from diff_sal_amd import _lib, jpeg, ops
from diff_sal_amd import postprocess as pp
from tests import _jpeg_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES, BIG, _ = ref.load_cases()
_BIG = {}      # the full-size input and the restatement's pixels for it, made once


def _big():
    if not _BIG:
        _BIG["u8"] = ref.big_input()
        _BIG["decoded"] = np.stack([ref.decode(img, BIG["quality"]) for img in _BIG["u8"]])
    return _BIG["u8"], _BIG["decoded"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _files(data, lengths):
    data, lengths = data.cpu().numpy(), lengths.cpu().numpy()
    assert data.dtype == np.uint8 and lengths.dtype == np.int32 and data.shape[0] == lengths.shape[0]
    assert (lengths > 0).all() and (lengths <= data.shape[1]).all()
    return [data[b, :n].tobytes() for b, n in enumerate(lengths)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_files_and_read_back_pixels_are_the_fixtures(name):
    c = CASES[name]
    x = _t(c["u8"][None])
    for q, want in c["q"].items():
        data, lengths, dec = jpeg.encode(x, q, return_decoded=True)
        assert data.shape == (1, jpeg.capacity(*c["u8"].shape))
        got = _files(data, lengths)[0]
        assert got == want["file"], (name, q, len(got), len(want["file"]))
        assert _files(*jpeg.encode(x, q))[0] == want["file"], (name, q)      # the launch without the read-back pixels
        rt = jpeg.roundtrip(x, q)
        assert rt.dtype == dec.dtype == torch.uint8 and rt.shape == dec.shape == x.shape
        assert np.array_equal(rt[0].cpu().numpy(), want["decoded"]) and torch.equal(rt, dec), (name, q)
        assert np.array_equal(want["decoded"], ref.decode(c["u8"], q)), (name, q)      # the restatement, every pixel


def test_full_size_batch():
    u8, want = _big()
    x = _t(u8)
    data, lengths, dec = jpeg.encode(x.unsqueeze(1), return_decoded=True)      # [B, 1, H, W] as the sampler returns it
    files = _files(data, lengths)
    assert [len(f) for f in files] == BIG["lengths"]
    assert [ref.sha256(f) for f in files] == BIG["sha256"]
    rt = jpeg.roundtrip(x).cpu().numpy()
    assert np.array_equal(rt[:, BIG["rows"]][:, :, BIG["cols"]], BIG["decoded"])      # Pillow's pixels on the recorded grid
    assert np.array_equal(rt, want) and np.array_equal(dec.cpu().numpy(), want)      # the restatement's on every pixel
    one = [_files(*jpeg.encode(x[b:b + 1]))[0] for b in range(3)]      # an image's bytes do not depend on its batch
    assert one == files


def test_pillow_opens_the_devices_bytes():
    Image = pytest.importorskip("PIL.Image")
    for name in ("r13x21", "s37x50", "bw24x32"):
        x = _t(CASES[name]["u8"][None])
        data, lengths = jpeg.encode(x)
        img = Image.open(io.BytesIO(_files(data, lengths)[0]))
        assert img.mode == "L" and img.size == (x.shape[2], x.shape[1])
        assert np.array_equal(np.asarray(img), jpeg.roundtrip(x)[0].cpu().numpy()), name


def test_an_image_of_a_mixed_batch_has_the_bytes_it_has_alone():
    names = ["r8x8", "padff8x8", "ac10_8x8", "padff8x8"]
    x = _t(np.stack([CASES[n]["u8"] for n in names]))
    data, lengths, dec = jpeg.encode(x, return_decoded=True)
    files = _files(data, lengths)
    for b, n in enumerate(names):
        assert files[b] == CASES[n]["q"][95]["file"], n
        assert np.array_equal(dec[b].cpu().numpy(), CASES[n]["q"][95]["decoded"]), n
    assert files[1] == files[3] and len(set(files)) == 3


def _raw_encode(x, quality, out, cap, lengths, ws, ws_bytes, recon=None):
    B, h, w = x.shape
    _lib.check(_lib.load().diffsal_jpeg_encode(x.data_ptr(), B, h, w, quality, out.data_ptr(), cap, lengths.data_ptr(),
                                               None if recon is None else recon.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream()), "jpeg_encode")


@pytest.mark.parametrize("name", ["bw24x32", "s1x4097"])
def test_dirty_workspace_and_guard_words(name):
    """Two calls into one workspace, which starts full of ones and is then dirty from the first call (the pack ORs into a bit stream
    that must be cleared on every call), give the fixture's bytes both times; the bytes behind `cap` of the last row and behind
    ws_bytes stay as they were."""
    lib = _lib.load()
    c = CASES[name]
    x = _t(np.stack([c["u8"], c["u8"][::-1, ::-1]]))
    B, h, w = x.shape
    cap, nws, guard = lib.diffsal_jpeg_capacity(h, w), lib.diffsal_jpeg_encode_ws_bytes(B, h, w), 256
    assert cap == jpeg.capacity(h, w) == 328 + 2 * ((((h + 7) // 8) * ((w + 7) // 8) * 1658 + 7) // 8) + 4 and nws % 16 == 0
    out = torch.full((B * cap + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((nws + guard,), 0xFF, dtype=torch.uint8, device=DEV)
    lengths = torch.zeros(B, dtype=torch.int32, device=DEV)
    seen = []
    for _ in range(2):
        _raw_encode(x, 95, out, cap, lengths, ws, nws)
        seen.append(_files(out[:B * cap].view(B, cap), lengths))
        assert bool((out[B * cap:] == 0xA5).all()) and bool((ws[nws:] == 0xFF).all())
    assert seen[0] == seen[1] and seen[0][0] == c["q"][95]["file"]
    assert seen[0][1] == ref.encode(np.ascontiguousarray(c["u8"][::-1, ::-1]), 95)
    assert _files(*jpeg.encode(x)) == seen[0]      # and the Python entry point, twice
    assert _files(*jpeg.encode(x)) == seen[0]
    assert torch.equal(jpeg.roundtrip(x), jpeg.roundtrip(x))


def test_graph_capture_and_replay_on_new_data():
    first = np.stack([CASES["r13x21"]["u8"], CASES["r13x21"]["u8"][::-1].copy()])
    second = np.stack([255 - CASES["r13x21"]["u8"], CASES["r13x21"]["u8"][:, ::-1].copy()])
    static = _t(first).clone()
    jpeg.encode(static, return_decoded=True)      # warm-up outside the capture: library load, allocator
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            data, lengths, dec = jpeg.encode(static, return_decoded=True)
            rt = jpeg.roundtrip(static)
    static.copy_(_t(second))
    graph.replay()
    torch.cuda.synchronize()
    assert _files(data, lengths) == [ref.encode(img, 95) for img in second]
    want = np.stack([ref.decode(img, 95) for img in second])
    assert np.array_equal(dec.cpu().numpy(), want) and np.array_equal(rt.cpu().numpy(), want)


def test_save_predictions_writes_the_reference_layout(tmp_path):
    g = torch.Generator(device=DEV).manual_seed(3)
    pred = torch.rand((3, 1, 24, 40), device=DEV, generator=g)
    vids, frames = ["avad/V01", "avad/V01", "0612"], torch.tensor([[7], [8], [120]])
    paths = jpeg.save_predictions(pred, vids, frames, str(tmp_path))
    assert [os.path.relpath(p, str(tmp_path)) for p in paths] == [os.path.join("avad/V01", "pred_sal_000007.jpg"),
                                                                   os.path.join("avad/V01", "pred_sal_000008.jpg"),
                                                                   os.path.join("0612", "pred_sal_000120.jpg")]
    u8 = pp.to_uint8(pred)
    files = _files(*jpeg.encode(u8))
    for b, p in enumerate(paths):
        with open(p, "rb") as f:
            assert f.read() == files[b] == ref.encode(u8[b].cpu().numpy(), 95), b
    with pytest.raises(ValueError, match="video ids"):
        jpeg.save_predictions(pred, vids[:2], frames, str(tmp_path))


def _annotations(B, H, W):
    rng = np.random.default_rng(5)
    fix = np.zeros((B, H * W), dtype=np.uint8)
    other = np.zeros((B, H * W), dtype=np.uint8)
    for b in range(B):
        fix[b, rng.choice(H * W, 60, replace=False)] = 1
        other[b, rng.choice(H * W, 200, replace=False)] = 1
    gt = rng.random((B, H, W), dtype=np.float32)
    return _t(fix.reshape(B, H, W)), _t(gt), _t(other.reshape(B, H, W))


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])) and torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k])), k


@pytest.mark.parametrize("size", [(37, 50), (60, 90)])      # the prediction's own resolution, and a resize in front of the scores
def test_protocol_metrics_on_the_jpeg_map_is_its_composition(size):
    g = torch.Generator(device=DEV).manual_seed(11)
    pred = torch.rand((2, 1, 37, 50), device=DEV, generator=g)
    fix, gt, other = _annotations(2, *size)
    kw = dict(n_rep=3, seed=7, image_ids=[4, 9])
    got = pp.protocol_metrics(pred, fix, gt, other, quantize="jpeg", **kw)
    m = pp.from_uint8(jpeg.roundtrip(pp.to_uint8(pred)))
    _same(got, pp.protocol_metrics(m, fix, gt, other, quantize=False, **kw))
    # quantize=True computes what it computed before this path existed: the 8-bit map, resized, scored
    was = pp.protocol_metrics(pp.from_uint8(pp.to_uint8(pred)), fix, gt, other, quantize=False, **kw)
    _same(pp.protocol_metrics(pred, fix, gt, other, quantize=True, **kw), was)
    _same(pp.protocol_metrics(pred, fix, gt, other, **kw), was)
    assert not torch.equal(got["cc"], was["cc"])      # the JPEG map is another map


def test_argument_errors():
    x = torch.zeros((2, 16, 24), dtype=torch.uint8, device=DEV)
    for q in (0, 101):
        for call in (lambda: jpeg.encode(x, q), lambda: jpeg.roundtrip(x, q), lambda: jpeg.save_predictions(x.float(), [1, 2], [1, 2], "unused", q)):
            with pytest.raises(ValueError, match="quality"):
                call()
    for call in (lambda: jpeg.encode(x[:0]), lambda: jpeg.roundtrip(x[:0]), lambda: jpeg.encode(x[:, :0])):
        with pytest.raises(ValueError, match="non-empty"):
            call()
    for call in (lambda: jpeg.encode(x.float()), lambda: jpeg.roundtrip(x.to(torch.int32))):
        with pytest.raises(ValueError, match="uint8"):
            call()
    with pytest.raises(RuntimeError, match="GPU only"):
        jpeg.encode(x.cpu())
    f = torch.zeros((2, 16, 24), dtype=torch.uint8, device=DEV)
    for bad in ("png", "JPEG", None, 2):
        with pytest.raises(ValueError, match="quantize"):
            pp.protocol_metrics(x.float(), f, quantize=bad)
    # the C entry points check for themselves, before any launch
    lib = _lib.load()
    cap, nws = lib.diffsal_jpeg_capacity(16, 24), lib.diffsal_jpeg_encode_ws_bytes(2, 16, 24)
    out = torch.zeros((2, cap), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((nws + 16,), dtype=torch.uint8, device=DEV)
    n = torch.zeros(2, dtype=torch.int32, device=DEV)
    for args, text in (((x, 0, out, cap, n, ws, nws), "quality"), ((x, 95, out, cap - 1, n, ws, nws), "cap"),
                       ((x, 95, out, cap, n, ws, nws - 16), "workspace"), ((x, 95, out, cap, n, ws[1:], nws), "misaligned")):
        with pytest.raises(RuntimeError, match=text):
            _raw_encode(*args)
    assert lib.diffsal_jpeg_capacity(0, 8) == 0 and lib.diffsal_jpeg_capacity(8, 65536) == 0 and lib.diffsal_jpeg_encode_ws_bytes(0, 8, 8) == 0
