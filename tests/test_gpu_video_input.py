"""The video front end on the GPU (csrc/video_input.hip through diff_sal_amd.video_input): Pillow's 8-bit resize in its fused and
its two-pass form against the outputs recorded from Pillow (tools/gen_video_input_golden.py) and against each other, the clip
gather against indexing the look-up table on the CPU, the target path, determinism, graph capture and the features MViT makes
of the result.

Every comparison is ``torch.equal`` / ``np.array_equal``: the resample is integer arithmetic and the normalisation a look-up,
so no tolerance is needed.  The shapes are the smallest at which each mechanism can still go wrong (a scale of about 9 with
dozens of taps and odd byte widths; an upscale whose bounds are clamped at both edges; one axis unchanged; equal sizes; one
channel; three frames; 77 output rows, a prime, so the last LDS band is part-filled); the protocol-size chain runs once."""
import numpy as np
import pytest
import torch

from diff_sal_amd import video_input as vi
from tests import _video_input_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = ref.load_golden()
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _case(name):
    """(input on the host, the same on the device, Pillow's output)"""
    def make():
        x = ref.case_input(name)
        assert ref.crc(x) == int(GOLD[f"crc/{name}"])
        return x, torch.from_numpy(x).to(DEV), GOLD[f"{name}/out"]
    return _memo(("case", name), make)


def _both_forms(x_dev, size, filt, **kw):
    """the resize in its fused and its two-pass form; the two must be the same bytes"""
    fused = vi.resize_u8(x_dev, size, filt, fused=True, **kw)
    two = vi.resize_u8(x_dev, size, filt, fused=False)
    assert fused.dtype == two.dtype == torch.uint8 and fused.is_contiguous() and two.is_contiguous()
    assert torch.equal(fused, two), "the fused and the two-pass form differ"
    return fused


# ------------------------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_resize_equals_pillow_in_both_forms(name):
    _, _, shape, size, filt = ref.CASES[name]
    x, xd, want = _case(name)
    keep = xd.clone()
    got = _both_forms(xd, size, filt)
    assert tuple(got.shape) == (shape[0],) + size + (shape[3],)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(vi.resize_u8(xd, size, filt).cpu(), got.cpu())          # the form the package picks
    assert torch.equal(xd, keep)                                               # the input is not modified


@pytest.mark.parametrize("band", [1, 3, 4, 13])
def test_strong_downscale_over_several_bands(band):
    """11 output rows in bands of 1, 3, 4 rows (a part-filled last band) and in one band: each band spans dozens of source rows
    and neighbouring bands redo the rows they share"""
    for name in ("down_bicubic", "down_blocks_bicubic", "down_bilinear"):
        _, _, _, size, filt = ref.CASES[name]
        _, xd, want = _case(name)
        assert np.array_equal(_both_forms(xd, size, filt, band=band).cpu().numpy(), want)


def test_band_boundaries_with_a_prime_number_of_rows():
    """200 x 64 -> 77 x 32: the band height the library picks does not divide 77, so the last band is part-filled; also with the
    heights it picks at the protocol sizes"""
    _, _, shape, size, filt = ref.CASES["bands"]
    _, xd, want = _case("bands")
    picked = vi.band_rows(shape[1:3], size, 3, filt)
    assert 1 <= picked < 77 and 77 % picked != 0
    others = {vi.band_rows((360, 640), (240, 320), 3, "bicubic"), vi.band_rows((1080, 1920), (240, 320), 3, "bicubic"),
              vi.band_rows((240, 320), (224, 384), 3, "bilinear")}
    print("band rows picked:", picked, "at the protocol sizes:", sorted(others))
    for band in sorted({picked} | others):
        assert band >= 1
        assert np.array_equal(_both_forms(xd, size, filt, band=band).cpu().numpy(), want), band


def test_equal_sizes_are_a_copy_and_one_axis_runs_one_pass():
    x, xd, _ = _case("x_only")
    for filt in ("bilinear", "bicubic"):
        same = _both_forms(xd, x.shape[1:3], filt)
        assert torch.equal(same, xd) and same.data_ptr() != xd.data_ptr()
    # an axis that keeps its size is not filtered: the result is the restatement's single pass, not a pass with unit weights
    assert np.array_equal(_both_forms(xd, (40, 24), "bicubic").cpu().numpy(), ref.resize(x, (40, 24), "bicubic"))
    assert np.array_equal(_both_forms(xd, (16, 64), "bilinear").cpu().numpy(), ref.resize(x, (16, 64), "bilinear"))


def test_single_channel_forms():
    """[N, H, W] is taken as one channel and comes back so; an upscale of it has an odd row width (53 bytes)"""
    x, xd, want = _case("gray")
    got = vi.resize_u8(xd[..., 0], (24, 40), "bilinear", fused=True)
    assert tuple(got.shape) == (1, 24, 40) and np.array_equal(got.cpu().numpy(), want[..., 0])
    small = torch.from_numpy(ref.noise((2, 11, 20, 1), 21)).to(DEV)
    assert np.array_equal(_both_forms(small, (37, 53), "bicubic").cpu().numpy(), ref.resize(small.cpu().numpy(), (37, 53), "bicubic"))


def test_an_unaligned_frame_pointer_takes_the_head_and_tail_paths():
    """a view that starts 1, 5 and 18 bytes into a 16-byte line: the 16-byte loads of the fused form begin after a head"""
    x, _, _ = _case("down_bicubic")
    flat = torch.zeros(x.size + 64, dtype=torch.uint8, device=DEV)
    want = GOLD["down_bicubic/out"]
    for off in (1, 5, 18):
        flat[off:off + x.size] = torch.from_numpy(x).to(DEV).view(-1)
        view = flat[off:off + x.size].view(x.shape)
        assert view.data_ptr() % 16 == off % 16 and view.is_contiguous()
        assert np.array_equal(_both_forms(view, (11, 20), "bicubic").cpu().numpy(), want), off


def test_protocol_chain_equals_pillow():
    """360 x 640 -> 240 x 320 bicubic (the loader) -> 224 x 384 bilinear (Scale), two frames: the fixture's strided sample and sums,
    and the fused form in full against the two-pass form"""
    _, _, _, pre, size = ref.PROTOCOL
    x = ref.protocol_input()
    assert ref.crc(x) == int(GOLD["crc/protocol"])
    xd = torch.from_numpy(x).to(DEV)
    mid = _both_forms(xd, pre, "bicubic")
    assert np.array_equal(mid.cpu().numpy().astype(np.int64).sum(axis=2), GOLD["protocol/mid_row_sums"])
    out = _both_forms(mid, size, "bilinear")
    for k, v in ref.protocol_digest(out.cpu().numpy()).items():
        assert np.array_equal(v, GOLD[f"protocol/{k}"]), k
    for fused in (None, True, False):
        assert torch.equal(vi.transform_frames(xd, size, pre, fused=fused), out)
    assert torch.equal(vi.transform_frames(xd, size, pre), out)      # two calls, the same bits


# ------------------------------------------------------------------------------------------------------------------- gather
def _gather_want(u8, idx, table):
    """table[c, u8[idx[b, t], y, x, c]] -> [B, C, T, h, w], indexed on the CPU"""
    u8, idx = torch.as_tensor(u8).long(), torch.as_tensor(idx).long()
    clips = u8[idx]                                                  # [B, T, h, w, C]
    C = clips.shape[-1]
    return torch.stack([table[c][clips[..., c]] for c in range(C)], dim=1)      # [B, C, T, h, w]


LOOP_PADDED = vi.center_crop_indices([2, 3, 4, 5, 6], 16)            # five frames walked again and again: repeated indices
GATHER_INDICES = [LOOP_PADDED, list(range(15, -1, -1)), [9, 0, 17, 3, 3, 12, 1, 16, 8, 8, 2, 11, 5, 14, 7, 0]]


@pytest.mark.parametrize("hw", [(6, 8), (6, 22), (5, 7), (3, 1)])
def test_gather_equals_indexing_the_table(hw):
    """w a multiple of four; w not, h * w a multiple of four (whole 16-byte stores, rows that start anywhere); neither (the scalar
    tail form); a single column"""
    h, w = hw
    assert LOOP_PADDED == [2, 3, 4, 5, 6] * 3 + [2] and len(set(GATHER_INDICES[2])) < 16
    u8 = ref.noise((18, h, w, 3), 31)
    table = vi.normalize_table()
    ud = torch.from_numpy(u8).to(DEV)
    keep = ud.clone()
    got = vi.gather_clips(ud, GATHER_INDICES)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 16, h, w) and got.is_contiguous()
    assert torch.equal(got.cpu(), _gather_want(u8, GATHER_INDICES, table))
    assert torch.equal(vi.gather_clips(ud, GATHER_INDICES).cpu(), got.cpu()) and torch.equal(ud, keep)
    # the ImageNet form, an explicit table, and indices as a device tensor
    t2 = vi.normalize_table(255, vi.IMAGENET_MEAN, vi.IMAGENET_STD)
    idx_dev = torch.tensor(GATHER_INDICES, dtype=torch.int64, device=DEV)
    assert torch.equal(vi.gather_clips(ud, idx_dev, t2).cpu(), _gather_want(u8, GATHER_INDICES, t2))
    assert torch.equal(vi.gather_clips(ud, GATHER_INDICES, norm_value=255, mean=vi.IMAGENET_MEAN, std=vi.IMAGENET_STD).cpu(),
                       _gather_want(u8, GATHER_INDICES, t2))


def test_gather_checks_host_indices_and_clamps_device_ones():
    u8 = ref.noise((4, 5, 7, 3), 32)
    ud = torch.from_numpy(u8).to(DEV)
    for bad in ([[0, 4]], [[-1, 0]]):
        with pytest.raises(ValueError, match="frame index outside"):
            vi.gather_clips(ud, bad)
    with pytest.raises(ValueError):
        vi.gather_clips(ud, [0, 1])
    with pytest.raises(ValueError):
        vi.gather_clips(ud, [[0.5, 1.0]])
    got = vi.gather_clips(ud, torch.tensor([[-3, 1, 9]], device=DEV, dtype=torch.int32))
    assert torch.equal(got.cpu(), _gather_want(u8, [[0, 1, 3]], vi.normalize_table()))


def test_clip_rgb_is_the_two_steps_and_the_reference_s_clip():
    """frames -> (240 x 320 bicubic) -> size bilinear -> gather: the composition, and the clip the reference assembles on the host
    (Pillow's arithmetic through the restatement, then ToTensor / Normalize with torch on the CPU, stack, permute)"""
    x = ref.noise((6, 97, 131, 3), 33)
    xd = torch.from_numpy(x).to(DEV)
    idx = [vi.center_crop_indices([0, 1, 2, 3, 4, 5], 4), [5, 5, 0, 2]]
    size, pre = (24, 40), (37, 53)
    got = vi.clip_rgb(xd, idx, size, pre)
    assert tuple(got.shape) == (2, 3, 4, 24, 40)
    assert torch.equal(got, vi.gather_clips(vi.transform_frames(xd, size, pre), idx))
    host = ref.chain(x, size, pre)
    clips = []
    for row in idx:
        frames = []
        for i in row:
            t = torch.from_numpy(host[i]).permute(2, 0, 1).contiguous().float().div(vi.DATASET_NORM_VALUE)      # ToTensor(norm_value)
            for ch, m, s in zip(t, vi.DATASET_MEAN, vi.DATASET_STD):                                          # Normalize
                ch.sub_(m).div_(s)
            frames.append(t)
        clips.append(torch.stack(frames, 0).permute(1, 0, 2, 3))
    assert torch.equal(got.cpu(), torch.stack(clips, 0))
    assert torch.equal(vi.clip_rgb(xd, idx, size).cpu(), vi.gather_clips(vi.resize_u8(xd, size), idx).cpu())      # DHF1K: no pre_size


def test_target_maps_equal_the_resized_bytes_over_255():
    x = ref.noise((3, 97, 131), 34)
    xd = torch.from_numpy(x).to(DEV)
    keep = xd.clone()
    for size in ((24, 40), (23, 41)):
        got = vi.target_maps(xd, size)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 1) + size
        want = torch.from_numpy(ref.resize(x[..., None], size, "bilinear")[..., 0]).float().div(255)[:, None]
        assert torch.equal(got.cpu(), want)
        assert torch.equal(vi.target_maps(xd[..., None], size), got)
    assert torch.equal(xd, keep)


# --------------------------------------------------------------------------------------------------------- the rest
def test_cpu_tensors_raise():
    x = torch.from_numpy(ref.noise((2, 9, 9, 3), 35))
    for call in (lambda: vi.resize_u8(x, (4, 4)), lambda: vi.transform_frames(x, (4, 4)), lambda: vi.clip_rgb(x, [[0, 1]], (4, 4)),
                 lambda: vi.gather_clips(x, [[0, 1]]), lambda: vi.target_maps(x[..., 0], (4, 4))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(ValueError):
        vi.resize_u8(x.to(DEV).float(), (4, 4))
    with pytest.raises(ValueError):
        vi.resize_u8(torch.zeros((2, 9, 9, 2), dtype=torch.uint8, device=DEV), (4, 4))


def test_replays_from_a_captured_graph_with_device_indices():
    x = ref.noise((8, 37, 53, 3), 36)
    xd = torch.from_numpy(x).to(DEV)
    size, pre = (16, 24), (20, 30)
    idx = torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]], dtype=torch.int32, device=DEV)
    vi.warm(DEV, (37, 53), size, pre)
    want = vi.clip_rgb(xd, idx, size, pre)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = vi.clip_rgb(xd, idx, size, pre)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # other frames and other indices through the same buffers
    x2 = ref.noise((8, 37, 53, 3), 37)
    xd.copy_(torch.from_numpy(x2).to(DEV))
    idx.copy_(torch.tensor([[7, 7, 0, 3], [2, 6, 1, 5]], dtype=torch.int32, device=DEV))
    g.replay()
    torch.cuda.synchronize()
    host = torch.from_numpy(ref.chain(x2, size, pre))
    assert torch.equal(out.cpu(), _gather_want(host, [[7, 7, 0, 3], [2, 6, 1, 5]], vi.normalize_table()))


def test_mvit_on_the_device_clip_equals_mvit_on_the_host_clip():
    """the same bits in, the same features out"""
    from diff_sal_amd.mvit import MViT
    from oracle import mvit_oracle as mo

    arch, shape = dict(embed_dims=96, num_layers=5, num_heads=1, downscale_indices=[1, 2, 4]), (2, 3, 16, 64, 96)
    B, _, T, h, w = shape
    net = MViT(arch=dict(arch), out_scales=[0, 1, 2, 3])
    net.load_state_dict(mo.synth_state_dict(mo.state_dict_template(mo.MViTConfig(arch=arch))), strict=True)
    net = net.to(DEV).eval().requires_grad_(False)
    x = ref.noise((20, 97, 131, 3), 38)
    idx = [list(range(0, 16)), list(range(4, 20))]
    assert (len(idx), len(idx[0])) == (B, T)
    clip_dev = vi.clip_rgb(torch.from_numpy(x).to(DEV), idx, (h, w), (80, 120))
    clip_host = _gather_want(ref.chain(x, (h, w), (80, 120)), idx, vi.normalize_table())
    assert tuple(clip_dev.shape) == shape and torch.equal(clip_dev.cpu(), clip_host)
    with torch.no_grad():
        a = net(clip_dev)
        b = net(clip_host.to(DEV))
    torch.cuda.synchronize()
    assert len(a) == len(b) == 4
    for fa, fb in zip(a, b):
        assert torch.isfinite(fa).all() and torch.equal(fa, fb)
