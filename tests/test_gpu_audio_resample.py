"""The resampling stage of the audio front end on the GPU (csrc/audio_input.hip, csrc/audio_resample.h through
diff_sal_amd.audio_input): ``resample_excerpts`` against the NumPy restatement of resampy 0.4.2's loop
(tests/_audio_resample_ref.py), and the three-launch chain ``clip_audio(..., sample_rate=22050, resample="kaiser_best")``.

Bars.  ``resample_excerpts``: ``torch.equal`` in float64.  Every operation of an output is one float64 operation rounded to
nearest in a fixed order, on the device as in numpy, so the result is a function of the inputs alone; a difference of a fused
multiply-add is a failure.  log-mel of the resampled excerpt: every element within one float32 step of the restatement,
``np.spacing(|ref|)``, the bar of test_gpu_audio_input.py with its reasoning (the resample is bit-equal, so the float64 values still
agree to about 1e-10 and only a value on a rounding boundary can differ); the share of bit-equal elements and the worst float64
difference are printed.  ``clip_audio`` against torch's float32 resize of the device's own examples: d <= yard, as there.
forward_vggish: the 1e-3 relative bar of test_gpu_encoders.py.  Silence, absent clips, prefixes, batches, repeats, replays: exact.

Shapes.  A window of 1500 samples at 22050 Hz gives 1088 outputs: four full tiles of 256 and a part-filled fifth; the wings of an
output are 88 taps, so outputs near 0 and near 1088 have truncated wings, and the excerpts below put the padding, the excerpt's
edges and a tile boundary inside the excerpt all within those five tiles."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diff_sal_amd import audio_input as ai
from tests import _audio_input_ref as ref
from tests import _audio_resample_ref as rs

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"int16": torch.int16, "float32": torch.float32, "float64": torch.float64}
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _to(x16, dtype):
    """[V, L] int16 in one of the three input types (the float forms hold x / 32768, exact in both)"""
    t = torch.from_numpy(np.ascontiguousarray(x16))
    return (t if dtype == "int16" else (t.to(DTYPES[dtype]) / 32768.0)).to(DEV)


def _want(key, x16, start, end, window, sr, filt="kaiser_best"):
    """the restatement of one clip's resampled padded excerpt, computed once"""
    return _memo(("want", key, start, end, window, sr, filt),
                 lambda: rs.resample(ref.padded_excerpt(x16, start, end, window), sr, 16000, filt))


# -------------------------------------------------------------------------------------------------------------- resample_excerpts
W1 = 1500
LENS = (4000, 3700, 3501)                        # valid samples of the three videos: noise, tone, +-2-LSB noise
SIGS = ("noise", "tone", "lsb")


def _videos():
    def make():
        wav = np.full((3, 4000), 12345, dtype=np.int16)      # beyond wav_len: must never be read
        for v, (s, n) in enumerate(zip(SIGS, LENS)):
            wav[v, :n] = ref.signal(s)[:n]
        return wav
    return _memo("videos", make)


def _clips(n):
    """(start, end) of four clips of a video of n samples: one that fills the window, an odd v with padding on both sides,
    v = 0 (past the end of the audio), an even v clamped at the end of the audio"""
    return [(7, 7 + W1 - 1), (100, 800), (n + 5, n + 900), (n - 600, n + 50)]


@pytest.mark.parametrize("rotation", [0, 1, 2])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_resample_excerpts_is_the_restatement_bit_for_bit(dtype, rotation):
    """B = 4 through the [V, Lmax] form; clip b reads video (b + rotation) % 3, so every kind of excerpt meets every signal"""
    wav16 = _videos()
    video = [(b + rotation) % 3 for b in range(4)]
    se = [_clips(LENS[v])[b] for b, v in enumerate(video)]
    assert [min(e + 1, LENS[v]) - min(s, LENS[v]) for (s, e), v in zip(se, video)] == [1500, 701, 0, 600]
    got = ai.resample_excerpts(_to(wav16, dtype), [s for s, _ in se], [e for _, e in se], window=W1, sample_rate=22050,
                               wav_len=list(LENS), video=video)
    assert got.shape == (4, 1088) and got.dtype == torch.float64 and 1088 % 256 != 0
    want = np.stack([_want(SIGS[v], wav16[v, :LENS[v]], s, e, W1, 22050) for (s, e), v in zip(se, video)])
    g = got.cpu().numpy()
    print(f"resample_excerpts {dtype} rotation {rotation}: bit-equal {100.0 * float((g == want).mean()):.4f} %, "
          f"worst |d| = {np.abs(g - want).max():.3e}")
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert not got[2].any()                                                      # v = 0: zeros


@pytest.mark.parametrize("sr,filt", [(44100, "kaiser_best"), (48000, "kaiser_best"), (8000, "kaiser_best"), (11025, "kaiser_best"),
                                     (22050, "kaiser_fast")])
def test_other_ratios_and_the_fast_filter(sr, filt):
    """window 1000, B = 2: a clip that fills the window and one of 333 samples.  44100: step 185; 48000: inc is exactly 3, frac is
    always 0, so the left wing starts at table entry 0 and the right wing at entry step; 8000 and 11025: upsamples, scale 1, the
    window unscaled"""
    x16 = ref.signal("noise")[:3000]
    se = [(11, 1010), (500, 832)]
    got = ai.resample_excerpts(_to(x16, "int16"), [s for s, _ in se], [e for _, e in se], window=1000, sample_rate=sr, filter=filt)
    want = np.stack([_want("noise3000", x16, s, e, 1000, sr, filt) for s, e in se])
    assert got.shape == (2, rs.out_len(1000, sr))
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    if filt == "kaiser_fast":      # a caller's own table, as (half_window, num_table), takes the same path
        own = ai.resample_excerpts(_to(x16, "int16"), [s for s, _ in se], [e for _, e in se], window=1000, sample_rate=sr,
                                   filter=rs.get_filter(filt))
        assert torch.equal(own, got)


def test_samples_batch_independence_and_repeatability():
    wav16 = _videos()
    wav = _to(wav16, "int16")
    video = [0, 1, 2, 0, 1]
    se = [_clips(LENS[v])[b % 4] for b, v in enumerate(video)]
    kw = dict(window=W1, sample_rate=22050, wav_len=list(LENS))
    s, e = [a for a, _ in se], [b for _, b in se]
    full = ai.resample_excerpts(wav, s, e, video=video, **kw)
    assert torch.equal(ai.resample_excerpts(wav, s, e, video=video, **kw), full)                   # a repeat call
    for k in (1, 256, 300):                                                                        # within, at and across a tile
        assert torch.equal(ai.resample_excerpts(wav, s, e, video=video, samples=k, **kw), full[:, :k])
    for b in (1, 3):                                                                               # alone and inside the batch of 5
        assert torch.equal(ai.resample_excerpts(wav, s[b:b + 1], e[b:b + 1], video=video[b:b + 1], **kw), full[b:b + 1])


# ----------------------------------------------------------------------------------------------------------------- the whole chain
FULL = ref.FULL                                   # 35280 samples at 22050 Hz -> 25600 at 16 kHz: 158 frames, nine examples
CHAIN = ("noise", "tone", "lsb", "silence")
CHAIN_CLIPS = [(0, FULL - 1), (1000, 30000), (5, 20004), (0, FULL - 1)]      # v = 35280, 29001 (odd), 20000 (even), silence


def _chain():
    def make():
        wav16 = np.stack([ref.signal(s) for s in CHAIN])
        res = [rs.resample(ref.padded_excerpt(wav16[b], s, e, FULL), 22050) for b, (s, e) in enumerate(CHAIN_CLIPS)]
        return wav16, [ref.log_mel(y) for y in res]
    return _memo("chain", make)


def _chain_kw():
    return dict(wav_len=[FULL] * 4, video=[0, 1, 2, 3], sample_rate=22050, resample="kaiser_best")


def test_log_mel_of_the_resampled_excerpt_at_the_protocol_window():
    wav16, lm_ref = _chain()
    wav = _to(wav16, "int16")
    s, e = [a for a, _ in CHAIN_CLIPS], [b for _, b in CHAIN_CLIPS]
    lm = ai.log_mel(wav, s, e, **_chain_kw())
    assert lm.shape == (4, 158, 64) and lm.dtype == torch.float32
    got, want = lm.cpu().numpy(), np.stack(lm_ref).astype(np.float32)
    lm64 = ai.log_mel(wav, s, e, dtype=torch.float64, **_chain_kw()).cpu().numpy()
    equal = float((got == want).mean())
    worst = float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())
    print(f"log_mel 22050 -> 16000: bit-equal {100.0 * equal:.4f} %, worst {worst:.1f} float32 steps; float64 against the restatement: "
          f"worst |d| = {np.abs(lm64 - np.stack(lm_ref)).max():.2e}")
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), worst
    assert (lm[3] == float(np.float32(np.log(0.01)))).all()                      # silence: exactly log(0.01)
    assert np.array_equal(lm64.astype(np.float32), got)
    ex = ai.examples(wav, s, e, **_chain_kw())                                   # clip_audio at 64 x 64
    assert ex.shape == (4, 9, 1, 64, 64)
    nine = torch.stack([lm[:, 11 * j:11 * j + 64] for j in range(9)], dim=1)[:, :, None]      # examples 0 .. 8, none repeated
    assert torch.equal(ex, nine)
    assert torch.equal(ai.log_mel(wav, s, e, frames=152, **_chain_kw()), lm[:, :152])


def test_clip_audio_against_torch_interpolate():
    wav16, _ = _chain()
    wav = _to(wav16, "int16")
    s, e = [a for a, _ in CHAIN_CLIPS], [b for _, b in CHAIN_CLIPS]
    exists = [1, 1, 0, 1]
    size = (112, 192)
    got = ai.clip_audio(wav, s, e, size=size, exists=exists, **_chain_kw())
    assert got.shape == (4, 1, 9) + size and got.dtype == torch.float32 and got.is_contiguous()
    x = ai.examples(wav, s, e, exists=exists, **_chain_kw()).cpu().reshape(36, 1, 64, 64)      # the device's own examples
    t32 = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    t64 = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False)
    g = got.cpu().reshape(36, 1, *size)
    d = (g - t32).abs().max().item()
    yard = (t32.double() - t64).abs().max().item()
    print(f"clip_audio 22050 {size}: d = {d:.3e}, yard = {yard:.3e}, bit-equal {100.0 * (g == t32).float().mean().item():.4f} %")
    assert d <= yard
    assert not got[2].any() and got[1].any()                                      # an absent clip is exactly zero


def test_graph_capture_replays_the_eager_bits():
    wav16, _ = _chain()
    wav = _to(wav16, "int16")
    s, e = [a for a, _ in CHAIN_CLIPS], [b for _, b in CHAIN_CLIPS]
    ai.warm(DEV, sample_rate=22050, resample="kaiser_best", clips=4)
    eager = ai.clip_audio(wav, s, e, size=(32, 64), **_chain_kw())
    # device-side arguments: nothing is copied from the host inside the capture
    dev = dict(wav_len=torch.tensor([FULL] * 4, device=DEV), video=torch.arange(4, dtype=torch.int32, device=DEV), sample_rate=22050,
               resample="kaiser_best")
    sd, ed = torch.tensor(s, dtype=torch.int32, device=DEV), torch.tensor(e, dtype=torch.int32, device=DEV)
    assert torch.equal(ai.clip_audio(wav, sd, ed, size=(32, 64), **dev), eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):                                  # one stream, a linear chain of three launches
            out = ai.clip_audio(wav, sd, ed, size=(32, 64), **dev)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_forward_vggish_on_the_device_tensor_equals_the_host_pipeline():
    """64 x 128 frames: audio is [B, 1, 9, 32, 64].  The host side is the restatement, clip by clip, copied to the device."""
    from diff_sal_amd.diff_model import VideoSaliencyModel
    from tests.test_gpu_encoders import RTOL, build_audio, rel_err

    wav16, lm_ref = _chain()
    s, e = [a for a, _ in CHAIN_CLIPS], [b for _, b in CHAIN_CLIPS]
    vgg, net, _, _ = build_audio()
    model = VideoSaliencyModel(channel_list=None, audio_net=vgg, spatiotemp_net=net)
    host = np.stack([ref.resize(ref.examples(lm), 32, 64)[None] for lm in lm_ref])
    dev = ai.clip_audio(_to(wav16, "int16"), s, e, size=(32, 64), **_chain_kw())
    assert dev.shape == host.shape == (4, 1, 9, 32, 64)
    with torch.no_grad():
        got, _ = model.forward_vggish(dev)
        want, _ = model.forward_vggish(torch.from_numpy(host).to(DEV))
    err = rel_err(got, want)
    print(f"forward_vggish 22050: relative error {err:.2e}; input max |d| = {np.abs(dev.cpu().numpy() - host).max():.2e}")
    assert err < RTOL


def test_guards():
    wav = _to(ref.signal("noise"), "int16")
    with pytest.raises(RuntimeError, match="GPU only"):
        ai.clip_audio(wav.cpu(), [0], [100], sample_rate=22050, resample="kaiser_best")
    with pytest.raises(RuntimeError, match="GPU only"):
        ai.resample_excerpts(wav.cpu(), [0], [100], window=W1, sample_rate=22050)
    for fn in (ai.clip_audio, ai.log_mel, ai.examples):
        with pytest.raises(ValueError, match="resample on load"):
            fn(wav, [0], [100], sample_rate=22050)
    with pytest.raises(ValueError, match="more than the window"):
        ai.resample_excerpts(wav, [0], [2000], window=W1, sample_rate=22050)      # v > window: the reference fails here too
    # at 16 kHz the keyword changes nothing
    assert torch.equal(ai.clip_audio(wav, [0], [9000], resample="kaiser_best"), ai.clip_audio(wav, [0], [9000]))
