"""The audio front end on the GPU (csrc/audio_input.hip through diff_sal_amd.audio_input): log-mel and examples against the
fixtures recorded from the reference's mel_features.py (tools/gen_audio_input_golden.py), the resize against ``F.interpolate`` on
the CPU, the batch forms, absent clips, silence, determinism, graph capture, and the features ``forward_vggish`` makes of it.

Bars.  log-mel and examples in float32: every element within one float32 step of the reference, ``np.spacing(|ref|)`` -- both
are one rounding of float64 values that agree to about 1e-10, four orders of magnitude below a float32 step of these values, so
only a value on a rounding boundary can differ.  The share of bit-equal elements and the worst float64 difference (through
``dtype=torch.float64``, against the restatement) are printed, not asserted.  ``clip_audio`` against torch's float32 resize of the
device's own examples: d = max|dev - torch_fp32| <= yard = max|torch_fp32 - torch_fp64|, both computed here on that input: a
result no farther from torch's float32 answer than exact arithmetic is cannot be told from the reference's own rounding.
Absent clips and silence: exact.  forward_vggish: the 1e-3 relative bar of test_gpu_encoders.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diff_sal_amd import audio_input as ai
from tests import _audio_input_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = ref.load_cases()
DTYPES = {"int16": torch.int16, "float32": torch.float32, "float64": torch.float64}
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _wav(x16, dtype):
    """the int16 signal in one of the three input types (the float forms hold x / 32768, exact in both)"""
    t = torch.from_numpy(np.ascontiguousarray(x16))
    return (t if dtype == "int16" else (t.to(DTYPES[dtype]) / 32768.0)).to(DEV)


def _within_one_step(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    equal = float((got == want).mean())
    worst = float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())
    print(f"{what}: bit-equal {100.0 * equal:.4f} %, worst {worst:.1f} float32 steps")
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), (what, worst)


def _video():
    def make():
        video = ref.signal("video", ref.VIDEO_SAMPLES)
        starts, ends = ai.excerpt_table(ref.VIDEO_FRAMES, ref.VIDEO_FPS, ref.RATE, video.shape[0])
        # clips 0-3: the recorded ones (video start with an odd v, an even v, one more, clamped at the end of the audio);
        # clip 4: v = 0 (starts past the end of the audio); clip 5: absent
        s = [int(starts[a]) for a, _ in ref.VIDEO_CLIPS] + [video.shape[0] + 5, int(starts[4])]
        e = [int(ends[b]) for _, b in ref.VIDEO_CLIPS] + [video.shape[0] + 900, int(ends[19])]
        exists = [1, 1, 1, 1, 1, 0]
        want = np.stack([GOLD[f"video/{a}_{b}/logmel"] for a, b in ref.VIDEO_CLIPS] +
                        [np.full((152, 64), np.float32(np.log(0.01)))] + [GOLD["video/4_19/logmel"]])
        return video, s, e, exists, want
    return _memo("video", make)


def _nine(lm, E):
    """[B, F, 64] log-mel -> [B, 9, 1, 64, 64] examples"""
    return np.stack([np.stack([l[11 * e:11 * e + 64] for e in ref.nine_map(E)])[:, None] for l in lm])


# ---------------------------------------------------------------------------------------------------------- log-mel and examples
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_log_mel_full_window_five_signals(dtype):
    """window 35280 (F = 219, E = 15), B = 5, one signal each, through the [V, Lmax] form with one video per clip"""
    names = ["full_" + s for s in ref.SIGNALS]
    wav = torch.stack([_wav(ref.signal(s), dtype) for s in ref.SIGNALS])
    B = len(names)
    lm = ai.log_mel(wav, [0] * B, [ref.FULL - 1] * B, wav_len=[ref.FULL] * B, video=list(range(B)))
    assert lm.shape == (B, 219, 64) and lm.dtype == torch.float32
    want = np.stack([GOLD[f"{n}/logmel"] for n in names])
    _within_one_step(lm.cpu().numpy(), want, f"log_mel 35280 {dtype}")
    assert (lm[4] == float(np.float32(np.log(0.01)))).all()                      # silence, before the resize: exactly log(0.01)
    ex = ai.examples(wav, [0] * B, [ref.FULL - 1] * B, wav_len=[ref.FULL] * B, video=list(range(B)))
    assert ex.shape == (B, 9, 1, 64, 64)
    _within_one_step(ex.cpu().numpy(), _nine(want, 15), f"examples 35280 {dtype}")
    assert torch.equal(ex, torch.from_numpy(_nine(lm.cpu().numpy(), 15)).to(DEV))      # the gather itself is exact
    if dtype == "int16":
        lm64 = ai.log_mel(wav, [0] * B, [ref.FULL - 1] * B, wav_len=[ref.FULL] * B, video=list(range(B)), dtype=torch.float64).cpu().numpy()
        want64 = np.stack([ref.log_mel(ref.padded_excerpt(ref.signal(s), 0, ref.FULL - 1, ref.FULL)) for s in ref.SIGNALS])
        print(f"log_mel 35280 float64 against the restatement: worst |d| = {np.abs(lm64 - want64).max():.2e}")
        assert np.array_equal(lm64.astype(np.float32), lm.cpu().numpy())          # the float32 result is that value rounded once


@pytest.mark.parametrize("name", ["w10480", "w12345", "w15760"])
def test_log_mel_and_examples_short_windows(name):
    """F = 64, E = 1 / F = 75, E = 2 (an odd window) / F = 97, E = 4: every branch of the nine-example map below nine"""
    sig, window, v = ref.CASES[name]
    wav = _wav(ref.signal(sig), "int16")
    want = GOLD[f"{name}/logmel"][None]
    E = int(GOLD[f"{name}/examples_shape"][0])
    lm = ai.log_mel(wav, [0], [v - 1], window=window)
    assert lm.shape == (1, ai.num_frames(window), 64) and E == ai.num_examples(window)
    _within_one_step(lm.cpu().numpy(), want, f"log_mel {name}")
    ex = ai.examples(wav, [0], [v - 1], window=window)
    _within_one_step(ex.cpu().numpy(), _nine(want, E), f"examples {name}")
    used = ai.frames_needed(window)
    assert torch.equal(ai.log_mel(wav, [0], [v - 1], window=window, frames=used), lm[:, :used])      # a prefix is the same bits


@pytest.mark.parametrize("form", ["one_video", "two_videos"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_batch_of_six_clips(dtype, form):
    """clips at the video start (odd and even v < W), clamped at the end of the audio, v = 0, absent; alone as a 1-D waveform and
    as video 1 of a [V, Lmax] pair whose video 0 is longer"""
    video, s, e, exists, want = _video()
    if form == "one_video":
        wav, kw = _wav(video, dtype), {}
    else:
        other = ref.signal("chirp", ref.VIDEO_SAMPLES + 777)
        wav = torch.zeros(2, other.shape[0], dtype=DTYPES[dtype], device=DEV)
        wav[0] = _wav(other, dtype)
        wav[1, :video.shape[0]] = _wav(video, dtype)
        wav[1, video.shape[0]:] = 1 if dtype == "int16" else 0.5                  # beyond wav_len: must never be read
        kw = {"wav_len": [other.shape[0], video.shape[0]], "video": [1] * 6}
    lm = ai.log_mel(wav, s, e, frames=152, **kw)
    _within_one_step(lm.cpu().numpy(), want, f"log_mel batch {dtype} {form}")
    assert (lm[4] == float(np.float32(np.log(0.01)))).all()                      # v = 0: silence
    ex = ai.examples(wav, s, e, exists=exists, **kw)
    want9 = _nine(want, 15)
    want9[5] = 0.0
    _within_one_step(ex[:5].cpu().numpy(), want9[:5], f"examples batch {dtype} {form}")
    assert not ex[5].any()                                                       # absent: exactly zero, not log(0.01)
    if form == "two_videos":
        # a clip of the other video in the same batch, against the restatement; the video's clips keep their bits
        s2, e2, v2 = s + [100], e + [9000], kw["video"] + [0]
        lm2 = ai.log_mel(wav, s2, e2, frames=152, wav_len=kw["wav_len"], video=v2)
        assert torch.equal(lm2[:6], lm)
        w0 = ref.log_mel(ref.padded_excerpt(other, 100, 9000, ref.FULL))[:152].astype(np.float32)
        _within_one_step(lm2[6].cpu().numpy(), w0, f"log_mel other video {dtype}")


# ------------------------------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("size", [(112, 192), (32, 64), (45, 77)])
def test_clip_audio_against_torch_interpolate(size):
    video, s, e, exists, _ = _video()
    wav = _wav(video, "int16")
    got = ai.clip_audio(wav, s, e, size=size, exists=exists)
    assert got.shape == (6, 1, 9) + size and got.dtype == torch.float32 and got.is_contiguous()
    ex = ai.examples(wav, s, e, exists=exists).cpu()                              # [6, 9, 1, 64, 64]: the device's own examples
    x = ex.reshape(54, 1, 64, 64)
    t32 = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    t64 = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False)
    g = got.cpu().reshape(54, 1, *size)
    d = (g - t32).abs().max().item()
    yard = (t32.double() - t64).abs().max().item()
    print(f"clip_audio {size}: d = {d:.3e}, yard = {yard:.3e}, bit-equal {100.0 * (g == t32).float().mean().item():.4f} %")
    assert d <= yard
    assert not got[5].any()                                                       # absent clips are exactly zero


def test_the_layout_is_the_one_forward_vggish_reads():
    """[B, 1, 9, h, w]: example j of clip b at [b, 0, j]; with h = w = 64 the resize is the identity"""
    video, s, e, exists, _ = _video()
    wav = _wav(video, "int16")
    same = ai.clip_audio(wav, s, e, size=(64, 64), exists=exists)
    assert torch.equal(same.transpose(1, 2), ai.examples(wav, s, e, exists=exists))


# ---------------------------------------------------------------------------------------------------- determinism, graph, errors
def test_two_calls_give_identical_bits():
    video, s, e, exists, _ = _video()
    wav = _wav(video, "int16")
    a = ai.clip_audio(wav, s, e, exists=exists)
    b = ai.clip_audio(wav, s, e, exists=exists)
    assert torch.equal(a, b)
    assert torch.equal(ai.log_mel(wav, s, e), ai.log_mel(wav, s, e))
    assert torch.equal(ai.clip_audio(wav, s[1:3], e[1:3]), a[1:3])                # a clip's bits do not depend on its batch


def test_graph_capture_replays_the_eager_bits():
    video, s, e, exists, _ = _video()
    wav = _wav(video, "int16")
    eager = ai.clip_audio(wav, s, e, exists=exists)
    # device-side tables: nothing is copied from the host inside the capture
    sd, ed = torch.tensor(s, dtype=torch.int32, device=DEV), torch.tensor(e, dtype=torch.int32, device=DEV)
    xd = torch.tensor(exists, dtype=torch.uint8, device=DEV)
    assert torch.equal(ai.clip_audio(wav, sd, ed, exists=xd), eager)              # also warms the table cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):                                  # one stream, a linear chain of two launches
            out = ai.clip_audio(wav, sd, ed, exists=xd)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_argument_rules_on_the_device():
    wav = _wav(ref.signal("noise"), "int16")
    with pytest.raises(ValueError, match="more than the window"):
        ai.clip_audio(wav, [0], [20000], window=15760)                            # v > window: the reference fails here too
    with pytest.raises(ValueError, match="resample on load"):
        ai.clip_audio(wav, [0], [100], sample_rate=44100)
    with pytest.raises(ValueError, match="too short for one example"):
        ai.clip_audio(wav, [0], [100], window=10479)
    with pytest.raises(ValueError, match="int16, float32 or float64"):
        ai.clip_audio(wav.int(), [0], [100])
    with pytest.raises(ValueError, match="wav_len"):
        ai.clip_audio(wav[None], [0], [100])
    with pytest.raises(RuntimeError, match="GPU only"):
        ai.clip_audio(wav.cpu(), [0], [100])
    on = torch.ones(1, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="more than the window"):
        ai.clip_audio(wav, [0], [20000], window=15760, exists=on)                 # host starts / ends are checked whatever else is on the GPU
    with pytest.raises(ValueError, match="starts must be sample indices"):
        ai.clip_audio(wav, [-1], torch.tensor([100], dtype=torch.int32, device=DEV))
    ex = ai.examples(wav, [0], [100])
    assert ex.is_contiguous() and ex.shape == (1, 9, 1, 64, 64)


# -------------------------------------------------------------------------------------------------------------------- end to end
def test_forward_vggish_on_the_device_tensor_equals_the_host_pipeline():
    """64 x 128 frames: audio is [B, 1, 9, 32, 64].  The host side is the restatement, clip by clip, copied to the device."""
    from diff_sal_amd.diff_model import VideoSaliencyModel
    from tests.test_gpu_encoders import RTOL, build_audio, rel_err

    video, s, e, exists, _ = _video()
    vgg, net, _, _ = build_audio()
    model = VideoSaliencyModel(channel_list=None, audio_net=vgg, spatiotemp_net=net)
    host = np.stack([ref.clip_audio(video, s[b], e[b], ref.FULL, 32, 64, exists=bool(exists[b])) for b in range(6)])
    dev = ai.clip_audio(_wav(video, "int16"), s, e, size=(32, 64), exists=exists)
    assert dev.shape == host.shape == (6, 1, 9, 32, 64)
    with torch.no_grad():
        got, _ = model.forward_vggish(dev)
        want, _ = model.forward_vggish(torch.from_numpy(host).to(DEV))
    err = rel_err(got, want)
    print(f"forward_vggish: relative error {err:.2e}; input max |d| = {np.abs(dev.cpu().numpy() - host).max():.2e}")
    assert err < RTOL
