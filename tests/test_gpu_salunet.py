"""End-to-end parity of the HIP SalUNet against the reference's golden vectors and the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import salunet_oracle as orc
from tests._cases import CASES, check_taps, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-3  # north_star: 1e-3 relative, fp32


def build(cfg, sd):
    from diff_sal_amd.sal_unet import SalUNet

    net = SalUNet(
        image_based=cfg.image_based, img_size=cfg.img_size, frames_len=1, mid_num_stages=cfg.num_stages,
        temporal_size=9, temporal_list=list(cfg.temporal_list), futr_num_stages=0, ori_embed_dim=cfg.ori_embed_dim,
        down_embed_dim=cfg.down_embed_dim, idx_to_planes={0: cfg.down_embed_dim, 1: 192, 2: 384, 3: cfg.ori_embed_dim},
        patch_size=[0, 3, 3, 3], patch_stride=[0, 1, 1, 1], patch_padding=list(cfg.dilation),
        up_channel=list(cfg.up_channel), num_heads=list(cfg.num_heads), mlp_ratio=[2.0] * 4,
        drop_path_rate=[0.15] * 4, qkv_bias=[True] * 4, kv_proj_method=["avg"] * 4, kernel_kv=list(cfg.kernel_kv),
        padding_kv=[0] * 4, stride_kv=list(cfg.kernel_kv), q_proj_method=["dw_bn"] * 4, kernel_q=[3] * 4,
        padding_q=[1] * 4, stride_q=[1] * 4)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


@pytest.mark.parametrize("name", list(CASES))
def test_hip_forward_matches_reference_golden(golden_dir, name):
    cfg, sd, x, t, feats, audio, g = load_case(golden_dir, name)
    net = build(cfg, sd)
    taps = {}
    feats_d = [f.to(DEV) for f in feats]
    before = [f.clone() for f in feats_d]
    with torch.no_grad():
        out = net(x.to(DEV), t.to(DEV), feats_d, None if audio is None else audio.to(DEV), taps=taps)
    torch.cuda.synchronize()
    ref = torch.from_numpy(g["output"])
    assert out.shape == ref.shape
    err = (out.cpu() - ref).abs().max().item()
    print(name, "max abs err", err)
    assert err < RTOL * ref.abs().max().item()
    # inputs are borrowed, never mutated (fixes reference defect D4)
    assert len(feats_d) == 4 and all(torch.equal(a, b) for a, b in zip(before, feats_d))
    # intermediate taps (F1: the visual-only output alone cannot see the noise path)
    # ... recorded while the SHIPPED forms run (tap / source-resolution convolutions, fused ResnetBlocks); the 4-scale sum exists
    # only in the reference's operator order, which a second pass takes
    ref_taps = {k: net.tap_to_reference_layout(k, v) for k, v in taps.items()}
    worst = check_taps(ref_taps, g, RTOL)
    assert {"temb", "down1", "res0", "noise0", "stage0", "stage3"} <= set(worst) and "multi_scale" not in taps
    taps_ref = {}
    net.taps_reference_forms = True
    with torch.no_grad():
        out_r = net(x.to(DEV), t.to(DEV), feats_d, None if audio is None else audio.to(DEV), taps=taps_ref)
    net.taps_reference_forms = False
    assert (out_r.cpu() - ref).abs().max().item() < RTOL * ref.abs().max().item()
    worst = check_taps({k: net.tap_to_reference_layout(k, v) for k, v in taps_ref.items()}, g, RTOL)
    assert {"temb", "down1", "res0", "noise0", "stage0", "stage3", "multi_scale"} <= set(worst)
    # without taps the eval path takes the restructured form of UpEmbed conv1 / mt_proj (nine 1x1 tap mixings at the source
    # resolution + gather, csrc/tapsum.hip) and the composed conv_in: same reference output, same bar
    assert net.tap_conv
    with torch.no_grad():
        out2 = net(x.to(DEV), t.to(DEV), feats_d, None if audio is None else audio.to(DEV))
        net.tap_conv = False
        out3 = net(x.to(DEV), t.to(DEV), feats_d, None if audio is None else audio.to(DEV))
    err2, err3 = (out2.cpu() - ref).abs().max().item(), (out3.cpu() - ref).abs().max().item()
    print(name, "max abs err, restructured path", err2, "direct path without taps", err3)
    assert err2 < RTOL * ref.abs().max().item() and err3 < RTOL * ref.abs().max().item()
    assert (out2 - out3).abs().max().item() < 2e-5


def test_hip_forward_matches_oracle_on_fresh_inputs(golden_dir):
    """Same seeded inputs through the oracle and the HIP path (not a stored fixture), B=3, AV."""
    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    x, feats, audio = orc.synth_inputs(cfg, 3, True, tag="fresh")
    t = torch.tensor([999.0, 431.5, 0.0])
    with torch.no_grad():
        ref = orc.salunet_forward(sd, cfg, x, t, feats, audio)
        out = build(cfg, sd)(x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], audio.to(DEV))
    assert (out.cpu() - ref).abs().max().item() < RTOL * ref.abs().max().item()


def test_full_size_batch4_properties():
    """BASELINE config sizes (B=4, 224x384): size-independent properties instead of a stored output:
    per-sample independence (batch of 4 == 4 batches of 1), determinism, range, and F1 (visual-only
    output ignores x and t)."""
    cfg = orc.SalUNetConfig()
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    net = build(cfg, sd)
    x, feats, audio = orc.synth_inputs(cfg, 4, True, tag="b4")
    xd, fd, ad = x.to(DEV), [f.to(DEV) for f in feats], audio.to(DEV)
    t = torch.tensor([999, 650, 300, 0], device=DEV)
    with torch.no_grad():
        o4 = net(xd, t, fd, ad)
        o4b = net(xd, t, fd, ad)
        assert torch.equal(o4, o4b)
        assert o4.shape == (4, 1, 224, 384) and o4.min() > 0 and o4.max() < 1 and torch.isfinite(o4).all()
        for i in (0, 3):
            oi = net(xd[i:i + 1], t[i:i + 1], [f[i:i + 1] for f in fd], ad[i:i + 1])
            assert (oi - o4[i:i + 1]).abs().max().item() < 1e-5
        v1 = net(xd, t, fd, None)
        v2 = net(1 - 2 * xd, t.flip(0), fd, None)
        assert torch.equal(v1, v2)  # F1
        assert (v1 - o4).abs().max().item() > 1e-3  # audio conditioning does change the output


def test_cpu_input_is_rejected():
    cfg = CASES["tiny_vis"][0]
    net = build(cfg, orc.synth_state_dict(orc.state_dict_template(cfg)))
    x, feats, _ = orc.synth_inputs(cfg, 1, False)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(x, torch.tensor([1]), feats)


def test_ragged_and_chunked_batches():
    """Batches that are not a multiple of the internal pass size are split and re-joined; empty batch -> empty."""
    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    net = build(cfg, sd)
    x, feats, audio = orc.synth_inputs(cfg, 5, True, tag="ragged")
    xd, fd, ad = x.to(DEV), [f.to(DEV) for f in feats], audio.to(DEV)
    t = torch.tensor([1, 200, 400, 600, 999], device=DEV)
    with torch.no_grad():
        whole = net(xd, t, fd, ad)
        net.max_clips_per_pass = 2  # force 2 + 2 + 1
        chunked = net(xd, t, fd, ad)
        empty = net(xd[:0], t[:0], [f[:0] for f in fd], ad[:0])
    assert chunked.shape == whole.shape and (chunked - whole).abs().max().item() < 1e-5
    assert empty.shape == (0, 1, 64, 128)


def test_image_based_false_uses_eight_frames():
    """image_based=False (the class default): the noise maps are not appended, T stays 8 (sal_unet.py:311)."""
    from diff_sal_amd.sal_unet import SalUNet

    cfg = CASES["tiny_vis"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    kw = dict(img_size=cfg.img_size, frames_len=1, mid_num_stages=4, temporal_size=9, temporal_list=[5] * 4,
              futr_num_stages=0, ori_embed_dim=256, down_embed_dim=32, idx_to_planes={0: 32, 1: 192, 2: 384, 3: 256},
              patch_size=[0, 3, 3, 3], patch_stride=[0, 1, 1, 1], patch_padding=[0, 2, 2, 2],
              up_channel=[256, 128, 64, 32], num_heads=[2] * 4, mlp_ratio=[2.0] * 4, drop_path_rate=[0.15] * 4,
              qkv_bias=[True] * 4, kv_proj_method=["avg"] * 4, kernel_kv=[2, 4, 8, 16], padding_kv=[0] * 4,
              stride_kv=[2, 4, 8, 16], q_proj_method=["dw_bn"] * 4, kernel_q=[3] * 4, padding_q=[1] * 4,
              stride_q=[1] * 4)
    net = SalUNet(image_based=False, **kw)
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    x, feats, _ = orc.synth_inputs(cfg, 2, False, tag="ib0")
    cfg0 = orc.SalUNetConfig(**{**cfg.__dict__, "image_based": False})
    with torch.no_grad():
        ref = orc.salunet_forward(sd, cfg0, x, torch.tensor([5, 50]), feats, None)
        out = net(x.to(DEV), torch.tensor([5, 50], device=DEV), [f.to(DEV) for f in feats], None)
    assert (out.cpu() - ref).abs().max().item() < RTOL * ref.abs().max().item()


def _launch_trace(net, args):
    """(class, note) of every launch of one forward (ops.PROFILE), and its output.  An untraced forward goes first, so that the
    launches that pack the weights (once per setting of the switches in SalUNet._cache_key) are not part of the trace."""
    from diff_sal_amd import ops

    with torch.no_grad():
        net(*args)
    ops.PROFILE = []
    try:
        with torch.no_grad():
            out = net(*args)
        torch.cuda.synchronize()
        return [(p[3], p[5]) for p in ops.PROFILE], out
    finally:
        ops.PROFILE = None


# (storage, fixture, switch under test, its non-default value, the other overrides)
SWITCH_CASES = [
    ("fp32", "small_av", "fused_front", False, {}),
    ("fp32", "small_av", "merge_qkv_prep", False, {}),
    ("fp32", "small_av", "group_qkv", False, {"fold_attn_proj": False}),
    ("fp32", "small_av", "pair_kv", False, {"fold_attn_proj": False, "group_qkv": False}),
    ("fp32", "small_av", "merge_align", False, {}),
    ("fp32", "small_av", "group_reduce_temp", False, {}),
    ("fp32", "small_av", "fold_head", False, {}),
    ("fp32", "small_av", "fold_norm1", True, {}),
    ("fp32", "full_av_b1", "up_commute", False, {}),
    ("fp32", "full_av_b1", "fuse_up_pe2", False, {}),
    ("fp32", "full_av_b1", "fuse_resblock", False, {}),
] + [(d, "small_av", s, False, {}) for s in ("fused_front", "pair_kv", "up_commute16", "mt_tap16_f32") for d in ("bf16", "fp16")]


@pytest.mark.parametrize("dname,name,switch,value,others", SWITCH_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in SWITCH_CASES])
def test_switch_off_default_settings_stay_inside_the_bar(golden_dir, dname, name, switch, value, others):
    """The class-level switches of SalUNet at the setting no other test runs: the output against the reference's fixture inside
    the file's bar (fp32: RTOL relative to the fixture's maximum; 16-bit storage: tests/test_gpu_lowp.py::LOWP_ATOL), and the
    launch trace differs from the one with the switch at its default, so the case did reach its branch."""
    from tests import test_gpu_lowp as lowp

    cfg, sd, x, t, feats, audio, g = load_case(golden_dir, name)
    net = build(cfg, sd) if dname == "fp32" else lowp.build(cfg, sd, lowp.DTYPES[dname])
    assert getattr(type(net), switch) == (not value)
    for k, v in others.items():
        setattr(net, k, v)
    args = (x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], None if audio is None else audio.to(DEV))
    base, _ = _launch_trace(net, args)
    setattr(net, switch, value)
    flipped, out = _launch_trace(net, args)
    ref = torch.from_numpy(g["output"])
    err = (out.cpu() - ref).abs().max().item()
    bar = RTOL * ref.abs().max().item() if dname == "fp32" else lowp.LOWP_ATOL[dname]
    print(f"SWITCH {dname} {name} {switch}={value}: max abs err {err:.3e} (bar {bar:.3e}); launches {len(base)} -> {len(flipped)}")
    assert out.shape == ref.shape and err < bar
    assert flipped != base


@pytest.fixture
def bf16x3():
    from diff_sal_amd import ops

    ops.set_gemm_precision("bf16x3")
    yield
    ops.set_gemm_precision("fp32")


@pytest.mark.parametrize("name", ["tiny_av", "small_vis", "full_av_b1"])
def test_bf16x3_mode_stays_inside_the_parity_bar(golden_dir, name, bf16x3):
    """Opt-in split-precision mode of the implicit-GEMM kernel (bf16 hi/lo operands, fp32 accumulation): the end-to-end
    output against the reference's golden vectors.  Bar: 1e-3 relative (north_star); measured ~1e-5."""
    cfg, sd, x, t, feats, audio, g = load_case(golden_dir, name)
    net = build(cfg, sd)
    with torch.no_grad():
        out = net(x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], None if audio is None else audio.to(DEV))
    ref = torch.from_numpy(g["output"])
    err = (out.cpu() - ref).abs().max().item()
    print(name, "bf16x3 max abs err vs reference", err, "(output range", ref.min().item(), ref.max().item(), ")")
    assert err < 1e-3 * ref.abs().max().item()
    assert err > 0.0        # it really is a different arithmetic from the fp32 path
