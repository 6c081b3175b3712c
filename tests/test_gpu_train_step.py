"""Whole-network training forward/backward: HIP autograd path vs PyTorch autograd through the
CPU oracle, train-mode BatchNorm, dropout disabled (masks cannot match by construction).

Tolerances.  Every backward kernel is pinned to ~1e-6 against autograd of the same op in test_gpu_train_ops.py.  A
whole-network gradient cannot be compared that tightly: the decoder has 11 ReLUs over ~1.5 M pre-activations, a few
of which land within 1e-6 of zero on any input, and two correct fp32 evaluations (different summation order) put such
an element on different sides of the kink.  One flipped element changes the local gradient by O(1e-2) of its layer's
maximum and everything upstream by ~1e-3 (measured: tests/diagnostics/relu_flip_census.py counts the flips against an fp64 run,
tests/diagnostics/grad_trace.py shows the error entering exactly at the flipped layer; with no flip the HIP gradients are
within 2e-6 of fp64).  Hence 5e-3 here."""
import pytest
import torch

from oracle import salunet_oracle as orc
from tests._cases import CASES
from tests.test_gpu_salunet import build

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _relu_spies():
    """Record the ReLU sign pattern of both forwards: the oracle's pre-activations (torch.nn.functional.relu inputs) and the
    HIP path's post-activation tensors (train BatchNorm+ReLU and conv epilogue ReLU), in call order."""
    import torch.nn.functional as F

    from diff_sal_amd import autograd_ops as ag

    ref, hip = [], []
    orig_relu, o_bn, o_conv = F.relu, ag.batchnorm_relu_train, ag.conv

    def spy_relu(v, *a, **k):
        ref.append(v.detach())
        return orig_relu(v, *a, **k)

    def spy_bn(x_, bn, relu=True):
        y = o_bn(x_, bn, relu)
        hip.append(y.detach())
        return y

    def spy_conv(x_, w, **k):
        y = o_conv(x_, w, **k)
        if k.get("act", 0) == 1:
            hip.append(y.detach())
        return y

    def install():
        orc.F.relu, ag.batchnorm_relu_train, ag.conv = spy_relu, spy_bn, spy_conv

    def remove():
        orc.F.relu, ag.batchnorm_relu_train, ag.conv = orig_relu, o_bn, o_conv

    def flips():
        assert len(ref) == len(hip) and ref, (len(ref), len(hip))
        n = 0
        for r, h in zip(ref, hip):
            if r.dim() == 5:
                r = r.squeeze(2)
            n += int(((r.permute(0, 2, 3, 1).reshape(-1) > 0) != (h.cpu().reshape(-1) > 0)).sum())
        return n

    return install, remove, flips


@pytest.mark.parametrize("av", [False, True])
def test_train_forward_and_all_parameter_gradients_match_oracle_autograd(av):
    """Gradient parity is asserted on an input where the HIP forward and the oracle forward take the SAME branch of every
    ReLU (counted here, not assumed): candidate inputs are tried in a fixed order and the first flip-free one is used.  A
    flipped element is two correct fp32 roundings landing on different sides of the kink, not a kernel error, and any
    change of summation order in any forward kernel moves which elements are at risk (module docstring)."""
    last = None
    for tag in ("train", "train.b", "train.c", "train.d", "train.e", "train.f"):
        n_flips, report = _gradient_case(av, tag)
        print(f"input {tag!r}: {n_flips} ReLU sign disagreements between the two forwards")
        if n_flips == 0:
            report()
            return
        last = n_flips
    raise AssertionError(f"no flip-free input among the candidates (last had {last} flips)")


def _gradient_case(av, tag):
    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    x, feats, audio = orc.synth_inputs(cfg, 2, av, tag=tag)
    x0 = torch.sigmoid(orc.synth_tensor(tag + ".x0", (2, 1, *cfg.img_size)))
    t = torch.tensor([321, 321])
    install, remove, flips = _relu_spies()
    install()
    try:
        return _gradient_case_body(cfg, sd, x, feats, audio, x0, t, flips)
    finally:
        remove()


def _gradient_case_body(cfg, sd, x, feats, audio, x0, t, flips):
    # reference: autograd through the oracle with batch-statistics BN
    leaf = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
    # the conditioning features come from trainable encoders upstream (MViT, AudioAttnNet): they need gradients too
    feats_r = [f.clone().requires_grad_(True) for f in feats]
    audio_r = None if audio is None else audio.clone().requires_grad_(True)
    x_r = x
    orc.BN_TRAIN = True
    try:
        pred = orc.salunet_forward(leaf, cfg, x_r, t, feats_r, audio_r)
    finally:
        orc.BN_TRAIN = False
    loss = ((pred - x0) ** 2).sum(dim=(1, 2, 3)).mean()
    loss.backward()

    net = build(cfg, sd)
    net.train()
    net.dropout_p = 0.0
    feats_d = [f.to(DEV).requires_grad_(True) for f in feats]
    audio_d = None if audio is None else audio.to(DEV).requires_grad_(True)
    x_d = x.to(DEV)
    out = net(x_d, t.to(DEV), feats_d, audio_d)
    n_flips = flips()

    def report():
        assert (out.detach().cpu() - pred.detach()).abs().max().item() < 1e-4
        l2 = ((out - x0.to(DEV)) ** 2).sum(dim=(1, 2, 3)).mean()
        l2.backward()
        assert abs(l2.item() - loss.item()) < 1e-3 * abs(loss.item())
        # gradient scale of the network: parameters whose true gradient is zero by symmetry (e.g. the K-projection
        # LayerNorm bias and proj_k bias: softmax is invariant to a shift common to all keys) hold pure rounding noise
        scale = torch.stack([g.grad.abs().max() for g in leaf.values() if g.grad is not None]).median().item()
        worst, checked = [], 0
        for name, p in net.named_parameters():
            ref = leaf[name].grad
            if ref is None:
                assert p.grad is None or float(p.grad.abs().max()) < 1e-6 * scale, name
                continue
            got = p.grad.cpu() if p.grad is not None else torch.zeros_like(ref)
            err = (got - ref).abs().max().item()
            tol = 5e-3 * ref.abs().max().item() + 5e-5 * scale
            worst.append((err / tol, name, err, ref.abs().max().item()))
            checked += 1
        worst.sort()
        print("worst gradient errors (fraction of tolerance, name, abs err, ref max):")
        for w in worst[-12:]:
            print("   ", w)
        print("median fraction:", worst[len(worst) // 2][0])
        assert checked > 150
        assert worst[-1][0] < 1.0, worst[-1]
        # input gradients (feat_list[3] is never read by the reference graph: quirk Q3, its gradient is None / zero)
        # (x_t itself is data -- R/diffusion_trainer.py:106-117 -- and gets no gradient: conv_in's backward is parameters-only)
        pairs = [(f"feat{i}", a, b) for i, (a, b) in enumerate(zip(feats_d, feats_r))]
        if audio is not None:
            pairs.append(("audio", audio_d, audio_r))
        for nm, a, b in pairs:
            if b.grad is None or float(b.grad.abs().max()) == 0.0:
                assert a.grad is None or float(a.grad.abs().max()) <= 1e-6 * scale, nm
                continue
            assert a.grad is not None, nm
            err = (a.grad.cpu() - b.grad).abs().max().item()
            assert err < 5e-3 * b.grad.abs().max().item() + 5e-5 * scale, (nm, err, b.grad.abs().max().item())

    return n_flips, report


def _oracle_train_steps(cfg, sd, batches, av, n_steps, lr):
    """The reference's step restated on the CPU: q_sample, train-mode forward, MSE, clip 1.0, torch Adam."""
    from diff_sal_amd.diffusion_utils import get_beta_schedule, to_torch

    betas = to_torch(get_beta_schedule("cosine", beta_start=1e-4, beta_end=0.02, num_diffusion_timesteps=1000))
    a_hat = (1.0 - betas).cumprod(dim=0)
    names = [k for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k]
    leaf = {k: (torch.nn.Parameter(v.clone()) if k in names else v.clone()) for k, v in sd.items()}
    opt = torch.optim.Adam([leaf[k] for k in names], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    losses, grads = [], None
    for it in range(n_steps):
        sal, dq, noise, t0, feats, audio = batches[it]
        x0 = sal + 0.01 * dq
        x_t = a_hat[t0].sqrt() * x0 + (1 - a_hat[t0]).sqrt() * noise
        orc.BN_TRAIN = True
        try:
            pred = orc.salunet_forward(leaf, cfg, x_t, torch.full((sal.shape[0],), t0), feats, audio)
        finally:
            orc.BN_TRAIN = False
        loss = (pred - x0).square().sum(dim=(1, 2, 3)).mean(dim=0)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([leaf[k] for k in names], 1.0)
        if it == 0:
            grads = {k: (None if leaf[k].grad is None else leaf[k].grad.clone()) for k in names}
        opt.step()
        losses.append(loss.item())
    return losses, {k: leaf[k].detach() for k in names}, grads


@pytest.mark.parametrize("av", [False, True])
def test_training_steps_match_oracle_adam(av):
    """Three full steps (prepare_data -> forward -> MSE -> backward -> clip -> Adam) of DiffusionTrainStep against
    the oracle + torch.optim.Adam.  lr = the reference value 1e-4 (R/cfgs/diffusion.yml:56)."""
    from diff_sal_amd.train_step import DiffusionTrainStep

    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    B, n_steps, lr = 2, 3, 1e-4
    batches = []
    for it in range(n_steps):
        x, feats, audio = orc.synth_inputs(cfg, B, av, tag=f"ts{it}")
        sal = torch.sigmoid(orc.synth_tensor(f"ts{it}.sal", (B, 1, *cfg.img_size)))
        batches.append((sal, orc.synth_tensor(f"ts{it}.dq", tuple(sal.shape)), x, (137 * (it + 1)) % 1000, feats, audio))
    ref_losses, ref_params, ref_grads = _oracle_train_steps(cfg, sd, batches, av, n_steps, lr)

    net = build(cfg, sd)
    net.dropout_p = 0.0
    ts = DiffusionTrainStep(net, lr=lr, grad_clip=1.0)
    assert ts.flat.live_numel == sum(p.numel() for p in net.parameters())
    losses = []
    for it in range(n_steps):
        sal, dq, noise, t0, feats, audio = batches[it]
        cond = {"feat_list": [f.to(DEV) for f in feats], "audio_feat": None if audio is None else audio.to(DEV)}
        loss = ts.step(sal.to(DEV), cond, t0=t0, noise=noise.to(DEV), dequant_noise=dq.to(DEV))
        losses.append(loss.item())
    print("losses", losses, "ref", ref_losses, "grad norm (last)", ts.last_norm.item())
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) < 1e-3 * abs(b), (losses, ref_losses)
    # parameters after three Adam steps: the step is ~lr * sign-like, so compare displacement in units of lr; parameters
    # whose gradient is rounding noise (zero by symmetry) may move in either direction and are skipped
    gscale = torch.stack([g.abs().max() for g in ref_grads.values() if g is not None]).median().item()
    # Why the bounds are loose: after clipping by a norm of ~6e3 most gradient entries are ~1e-8 = Adam's eps, where the
    # update lr*g/(|g|+eps) is linear in g, so a 1e-3-of-max gradient difference (fp32 order of summation, and the odd
    # ReLU whose pre-activation of ~1e-7 falls on the other side of zero) becomes a few % of one step.  The Adam kernel
    # itself is pinned to 1e-6 against torch.optim.Adam in test_gpu_train_ops.py.
    errs = []
    for name, p in net.named_parameters():
        g = ref_grads[name]
        if g is None or g.abs().max().item() < 1e-3 * gscale:
            continue
        mask = g.abs() > 1e-2 * g.abs().max()
        d_got = (p.detach().cpu() - sd[name])[mask]
        d_ref = (ref_params[name] - sd[name])[mask]
        errs.append(((d_got - d_ref).abs().max().item() / (n_steps * lr), name))
    errs.sort()
    print("displacement error / (steps*lr): median %.4f, worst %s" % (errs[len(errs) // 2][0], errs[-3:]))
    assert len(errs) > 100
    assert errs[len(errs) // 2][0] < 0.15 and errs[-1][0] < 1.0, errs[-3:]
    # eval-mode forward after training uses the UPDATED weights (packed-weight cache invalidated by the optimizer)
    net.eval()
    sal, dq, noise, t0, feats, audio = batches[0]
    with torch.no_grad():
        out = net(noise.to(DEV), torch.full((B,), t0, device=DEV), [f.to(DEV) for f in feats],
                  None if audio is None else audio.to(DEV))
    full_sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = orc.salunet_forward(full_sd, cfg, noise, torch.full((B,), t0), feats, audio)
    assert (out.cpu() - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize("name", ["train_tiny_av", "train_tiny_vis"])
def test_training_step_matches_reference_fixture(golden_dir, name):
    """One step of DiffusionTrainStep vs the REAL reference's step (tests/golden/train_*.npz, oracle/gen_golden.py::
    gen_train_step: .train() mode, dropout off, MSE, clip 1.0, Adam 1e-4): loss, output, every parameter gradient,
    clip norm, BatchNorm running statistics and the updated parameters.  The fixture inputs were chosen so that no ReLU
    pre-activation sits within 1.5e-6 of zero (see the module docstring)."""
    from diff_sal_amd.train_step import DiffusionTrainStep
    from tests._cases import sampled_err, train_fixture_inputs

    cfg, sd, sal, dq, noise, t0, feats, audio, g = train_fixture_inputs(golden_dir, name)
    net = build(cfg, sd)
    net.dropout_p = 0.0
    ts = DiffusionTrainStep(net, lr=1e-4, grad_clip=1.0)
    cond = {"feat_list": [f.to(DEV) for f in feats], "audio_feat": None if audio is None else audio.to(DEV)}
    x0, x_t, t, _ = ts.prepare_data(sal.to(DEV), t0=t0, noise=noise.to(DEV), dequant_noise=dq.to(DEV))
    net.train()
    with torch.no_grad():
        pred = net.forward_train(x_t, t, cond["feat_list"], cond["audio_feat"])   # output check; running stats advance once
    e, _ = sampled_err(pred, g, "pred")
    assert e < 1e-4
    for k, b in net.named_buffers():            # running statistics after exactly one train-mode forward
        if "running" in k:
            e, m = sampled_err(b, g, "buf." + k)
            assert e < 1e-5 * max(m, 1.0), (k, e, m)
    net.load_state_dict(sd)                     # rewind the buffers; parameters are untouched
    loss = ts.loss_and_backward(x0, x_t, t, cond)
    assert abs(loss.item() - float(g["loss"])) < 1e-4 * float(g["loss"])
    no_grad = set(g["no_grad"].tolist())
    names = [k for k, _ in net.named_parameters()]
    gmax = max(float(g[f"tap.grad.{k}.stats"][2]) for k in names if k not in no_grad)
    worst = []
    for k, p in net.named_parameters():
        if k in no_grad:
            assert p.grad is None or float(p.grad.abs().max()) <= 1e-6 * gmax, k
            continue
        e, m = sampled_err(p.grad, g, "grad." + k)
        worst.append((e / (1e-4 * m + 2e-6 * gmax), k, e, m))
    worst.sort()
    print("worst gradient errors (fraction of tolerance 1e-4*max + 2e-6*gmax):", worst[-4:])
    assert worst[-1][0] < 1.0, worst[-1]
    ts.optimizer_step()
    assert abs(ts.last_norm.item() - float(g["total_norm"])) < 1e-4 * float(g["total_norm"])
    for k, p in net.named_parameters():
        if k in no_grad or float(g[f"tap.grad.{k}.stats"][2]) < 1e-4 * gmax:
            continue
        e, _ = sampled_err(p, g, "after." + k)
        # after clipping by ~3e3-6e3 most entries are ~1e-8 = Adam's eps, where the update lr*g/(|g|+eps) is linear in g:
        # a 1e-3-of-max gradient difference becomes tenths of one step (the kernel itself is pinned to 1e-6 in test_gpu_train_ops)
        assert e < 5e-5, (k, e)                 # half of one Adam step (lr = 1e-4)


def test_end_to_end_training_through_video_saliency_model_with_a_torch_encoder():
    """The drop-in story for training: VideoSaliencyModel with an ordinary PyTorch visual encoder (stand-in for MViT,
    which is outside the path) in front of the HIP denoiser.  DiffusionTrainStep flattens BOTH modules' parameters; the
    encoder's gradients come through the denoiser's hand-written backward (feature gradients) and torch autograd."""
    from diff_sal_amd import VideoSaliencyModel
    from diff_sal_amd.train_step import DiffusionTrainStep

    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    H, W = cfg.img_size

    class ToyEncoder(torch.nn.Module):       # clip [B,3,8,H,W] -> 4 feature maps, coarsest first (R/models/diff_model.py:96-104)
        def __init__(self):
            super().__init__()
            self.proj = torch.nn.ModuleList([torch.nn.Conv3d(3, c, 1) for c in cfg.up_channel])

        def forward(self, clip):
            outs = []
            for p, s in zip(self.proj, (32, 16, 8, 4)):
                outs.append(p(torch.nn.functional.adaptive_avg_pool3d(clip, (8, H // s, W // s))))
            return outs

    torch.manual_seed(0)
    model = VideoSaliencyModel(channel_list=None, visual_net=ToyEncoder(), decoder_net=build(cfg, sd)).to(DEV)
    model.decoder_net.dropout_p = 0.0
    ts = DiffusionTrainStep(model, lr=2e-4, grad_clip=1.0)
    n_dec = sum(p.numel() for p in model.decoder_net.parameters())
    n_enc = sum(p.numel() for p in model.visual_net.parameters())
    assert ts.flat.live_numel == n_dec + n_enc
    enc_before = [p.detach().clone() for p in model.visual_net.parameters()]
    g = torch.Generator().manual_seed(5)
    clip = torch.randn((2, 3, 8, H, W), generator=g).to(DEV)
    sal = torch.rand((2, 1, H, W), generator=g).to(DEV)
    noise = torch.randn((2, 1, H, W), generator=g).to(DEV)
    losses = [ts.step(sal, {"img": clip}, t0=300, noise=noise, dequant_noise=torch.zeros_like(sal)).item() for _ in range(6)]
    print("losses", losses)
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0]                                     # same batch every step: the loss must go down
    moved = [float((p.detach() - b).abs().max()) for p, b in zip(model.visual_net.parameters(), enc_before)]
    assert min(moved[:6]) > 0.0                                       # the three feature maps the graph reads train the encoder
    assert all(p.grad is None or p.grad.data_ptr() >= ts.flat.flat_g.data_ptr() for p in model.parameters())


@pytest.mark.parametrize("B", [1, 4])
def test_full_size_training_gradients_match_oracle_autograd(B):
    """BASELINE-size (224x384, 768/384/192/96 channels) audio-visual clips, B=1 and B=4 (the per-GPU batch of BASELINE
    configs[3]): every parameter gradient of the HIP path vs autograd through the CPU oracle.  This is the only test that runs the training kernels in the configurations the
    benchmark uses (streaming token GEMMs in the data gradient, all weight-gradient tile shapes and split plans, the
    segmented GEMMs of the attention backward at Lq=5376, the disjoint-tap data gradients, 9.3 M-element reductions).
    With 23.8 M ReLU pre-activations sign flips are certain (measured on this very input with tests/diagnostics/relu_flip_census.py
    against an fp64 run: 13 flips, 251 pre-activations within 1e-5 of zero; each flip perturbs everything upstream by ~1e-3), so this is a gross-error detector: median error over parameters < 5e-3 of each tensor's max, worst < 5e-2.
    (It caught a column-sum kernel that dropped channels >= 1024: error 0.91 on the 1536-wide MLP bias.)  Kernel-level
    accuracy at these shapes is pinned separately, kink-free, in test_gpu_train_ops.py (full-size cases)."""
    torch.manual_seed(0)
    cfg = orc.SalUNetConfig()
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    tag = "fulltrain" if B == 1 else f"fulltrain{B}"
    x, feats, audio = orc.synth_inputs(cfg, B, True, tag=tag)
    x0 = torch.sigmoid(orc.synth_tensor(tag + ".x0", (B, 1, *cfg.img_size)))
    t = torch.tensor([637] * B)
    leaf = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
    orc.BN_TRAIN = True
    try:
        pred = orc.salunet_forward(leaf, cfg, x, t, feats, audio)
    finally:
        orc.BN_TRAIN = False
    loss = ((pred - x0) ** 2).sum(dim=(1, 2, 3)).mean()
    loss.backward()

    net = build(cfg, sd)
    net.train()
    net.dropout_p = 0.0
    out = net(x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], audio.to(DEV))
    assert (out.detach().cpu() - pred.detach()).abs().max().item() < 1e-4
    l2 = ((out - x0.to(DEV)) ** 2).sum(dim=(1, 2, 3)).mean()
    l2.backward()
    assert abs(l2.item() - loss.item()) < 1e-4 * abs(loss.item())
    scale = torch.stack([g.grad.abs().max() for g in leaf.values() if g.grad is not None]).median().item()
    errs = []
    for name, p in net.named_parameters():
        ref = leaf[name].grad
        if ref is None or ref.abs().max().item() < 1e-4 * scale:
            continue
        errs.append(((p.grad.cpu() - ref).abs().max().item() / ref.abs().max().item(), name))
    errs.sort()
    med, p90, worst = errs[len(errs) // 2][0], errs[int(0.9 * len(errs))][0], errs[-1]
    print("full-size gradient errors relative to each tensor's max: median %.2e, p90 %.2e, worst %s (%d tensors)"
          % (med, p90, worst, len(errs)))
    assert len(errs) > 150
    assert med < 5e-3 and p90 < 1e-2 and worst[0] < 5e-2, (med, p90, worst)


@pytest.mark.parametrize("B,av", [(1, True), (3, False)])
def test_train_step_odd_batches_and_dropout_determinism(B, av):
    """Ragged cases of the training forward: batch 1 and 3 (BatchNorm statistics over 9 / 27 frames), active dropout with an
    explicit seed is reproducible and differs from another seed; an empty batch raises like nn.BatchNorm2d does."""
    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    x, feats, audio = orc.synth_inputs(cfg, B, av, tag=f"odd{B}")
    t = torch.full((B,), 77)
    leaf = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
    orc.BN_TRAIN = True
    try:
        pred = orc.salunet_forward(leaf, cfg, x, t, feats, audio)
    finally:
        orc.BN_TRAIN = False
    net = build(cfg, sd)
    net.train()
    args = (x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], None if audio is None else audio.to(DEV))
    net.dropout_p = 0.0
    out = net(*args)
    assert (out.detach().cpu() - pred.detach()).abs().max().item() < 1e-4
    net.dropout_p = 0.1
    a = net.forward_train(*args, dropout_seed=1234)
    b = net.forward_train(*args, dropout_seed=1234)
    c = net.forward_train(*args, dropout_seed=99)
    assert torch.equal(a, b)
    if av:   # visual-only output does not see the ResnetBlock path in a way dropout could change much; AV must differ
        assert (a - c).abs().max().item() > 0
    with pytest.raises(RuntimeError):
        net.forward_train(args[0][:0], args[1][:0], [f[:0] for f in args[2]], None if args[3] is None else args[3][:0])


def test_fused_tape_nodes_leave_every_gradient_where_the_separate_nodes_put_it(monkeypatch):
    """LayerNorm + residual accumulation and GELU + fc2 are single tape nodes (autograd_ops.layernorm_fork / linear(in_gelu)); with
    the switches off the same step runs on the separate nodes.  Same forward bit for bit, gradients equal up to the order of one
    addition per element.  FUSE_RELPOS is toggled along with them, but the denoiser built here has no rel-pos attention: the encoder's
    fused node (encoder_autograd.relpos_attention) is compared with its two-node form in
    tests/test_gpu_encoder_nodes.py::test_relpos_attention_node_against_the_two_nodes_and_fp64."""
    from diff_sal_amd import autograd_ops as ag

    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    x, feats, audio = orc.synth_inputs(cfg, 2, True, tag="fuse")
    t = torch.full((2,), 311)
    args = (x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], audio.to(DEV))
    gy = orc.synth_tensor("fuse_gy", tuple(x.shape), 1.0).to(DEV)

    def run(fused):
        for name in ("FUSE_LN_FORK", "FUSE_GELU", "FUSE_RELPOS"):
            monkeypatch.setattr(ag, name, fused)
        net = build(cfg, sd)
        net.train()
        net.dropout_p = 0.0
        out = net(*args)
        out.backward(gy)
        return out.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    out_f, g_f = run(True)
    out_s, g_s = run(False)
    assert torch.equal(out_f, out_s)
    assert g_f.keys() == g_s.keys() and len(g_f) > 100
    for k in g_f:
        den = g_s[k].abs().max().item() + 1e-12
        assert (g_f[k] - g_s[k]).abs().max().item() / den < 2e-5, k


def test_train_step_with_the_reference_loss_dictionary_and_a_scheduler():
    """DiffusionTrainStep(loss_config=...) trains on get_lossv2's total (R/diffusion_trainer.py:219: MSE main term + weighted
    CC / NSS here), every term's gradient reaching the parameters: loss values equal the stand-alone losses of the same
    prediction, the gradient equals autograd of (mse + cc + nss) assembled by hand from the same operators, the update differs
    from the MSE-only step, and torch's MultiStepLR drives the flat Adam's learning rate."""
    from diff_sal_amd import autograd_ops as ag
    from diff_sal_amd import sal_losses
    from diff_sal_amd.train_step import DiffusionTrainStep

    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    B = 2
    x, feats, audio = orc.synth_inputs(cfg, B, True, tag="losshook")
    sal = torch.sigmoid(x).to(DEV)
    cond = {"feat_list": [f.to(DEV) for f in feats], "audio_feat": audio.to(DEV)}
    lc = type("L", (), dict(loss_kl=False, loss_ce=False, loss_mse=True, mse_weight=1.0, loss_cc=True, cc_weight=-300.0,
                            loss_sim=False, sim_weight=0.0, loss_nss=True, nss_weight=-100.0))()
    config = type("C", (), {"loss": lc})()

    def make(**kw):
        net = build(cfg, sd)
        net.dropout_p = 0.0
        return net, DiffusionTrainStep(net, lr=1e-3, gaussian_dequantization=False, **kw)

    noise = torch.randn(sal.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    net_a, ts_a = make(loss_config=config)
    x0, x_t, t, _ = ts_a.prepare_data(sal, t0=321, noise=noise)
    loss_a = ts_a.loss_and_backward(x0, x_t, t, cond)
    d = ts_a.last_losses
    assert set(d) == {"total", "main", "cc", "sim", "nss"}
    assert abs(float(d["total"]) - float(d["main"] + d["cc"] + d["sim"] + d["nss"])) < 1e-5 * max(1.0, abs(float(d["total"])))
    assert float(loss_a) == pytest.approx(float(d["total"]))
    g_a = ts_a.flat.flat_g.clone()
    # the same total assembled by hand on a second copy of the network
    net_b, ts_b = make(loss_fn=lambda p, g: ag.mse_loss(p, g, 1.0 / p.shape[0]) - 300.0 * sal_losses.cc_s2(p, g) - 100.0 * sal_losses.nss2(p, g))
    loss_b = ts_b.loss_and_backward(x0, x_t, t, cond)
    assert float(loss_b) == pytest.approx(float(loss_a), rel=1e-5)
    assert (ts_b.flat.flat_g - g_a).abs().max().item() <= 1e-5 * g_a.abs().max().item()
    # MSE only: a different gradient
    net_c, ts_c = make()
    ts_c.loss_and_backward(x0, x_t, t, cond)
    assert (ts_c.flat.flat_g - g_a).abs().max().item() > 1e-3 * g_a.abs().max().item()
    # scheduler on the optimizer face: lr 1e-3 for two steps, then 1e-4
    sched = torch.optim.lr_scheduler.MultiStepLR(ts_a.optimizer, milestones=[2], gamma=0.1)
    before = ts_a.flat.flat_p.clone()
    deltas = []
    for _ in range(3):
        ts_a.optimizer.step()
        sched.step()
        deltas.append((ts_a.flat.flat_p - before).abs().max().item())
        before = ts_a.flat.flat_p.clone()
    assert ts_a.lr == pytest.approx(1e-4) and ts_a.step_count == 3
    assert deltas[2] < 0.2 * deltas[0]              # Adam's step size follows the learning rate
