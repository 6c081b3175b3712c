"""Device noise on the GPU: the Philox4x32-10 kernels against the NumPy restatement, the fused stochastic step tail against
the stand-alone launches, layout independence of whole trajectories, and graph replay of stochastic trajectories."""
import numpy as np
import pytest
import torch

from oracle import salunet_oracle as orc
from tests import _philox_ref as ref
from tests._cases import CASES
from tests.test_gpu_salunet import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS6 = [0, 7, (1 << 32) + 5, 1 << 40, 3, 123456789]


class Top(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.decoder_net = net
        self.audio_net = None
        self.visual_net = None


@pytest.fixture(scope="module")
def tiny6():
    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    _, feats, audio = orc.synth_inputs(cfg, 6, True, tag="noise6")
    return Top(build(cfg, sd)), [f.to(DEV) for f in feats], audio.to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("seed", [1234, (0x9A << 32) | 0x1234567])
@pytest.mark.parametrize("per", [86016, 1001])
def test_raw_bits_equal_the_restatement(seed, per):
    from diff_sal_amd import ops

    ids = [0, (1 << 32) + 5, 1 << 40]
    for draw in (0, 1, 1000):
        got = _u32(ops.philox_bits(ids, seed, draw, per))
        assert got.shape == (3, per) and np.array_equal(got, ref.bits(seed, ids, draw, per))
    # ids already on the device are used as they are
    dev_ids = torch.tensor(ids, dtype=torch.int64, device=DEV)
    assert np.array_equal(_u32(ops.philox_bits(dev_ids, seed, 1, per)), ref.bits(seed, ids, 1, per))


@pytest.mark.parametrize("shape", [(1, 224, 384), (1, 7, 143)])
def test_normals_against_the_fp64_restatement(shape):
    """Bar 2e-5 absolute: |z| <= 5.77, the angle carries up to 2 pi 2^-24 = 3.7e-7, five fp32 operations of ~2 ulp each give
    <= 5.6e-6; a plain fp32 evaluation of the formulas in NumPy measures 3.8e-6."""
    from diff_sal_amd import ops

    ids, seed = [3, (1 << 32) + 5, 1 << 40], (7 << 32) | 99
    per = shape[0] * shape[1] * shape[2]
    for draw in (0, 7):
        z = ops.philox_normal(ids, seed, draw, shape)
        assert z.shape == (3,) + shape and z.dtype == torch.float32
        want = ref.normals(seed, ids, draw, per)
        err = np.abs(z.cpu().numpy().reshape(3, per).astype(np.float64) - want).max()
        print(f"philox_normal {shape} draw {draw}: max |z - fp64| = {err:.3e}")
        assert err < 2e-5
        assert np.abs(want).max() <= 5.77
    half = ops.philox_normal(ids, seed, 7, shape, scale=0.5)
    assert torch.equal(half, 0.5 * z)


def test_statistics_of_16_maps():
    """Five-sigma bounds over n = 16 x 224 x 384 draws: |mean| < 5 / sqrt(n) = 4.3e-3, |var - 1| < 5 sqrt(2 / n) = 6.0e-3."""
    from diff_sal_amd import ops

    z = ops.philox_normal(list(range(3, 19)), 1234, 7, (1, 224, 384)).double()
    n = z.numel()
    assert n == 1376256
    mean, var = z.mean().item(), z.var(unbiased=False).item()
    print(f"device noise over {n} draws: mean {mean:.3e}, var - 1 {var - 1:.3e}")
    assert abs(mean) < 5 / n ** 0.5 and abs(var - 1) < 5 * (2 / n) ** 0.5
    # one clip's stream of the same length (seed 1234, id 3, draw 7; the restatement gives mean 3.3e-4, var - 1 = -8.0e-4)
    z1 = ops.philox_normal([3], 1234, 7, (16, 224, 384)).double()
    mean, var = z1.mean().item(), z1.var(unbiased=False).item()
    print(f"one clip, {n} draws: mean {mean:.3e}, var - 1 {var - 1:.3e}")
    assert abs(mean) < 5 / n ** 0.5 and abs(var - 1) < 5 * (2 / n) ** 0.5
    assert abs(mean - 3.318e-4) < 1e-5 and abs(var - 1 + 7.975e-4) < 1e-5


def _layouts(run):
    """Per-clip results of ``run(ids, rows)`` in three layouts: B = 6; 4 + 2; six times B = 1 with the ids permuted."""
    whole = run(IDS6, list(range(6)))
    split = torch.cat([run(IDS6[:4], [0, 1, 2, 3]), run(IDS6[4:], [4, 5])])
    single = [None] * 6
    for i in (4, 0, 5, 2, 1, 3):
        single[i] = run([IDS6[i]], [i])
    return whole, split, torch.cat(single)


def test_initial_noise_and_trajectories_do_not_depend_on_the_layout(tiny6):
    from diff_sal_amd.sampling import DiffusionSampler

    top, feats, audio = tiny6
    shape = (1, 64, 128)

    def sel(rows):
        return [f[rows] for f in feats], audio[rows]

    for name, kw in (("ddim", dict(sample_type="ddim", eta=1.0)), ("ddpm", dict(sample_type="ddpm"))):
        s = DiffusionSampler(top, timesteps=4, noise_source="device", seed=11, **kw)
        s2 = DiffusionSampler(top, timesteps=4, noise_source="device", seed=12, **kw)
        xa, xb, xc = _layouts(lambda ids, rows: s.initial_noise(ids, (len(ids),) + shape))
        assert torch.equal(xa, xb) and torch.equal(xa, xc)
        assert np.abs(xa.cpu().numpy().reshape(6, -1) - ref.normals(11, IDS6, 0, 64 * 128)).max() < 2e-5      # draw 0

        def run(ids, rows, smp=s):
            f, a = sel(rows)
            fn = smp.sample_ddim if name == "ddim" else smp.sample_ddpm
            return fn(None, f, a, clip_ids=ids)

        a, b, c = _layouts(run)
        for i in range(6):
            print(f"{name} clip {i}: |B=6 - (4+2)| = {(a[i] - b[i]).abs().max().item():.3e}, "
                  f"|B=6 - B=1| = {(a[i] - c[i]).abs().max().item():.3e}")
        for i in range(6):
            assert torch.equal(a[i], b[i]) and torch.equal(a[i], c[i]), (name, i)
        assert torch.equal(run(IDS6, list(range(6))), a)                         # same ids and seed twice
        other = run(IDS6, list(range(6)), s2)
        assert not torch.equal(other, a) and (other - a).abs().max().item() > 1e-4
        # x given by the caller == x=None for the same ids
        f, au = sel(list(range(6)))
        fn = s.sample_ddim if name == "ddim" else s.sample_ddpm
        assert torch.equal(fn(xa, f, au, clip_ids=IDS6), a)


def test_fused_stochastic_tail_equals_the_stand_alone_launches(tiny6):
    from diff_sal_amd.sampling import DiffusionSampler

    top, feats, audio = tiny6
    f2, a2 = [f[:2] for f in feats], audio[:2]
    ids = IDS6[2:4]
    x = DiffusionSampler(top, noise_source="device", seed=5).initial_noise(ids, (2, 1, 64, 128))
    # clip_passes: one clip per denoiser pass (the default with device noise) and the batched passes torch noise uses
    for passes in (True, False):
        for eta in (0.0, 0.5, 1.0):
            kw = dict(timesteps=5, sample_type="ddim", eta=eta, noise_source="device", seed=5, hip_graph=False, clip_passes=passes)
            fused = DiffusionSampler(top, fused_update=True, **kw).sample_ddim(x, f2, a2, clip_ids=ids)
            plain = DiffusionSampler(top, fused_update=False, **kw).sample_ddim(x, f2, a2, clip_ids=ids)
            assert torch.equal(fused, plain), (passes, eta)
            if eta == 0.0:      # nothing is drawn: the torch-noise sampler takes the fused tail too, and both equal its old loop
                for fu in (True, False):
                    tor = DiffusionSampler(top, timesteps=5, sample_type="ddim", eta=0.0, fused_update=fu, hip_graph=False,
                                           clip_passes=passes)
                    assert tor.noise_source == "torch" and torch.equal(tor.sample_ddim(x, f2, a2), fused), (passes, fu)
        kw = dict(timesteps=5, sample_type="ddpm", noise_source="device", seed=5, hip_graph=False, clip_passes=passes)
        fused = DiffusionSampler(top, fused_update=True, **kw).sample_ddpm(x, f2, a2, clip_ids=ids)
        plain = DiffusionSampler(top, fused_update=False, **kw).sample_ddpm(x, f2, a2, clip_ids=ids)
        assert torch.equal(fused, plain), passes
        assert torch.isfinite(fused).all() and (fused - x).abs().max().item() > 1e-3
    # one clip: the defaults of both noise sources agree at eta = 0
    x1, f1, a1 = x[:1], [f[:1] for f in f2], a2[:1]
    dev0 = DiffusionSampler(top, timesteps=5, sample_type="ddim", noise_source="device", hip_graph=False)
    tor0 = DiffusionSampler(top, timesteps=5, sample_type="ddim", fused_update=False, hip_graph=False)
    assert torch.equal(dev0.sample_ddim(x1, f1, a1), tor0.sample_ddim(x1, f1, a1))


@pytest.mark.parametrize("HW", [(64, 128), (9, 13)])
def test_tail_kernel_against_the_launches_it_replaces(HW):
    from diff_sal_amd import ops

    H, W = HW
    h, w = (32, 64) if HW == (64, 128) else (5, 7)
    g = torch.Generator(device=DEV).manual_seed(3)
    s_low = torch.rand(2, h, w, 1, device=DEV, generator=g)
    xs, mp = torch.randn(2, 1, H, W, device=DEV, generator=g), torch.randn(2, 1, H, W, device=DEV, generator=g)
    ex, e0, A, c0, c1 = 1.7, -0.6, 0.9, -0.3, 0.2
    m_ref, xn_ref, x0_ref = ops.resize_update(s_low, xs, mp, ex, e0, A, c0, c1, want_x0=True)
    m, xn, x0 = ops.resize_update_noise(s_low, xs, mp, ex, e0, A, c0, c1, want_x0=True)
    assert torch.equal(m, m_ref) and torch.equal(xn, xn_ref) and torch.equal(x0, x0_ref)
    m1, xn1, _ = ops.resize_update_noise(s_low, xs, None, ex, e0, A, c0)
    assert torch.equal(xn1, ops.resize_update(s_low, xs, None, ex, e0, A, c0, 0.0)[1]) and torch.equal(m1, m_ref)
    # with noise: x_next = b0 x0 + A x + cz z + c0 m + c1 m_prev, first term a product, every further one an fma
    ids, seed = ops.noise_key([(1 << 32) + 5, 3], 77, DEV)
    b0, cz = 0.8, 0.45
    z = ops.philox_normal(ids, seed, 4, (1, H, W))
    m2, xn2, x02 = ops.resize_update_noise(s_low, xs, mp, ex, e0, A, c0, c1, b0=b0, cz=cz, noise_key=(ids, seed, 4), want_x0=True)
    assert torch.equal(m2, m_ref) and torch.equal(x02, x0_ref)
    want = ops.axpbypcz(ops.axpbypcz(x0_ref, b0, xs, A, z, cz), 1.0, m_ref, c0, mp, c1)
    assert torch.equal(xn2, want)
    # the DDIM form (A = 0, no m_prev) and the DDPM form (c0 = 0): the sampler's own launch order
    _, xd, _ = ops.resize_update_noise(s_low, xs, None, ex, e0, 0.0, c0, b0=b0, cz=cz, noise_key=(ids, seed, 4))
    assert torch.equal(xd, ops.axpbypcz(x0_ref, b0, z, cz, m_ref, c0))
    _, xp, _ = ops.resize_update_noise(s_low, xs, None, 0.0, 1.0, A, 0.0, b0=b0, cz=cz, noise_key=(ids, seed, 4))
    assert torch.equal(xp, ops.axpbypcz(ops.axpbypcz(x0_ref, b0, xs, A), 1.0, z, cz))
    with pytest.raises(ValueError, match="noise_key"):
        ops.resize_update_noise(s_low, xs, None, ex, e0, A, c0, cz=0.3)


def test_stochastic_trajectories_replay_from_a_graph(tiny6):
    from diff_sal_amd import ops
    from diff_sal_amd.sampling import DiffusionSampler

    top, feats, audio = tiny6
    f2, a2 = [f[:2] for f in feats], audio[:2]
    kw = dict(timesteps=4, sample_type="ddim", eta=1.0, noise_source="device", seed=21)
    auto = DiffusionSampler(top, **kw)
    eager = DiffusionSampler(top, hip_graph=False, **kw)
    ids_a, ids_b = IDS6[:2], IDS6[3:5]
    first = auto.sample_ddim(None, f2, a2, clip_ids=ids_a)
    assert len(auto._graphs) == 1 and next(iter(auto._graphs.values()))[1] is not None and not eager._graphs
    assert torch.equal(first, eager.sample_ddim(None, f2, a2, clip_ids=ids_a))
    assert torch.equal(auto.sample_ddim(None, f2, a2, clip_ids=ids_a), first)
    second = auto.sample_ddim(None, f2, a2, clip_ids=ids_b)
    assert len(auto._graphs) == 1
    assert torch.equal(second, eager.sample_ddim(None, f2, a2, clip_ids=ids_b)) and not torch.equal(second, first)
    auto.seed = eager.seed = 22                                     # another seed: the same capture, other numbers
    third = auto.sample_ddim(None, f2, a2, clip_ids=ids_b)
    assert len(auto._graphs) == 1 and torch.equal(third, eager.sample_ddim(None, f2, a2, clip_ids=ids_b))
    assert not torch.equal(third, second)
    # DDPM
    kwp = dict(timesteps=4, sample_type="ddpm", noise_source="device", seed=21)
    autop, eagerp = DiffusionSampler(top, **kwp), DiffusionSampler(top, hip_graph=False, **kwp)
    outp = autop.sample_ddpm(None, f2, a2, clip_ids=ids_a)
    assert len(autop._graphs) == 1 and torch.equal(outp, eagerp.sample_ddpm(None, f2, a2, clip_ids=ids_a))
    # torch noise with eta = 1 still runs eagerly and draws from torch's generator
    tor = DiffusionSampler(top, timesteps=4, sample_type="ddim", eta=1.0)
    x = eager.initial_noise(ids_a, (2, 1, 64, 128))
    torch.manual_seed(5)
    t1 = tor.sample_ddim(x, f2, a2)
    torch.manual_seed(5)
    t2 = tor.sample_ddim(x, f2, a2)
    assert not tor._graphs and torch.equal(t1, t2)
    # a fused stochastic step: one K15 entry (the tail kernel), nothing element-wise between two evaluations
    x1, f1, a1 = x[:1], [f[:1] for f in f2], a2[:1]
    ops.PROFILE = []
    try:
        eager.sample_ddim(x1, f1, a1, clip_ids=ids_a[:1])
        events = ops.PROFILE
    finally:
        ops.PROFILE = None
    assert [e[3] for e in events].count("K15") == 3                 # 4 evaluations: 3 fused tails, the last step returns x0
    plain = DiffusionSampler(top, hip_graph=False, fused_update=False, **kw)
    ops.PROFILE = []
    try:
        plain.sample_ddim(x1, f1, a1, clip_ids=ids_a[:1])
        events = ops.PROFILE
    finally:
        ops.PROFILE = None
    assert [e[3] for e in events].count("K15") == 9                 # per stochastic step: x0 -> noise, the normals, the update


def test_sample_sharded_draws_the_noise_of_the_clips_it_owns(tiny6):
    from diff_sal_amd import dist as dsd
    from diff_sal_amd.sampling import DiffusionSampler

    top, feats, audio = tiny6
    s = DiffusionSampler(top, timesteps=3, sample_type="ddim", eta=1.0, noise_source="device", seed=9, hip_graph=False)
    a = dsd.sample_sharded(s, None, feats, audio, batch=4, clip_ids=IDS6)
    b = dsd.sample_sharded(s, None, feats, audio, batch=1, clip_ids=IDS6)
    assert a.shape == (6, 1, 64, 128) and torch.equal(a, b)
    assert torch.equal(a, s.sample_ddim(None, feats, audio, clip_ids=IDS6))
