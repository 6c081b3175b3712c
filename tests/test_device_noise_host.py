"""Device noise (Philox4x32-10, include/diffsal.h "sampler noise") without a GPU: the NumPy restatement against the published
known-answer vectors, argument validation of the three C entries, and the sampler's host logic."""
import numpy as np
import pytest
import torch

from diff_sal_amd import _lib
from tests import _philox_ref as ref


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_restatement_reproduces_the_random123_vectors(ctr, key, want):
    assert _hex(v.reshape(-1)[0] for v in ref.philox4x32_10(ctr, key)) == want


def test_restatement_layout_and_statistics():
    """Counter layout (q, draw, id_lo, id_hi), key (seed_lo, seed_hi); five-sigma statistics of seed 1234, id 3, draw 7."""
    seed, cid = (5 << 32) | 9, (1 << 40) + 3
    b = ref.bits(seed, [cid], 1000, 10)
    r = ref.philox4x32_10((2, 1000, 3, 1 << 8), (9, 5))
    assert b.shape == (1, 10) and [int(v) for v in b[0, 8:10]] == [int(r[0]), int(r[1])]
    z = ref.normals(1234, [3], 7, 16 * 224 * 384)           # this restatement: mean 3.3e-4, var - 1 = -8.0e-4
    n = z.size
    assert abs(z.mean()) < 5 / n ** 0.5 and abs(z.var() - 1) < 5 * (2 / n) ** 0.5
    assert np.abs(z).max() <= 5.77
    z32 = ref.normals(1234, [3], 7, 86016, dtype=np.float32)
    assert np.abs(z32 - z[:, :86016]).max() < 2e-5


def test_noise_entries_validate_their_arguments_without_a_gpu():
    """Validation happens before any launch: null pointers, per = 0, N = 0; noise without ids.  Ids live in device memory, so
    the library cannot see a negative one: the binding refuses it on the host before anything is uploaded."""
    from diff_sal_amd import ops

    lib = _lib.load()
    assert lib.diffsal_philox_bits(None, 1, 16, 16, 16, 0, None) == -4 and b"null" in lib.diffsal_last_error()
    assert lib.diffsal_philox_bits(16, 1, 16, None, 16, 0, None) == -4
    assert lib.diffsal_philox_normal(16, 1, 16, 16, None, 0, 1.0, None) == -4 and b"philox_normal" in lib.diffsal_last_error()
    assert lib.diffsal_philox_bits(16, 1, 0, 16, 16, 0, None) != 0 and b"per" in lib.diffsal_last_error()
    assert lib.diffsal_philox_normal(16, 1, 0, 16, 16, 0, 1.0, None) != 0 and b"per" in lib.diffsal_last_error()
    assert lib.diffsal_philox_normal(16, 0, 16, 16, 16, 0, 1.0, None) != 0
    assert lib.diffsal_philox_normal(16, 1, (1 << 34) + 1, 16, 16, 0, 1.0, None) != 0
    z7 = [0.0] * 7
    assert lib.diffsal_resize_update_noise(None, 16, None, None, 16, 16, 1, 4, 4, 8, 8, *z7, None, None, 0, None) == -4
    assert lib.diffsal_resize_update_noise(16, 16, None, None, 16, 16, 1, 4, 4, 0, 8, *z7, None, None, 0, None) != 0
    assert b"shape" in lib.diffsal_last_error()
    cz1 = [0.0] * 6 + [0.5]
    assert lib.diffsal_resize_update_noise(16, 16, None, None, 16, 16, 1, 4, 4, 8, 8, *cz1, None, 16, 1, None) == -4
    assert b"cz" in lib.diffsal_last_error()
    assert lib.diffsal_resize_update_noise(16, 16, None, None, 16, None, 1, 4, 4, 8, 8, *cz1, 16, 16, 1, None) == -4
    for bad in ([-1], [0, -7], torch.tensor([3, -2])):
        with pytest.raises(ValueError, match="non-negative"):
            ops.philox_normal(bad, 0, 0, (1, 4, 4))
        with pytest.raises(ValueError, match="non-negative"):
            ops.philox_bits(bad, 0, 0, 16)
    with pytest.raises(ValueError, match="per"):
        ops.philox_bits([0], 0, 0, 0)
    with pytest.raises(ValueError, match="seed"):
        ops.philox_bits([0], -1, 0, 4)
    with pytest.raises(ValueError, match="draw"):
        ops._draw(1 << 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.philox_normal([0], 0, 0, (1, 4, 4), device="cpu")


class _Top:
    decoder_net = staticmethod(lambda x, t, img, a=None: torch.sigmoid(x))


def test_sampler_noise_source_host_logic():
    from diff_sal_amd.sampling import DiffusionSampler

    assert DiffusionSampler(_Top()).noise_source == "torch" and DiffusionSampler(_Top()).seed == 0
    with pytest.raises(ValueError, match="noise_source"):
        DiffusionSampler(_Top(), noise_source="philox")
    x = torch.zeros(2, 1, 4, 6)
    dev = DiffusionSampler(_Top(), noise_source="device", seed=7, timesteps=4, eta=1.0)
    for call in (lambda: dev.sample_ddim(x, None, None, clip_ids=[0, 1]),
                 lambda: dev.sample_ddpm(x, None, None, clip_ids=[0, 1]),
                 lambda: dev.sample_dpm_solver(x, None, None),
                 lambda: dev.sample_image(x, clip_ids=[0, 1])):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    # clip ids mean nothing to torch's generator: refuse them instead of ignoring them
    tor = DiffusionSampler(_Top(), timesteps=4)
    with pytest.raises(ValueError, match="clip_ids"):
        tor.sample_ddim(x, None, None, clip_ids=[0, 1])
    with pytest.raises(ValueError, match="noise_source"):
        tor.initial_noise([0, 1], (2, 1, 4, 6))
    with pytest.raises(ValueError, match="x=None"):
        tor.sample_ddim(None, None, None)
    with pytest.raises(ValueError, match="non-negative"):
        dev.initial_noise([4, -1], (2, 1, 4, 6))
    # the default path is untouched: same call, same result as before
    assert tor.sample_ddim(x, None, None).shape == x.shape
    assert tor._graph_state()[-1] == "torch" and dev._graph_state()[-1] == "device"


def test_sample_sharded_needs_ids_when_it_draws_the_noise():
    from diff_sal_amd import dist as dsd
    from diff_sal_amd.sampling import DiffusionSampler

    s = DiffusionSampler(_Top(), timesteps=2)
    with pytest.raises(ValueError, match="clip_ids"):
        dsd.sample_sharded(s, None, [torch.zeros(2, 1)], None, batch=2)
    with pytest.raises(ValueError, match="clip ids"):
        dsd.sample_sharded(s, torch.zeros(2, 1, 4, 6), [torch.zeros(2, 1)], None, batch=2, clip_ids=[1])
    # the existing call form
    x = torch.zeros(3, 1, 4, 6)
    assert dsd.sample_sharded(s, x, [torch.zeros(3, 1)], None, batch=2).shape == x.shape
