"""EMA weights in the training step, the parts that need no GPU: the rate's warm-up, the argument checks of the new entry points
(made before any launch), the sizes of the two argument blocks, the integration table, the constructor's rules."""
import ctypes
import os

import pytest
import torch

from diff_sal_amd import _lib
from diff_sal_amd.train_step import DiffusionTrainStep, FlatParams, ema_rate_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("diffsal_adam_ema_step", "diffsal_adam_ema_args", "diffsal_adam_ema_args_size", "diffsal_adam_ema_step_args", "diffsal_ema_swap")
E_SHAPE, E_ARG = _lib.K["DIFFSAL_E_SHAPE"], _lib.K["DIFFSAL_E_ARG"]


def _crossing(mu):
    n = 0
    while (1.0 + n) / (10.0 + n) < mu:
        n += 1
    return n


def test_rate_without_warmup_is_mu():
    for mu in (0.0, 0.9, 0.9999, 1.0):
        assert [ema_rate_at(mu, n, False) for n in (0, 1, 9, 10 ** 6)] == [mu] * 4


@pytest.mark.parametrize("mu, first", [(0.9, 80), (0.9999, 89990)])
def test_rate_with_warmup(mu, first):
    """(1 + n) / (10 + n) reaches 0.9 at n = 80 (81 / 90) and 0.9999 at n = 89 990 (89 991 / 90 000): exact ties, which the
    correctly rounded double division turns into the literal's own double."""
    assert ema_rate_at(mu, 0, True) == 0.1
    assert ema_rate_at(mu, 1, True) == 2.0 / 11.0 and ema_rate_at(mu, 9, True) == 10.0 / 19.0
    cross = _crossing(mu)
    assert cross == first
    probe = sorted({0, 1, 2, 9, 10, 50, cross - 2, cross - 1, cross, cross + 1, cross + 1000})
    rates = [ema_rate_at(mu, n, True) for n in probe]
    assert all(a <= b for a, b in zip(rates, rates[1:])) and all(a < b for a, b in zip(rates, rates[1:]) if b < mu)
    assert ema_rate_at(mu, cross - 1, True) == float(cross) / (9.0 + cross) < mu
    assert [ema_rate_at(mu, n, True) for n in (cross, cross + 1, cross + 12345)] == [mu] * 3


def test_argument_errors_are_reported_without_a_gpu():
    """in the manner of test_abi.py: made-up addresses, every call refused before a launch"""
    lib = _lib.load()
    A = 4096                                     # a 16-byte aligned made-up address; 4100 is not
    hp = (1e-4, 0.9, 0.999, 1e-8, 0.0)

    def step(p=A, g=A, m=A, v=A, s=A, n=8, st=1, mu=0.5):
        return lib.diffsal_adam_ema_step(p, g, m, v, s, n, *hp, st, 1.0, None, 1.0, 0, mu, None)

    assert step(s=None) == E_ARG and b"null" in lib.diffsal_last_error()
    assert step(n=0) == E_SHAPE
    assert step(st=0) == E_SHAPE
    assert step(mu=1.5) == E_ARG and b"ema_mu" in lib.diffsal_last_error()
    assert step(mu=-0.1) == E_ARG
    assert step(s=A + 4) == E_ARG and b"aligned" in lib.diffsal_last_error()

    def step_args(s=A, n=8, args=A):
        return lib.diffsal_adam_ema_step_args(A, A, A, A, s, n, args, None, 0, None)

    assert step_args(s=None) == E_ARG and step_args(args=None) == E_ARG
    assert step_args(n=0) == E_SHAPE
    assert step_args(s=A + 4) == E_ARG and step_args(args=A + 4) == E_ARG

    assert lib.diffsal_ema_swap(A, None, 8, None) == E_ARG and lib.diffsal_ema_swap(None, A, 8, None) == E_ARG
    assert lib.diffsal_ema_swap(A, 2 * A, 0, None) == E_SHAPE
    assert lib.diffsal_ema_swap(A, 2 * A + 4, 8, None) == E_ARG and b"aligned" in lib.diffsal_last_error()
    assert lib.diffsal_ema_swap(A, A + 16, 8, None) == E_ARG and b"overlap" in lib.diffsal_last_error()

    out = (ctypes.c_ubyte * 64)()
    assert lib.diffsal_adam_ema_args(*hp, 1, 1.0, 1.0, 0.5, None) == E_ARG
    assert lib.diffsal_adam_ema_args(*hp, 0, 1.0, 1.0, 0.5, out) == E_SHAPE
    assert lib.diffsal_adam_ema_args(*hp, 1, 1.0, 1.0, 1.5, out) == E_ARG


def test_block_sizes_and_layout():
    """the EMA block is Adam's block, untouched, followed by fl(1 - mu) and fl(mu)"""
    lib = _lib.load()
    assert lib.diffsal_adam_args_size() == 36
    assert lib.diffsal_adam_ema_args_size() == lib.diffsal_adam_args_size() + 8
    hp = (3e-4, 0.9, 0.999, 1e-8, 0.01, 7, 0.5, 1.0)
    plain, ext = (ctypes.c_ubyte * 36)(), (ctypes.c_ubyte * 44)()
    mu = 0.9999
    assert lib.diffsal_adam_args(*hp, plain) == 0 and lib.diffsal_adam_ema_args(*hp, mu, ext) == 0
    assert bytes(ext)[:36] == bytes(plain)
    omm, m = (ctypes.c_float * 2).from_buffer_copy(bytes(ext)[36:])
    assert omm == ctypes.c_float(1.0 - mu).value and m == ctypes.c_float(mu).value


def test_integration_md_names_every_new_entry_point():
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "diffsal.h")).read()
    for name in NEW:
        assert "`" + name + "`" in md, name
        assert name + "(" in header, name


class _Two(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(3, 5)
        self.b = torch.nn.Parameter(torch.arange(7.0))
        self.frozen = torch.nn.Parameter(torch.ones(2), requires_grad=False)


def test_constructor_rules_and_the_shadow_buffer():
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="ema"):
            DiffusionTrainStep(_Two(), ema=bad)
    with pytest.raises(ValueError, match="ema_warmup"):
        DiffusionTrainStep(_Two(), ema_warmup=True)
    assert FlatParams(_Two()).shadow is None
    plain = DiffusionTrainStep(_Two())
    assert plain.ema is None and plain.flat.shadow is None
    for call in (plain.ema_state_dict, plain.reset_ema, lambda: plain.load_ema_state_dict({"shadow": {}}),
                 lambda: plain.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema="):
            call()
    ts = DiffusionTrainStep(_Two(), ema=0.99, ema_warmup=True)
    f = ts.flat
    assert torch.equal(f.shadow, f.flat_p) and f.shadow.data_ptr() != f.flat_p.data_ptr() and f.shadow.numel() == f.numel
    live = torch.zeros(f.numel, dtype=torch.bool)
    for p, o in zip(f.params, f.offsets):
        live[o:o + p.numel()] = True
    assert not f.shadow[~live].any() and (~live).any()            # the alignment padding is zero
    sd = ts.ema_state_dict()
    assert set(sd) == {"shadow", "updates", "mu", "warmup"} and (sd["updates"], sd["mu"], sd["warmup"]) == (0, 0.99, True)
    assert list(sd["shadow"]) == ["b", "a.weight", "a.bias"]      # EMAHelper's keys: the trained parameters by name
    for name, p in ts.model.named_parameters():
        if p.requires_grad:
            assert torch.equal(sd["shadow"][name], p.data) and sd["shadow"][name].data_ptr() != p.data_ptr()


def test_load_ema_state_dict_checks_names_and_shapes_before_writing():
    ts = DiffusionTrainStep(_Two(), ema=0.9)
    good = ts.ema_state_dict()
    before = ts.flat.shadow.clone()
    sd = {"shadow": {k: v + 1 for k, v in good["shadow"].items()}, "updates": 5, "mu": 0.5, "warmup": True}
    miss = {"shadow": {k: v for k, v in sd["shadow"].items() if k != "a.bias"}}
    with pytest.raises(ValueError, match="a.bias"):
        ts.load_ema_state_dict(miss)
    with pytest.raises(ValueError, match="ghost"):
        ts.load_ema_state_dict({"shadow": dict(sd["shadow"], ghost=torch.zeros(1))})
    with pytest.raises(ValueError, match="'b'.*shape"):
        ts.load_ema_state_dict({"shadow": dict(sd["shadow"], b=torch.zeros(8))})
    with pytest.raises(ValueError):
        ts.load_ema_state_dict(sd["shadow"])                       # the bare dictionary is not the format
    assert torch.equal(ts.flat.shadow, before) and ts.ema_updates == 0
    ptr = ts.flat.shadow.data_ptr()
    ts.load_ema_state_dict(sd)
    assert ts.flat.shadow.data_ptr() == ptr and (ts.ema_updates, ts.ema, ts.ema_warmup) == (5, 0.5, True)
    got = ts.ema_state_dict()
    assert all(torch.equal(got["shadow"][k], sd["shadow"][k]) for k in sd["shadow"])
    ts.load_ema_state_dict({"shadow": good["shadow"]})              # EMAHelper.state_dict() under the key: counts restart
    assert torch.equal(ts.flat.shadow, before) and (ts.ema_updates, ts.ema, ts.ema_warmup) == (0, 0.5, True)
    ts.flat.flat_p.add_(2.0)
    ts.reset_ema()
    assert torch.equal(ts.flat.shadow, ts.flat.flat_p) and ts.ema_updates == 0
