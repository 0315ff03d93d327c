"""CPU: the β word without a GPU — (1) the six lde_*_dev entry points (include/lde.h) exist and refuse a NULL beta_dev, a divisor that is
not finite or not > 0, and what their twins refuse, before any device call; (2) `train(graphed=True)` refuses a CPU model, and
`grad_sync` with it; (3) a CPU β tensor is read as the number it holds: the loss terms have no CPU path (tests/test_train_host.py), so
with CPU operands it takes the refusal the float takes, and `beta_word` tells the two kinds of β apart."""
import ctypes as C
import inspect

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(0x1000)      # a non-NULL, 16-byte aligned pointer that is never dereferenced: every call below is refused on the host
BAD_DIVISORS = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))
NAMES = ["lde_kl_forward_dev", "lde_kl_backward_dev", "lde_sample_kl_forward_dev", "lde_sample_kl_backward_dev",
         "lde_sample_kl_pair_forward_dev", "lde_sample_kl_pair_backward_dev"]


def _calls(lib):
    """name → f(beta_dev, divisor, n=37, first=FAKE): the entry point with fake pointers everywhere else."""
    F = FAKE
    return {
        "lde_kl_forward_dev": lambda w, d, n=37, first=F: lib.lde_kl_forward_dev(first, F, n, w, d, None, F, F, None),
        "lde_kl_backward_dev": lambda w, d, n=37, first=F: lib.lde_kl_backward_dev(first, F, n, w, d, F, F, F, None),
        "lde_sample_kl_forward_dev": lambda w, d, n=37, first=F: lib.lde_sample_kl_forward_dev(first, F, F, n, w, d, None, F, F, F, None),
        "lde_sample_kl_backward_dev": lambda w, d, n=37, first=F: lib.lde_sample_kl_backward_dev(first, F, F, F, F, w, d, n, F, F, None),
        "lde_sample_kl_pair_forward_dev": lambda w, d, n=37, first=F, d2=2.0: lib.lde_sample_kl_pair_forward_dev(
            first, F, n, d, F, F, 5, d2, w, None, 1, 0, 0, 0, 1, None, F, F, F, F, F, F, None),
        "lde_sample_kl_pair_backward_dev": lambda w, d, n=37, first=F, d2=2.0: lib.lde_sample_kl_pair_backward_dev(
            first, F, F, F, n, d, F, F, F, F, 5, d2, w, F, F, F, F, F, None),
    }


def test_the_six_entry_points_exist_and_refuse_on_the_host():
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    assert set(NAMES) <= set(L.EXPORTS)
    calls = _calls(lib)
    assert sorted(calls) == sorted(NAMES)
    for name, f in calls.items():
        assert f(None, 2.0) == INVALID, name                         # NULL beta_dev
        for bad in BAD_DIVISORS:
            assert f(FAKE, bad) == INVALID, (name, bad)
        assert f(FAKE, 2.0, first=None) == INVALID, name             # what the twin refuses: a NULL operand …
        if "pair" in name:
            for bad in BAD_DIVISORS:                                 # … the second part's divisor …
                assert f(FAKE, 2.0, d2=bad) == INVALID, (name, bad)
            assert f(FAKE, 2.0, n=0) == UNSUPPORTED, name            # … an empty part, as the twin
        else:
            assert f(FAKE, 2.0, n=-1) == INVALID, name
    assert calls["lde_sample_kl_pair_forward_dev"](FAKE, 2.0, n=8193) == UNSUPPORTED
    assert calls["lde_sample_kl_pair_forward_dev"](FAKE, 2.0, n=8192, first=None) == INVALID      # (8192 itself is served)
    # an empty single-part pullback launches nothing, as its twin
    assert calls["lde_kl_backward_dev"](FAKE, 2.0, n=0) == 0 and calls["lde_sample_kl_backward_dev"](FAKE, 2.0, n=0) == 0


def test_graphed_train_refuses_a_cpu_model_and_grad_sync():
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import train as TR
    sig = inspect.signature(TR.train).parameters
    assert sig["graphed"].default is False and sig["check_every"].default == 50
    mt, diffeq = la.GOKU_basic(), la.Pendulum()
    enc, dec = TR.default_layers(mt, 16, diffeq, device="cpu")
    model = TR.LatentDiffEqModel(mt, enc, dec)
    data = torch.rand(16, 4, 6)
    args = dict(dt=0.05, epochs=1, seq_len=4, full_seq_len=6)
    with pytest.raises(ValueError, match="GPU"):
        TR.train(model, [data], data, graphed=True, **args)
    with pytest.raises(ValueError, match=r"GraphedStep\(between=, fn2=\)"):
        TR.train(model, [data], data, graphed=True, grad_sync=lambda: None, **args)
    assert not hasattr(model, "optimizer")                           # refused before anything is built


def test_a_cpu_beta_tensor_is_the_number_it_holds():
    import torch
    from latentdiffeq_amd import loss as LS
    from latentdiffeq_amd import train as TR
    from latentdiffeq_amd._lib import LdeError
    assert LS.beta_word(0.3) == (None, 0.3)
    b = np.float32(0.3)
    assert LS.beta_word(b)[0] is None and LS.beta_word(b)[1] is b     # a number goes through as it is: the existing path, the same bits
    word, number = LS.beta_word(torch.tensor([0.25]))
    assert word is None and number == 0.25 and isinstance(number, float)
    mu = torch.tensor([[0.5, -1.0], [0.0, 2.0]])
    ls = torch.tensor([[0.0, 0.3], [-0.2, 0.1]])
    # no loss term has a CPU path: a CPU β tensor with CPU operands ends where the float ends
    for beta in (0.25, torch.tensor(0.25), torch.tensor([0.25])):
        for call in (lambda: LS.sample_with_kl(mu, ls, beta), lambda: LS.sample_with_kl((mu, mu), (ls, ls), beta),
                     lambda: LS.beta_kl(mu, ls, beta)):
            with pytest.raises(LdeError):
                call()
    assert "beta_kl" in dir(TR) and "beta" in inspect.signature(LS.beta_kl).parameters
