"""GPU parity of the GRU cell of the recurrent pattern extractor (LDE_CELL_GRU = 3, include/lde.h; csrc/lde_rnn_gru.h) against the numpy
restatement tests/gru_ref.py (itself checked against torch.nn.GRU in float64 by tests/test_gru_host.py).

Tolerances: those of tests/test_gpu_rnn.py — f32 round-off only (hardware exp / rcp in σ and tanh, ≈ 1e-7): forward ≤ 2e-5 of both
references; gradients finite, ≤ 1e-4 of the float64 scale from the f32 reference and no farther from float64 than 2× the f32 reference
+ 2e-5 of the scale. (The f32 reference alone stays within 4.7e-7 of f64: 40× inside.)"""
import ctypes as C

import numpy as np
import pytest

from tests import gru_ref as G

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]   # (the shared references are read-only on purpose)

GRU = 3
FOUR = [((32, 16, 16), False), ((32, 16, 16), True), ((5, 7, 3, 9), False), ((3, 10), False)]
# (40,21,11): 63 gate rows; (40,22): 66; (32,32,32): LatentODE's width; (16,64): the widest. Added to the issue's list: (20,17) — the first
# width with more than 64 PSEUDO-rows (68: a lane owns two) — and (6,3,2) — 12 pseudo-rows: 16 lanes per trajectory, four trajectories per wave.
MORE = [((40, 21, 11), False), ((40, 22), False), ((32, 32, 32), True), ((16, 64), False), ((20, 17), True), ((6, 3, 2), False)]
CASES = [(s, r, 1, 1) for s, r in FOUR + MORE] + [(s, r, T, B) for T, B in ((9, 37), (50, 256)) for s, r in FOUR] + [(s, r, 9, 37) for s, r in MORE]

_refs = {}


def _inputs(sizes, T, B, seed):
    rng = np.random.default_rng(seed + 1)
    W = G.weights(sizes, seed=seed)
    x = rng.standard_normal((T, B, sizes[0])).astype(np.float32)
    dy = (rng.standard_normal((B, sizes[-1])) / B).astype(np.float32)
    return W, x, dy


def _reference(sizes, reverse, T, B, seed=4):
    """(W, x, dy) and the f32 / f64 references of one case: computed once, shared, read-only."""
    key = (sizes, reverse, T, B, seed)
    if key not in _refs:
        W, x, dy = _inputs(sizes, T, B, seed)
        r32 = (G.forward(sizes, W, x, reverse, np.float32),) + G.backward(sizes, W, x, dy, reverse, np.float32)
        r64 = (G.forward(sizes, W, x, reverse),) + G.backward(sizes, W, x, dy, reverse)
        for a in (W, x, dy) + r32 + r64:
            a.setflags(write=False)
        _refs[key] = (W, x, dy, r32, r64)
    return _refs[key]


def _check(y, dx, dW, r32, r64, what=""):
    figs = {"y32": np.abs(y - r32[0]).max(), "y64": np.abs(y - r64[0]).max()}
    ok = figs["y32"] <= 2e-5 and figs["y64"] <= 2e-5
    for g, r, t, name in ((dx, r32[1], r64[1], "dx"), (dW, r32[2], r64[2], "dW")):
        s = np.abs(t).max()
        fin = bool(np.isfinite(g).all())
        e32, e64, ref = np.abs(g - r).max() / s, np.abs(g - t).max() / s, np.abs(r - t).max() / s
        figs[name] = (e32, e64, ref)
        ok = ok and fin and e32 <= 1e-4 and e64 <= 2 * ref + 2e-5
    print(f"PARITY {what} y {figs['y32']:.2e}/{figs['y64']:.2e} dx {figs['dx'][0]:.2e}/{figs['dx'][1]:.2e} (ref {figs['dx'][2]:.2e}) "
          f"dW {figs['dW'][0]:.2e}/{figs['dW'][1]:.2e} (ref {figs['dW'][2]:.2e})")
    assert ok, (what, figs)


def _native(sizes, reverse, W, **opts):
    from tests.gpu_util import NativeRnn
    nat = NativeRnn(GRU, sizes, reverse)
    assert nat.nW == W.size == G.num_weights(sizes)
    for k, v in opts.items():
        nat.set_option(k, v)
    nat.set_weights(W)
    return nat


@pytest.mark.parametrize("sizes,reverse,T,B", CASES)
def test_gru_forward_backward_parity(sizes, reverse, T, B):
    W, x, dy, r32, r64 = _reference(sizes, reverse, T, B)
    nat = _native(sizes, reverse, W)
    y = nat.forward(x)
    dx, dW = nat.backward(x, dy)
    _check(y, dx, dW, r32, r64, f"{sizes} rev={int(reverse)} T={T} B={B}")


def test_gru_more_than_1024_workgroups_worth_of_trajectories():
    """B = 1100: the first batch at which two trajectories share a workgroup — the instantiated kernel with its weight rows in LDS."""
    sizes, T, B = (32, 16, 16), 5, 1100
    W, x, dy, r32, r64 = _reference(sizes, True, T, B, seed=8)
    nat = _native(sizes, True, W)
    y = nat.forward(x)
    dx, dW = nat.backward(x, dy)
    _check(y, dx, dW, r32, r64, f"{sizes} T={T} B={B}")


def test_gru_kernel_variants_agree():
    """"generic" = 1 (the run-time-shaped kernel) and "regw" = 0 (weight rows in LDS, one wave per stack) against the default (instantiated,
    rows in registers, one wave per cell)."""
    sizes, T, B = (32, 16, 16), 9, 37
    W, x, dy, _, _ = _reference(sizes, True, T, B)
    res = []
    for opts in ({}, {"generic": 1}, {"regw": 0}):
        nat = _native(sizes, True, W, **opts)
        res.append((nat.forward(x),) + nat.backward(x, dy))
    for other, name in ((res[1], "generic"), (res[2], "regw")):
        for a, b, what in zip(other, res[0], ("y", "dx", "dW")):
            e = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
            print(f"VARIANT {name} {what} {e:.2e}")
            assert e <= 2e-6, (name, what, e)


@pytest.mark.parametrize("T,B,rev", [(23, 37, True), (1, 5, False), (8, 16, True), (9, 64, False), (50, 256, True)])
def test_gru_one_wave_per_cell_equals_one_wave_per_stack(T, B, rev):
    """The 32-16-16 stack runs a workgroup of two waves, one per cell (rnn_body2), up to 1024 trajectories; "pipe" = 0 keeps the single wave
    that walks both cells (gru_body). Same arithmetic per cell in the same order ⇒ the same bits, on sweeps shorter than, equal to and
    longer than the ring, ragged batches, both directions of time — as tests/test_gpu_rnn.py checks for the other cells."""
    sizes = (32, 16, 16)
    W, x, dy = _inputs(sizes, T, B, seed=9)
    res = []
    for flag in (1, 0):
        nat = _native(sizes, rev, W, pipe=flag)
        res.append((nat.forward(x),) + nat.backward(x, dy))
    for a, b, what in zip(res[0], res[1], ("y", "dx", "dW")):
        assert np.array_equal(a, b), what


def test_gru_dw_accumulates_dx_optional_and_repeatable():
    sizes, T, B = (32, 16, 16), 9, 37
    W, x, dy, r32, r64 = _reference(sizes, True, T, B)
    nat = _native(sizes, True, W)
    dx, dW = nat.backward(x, dy)
    base = np.full(nat.nW, 0.5, np.float32)
    dx2, dW2 = nat.backward(x, dy, need_dx=False, dW0=base)
    assert dx2 is None and np.abs((dW2 - base) - dW).max() <= 1e-6 * max(1.0, np.abs(dW).max())
    a, b = nat.backward(x, dy), nat.backward(x, dy)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(nat.forward(x), nat.forward(x))
    # a run-time shape with several rows per lane too
    sizes = (32, 32, 32)
    W, x, dy, _, _ = _reference(sizes, True, T, B)
    nat = _native(sizes, True, W)
    dx, dW = nat.backward(x, dy)
    dx2, dW2 = nat.backward(x, dy, need_dx=False, dW0=np.full(nat.nW, 0.5, np.float32))
    assert dx2 is None and np.abs((dW2 - 0.5) - dW).max() <= 1e-6 * max(1.0, np.abs(dW).max())
    assert np.array_equal(nat.backward(x, dy)[1], dW)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda")


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("sizes,T,B", [((32, 16, 16), 9, 37), ((32, 16, 16), 5, 1100), ((40, 22), 9, 37)])
def test_gru_training_forward_and_split_pullback_equal_the_plain_pair(sizes, T, B):
    """lde_rnn_forward_train + pullback (records kept: modes 2 + 3) and lde_rnn_backward_dx + lde_rnn_backward_dw equal lde_rnn_forward +
    lde_rnn_backward (mode 1) bit for bit; the accumulate flag = 0 writes dW."""
    import torch
    from latentdiffeq_amd import _lib as L
    W, x, dy, _, _ = _reference(sizes, True, T, B, seed=8 if B == 1100 else 4)
    nat = _native(sizes, True, W)
    lib, h, s = nat.lib, nat.h, L.raw_stream(0)
    xd, dyd = _dev(x), _dev(dy)

    def run(train, split):
        y = torch.empty(B, sizes[-1], device="cuda")
        dx, dW = torch.full_like(xd, 7.0), torch.zeros(nat.nW, device="cuda")
        assert (lib.lde_rnn_forward_train if train else lib.lde_rnn_forward)(h, _p(xd), T, B, _p(y), s) == 0
        if split:
            assert lib.lde_rnn_backward_dx(h, _p(xd), _p(dyd), T, B, _p(dx), s) == 0
            assert lib.lde_rnn_backward_dw(h, _p(dW), s) == 0
        else:
            assert lib.lde_rnn_backward(h, _p(xd), _p(dyd), T, B, _p(dx), _p(dW), s) == 0
        torch.cuda.synchronize()
        return y, dx, dW

    plain = run(False, False)
    for other in (run(True, False), run(False, True), run(True, True)):
        for a, b in zip(plain, other):
            assert torch.equal(a, b)
    assert lib.lde_rnn_set_accumulate(h, 0) == 0
    dW = torch.full((nat.nW,), 3.0, device="cuda")
    assert lib.lde_rnn_backward(h, _p(xd), _p(dyd), T, B, None, _p(dW), s) == 0     # dx = NULL, dW written over the 3.0
    torch.cuda.synchronize()
    assert torch.equal(dW, plain[2])


def test_gru_in_grouped_calls_equals_single_calls():
    """lde_rnn_group_forward / _backward (and the _ld forms with column blocks and a second gradient source) over [GRU, LSTM, RNN-relu]
    stacks of (32,16,16) on the same frames: per stack the single calls' bits."""
    import torch
    from latentdiffeq_amd import _lib as L
    from oracle import oracle as O
    from tests.gpu_util import NativeRnn
    sizes, T, B = (32, 16, 16), 8, 16
    rng = np.random.default_rng(12)
    x = rng.standard_normal((T, B, 32)).astype(np.float32)
    nats = []
    for cell, rev in ((GRU, True), (O.CELL_LSTM, False), (O.CELL_RNN_RELU, True)):
        nat = NativeRnn(cell, sizes, rev)
        nat.set_weights(G.weights(sizes, seed=5) if cell == GRU else O.rnn_weights(cell, sizes, seed=5))
        nats.append(nat)
    lib, s = nats[0].lib, L.raw_stream(0)
    xd = _dev(x)
    dys = [_dev(rng.standard_normal((B, 16)) / B) for _ in nats]
    dys2 = [_dev(rng.standard_normal((B, 16)) / B) for _ in nats]
    arr = lambda ptrs: (C.c_void_p * 3)(*ptrs)
    hs = arr([n.h.value for n in nats])

    single = []
    for n, dy in zip(nats, dys):
        y = torch.empty(B, 16, device="cuda")
        dx, dW = torch.empty_like(xd), torch.zeros(n.nW, device="cuda")
        assert lib.lde_rnn_forward(n.h, _p(xd), T, B, _p(y), s) == 0
        assert lib.lde_rnn_backward(n.h, _p(xd), _p(dy), T, B, _p(dx), _p(dW), s) == 0
        single.append((y, dx, dW))
    torch.cuda.synchronize()

    for train in (False, True):
        ys = [torch.empty(B, 16, device="cuda") for _ in nats]
        dxs = [torch.empty_like(xd) for _ in nats]
        dWs = [torch.zeros(n.nW, device="cuda") for n in nats]
        fwd = lib.lde_rnn_group_forward_train if train else lib.lde_rnn_group_forward
        assert fwd(3, hs, arr([xd.data_ptr()] * 3), T, B, arr([y.data_ptr() for y in ys]), s) == 0
        assert lib.lde_rnn_group_backward(3, hs, arr([xd.data_ptr()] * 3), arr([d.data_ptr() for d in dys]), T, B,
                                          arr([d.data_ptr() for d in dxs]), arr([d.data_ptr() for d in dWs]), s) == 0
        torch.cuda.synchronize()
        for (y0, dx0, dW0), y, dx, dW in zip(single, ys, dxs, dWs):
            assert torch.equal(y0, y) and torch.equal(dx0, dx) and torch.equal(dW0, dW), train

    # column blocks of one (B, 48) array, the output gradient as two sources
    wide = torch.full((B, 48), 7.0, device="cuda")
    ld = (C.c_int32 * 3)(48, 48, 48)
    assert lib.lde_rnn_group_forward_ld(3, hs, arr([xd.data_ptr()] * 3), T, B, arr([wide.data_ptr() + 64 * i for i in range(3)]), ld, 1, s) == 0
    g1, g2 = torch.cat(dys, dim=1).contiguous(), torch.cat(dys2, dim=1).contiguous()
    dxs = [torch.empty_like(xd) for _ in nats]
    dWs = [torch.zeros(n.nW, device="cuda") for n in nats]
    assert lib.lde_rnn_group_backward_ld(3, hs, arr([xd.data_ptr()] * 3), arr([g1.data_ptr() + 64 * i for i in range(3)]),
                                         arr([g2.data_ptr() + 64 * i for i in range(3)]), ld, T, B, arr([d.data_ptr() for d in dxs]),
                                         arr([d.data_ptr() for d in dWs]), s) == 0
    torch.cuda.synchronize()
    for i, (n, (y0, _, _)) in enumerate(zip(nats, single)):
        assert torch.equal(wide[:, 16 * i:16 * i + 16], y0)
        dx, dW = torch.empty_like(xd), torch.zeros(n.nW, device="cuda")
        both = (dys[i] + dys2[i]).contiguous()
        assert lib.lde_rnn_backward(n.h, _p(xd), _p(both), T, B, _p(dx), _p(dW), s) == 0
        torch.cuda.synchronize()
        assert torch.equal(dx, dxs[i]) and torch.equal(dW, dWs[i]), i


def test_one_gru_handle_changing_shapes():
    from tests.gpu_util import NativeRnn
    for sizes in ((32, 16, 16), (5, 7, 3, 9)):
        W = G.weights(sizes, seed=3)
        nat = NativeRnn(GRU, sizes, True)
        nat.set_weights(W)
        for T, B in ((3, 5), (20, 40), (7, 300), (2, 1), (9, 37)):
            rng = np.random.default_rng(T * 1000 + B)
            x = rng.standard_normal((T, B, sizes[0])).astype(np.float32)
            dy = (rng.standard_normal((B, sizes[-1])) / B).astype(np.float32)
            assert np.abs(nat.forward(x) - G.forward(sizes, W, x, True, np.float32)).max() <= 2e-5, (T, B)
            dx, dW = nat.backward(x, dy)
            rx, rW = G.backward(sizes, W, x, dy, True, np.float32)
            assert np.abs(dx - rx).max() <= 1e-4 * np.abs(rx).max() and np.abs(dW - rW).max() <= 1e-4 * np.abs(rW).max(), (T, B)


def test_gru_weights_through_refresh_and_device_upload():
    """lde_rnn_set_weights_device and lde_refresh_weights hand a GRU stack its flat weights like any other stack's."""
    import torch
    from latentdiffeq_amd import _lib as L
    sizes, T, B = (5, 7, 3, 9), 9, 37
    W, x, dy, r32, r64 = _reference(sizes, False, T, B)
    nat = _native(sizes, False, W * 0)
    lib, s = nat.lib, L.raw_stream(0)
    Wd = _dev(W)
    for how in ("device", "refresh"):
        nat.set_weights(W * 0)
        if how == "device":
            assert lib.lde_rnn_set_weights_device(nat.h, _p(Wd), Wd.numel(), s) == 0
        else:
            kinds = (C.c_int32 * 1)(1)
            assert lib.lde_refresh_weights(1, kinds, (C.c_void_p * 1)(nat.h.value), (C.c_void_p * 1)(Wd.data_ptr()), s) == 0
        torch.cuda.synchronize()
        assert np.abs(nat.forward(x) - r32[0]).max() <= 2e-5, how


def test_gru_through_autograd():
    """Recurrent(GRU(8,12), GRU(12,12), reverse=True) on x [8, 37, 9]: the output and theta.grad against tests/gru_ref.py."""
    import torch
    from latentdiffeq_amd.recurrent import GRU as GRUCell, Recurrent
    torch.manual_seed(2)
    sizes, B, T = (8, 12, 12), 37, 9
    m = Recurrent(GRUCell(8, 12), GRUCell(12, 12), reverse=True)
    with torch.no_grad():
        m.theta.add_(torch.empty_like(m.theta).uniform_(-0.2, 0.2))     # biases and initial states away from zero
    m = m.to("cuda")
    x = torch.randn(8, B, T, device="cuda", requires_grad=True)
    ct = torch.randn(12, B, device="cuda") / B
    y = m(x)
    assert y.shape == (12, B)
    (y * ct).sum().backward()
    W = m.theta.detach().cpu().numpy()
    xr = x.detach().cpu().numpy().transpose(2, 1, 0)
    dyr = ct.cpu().numpy().T
    r32 = (G.forward(sizes, W, xr, True, np.float32),) + G.backward(sizes, W, xr, dyr, True, np.float32)
    r64 = (G.forward(sizes, W, xr, True),) + G.backward(sizes, W, xr, dyr, True)
    _check(y.detach().cpu().numpy().T, x.grad.cpu().numpy().transpose(2, 1, 0), m.theta.grad.cpu().numpy(), r32, r64, "autograd")
