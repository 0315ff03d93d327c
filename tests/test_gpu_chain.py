"""GPU parity of the dense chains either side of the solve (lde_chain_*, scope row f-1) against the CPU oracle.

Tolerance: exact-f32 MFMA vs the oracle's sequential f32 sums ⇒ round-off only. Forward |Δy| ≤ 2e-5·max(1,|y|);
gradients ≤ 1e-4 relative to the largest entry of the float64 reference, and no farther from float64 than 2× the f32
oracle + 2e-5."""
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

RECON = ((2, 200, 200, 200, 784), (O.CACT_RELU, O.CACT_RELU, O.CACT_RELU, O.CACT_SIGMOID), (0, 1, 1, 0))
LO_Z0 = ((16, 200, 2), (O.CACT_RELU, O.CACT_IDENTITY), (0, 0))
LO_TH = ((16, 200, 1), (O.CACT_RELU, O.CACT_SOFTPLUS), (0, 0))
ODD = ((5, 33, 33, 7, 7, 19), (O.CACT_TANH, O.CACT_SOFTPLUS, O.CACT_RELU, O.CACT_SIGMOID, O.CACT_IDENTITY), (0, 1, 0, 1, 0))
WIDE = ((32, 512, 512, 40), (O.CACT_RELU, O.CACT_TANH, O.CACT_IDENTITY), (0, 1, 0))      # panels force 32 / 16 columns per tile
ONE = ((24, 10), (O.CACT_SIGMOID,), (0,))
FE = ((784, 200, 200, 200, 32), (O.CACT_RELU,) * 4, (0, 1, 1, 0))   # feature extractor [REF src/models/GOKU.jl:219-226]: x read in place
ONE_WIDE = ((256, 24), (O.CACT_TANH,), (0,))                         # single layer, wide input: in place too


def _run(spec, N, o32, o64, seed=5, need_dx=True, options=()):
    from tests.gpu_util import NativeChain
    sizes, acts, skips = spec
    d = O.make_chain_desc(sizes, acts, skips)
    W = O.mlp_weights(sizes, seed=seed + 2)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, sizes[0])).astype(np.float32)
    dy = (rng.standard_normal((N, sizes[-1])) / N).astype(np.float32)
    nat = NativeChain(sizes, acts, skips)
    assert nat.nW == W.size
    for k_, v_ in options:
        nat.set_option(k_, v_)
    nat.set_weights(W)
    y = nat.forward(x)
    yr = o32.chain_forward(d, W, x)
    y64 = o64.chain_forward(d, W.astype(np.float64), x.astype(np.float64))
    sc = max(1.0, np.abs(y64).max())
    assert np.abs(y - yr).max() <= 2e-5 * sc
    assert np.abs(y - y64).max() <= 2e-5 * sc
    dx, dW = nat.backward(x, y, dy, need_dx=need_dx)
    rx, rW = o32.chain_backward(d, W, x, dy)
    tx, tW = o64.chain_backward(d, W.astype(np.float64), x.astype(np.float64), dy.astype(np.float64))
    for g, r, t, what in ((dx, rx, tx, "dx"), (dW, rW, tW, "dW")):
        if g is None:
            continue
        s = np.abs(t).max()
        assert np.isfinite(g).all(), what
        assert np.abs(g - r).max() <= 1e-4 * s, what
        assert np.abs(g - t).max() <= 2 * np.abs(r - t).max() + 2e-5 * s, what
    return nat, (x, y, dy, dx, dW)


@pytest.mark.parametrize("spec", [RECON, LO_Z0, LO_TH, ODD, WIDE, ONE, FE, ONE_WIDE],
                         ids=["reconstructor", "lo_z0", "lo_theta", "odd", "wide", "one", "feature_extractor", "one_wide"])
@pytest.mark.parametrize("N", [1, 37, 256])
def test_chain_forward_backward_parity(o32, o64, spec, N):
    _run(spec, N, o32, o64)


def test_reconstructor_at_the_metric_shape(o32, o64):
    """x̂ = reconstructor(ẑ) on N = B·T = 256·50 columns (the metric config's ẑ), ragged by one column."""
    _run(RECON, 256 * 50 - 1, o32, o64, seed=9)


def test_wide_input_layouts_agree(o32, o64):
    """Wide inputs are read in place from x (no LDS input panel, ragged last tile shifted back with zero-weight repeats);
    lde_chain_set_option("gx", 0) forces the panel layout. Both must give the same numbers to round-off, on a ragged N."""
    outs = []
    for flag in (1, 0):
        _, (x, y, dy, dx, dW) = _run(FE, 16 * 7 + 5, o32, o64, seed=13, options=(("gx", flag),))
        outs.append((y, dx, dW))
    (ya, dxa, dWa), (yb, dxb, dWb) = outs
    assert np.abs(ya - yb).max() <= 1e-6 * max(1.0, np.abs(ya).max())
    assert np.abs(dxa - dxb).max() <= 1e-5 * np.abs(dxa).max()
    assert np.abs(dWa - dWb).max() <= 1e-5 * np.abs(dWa).max()


@pytest.mark.parametrize("spec", [RECON, ODD, FE, ONE, LO_TH], ids=["reconstructor", "odd", "feature_extractor", "one", "lo_theta"])
@pytest.mark.parametrize("N", [37, 256])
def test_saved_activation_variant_gives_the_same_numbers(o32, spec, N):
    """lde_chain_forward_save + lde_chain_backward_saved (the pullback reads the hidden activations the forward call kept in
    a caller-owned buffer) against lde_chain_forward + lde_chain_backward (it recomputes them): identical outputs and —
    same staged panels, same summation order — identical gradients."""
    from tests.gpu_util import NativeChain
    sizes, acts, skips = spec
    W = O.mlp_weights(sizes, seed=4)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((N, sizes[0])).astype(np.float32)
    dy = (rng.standard_normal((N, sizes[-1])) / N).astype(np.float32)
    nat = NativeChain(sizes, acts, skips)
    nat.set_weights(W)
    y = nat.forward(x)
    dx, dW = nat.backward(x, y, dy)
    y2, saved = nat.forward_save(x)
    assert np.array_equal(y, y2)
    dx2, dW2 = nat.backward_saved(x, y2, dy, saved)
    assert np.array_equal(dx, dx2) and np.array_equal(dW, dW2)


def test_chain_dw_accumulates_and_dx_is_optional(o32):
    nat, (x, y, dy, dx, dW) = _run(LO_TH, 100, o32, O.Oracle("f64"))
    base = np.full(nat.nW, 0.25, np.float32)
    dx2, dW2 = nat.backward(x, y, dy, need_dx=False, dW0=base)
    assert dx2 is None
    assert np.abs((dW2 - base) - dW).max() <= 1e-6 * max(1.0, np.abs(dW).max())
    _, dW3 = nat.backward(x, y, dy)            # same call twice: same bits (fixed summation order)
    _, dW4 = nat.backward(x, y, dy)
    assert np.array_equal(dW3, dW4)


def test_chain_golden_fixture():
    from tests.gpu_util import NativeChain
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "chain_decoder.npz"))
    nat = NativeChain(tuple(g["sizes"]), tuple(g["acts"]), tuple(g["skips"]))
    nat.set_weights(g["W"])
    y = nat.forward(g["x"])
    assert np.abs(y - g["y_f32"]).max() <= 2e-6 and np.abs(y - g["y_f64"]).max() <= 2e-6
    dx, dW = nat.backward(g["x"], y, g["dy"])
    assert np.abs(dx - g["dx_f64"]).max() <= 3e-5 * np.abs(g["dx_f64"]).max()
    assert np.abs(dW - g["dW_f64"]).max() <= 3e-5 * np.abs(g["dW_f64"]).max()


def test_chain_errors_are_reported_not_thrown():
    import ctypes as C
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import NativeChain
    with pytest.raises(L.LdeError, match="UNSUPPORTED"):
        NativeChain((8, 8, 4, 4), (1, 1, 1), (0, 0, 1))            # skip around the last layer
    with pytest.raises(L.LdeError, match="INVALID_ARG"):
        NativeChain((8, 9, 4), (1, 1), (1, 0))                      # skip needs in == out
    nat = NativeChain((4, 8, 2), (1, 0))
    import torch
    x = torch.zeros((3, 4), device="cuda")
    y = torch.zeros((3, 2), device="cuda")
    rc = nat.lib.lde_chain_forward(nat.h, C.c_void_p(x.data_ptr()), 3, C.c_void_p(y.data_ptr()), C.c_void_p())
    assert rc == -5 and b"weights" in nat.lib.lde_chain_last_error(nat.h)      # LDE_ERR_NO_WEIGHTS


def test_torch_decoder_path_end_to_end(o64):
    """decode(decoder, l̃, t) = apply_latent_out → diffeq_layer → apply_reconstructor with autograd through all three:
    gradients of an MSE loss wrt every Dense parameter and wrt l̃ match the float64 oracle composition."""
    import torch
    import latentdiffeq_amd as M
    from latentdiffeq_amd.chain import decode, default_decoder_layers
    torch.manual_seed(0)
    diffeq = M.Pendulum(abstol=1e-7, reltol=1e-7)
    layers = default_decoder_layers(M.GOKU_basic(), 784, diffeq, device="cuda")
    dec = M.Decoder(M.GOKU_basic(), layers)
    B, T = 24, 10
    ts = O.time_grid(T)
    z0_t = torch.randn(16, B, device="cuda", requires_grad=True)
    th_t = torch.randn(16, B, device="cuda", requires_grad=True)
    # biases away from zero so that every term is exercised
    with torch.no_grad():
        for m in list(layers[0]) + [layers[2]]:
            for p in m.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.1, 0.1)
    x_hat, z_hat, (z0_hat, th_hat) = decode(dec, (z0_t, th_t), ts)
    assert x_hat.shape == (784, B, T) and z_hat.shape == (2, B, T) and z0_hat.shape == (2, B) and th_hat.shape == (1, B)
    target = torch.rand(784, B, T, device="cuda")
    loss = ((x_hat - target) ** 2).mean()
    loss.backward()

    # float64 composition with the oracle
    lo_z0, lo_th = layers[0]
    rec = layers[2]

    def od(ch):
        return O.make_chain_desc(ch.sizes, ch.acts, ch.skips), ch.flat_weights().detach().cpu().numpy().astype(np.float64)

    (dz, Wz), (dt, Wt), (dr, Wr) = od(lo_z0), od(lo_th), od(rec)
    z0t = z0_t.detach().cpu().numpy().T.astype(np.float64)
    tht = th_t.detach().cpu().numpy().T.astype(np.float64)
    z0h = o64.chain_forward(dz, Wz, z0t)
    thh = o64.chain_forward(dt, Wt, tht)
    assert np.abs(z0h - z0_hat.detach().cpu().numpy().T).max() <= 1e-5
    assert np.abs(thh - th_hat.detach().cpu().numpy().T).max() <= 1e-5
    sd = O.make_desc(abstol=1e-11, reltol=1e-11)
    z64, _, _ = o64.forward(sd, z0h, thh, ts)
    assert np.abs(z64 - z_hat.detach().cpu().numpy().transpose(2, 1, 0)).max() <= 2e-5
    xh = o64.chain_forward(dr, Wr, z64.reshape(T * B, 2))
    tg = target.cpu().numpy().transpose(2, 1, 0).reshape(T * B, 784).astype(np.float64)
    dxh = 2.0 * (xh - tg) / xh.size
    dz64, dWr = o64.chain_backward(dr, Wr, z64.reshape(T * B, 2), dxh)
    g0, gth, _, _ = o64.adjoint(sd, z64, thh, ts, dz64.reshape(T, B, 2))
    dz0t, dWz = o64.chain_backward(dz, Wz, z0t, g0)
    dtht, dWt = o64.chain_backward(dt, Wt, tht, gth)

    def flat_grad(ch):
        return ch.theta.grad.cpu().numpy()

    for got, ref, what in ((flat_grad(rec), dWr, "reconstructor dW"), (flat_grad(lo_z0), dWz, "lo_z0 dW"),
                           (flat_grad(lo_th), dWt, "lo_theta dW"), (z0_t.grad.cpu().numpy().T, dz0t, "dz̃0"),
                           (th_t.grad.cpu().numpy().T, dtht, "dθ̃")):
        s = np.abs(ref).max()
        assert s > 0 and np.abs(got - ref).max() <= 2e-4 * s, what


def test_chain_large_column_count(o32):
    """N = 300 001 columns (ragged, many tiles per CU, > 16 slots per virtual tile of the weight gradient): forward and
    gradients against the oracle."""
    from tests.gpu_util import NativeChain
    sizes, acts, skips = (8, 32, 32, 8), (O.CACT_TANH, O.CACT_RELU, O.CACT_IDENTITY), (0, 1, 0)
    N = 300_001
    d = O.make_chain_desc(sizes, acts, skips)
    W = O.mlp_weights(sizes, seed=2)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N, 8)).astype(np.float32)
    dy = (rng.standard_normal((N, 8)) / N).astype(np.float32)
    nat = NativeChain(sizes, acts, skips)
    nat.set_weights(W)
    y = nat.forward(x)
    yr = o32.chain_forward(d, W, x)
    assert np.abs(y - yr).max() <= 2e-5 * max(1.0, np.abs(yr).max())
    dx, dW = nat.backward(x, y, dy)
    rx, rW = o32.chain_backward(d, W, x, dy)
    # 300 001 columns × 32 relu units behind a tanh layer: about one unit in 10⁷ has a pre-activation within an ulp of zero, and two
    # correct f32 tanh implementations (the kernel's v_exp-based one, ≤ 3e-7 relative; libm's on the CPU) put it on different sides of
    # the kink — that column's input gradient then moves by a few per cent. At most three such columns are tolerated; every other
    # column agrees to 1e-4 of the scale.
    col_err = np.abs(dx - rx).max(axis=1)
    bad = col_err > 1e-4 * np.abs(rx).max()
    assert bad.sum() <= 3 and col_err.max() <= 0.1 * np.abs(rx).max(), (int(bad.sum()), float(col_err.max()))
    # dW entries are sums of 3e5 zero-mean terms (magnitude ≈ √N single terms): ONE flipped relu term moves an entry by ≈ 1/√N = 1.8e-3 of
    # the scale — the gate is 2e-4 (f32 summation order) when no column flipped, 3e-3 otherwise
    assert np.abs(dW - rW).max() <= (2e-4 if bad.sum() == 0 else 3e-3) * np.abs(rW).max()


@pytest.mark.parametrize("spec", [RECON, FE, ONE], ids=["reconstructor", "feature_extractor", "one"])
def test_one_chain_handle_changing_column_counts(o32, spec):
    """One handle, column counts growing and shrinking (ragged last minibatch, validation set after a training batch):
    every workspace regrows cleanly, results match the oracle at each size, plain and saved-activation variants."""
    from tests.gpu_util import NativeChain
    sizes, acts, skips = spec
    d = O.make_chain_desc(sizes, acts, skips)
    W = O.mlp_weights(sizes, seed=9)
    nat = NativeChain(sizes, acts, skips)
    nat.set_weights(W)
    for N in (5, 300, 17, 2000, 64, 2001):
        rng = np.random.default_rng(N)
        x = rng.standard_normal((N, sizes[0])).astype(np.float32)
        dy = (rng.standard_normal((N, sizes[-1])) / N).astype(np.float32)
        yr = o32.chain_forward(d, W, x)
        rx, rW = o32.chain_backward(d, W, x, dy)
        y = nat.forward(x)
        assert np.abs(y - yr).max() <= 2e-5 * max(1.0, np.abs(yr).max()), N
        y2, saved = nat.forward_save(x)
        assert np.array_equal(y, y2), N
        for dx, dW in (nat.backward(x, y, dy), nat.backward_saved(x, y2, dy, saved)):
            assert np.abs(dx - rx).max() <= 1e-4 * np.abs(rx).max() and np.abs(dW - rW).max() <= 1e-4 * np.abs(rW).max(), N


def test_overwrite_mode_of_the_weight_gradient(o32):
    """lde_chain_set_accumulate(0) / lde_rnn_set_accumulate(0): dW = gradient — a dW buffer full of garbage comes back as the plain
    gradient (bit-identical to accumulating into zeros), for a multi-layer chain, a one-layer chain and an LSTM stack."""
    import ctypes as C
    from tests.gpu_util import NativeChain, NativeRnn
    for spec, N in ((RECON, 300), (ONE, 37)):
        sizes, acts, skips = spec
        W = O.mlp_weights(sizes, seed=3)
        rng = np.random.default_rng(N)
        x = rng.standard_normal((N, sizes[0])).astype(np.float32)
        dy = (rng.standard_normal((N, sizes[-1])) / N).astype(np.float32)
        nat = NativeChain(sizes, acts, skips)
        nat.set_weights(W)
        y = nat.forward(x)
        _, ref = nat.backward(x, y, dy)
        assert nat.lib.lde_chain_set_accumulate(nat.h, 0) == 0
        _, got = nat.backward(x, y, dy, dW0=np.full(nat.nW, 123.0, np.float32))
        assert np.array_equal(got, ref)
        assert nat.lib.lde_chain_set_accumulate(nat.h, 1) == 0
        _, acc = nat.backward(x, y, dy, dW0=np.full(nat.nW, 0.5, np.float32))
        assert np.abs((acc - 0.5) - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
    cell, sizes = O.CELL_LSTM, (32, 16, 16)
    W = O.rnn_weights(cell, sizes, seed=3)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((9, 37, 32)).astype(np.float32)
    dy = (rng.standard_normal((37, 16)) / 37).astype(np.float32)
    nat = NativeRnn(cell, sizes, True)
    nat.set_weights(W)
    _, ref = nat.backward(x, dy)
    assert nat.lib.lde_rnn_set_accumulate(nat.h, 0) == 0
    _, got = nat.backward(x, dy, dW0=np.full(nat.nW, -7.0, np.float32))
    assert np.array_equal(got, ref)


def test_torch_bridge_takes_the_training_variant():
    """Through autograd the forward call must keep the hidden activations (lde_chain_forward_save) so that the pullback does not
    recompute them: inside torch.autograd.Function.forward grad mode is off, so the decision has to come from ctx.needs_input_grad
    (until round 3 it asked torch.is_grad_enabled() and never took the variant). Same numbers either way (bit-equal, test above)."""
    import torch
    from latentdiffeq_amd.chain import Chain, Dense
    c = Chain(Dense(16, 40, "relu"), Dense(40, 3, "identity")).to("cuda")
    x = torch.randn(50, 16, device="cuda")
    y = c.apply_batch_major(x)                                   # the parameter requires a gradient
    assert y.grad_fn is not None and y.grad_fn.has_saved is True
    y.sum().backward()
    g_saved = c.theta.grad.clone()
    with torch.no_grad():
        assert c.apply_batch_major(x).grad_fn is None
    c.theta.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    y2 = c.apply_batch_major(xr)                                 # only the input does: still the training variant
    assert y2.grad_fn.has_saved is True and torch.equal(y2, y)
    assert c.apply_batch_major(x).grad_fn is None                # nothing does: plain forward
    # the recomputing pullback (C ABI, no saved buffer) gives the same weight gradient bit for bit
    from tests.gpu_util import NativeChain
    nat = NativeChain(c.sizes, c.acts, c.skips)
    nat.set_weights(c.theta.detach().cpu().numpy())
    xn = x.cpu().numpy()
    yn = nat.forward(xn)
    _, dW = nat.backward(xn, yn, np.ones_like(yn))
    assert np.array_equal(dW, g_saved.cpu().numpy())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reconstructor_under_mse_as_one_node(dtype):
    """chain.decode_loss: the reconstructor and reconstruction_loss (+ the β·KL term) as ONE autograd node whose pullback forms the loss's
    cotangent 2·g·scale·(x̂ − x) where the chain's pullback reads its output gradient (lde_chain_backward_saved_mse) — against `decode`
    followed by `reconstruction_loss` (lde_mse_backward writes that array, lde_chain_backward_saved reads it back): the loss and every
    gradient bit for bit, f32 and bf16 chains, full and ragged tiles, a loss cotangent other than 1, and x̂ used a second time downstream
    (its own cotangent is then added in the kernel instead of by autograd)."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import chain as CH
    from latentdiffeq_amd.loss import reconstruction_loss
    torch.manual_seed(4)
    mt, diffeq = la.GOKU_basic(), la.Pendulum()
    NI = 96
    lo, de, rec = CH.default_decoder_layers(mt, NI, diffeq, device="cuda", hidden_dim_resnet=56)
    with torch.no_grad():
        lo[1]._dense[-1].bias.fill_(1.0)
    rec.set_dtype(dtype)
    dec = la.Decoder(mt, (lo, de, rec))
    params = [p for m in (*lo, rec) for p in m.parameters()]
    keep = CH._RECON_MSE
    try:
        # (gfac: the loss's cotangent. The bf16 chain's one node leaves δ_L′ = 2·scale·(x̂ − x)·σ′ in the forward launch and multiplies by g
        #  at the END of the pullback — lde_chain_backward_saved_delta, round 4 — so with g = 1 its bits are the two-call path's, and with
        #  g ≠ 1 they differ by the bf16 rounding of δ (g·δ rounded against δ rounded): compared to that level. x̂ used a second time
        #  carries its own cotangent: the staged δ is not used then.)
        for B, T, second_use, gfac in ((24, 12, False, 1.7), (64, 50, False, 1.7), (64, 50, False, 1.0), (33, 9, True, 1.7)):
            ts = np.arange(T) * 0.05
            x = torch.rand(T, B, NI, device="cuda").permute(2, 1, 0)
            l0 = (torch.randn(16, B, device="cuda"), torch.randn(16, B, device="cuda"))
            plus0 = torch.tensor(0.37, device="cuda")
            w2 = torch.randn(NI, B, T, device="cuda")
            res = []
            for fused in (True, False):
                CH._RECON_MSE = fused
                for p in params:
                    p.grad = None
                lt = tuple(t_.clone().requires_grad_(True) for t_ in l0)
                plus = plus0.clone().requires_grad_(True)
                loss, (x_hat, z_hat, _) = CH.decode_loss(dec, lt, ts, x, 4 * B, plus=plus)
                total = gfac * loss + ((x_hat * w2).sum() if second_use else 0.0)
                total.backward()
                torch.cuda.synchronize()
                res.append((loss.detach().clone(), x_hat.detach().clone(), [p.grad.clone() for p in params] + [t_.grad.clone() for t_ in lt] + [plus.grad.clone()]))
            # (the one node sums the squares per column tile in the reconstructor's last epilogue, lde_mse_forward per slice of the flat array:
            #  the loss value agrees to rounding — 2e-6 —, and bit for bit with LDE_RECON_MSE_FWD=0; x̂ and every gradient are the same bits)
            assert abs(float(res[0][0]) - float(res[1][0])) <= 2e-6 * abs(float(res[1][0])) and torch.equal(res[0][1], res[1][1]), (B, T)
            rounded = dtype == "bf16" and gfac != 1.0 and not second_use
            for i, (a, b) in enumerate(zip(res[0][2], res[1][2])):
                if rounded:
                    assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max()) and float((a - b).norm()) <= 5e-3 * float(b.norm()), (B, T, i)
                else:
                    assert torch.equal(a, b), (B, T, second_use, gfac, i)
    finally:
        CH._RECON_MSE = keep


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_chains_equal_separate_calls(dtype):
    """lde_chain_group_forward_save / _backward_saved (chain.apply_chains_grouped): independent chains as ONE autograd node, one launch
    per stage when the library can merge them — the reference's apply_latent_in heads and apply_latent_out chains. Per chain the same
    kernels on the same arguments: outputs, input gradients and weight gradients equal the separate calls bit for bit. Cases: the
    GOKU bottleneck's shapes (four single Dense heads; 16→200→2 and 16→200→1), different column counts per chain, a skip / tanh
    chain, a group whose members ask for different kernels (a 12 800-column reconstructor beside a small chain: not merged, still
    equal), and more chains than one group takes (run separately)."""
    import torch
    from latentdiffeq_amd.chain import Chain, Dense, SkipConnection, apply_chains_grouped
    torch.manual_seed(5)
    dev = "cuda"

    def mk(*layers):
        c = Chain(*layers).to(dev)
        if dtype == "bf16":
            c.set_dtype("bf16")
        return c

    cases = {
        "latent_in": [(mk(Dense(16, 16)), 256), (mk(Dense(32, 16)), 256), (mk(Dense(16, 16)), 256), (mk(Dense(32, 16)), 256)],
        "latent_out": [(mk(Dense(16, 200, "relu"), Dense(200, 2)), 256), (mk(Dense(16, 200, "relu"), Dense(200, 1, "softplus")), 256)],
        "ragged": [(mk(Dense(7, 33, "tanh"), SkipConnection(Dense(33, 33, "tanh")), Dense(33, 5)), 40), (mk(Dense(16, 16, "sigmoid")), 1000),
                   (mk(Dense(3, 64, "relu"), Dense(64, 3)), 17)],
        "mixed_kernels": [(mk(Dense(2, 200, "relu"), SkipConnection(Dense(200, 200, "relu")), Dense(200, 784, "sigmoid")), 12800),
                          (mk(Dense(16, 200, "relu"), Dense(200, 2)), 256)],
        "five": [(mk(Dense(8, 8)), 64) for _ in range(5)],
    }
    for name, members in cases.items():
        xs = [torch.randn(c.sizes[0], N, device=dev) for c, N in members]
        gs = [torch.randn(c.sizes[-1], N, device=dev) for c, N in members]

        def run(grouped):
            xr = [x.clone().requires_grad_(True) for x in xs]
            for c, _ in members:
                c.theta.grad = None
            pairs = [(c, x) for (c, _), x in zip(members, xr)]
            ys = apply_chains_grouped(pairs) if grouped else [c(x) for c, x in pairs]
            torch.autograd.backward(ys, gs)
            torch.cuda.synchronize()
            return [y.detach().clone() for y in ys], [x.grad.clone() for x in xr], [c.theta.grad.clone() for c, _ in members]

        a, b = run(False), run(True)
        for what, u, v in zip(("y", "dx", "dW"), a, b):
            for i, (p, q) in enumerate(zip(u, v)):
                assert torch.equal(p, q), (dtype, name, what, i, float((p - q).abs().max()))
    # the SAME chain twice in a group (one module applied to two inputs): its workspace serves one call at a time — run one after the other
    c = mk(Dense(16, 200, "relu"), Dense(200, 2))
    xa, xb = torch.randn(16, 256, device=dev), torch.randn(16, 256, device=dev)
    ga, gb = torch.randn(2, 256, device=dev), torch.randn(2, 256, device=dev)
    ref = []
    for grouped in (False, True):
        c.theta.grad = None
        xr = [xa.clone().requires_grad_(True), xb.clone().requires_grad_(True)]
        ys = apply_chains_grouped([(c, xr[0]), (c, xr[1])]) if grouped else [c(xr[0]), c(xr[1])]
        torch.autograd.backward(ys, [ga, gb])
        ref.append(([y.detach().clone() for y in ys], [x.grad.clone() for x in xr], c.theta.grad.clone()))
    assert all(torch.equal(u, v) for u, v in zip(ref[0][0] + ref[0][1], ref[1][0] + ref[1][1]))
    assert torch.allclose(ref[0][2], ref[1][2], rtol=0, atol=1e-6 * float(ref[0][2].abs().max()))     # (Σ of two gradients: the order of the two adds)
    # frozen inputs (no dx asked for) and evaluation without gradients go through the same entry points
    c1, c2 = mk(Dense(16, 16)), mk(Dense(16, 200, "relu"), Dense(200, 2))
    x = torch.randn(16, 64, device=dev)
    y1, y2 = apply_chains_grouped([(c1, x), (c2, x)])
    torch.autograd.backward([y1, y2], [torch.ones_like(y1), torch.ones_like(y2)])
    with torch.no_grad():
        z1, z2 = apply_chains_grouped([(c1, x), (c2, x)])
    assert torch.equal(z1, y1) and torch.equal(z2, y2) and c1.theta.grad is not None


def test_group_entry_points_validate():
    import ctypes as C
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    assert lib.lde_chain_group_forward_save(0, None, None, None, None, None, None) == -1
    assert lib.lde_chain_group_forward_save(2, None, None, None, None, None, None) == -1
    hs = (C.c_void_p * 2)(None, None)
    assert lib.lde_chain_group_forward_save(2, hs, hs, (C.c_int64 * 2)(1, 1), hs, None, None) == -1        # NULL chain handle
    assert lib.lde_chain_group_backward_saved(2, hs, hs, hs, hs, None, (C.c_int64 * 2)(1, 1), None, hs, None) == -1



@pytest.mark.parametrize("dtype,out", [("f32", 1), ("bf16", 1), ("bf16", 8)], ids=["f32", "bf16", "bf16_out8"])
def test_extras_of_one_entry_point_do_not_reach_the_next(dtype, out):
    """What a call carries beyond its arrays — further output gradients, the loss target and cotangent, the staged-δ cotangent, the loss
    target of the forward pass — belongs to THAT call: on one handle, after each of lde_chain_backward_saved_sum (three arrays),
    lde_chain_backward_saved_mse (with a further cotangent), two refused lde_chain_backward_saved_sum calls, the staged-δ pair (bf16) and
    lde_chain_forward_save_mse, a plain lde_chain_forward_save + lde_chain_backward_saved gives the bits a fresh handle gave. C ABI through
    ctypes; 16 → 200 → out (relu, softplus), N = 37: three 16-column tiles, the last ragged; overwrite mode. out = 1: the latent_out head
    (lde_chain_forward_save_mse_delta needs an output width that is a multiple of 8 and is refused there); out = 8: the pair runs.
    The three-array sum is formed as (dy₁ + dy₂) + dy₃ in f32 where the output gradient is read: against the plain call on the array
    summed beforehand it may differ by the rounding of a three-term sum, 3·2⁻²⁴ of the largest entry."""
    import ctypes as C
    import torch
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import NativeChain
    sizes, acts, N = (16, 200, out), (O.CACT_RELU, O.CACT_SOFTPLUS), 37
    W = O.mlp_weights(sizes, seed=11)
    g = torch.Generator().manual_seed(3)
    dev = "cuda"
    x = torch.randn(N, 16, generator=g).to(dev)
    dys = [(torch.randn(N, out, generator=g) / N).to(dev) for _ in range(3)]
    target = torch.rand(N, out, generator=g).to(dev)
    gdev = torch.tensor([1.3], device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()

    def handle():
        nat = NativeChain(sizes, acts)
        nat.set_weights(W)
        nat.set_dtype(dtype)
        assert nat.lib.lde_chain_set_accumulate(nat.h, 0) == 0
        return nat

    def plain(nat, dy):
        lib, s = nat.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        y, dx, dW = torch.full((N, out), 7.0, device=dev), torch.full((N, 16), 7.0, device=dev), torch.full((nat.nW,), 7.0, device=dev)
        saved = torch.full((int(lib.lde_chain_saved_floats(nat.h, N)),), 7.0, device=dev)
        assert lib.lde_chain_forward_save(nat.h, vp(x), N, vp(y), vp(saved), s) == 0
        assert lib.lde_chain_backward_saved(nat.h, vp(x), vp(y), vp(dy), vp(saved), N, vp(dx), vp(dW), s) == 0
        torch.cuda.synchronize()
        return y.cpu().numpy(), dx.cpu().numpy(), dW.cpu().numpy(), saved, y

    fresh = handle()
    ref = plain(fresh, dys[0])[:3]
    presum = plain(fresh, (dys[0] + dys[1]) + dys[2])[:3]
    nat = handle()
    lib, s = nat.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    y0, dx0, dW0, saved, yd = plain(nat, dys[0])
    assert np.array_equal(y0, ref[0]) and np.array_equal(dx0, ref[1]) and np.array_equal(dW0, ref[2])

    def still_plain(after):
        got = plain(nat, dys[0])
        for a, b, what in zip(got[:3], ref, ("y", "dx", "dW")):
            assert np.array_equal(a, b), (after, what, float(np.abs(a - b).max()))

    dx, dW = torch.full((N, 16), 7.0, device=dev), torch.full((nat.nW,), 7.0, device=dev)
    scratch = torch.zeros((int(lib.lde_chain_mse_scratch_floats(nat.h, N)),), device=dev)
    loss = torch.zeros((1,), device=dev)
    # (i) three output gradients, summed where they are read
    arr = (C.c_void_p * 4)(*[t.data_ptr() for t in dys], dys[0].data_ptr())
    assert lib.lde_chain_backward_saved_sum(nat.h, vp(x), vp(yd), 3, arr, vp(saved), N, vp(dx), vp(dW), s) == 0
    torch.cuda.synchronize()
    for a, b, what in ((dx.cpu().numpy(), presum[1], "dx"), (dW.cpu().numpy(), presum[2], "dW")):
        err, bound = float(np.abs(a - b).max()), 3 * 2.0 ** -24 * float(np.abs(b).max())
        print(f"saved_sum vs pre-summed {dtype} out={out} {what}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, err, bound)
    still_plain("saved_sum")
    # (ii) the loss's cotangent formed in the kernel, plus a further one
    assert lib.lde_chain_backward_saved_mse(nat.h, vp(x), vp(yd), vp(target), vp(gdev), 0.25, vp(dys[1]), vp(saved), N, vp(dx), vp(dW), s) == 0
    torch.cuda.synchronize()
    # (the kernel forms 2·(g·scale)·(y − target) + dy_more in f32, each product and sum rounded on its own — the same four operations as
    #  the torch expression below: against the plain call on that array at most their four roundings, 4·2⁻²⁴ of the largest entry)
    dy_mse = (2.0 * (gdev * 0.25)) * (yd - target) + dys[1]
    want_mse = plain(fresh, dy_mse)[:3]
    for a, b, what in ((dx.cpu().numpy(), want_mse[1], "dx"), (dW.cpu().numpy(), want_mse[2], "dW")):
        err, bound = float(np.abs(a - b).max()), 4 * 2.0 ** -24 * float(np.abs(b).max())
        print(f"saved_mse vs the cotangent formed beforehand {dtype} out={out} {what}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, err, bound)
    still_plain("saved_mse")
    # (iii) refused calls: four arrays; a misaligned second array
    assert lib.lde_chain_backward_saved_sum(nat.h, vp(x), vp(yd), 4, arr, vp(saved), N, vp(dx), vp(dW), s) == -1      # LDE_ERR_INVALID_ARG
    assert len(lib.lde_chain_last_error(nat.h)) > 0
    odd = torch.zeros((N * out + 1,), device=dev)
    arr2 = (C.c_void_p * 2)(dys[0].data_ptr(), odd.data_ptr() + 4)
    assert lib.lde_chain_backward_saved_sum(nat.h, vp(x), vp(yd), 2, arr2, vp(saved), N, vp(dx), vp(dW), s) == -1
    assert b"unaligned" in lib.lde_chain_last_error(nat.h)
    still_plain("refused saved_sum")
    # (iv) bf16: the forward pass leaves δ_L′, the pullback starts from it
    if dtype == "bf16":
        rc = lib.lde_chain_forward_save_mse_delta(nat.h, vp(x), N, vp(yd), vp(saved), vp(target), 0.25, None, vp(loss), vp(scratch), s)
        if out % 8 == 0:
            assert rc == 0 and lib.lde_chain_delta_is_staged(nat.h, vp(saved), N) == 1
            assert lib.lde_chain_backward_saved_delta(nat.h, vp(x), vp(gdev), vp(saved), N, vp(dx), vp(dW), s) == 0
            torch.cuda.synchronize()
            assert torch.isfinite(dx).all() and torch.isfinite(dW).all() and lib.lde_chain_delta_is_staged(nat.h, vp(saved), N) == 0
        else:
            assert rc == -2 and len(lib.lde_chain_last_error(nat.h)) > 0                                               # LDE_ERR_UNSUPPORTED
            assert lib.lde_chain_backward_saved_delta(nat.h, vp(x), vp(gdev), vp(saved), N, vp(dx), vp(dW), s) == -1   # nothing staged
        still_plain("staged delta")
    # (v) the loss from the forward pass's last epilogue
    ym = torch.full((N, out), 7.0, device=dev)
    assert lib.lde_chain_forward_save_mse(nat.h, vp(x), N, vp(ym), vp(saved), vp(target), 0.25, None, vp(loss), vp(scratch), s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ym.cpu().numpy(), ref[0])
    want = 0.25 * float(((ym.double() - target.double()) ** 2).sum())
    assert abs(float(loss) - want) <= 1e-5 * want
    still_plain("forward_save_mse")
