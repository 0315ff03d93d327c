"""CPU: tests/step_ref.py — the composed reference the GPU step tests judge the product by — held to something independent of it.

(1) Its gradients against central differences of ITS OWN float64 loss. Tiny models of each type (pixels ≤ 12, resnet width ≤ 10, B = 3,
    T = 5; `default_layers(..., device="cpu")` only hands over shapes and weights) with a fixed-step solver, so that the loss is a smooth
    function of the weights and the discrete pullback is its exact derivative: GOKU + Pendulum (RK4), GOKU + LotkaVolterra (RK4), LatentODE
    + NODE with augment_dim = 2 (RK4, coupled), and a GOKU with the custom encoder of tests/test_gpu_step_models.py in small (tanh-RNN and
    GRU stacks of unequal widths) on the stochastic pendulum (EulerHeun along one drawn path). One random unit direction per module; the
    directional derivative by central differences at h = 2e-5 and h = 1e-5 must equal ⟨gradient, direction⟩.
(2) Each fault of step_ref.FAULTS — a swapped μ / log σ² head, a dropped second gradient source, D for D′ as the reconstructor's leading
    dimension, θ̂'s columns permuted — moves the reference's gradients by more than the GPU tests' tolerance: the comparison would notice.
(3) The same code at f32 (Oracle("f32"), the numpy references at np.float32) stays beside the float64 result.
"""
import numpy as np
import pytest

from tests import step_ref as S

GPU_GRAD_TOL = 2e-3          # tests/test_gpu_composed_step.py, tests/test_gpu_step_models.py: relative L2 per module
FD_BOUND = 9e-6              # 10 × the measured worst case, 8.5e-7 (the docstrings of the two central-difference tests)
KINDS = ["goku_pendulum", "goku_lv", "latentode_aug", "goku_gru_sde"]
B, T, NI, BETA = 3, 5, 12, 0.5


def _build(kind):
    import torch
    import latentdiffeq_amd as M
    from latentdiffeq_amd import train as TR
    from latentdiffeq_amd.chain import Chain, Dense
    from latentdiffeq_amd.recurrent import GRU, RNN, Recurrent
    torch.manual_seed({"goku_pendulum": 11, "goku_lv": 12, "latentode_aug": 13, "goku_gru_sde": 14}[kind])
    fixed = dict(solver=M.RK4(), adaptive=False, dt=0.05)
    kw = dict(device="cpu", hidden_dim_resnet=10, latent_to_diffeq_dim=10, rnn_input_dim=6, latent_dim_z0=4, latent_dim_theta=4)
    if kind == "latentode_aug":
        mt = M.LatentODE()
        diffeq = M.NODE(4, hidden_dim=8, augment_dim=2, sensealg=M.DiscreteSensitivity(), activation="tanh", **fixed)
        enc, dec = TR.default_layers(mt, NI, diffeq, rnn_output_dim=7, **kw)
    else:
        mt = M.GOKU_basic()
        diffeq = {"goku_pendulum": lambda: M.Pendulum(**fixed), "goku_lv": lambda: M.LotkaVolterra(**fixed),
                  "goku_gru_sde": lambda: M.SPendulum(seed=3)}[kind]()
        enc, dec = TR.default_layers(mt, NI, diffeq, rnn_output_dim=5, **kw)
        if kind == "goku_gru_sde":
            diffeq.offset = 2
            pe = (Recurrent(RNN(6, 5, "tanh"), RNN(5, 5, "tanh"), reverse=True), Recurrent(GRU(6, 3), GRU(3, 3)),
                  Recurrent(GRU(6, 4), GRU(4, 4), reverse=True))
            li = (Chain(Dense(5, 4)), Chain(Dense(5, 4)), Chain(Dense(7, 4)), Chain(Dense(7, 4)))
            enc = (enc[0], pe, li)
    model = TR.LatentDiffEqModel(mt, enc, dec)
    with torch.no_grad():
        for m in model.modules():
            for p in m.parameters():
                if p.dim() == 1:
                    p.add_(torch.empty_like(p).uniform_(-0.2, 0.2))
        if mt.__class__.__name__ == "GOKU_basic":
            dec[0][1]._dense[-1].bias.fill_(1.0)             # pendulum lengths / Lotka–Volterra rates away from zero
            if kind == "goku_lv":
                dec[0][0]._dense[-1].bias.fill_(1.0)         # populations too
    spec, names, W = S.spec_of(model)
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (T, B, NI))
    eps = rng.standard_normal((B, 4)) if kind == "latentode_aug" else (rng.standard_normal((B, 4)), rng.standard_normal((B, 4)))
    return spec, names, W, x, eps, 0.05 * np.arange(T)


_built = {}


def _case(kind):
    if kind not in _built:
        _built[kind] = _build(kind)
    return _built[kind]


_clean = {}


def _reference(kind, o64):
    if kind not in _clean:
        spec, _, W, x, eps, ts = _case(kind)
        _clean[kind] = S.evaluate(spec, W, x, eps, BETA, ts, o64, want_dx=True)
    return _clean[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_equal_central_differences(o64, kind):
    """Per module m and a random unit direction d: (loss(W_m + h·d) − loss(W_m − h·d)) / 2h at h = 2e-5 and 1e-5 against ⟨∂loss/∂W_m, d⟩,
    relative to |⟨∂loss/∂W_m, d⟩|; the two difference quotients must also agree with each other to the same bound (no relu kink crossed).

    Measured worst case over the modules, both step sizes (float64, this file's seeds):
        goku_pendulum 7.9e-08   goku_lv 7.0e-07   latentode_aug 3.4e-07   goku_gru_sde 2.3e-08
    (the largest where ⟨g, d⟩ itself is small, 4.5e-5: the difference quotient's own round-off, ≈ 1e-15 / h). With the frames' check below the
    worst is 8.5e-07; FD_BOUND = 9e-6 is 10 × that, and 220 × below the GPU tests' gradient tolerance 2e-3 (it has to be ≥ 100 × below)."""
    spec, names, W, x, eps, ts = _case(kind)
    ref = _reference(kind, o64)
    rng = np.random.default_rng(17)
    worst = 0.0
    for m, name in enumerate(names):
        d = rng.standard_normal(W[m].shape)
        d /= np.linalg.norm(d)
        want = float(ref["grads"][m] @ d)
        fds = []
        for h in (2e-5, 1e-5):
            lp, lm = (S.evaluate(spec, W[:m] + [W[m] + sg * h * d] + W[m + 1:], x, eps, BETA, ts, o64)["loss"] for sg in (1, -1))
            fds.append((lp - lm) / (2 * h))
        rel = max(abs(fd - want) for fd in fds) / abs(want)
        print(f"{kind} {name}: <g,d> = {want:.6e}, fd = {fds[0]:.6e} / {fds[1]:.6e}, rel = {rel:.2e}")
        assert abs(fds[0] - fds[1]) <= FD_BOUND * abs(want), (name, "the two step sizes disagree", fds)
        assert rel <= FD_BOUND, (name, rel)
        worst = max(worst, rel)
    print(f"{kind}: worst {worst:.2e}")
    assert FD_BOUND <= GPU_GRAD_TOL / 100


@pytest.mark.parametrize("kind", KINDS)
def test_frame_gradient_equals_central_differences(o64, kind):
    """dx of the reference = the derivative of the loss through the ENCODER's reading of the frames, the loss's target held fixed: the
    difference quotient perturbs the frames, and the change of the target's own term, Σ 2·(x − x̂)·d/(B·T) (known in closed form from the
    unperturbed x̂: the term is quadratic in x), is taken off. Same step sizes and bound as the weights' check. Measured: goku_pendulum 2.8e-07, goku_lv 6.3e-08, latentode_aug 8.5e-07,
    goku_gru_sde 5.6e-08."""
    spec, names, W, x, eps, ts = _case(kind)
    ref = _reference(kind, o64)
    d = np.random.default_rng(23).standard_normal(x.shape)
    d /= np.linalg.norm(d)
    want = float((ref["dx"] * d).sum())
    # x̂ of the unperturbed step, from the reference's own pieces: ∂/∂x of scale·Σ(x − x̂)² at fixed x̂ is 2·scale·(x − x̂)
    xh = _x_hat(spec, W, x, eps, ts, o64)
    direct = float((2.0 / (B * T) * (x - xh) * d).sum())
    fds = []
    for h in (2e-5, 1e-5):
        lp, lm = (S.evaluate(spec, W, x + sg * h * d, eps, BETA, ts, o64)["loss"] for sg in (1, -1))
        fds.append((lp - lm) / (2 * h) - direct)
    rel = max(abs(fd - want) for fd in fds) / abs(want)
    print(f"{kind} frames: <g,d> = {want:.6e}, fd = {fds[0]:.6e} / {fds[1]:.6e}, rel = {rel:.2e}")
    assert rel <= FD_BOUND, rel


def _x_hat(spec, W, x, eps, ts, o64):
    """x̂ (T, B, pixels) recovered from the reference's loss: evaluate() does not return it, so it is rebuilt from ẑ and the reconstructor."""
    z = S.evaluate(spec, W, x, eps, BETA, ts, o64)["z"]
    return S._Ops(o64).fwd(spec["rec"], W[-1], z.reshape(T * B, -1)).reshape(x.shape)


FAULT_CASES = [("swap_heads", "goku_pendulum"), ("swap_heads", "latentode_aug"), ("drop_second_source", "goku_pendulum"),
               ("drop_second_source", "latentode_aug"), ("drop_second_source", "goku_gru_sde"), ("rec_width_D", "latentode_aug"),
               ("theta_perm", "goku_lv")]


@pytest.mark.parametrize("fault,kind", FAULT_CASES)
def test_injected_faults_move_the_result(o64, fault, kind):
    """The faulty composition's gradients sit farther from the clean ones than the GPU tolerance (relative L2, some module) — by a factor of
    ten at least, so that the comparison in tests/test_gpu_step_models.py cannot mistake one for round-off."""
    spec, names, W, x, eps, ts = _case(kind)
    ref = _reference(kind, o64)
    bad = S.evaluate(spec, W, x, eps, BETA, ts, o64, fault=fault)
    rels = {n: S.rel_l2(a, b) for n, a, b in zip(names, bad["grads"], ref["grads"])}
    print(fault, kind, "loss", abs(bad["loss"] - ref["loss"]) / abs(ref["loss"]), {n: f"{r:.1e}" for n, r in rels.items()})
    assert max(rels.values()) > 10 * GPU_GRAD_TOL, rels


@pytest.mark.parametrize("kind", KINDS)
def test_the_same_code_runs_in_f32(o32, o64, kind):
    """Oracle("f32") and dtype = np.float32 through every branch of the composition: f32 round-off through ≈ 20 layers against float64 —
    the loss to 1e-5, every gradient to 2e-3 (the GPU tests' own numbers: a correct f32 step sits inside them)."""
    spec, names, W, x, eps, ts = _case(kind)
    ref = _reference(kind, o64)
    r32 = S.evaluate(spec, W, x.astype(np.float32), eps, BETA, ts, o32, want_dx=True)
    assert r32["z"].dtype == np.float32
    assert abs(r32["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    for n, a, b in zip(names, r32["grads"], ref["grads"]):
        assert S.rel_l2(a, b) <= GPU_GRAD_TOL, (n, S.rel_l2(a, b))
    assert S.rel_l2(r32["dx"], ref["dx"]) <= GPU_GRAD_TOL
