"""GPU: one whole f32 training step of every model the library ships — forward and pullback in one autograd graph — against the composed
float64 reference tests/step_ref.py (pinned on the CPU by tests/test_step_ref.py). tests/test_gpu_composed_step.py anchors the default
GOKU + Pendulum() step at 784 pixels; here, at 48 pixels, resnet width 40, T = 12 and B = 20 (a ragged 16-row tile, T·B = 240 no multiple
of 64; one case again at B = 64, the full-tile twin):

    latentode_default       LatentODE(), NODE(6, hidden_dim=32) coupled, InterpolatingAdjoint: the non-GOKU encode, the generic recurrent kernel
                            (32-32-32), the non-pair sample / KL, the NODE's dW through flat_weights()
    latentode_discrete_aug  the same with augment_dim = 2, DiscreteSensitivity(), tanh: D′ = 8 ≠ D = 6 through ẑ, the reconstructor, _ChainMseFn
    latentode_per_traj      batching="per_trajectory": the other control mode under the same model code
    goku_friction           Pendulum_friction(): k_pend_forward_sh + the discrete sweep inside the step
    goku_lv                 LotkaVolterra(): the 4-wide softplus θ head, the dual record on the autograd node, k_lv_adjoint_dual
    goku_sde                SPendulum(seed=11), EulerHeun: the (seed, offset) carried by the node — the reference draws the same path
    goku_custom_encoder     Pendulum(); stacks tanh-RNN 32-20-20 (reversed), GRU 32-12-12, GRU 32-16-16 (reversed): hf ≠ hb in the vcat, GRU
                            in the group, a non-default ẑ₀ stack; also at B = 64

Every case runs (a) encode → sample_with_kl(eps=ε) → decode → reconstruction_loss(plus=β·KL) with ε handed to both sides, (b) the same through
decode_loss(want_x_hat=False) — the fused path of train.loss_batch — with β a number and β a device word, which must agree bit for bit, and
(c) train.loss_batch(model, x, t, β, variational=False) with β a number and β a word, which must agree with each other and with the reference
of l̃ = μ. goku_custom_encoder and latentode_default run (a) with recurrent._BRANCH_STREAMS True and False; for GOKU the False run must have
gone through the one-node encoder (recurrent._GokuEncoderFn). Compared every time: the loss, ẑ, every module's flat weight gradient (relative
L2, and finite), the frames' gradient. Weights: biases and initial states nudged off zero; solver abstol = reltol = 1e-6.
β = 0.25 is a power of two: f32(β/B) is the same number however it is formed — the values at which the project states the number / word
property (tests/test_gpu_beta_dev.py::test_python_layer_routes_a_beta_word_to_the_dev_entry_points).

Tolerances. The numbers of tests/test_gpu_composed_step.py — loss 1e-5 relative, ẑ 2e-5, gradients 2e-3 relative L2 — hold for a case when
the GPU result AND the f32 restatement of the reference (step_ref with Oracle("f32"), on the case's inputs) sit inside them; otherwise the
bound is 2 × the f32 restatement's distance from float64 (Z_TOL below: the only two). The two continuous-adjoint cases (latentode_default,
latentode_per_traj) follow tests/test_gpu_mlp.py::_check_grads for the gradients: float64 truth is the reference at abstol = reltol = 1e-10,
every gradient lies within LIM_O·max|truth| of the f32 restatement at the step's own tolerances and no farther from truth than 1.5 × that
restatement plus LIM_T·max|truth| (LIM_O = LIM_T = 5e-3, that file's numbers for the Tsit5 MLP adjoint; the restatement itself sits 3.1e-3
from truth on the NODE's weights, so they cannot be tightened). No case needs the "relu units within round-off of zero may switch" caveat.

MEASURED on an MI355X, worst over the runs of a case, GPU | f32 restatement, each against the float64 reference:

    case                      loss (rel)           ẑ (max abs)          worst module gradient (rel L2)   frames' gradient (rel L2)
    latentode_discrete_aug    1.0e-07 | 9.3e-09    6.8e-07 | 5.9e-07    1.6e-07 | 1.7e-07                2.8e-07 | 3.5e-07
    goku_friction             5.0e-08 | 4.0e-09    9.7e-07 | 3.6e-07    2.1e-07 | 2.9e-07                2.3e-07 | 3.2e-07
    goku_lv                   1.1e-07 | 1.8e-09    5.1e-07 | 7.2e-07    2.2e-07 | 3.0e-07                3.2e-07 | 3.7e-07
    goku_sde                  7.4e-08 | 1.7e-09    5.6e-07 | 5.2e-07    2.6e-07 | 2.5e-07                2.4e-07 | 3.5e-07
    goku_custom_encoder       9.3e-08 | 7.5e-09    2.0e-06 | 9.1e-07    1.5e-07 | 1.8e-07                4.1e-07 | 4.4e-07
    goku_custom_encoder-B64   8.6e-08 | 6.2e-09    3.1e-06 | 3.3e-06    2.4e-07 | 1.4e-07                3.9e-07 | 4.5e-07
    latentode_default         1.1e-07 | 1.5e-08    2.05e-05 | 1.83e-05  (rule above)                     (rule above)
    latentode_per_traj        3.9e-07 | 1.1e-07    5.46e-05 | 4.76e-05  (rule above)                     (rule above)

  latentode_default / latentode_per_traj against truth at 1e-10: ẑ of the f32 restatement is outside 2e-5 on one and the GPU on both, so
  Z_TOL = 2 × the restatement's 1.83e-05 and 4.76e-05. Gradients, in units of max|truth|, worst module (the NODE's weights every time):
      latentode_default   |gpu − f32| 3.4e-3   |gpu − truth| 3.2e-3   |f32 − truth| 3.1e-3
      latentode_per_traj  |gpu − f32| 1.9e-3   |gpu − truth| 2.6e-3   |f32 − truth| 2.1e-3     (frames: |gpu − f32| 1.25e-3)
  In every case the number / word pairs agreed bit for bit; the two stream modes differ only in the frames' gradient's last digits.
"""
import numpy as np
import pytest

from tests import step_ref as S

pytestmark = pytest.mark.gpu

NI, HR, LD, T, BETA = 48, 40, 40, 12, 0.25
TS = 0.05 * np.arange(T)
TOL = 1e-6
LOSS_TOL, GRAD_TOL = 1e-5, 2e-3                        # tests/test_gpu_composed_step.py
Z_TOL = {"latentode_default": 2 * 1.83e-5, "latentode_per_traj": 2 * 4.76e-5}      # 2 × the f32 restatement (module docstring); every other case:
Z_TOL_DEFAULT = 2e-5                                   # tests/test_gpu_composed_step.py
LIM_O = LIM_T = 5e-3                                   # tests/test_gpu_mlp.py::test_tsit5_mlp_adjoint
CONTINUOUS = ("latentode_default", "latentode_per_traj")
BOTH_STREAM_MODES = ("goku_custom_encoder", "latentode_default")
KERNELS = {"goku_friction": (b"k_pend_forward_sh", b"k_pend_adjoint_disc"), "goku_lv": (b"k_lv_forward_dual", b"k_lv_adjoint_dual"),
           "goku_sde": (b"k_pend_forward_sde", b"k_pend_adjoint_dual")}
CASES = [("latentode_default", 20), ("latentode_discrete_aug", 20), ("latentode_per_traj", 20), ("goku_friction", 20), ("goku_lv", 20),
         ("goku_sde", 20), ("goku_custom_encoder", 20), ("goku_custom_encoder", 64)]


def _build(case, dev):
    import torch
    import latentdiffeq_amd as M
    from latentdiffeq_amd import train as TR
    from latentdiffeq_amd.chain import Chain, Dense
    from latentdiffeq_amd.recurrent import GRU, RNN, Recurrent
    torch.manual_seed(40 + [c for c, _ in CASES].index(case))
    tol = dict(abstol=TOL, reltol=TOL)
    kw = dict(device=dev, hidden_dim_resnet=HR, latent_to_diffeq_dim=LD)
    if case.startswith("latentode"):
        mt = M.LatentODE()
        diffeq = {"latentode_default": lambda: M.NODE(6, hidden_dim=32, device=dev, **tol),
                  "latentode_discrete_aug": lambda: M.NODE(6, hidden_dim=32, augment_dim=2, device=dev, sensealg=M.DiscreteSensitivity(),
                                                           activation="tanh", **tol),
                  "latentode_per_traj": lambda: M.NODE(6, hidden_dim=32, device=dev, batching="per_trajectory", **tol)}[case]()
        enc, dec = TR.default_layers(mt, NI, diffeq, **kw)
    else:
        mt = M.GOKU_basic()
        diffeq = {"goku_friction": lambda: M.Pendulum_friction(**tol), "goku_lv": lambda: M.LotkaVolterra(**tol),
                  "goku_sde": lambda: M.SPendulum(seed=11), "goku_custom_encoder": lambda: M.Pendulum(**tol)}[case]()
        enc, dec = TR.default_layers(mt, NI, diffeq, **kw)
        if case == "goku_custom_encoder":
            pe = (Recurrent(RNN(32, 20, "tanh"), RNN(20, 20, "tanh"), reverse=True), Recurrent(GRU(32, 12), GRU(12, 12)),
                  Recurrent(GRU(32, 16), GRU(16, 16), reverse=True))
            li = (Chain(Dense(20, 16)), Chain(Dense(20, 16)), Chain(Dense(28, 16)), Chain(Dense(28, 16)))
            enc = (enc[0], tuple(m.to(dev) for m in pe), tuple(m.to(dev) for m in li))
    model = TR.LatentDiffEqModel(mt, enc, dec)
    with torch.no_grad():      # biases / initial states away from zero so that every term is exercised (tests/test_gpu_rnn.py::test_torch_encoder_path_end_to_end)
        for m in model.modules():
            for p in m.parameters():
                if p.dim() == 1:
                    p.add_(torch.empty_like(p).uniform_(-0.2, 0.2))
        if not case.startswith("latentode"):
            dec[0][1]._dense[-1].bias.fill_(1.0)               # pendulum lengths / Lotka–Volterra rates inside the data range
            if case == "goku_lv":
                dec[0][0]._dense[-1].bias.fill_(1.0)           # populations too
    return model, diffeq


class Step:
    """One case: the model, its inputs, and the runs of the product."""

    def __init__(self, case, B):
        import torch
        self.case, self.B = case, B
        self.dev = torch.device("cuda", 0)
        self.model, self.diffeq = _build(case, self.dev)
        self.goku = not case.startswith("latentode")
        self.spec, self.names, self.W = S.spec_of(self.model)
        rng = np.random.default_rng(7)
        self.x = rng.uniform(0, 1, (T, B, NI)).astype(np.float32)
        n_z = self.model.encoder.latent_in[0].sizes[-1]
        e = [rng.standard_normal((B, n_z)).astype(np.float32), rng.standard_normal((B, 16)).astype(np.float32)]
        self.eps = (e[0], e[1]) if self.goku else e[0]

    def spec_at(self, offset):
        """The structure with the stochastic pendulum's noise offset of one particular forward call."""
        s = dict(self.spec)
        s["solve"] = dict(s["solve"], offset=offset)
        return s

    def reference(self, orc, eps, offset, tol=None):
        return S.evaluate(self.spec_at(offset), self.W, self.x, eps, BETA, TS, orc, want_dx=True, tol=tol)

    def _begin(self, offset):
        import torch
        for p in self.model.parameters():
            p.grad = None
        if hasattr(self.diffeq, "offset"):
            self.diffeq.offset = offset                        # the forward about to be made draws at (seed, offset)
        xb = torch.from_numpy(self.x).to(self.dev).requires_grad_(True)
        return xb, xb.permute(2, 1, 0)

    def _end(self, loss, xb, z_hat=None):
        import torch
        from latentdiffeq_amd import _lib as L
        loss.backward()
        L.join_weight_gradients()
        torch.cuda.synchronize()
        return dict(loss=loss.detach().clone(), z=None if z_hat is None else z_hat.detach().permute(2, 1, 0).cpu().numpy(),
                    grads=S.flat_grads(self.model), dx=xb.grad.detach().cpu().numpy().astype(np.float64))

    def _beta(self, word):
        import torch
        return torch.full((1,), BETA, device=self.dev, dtype=torch.float32) if word else BETA

    def run_eps(self, offset, fused=False, word=False, expect_fused_encoder=False):
        """(a) / (b): ε handed in. fused: decode_loss(want_x_hat=False) instead of decode + reconstruction_loss."""
        import torch
        from latentdiffeq_amd.chain import decode, decode_loss
        from latentdiffeq_amd.loss import reconstruction_loss, sample_with_kl
        from latentdiffeq_amd.recurrent import encode
        xb, x = self._begin(offset)
        mu, logvar = encode(self.model.encoder, x)
        if expect_fused_encoder:                               # the node is the one that ran
            assert "GokuEncoderFn" in type(mu[0].grad_fn.next_functions[0][0]).__name__
        dev_eps = lambda e: torch.from_numpy(e).to(self.dev).t()
        eps = tuple(dev_eps(e) for e in self.eps) if self.goku else dev_eps(self.eps)
        l_tilde, bkl = sample_with_kl(mu, logvar, self._beta(word), self.B, eps=eps)
        if fused:
            loss, (x_hat, z_hat, _) = decode_loss(self.model.decoder, l_tilde, TS, x, self.B, plus=bkl, want_x_hat=False)
        else:
            x_hat, z_hat, _ = decode(self.model.decoder, l_tilde, TS)
            loss = reconstruction_loss(x, x_hat, self.B, plus=bkl)
        return self._end(loss, xb, z_hat)

    def run_loss_batch(self, offset, word):
        """(c): train.loss_batch(variational=False): l̃ = μ, no ε."""
        from latentdiffeq_amd import train as TR
        xb, x = self._begin(offset)
        return self._end(TR.loss_batch(self.model, x, TS, self._beta(word), False), xb)

    def check_kernels(self):
        if self.case in KERNELS:
            h = self.diffeq._native()
            fwd, adj = h.lib.lde_last_kernel(h.ptr, 0), h.lib.lde_last_kernel(h.ptr, 1)
            assert fwd == KERNELS[self.case][0] and adj.startswith(KERNELS[self.case][1]), (fwd, adj)


def distances(names, got, ref):
    """How far a result sits from a reference: the loss (relative), ẑ (max abs), per module the gradient's relative L2, the frames' gradient."""
    d = dict(loss=abs(float(got["loss"]) - ref["loss"]) / abs(ref["loss"]),
             grads={n: S.rel_l2(a, b) for n, a, b in zip(names, got["grads"], ref["grads"])}, dx=S.rel_l2(got["dx"], ref["dx"]))
    if got.get("z") is not None:
        d["z"] = float(np.abs(got["z"].astype(np.float64) - ref["z"]).max())
    return d


def product_runs(st):
    """name → (result, which reference: "eps" or "mu"). The stochastic pendulum's offsets: 2 for the ε runs, 5 for the l̃ = μ runs."""
    from latentdiffeq_amd import recurrent as R
    runs = {}
    keep = R._BRANCH_STREAMS
    try:
        for mode in (True, False) if st.case in BOTH_STREAM_MODES else (keep,):
            R._BRANCH_STREAMS = mode
            one_node = st.goku and not mode and R._ENCODER_FUSED and not R._RNN_GROUP
            runs[f"eps_streams_{mode}"] = (st.run_eps(2, expect_fused_encoder=one_node), "eps")
    finally:
        R._BRANCH_STREAMS = keep
    st.check_kernels()
    runs["fused_number"] = (st.run_eps(2, fused=True), "eps")
    runs["fused_word"] = (st.run_eps(2, fused=True, word=True), "eps")
    runs["loss_batch_number"] = (st.run_loss_batch(5, False), "mu")
    runs["loss_batch_word"] = (st.run_loss_batch(5, True), "mu")
    st.check_kernels()
    return runs


def same_bits(a, b):
    import torch
    if torch.is_tensor(a):
        return torch.equal(a, b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case,B", CASES, ids=[f"{c}-B{b}" if b != 20 else c for c, b in CASES])
def test_f32_step_equals_the_composed_reference(o32, o64, case, B):
    st = Step(case, B)
    runs = product_runs(st)
    cont = case in CONTINUOUS
    refs = {"eps": st.reference(o64, st.eps, 2, tol=1e-10 if cont else None), "mu": st.reference(o64, None, 5, tol=1e-10 if cont else None)}
    near = {"eps": st.reference(o32, st.eps, 2), "mu": st.reference(o32, None, 5)} if cont else None
    for name, (got, which) in runs.items():
        ref = refs[which]
        d = distances(st.names, got, ref)
        print(case, B, name, "loss", f"{d['loss']:.2e}", "z", f"{d.get('z', float('nan')):.2e}", "dx", f"{d['dx']:.2e}",
              "grads", {n: f"{r:.1e}" for n, r in d["grads"].items()})
        assert d["loss"] <= LOSS_TOL, (name, "loss", d["loss"])
        if "z" in d:
            assert got["z"].shape == ref["z"].shape and d["z"] <= Z_TOL.get(case, Z_TOL_DEFAULT), (name, "z", d["z"])
        pairs = list(zip(st.names, got["grads"], ref["grads"])) + [("frames", got["dx"], ref["dx"])]
        for i, (n, g, t) in enumerate(pairs):
            assert g.shape == t.shape and np.isfinite(g).all(), (name, n)
            if cont:           # tests/test_gpu_mlp.py::_check_grads
                r = (near[which]["grads"] + [near[which]["dx"]])[i]
                s = np.abs(t).max()
                assert np.abs(g - r).max() <= LIM_O * s, (name, n, np.abs(g - r).max() / s)
                assert np.abs(g - t).max() <= 1.5 * np.abs(r - t).max() + LIM_T * s, (name, n, np.abs(g - t).max() / s, np.abs(r - t).max() / s)
            else:
                assert S.rel_l2(g, t) <= GRAD_TOL, (name, n, S.rel_l2(g, t))
    # β as a number and β as a device word: the same bits
    for a, b in (("fused_number", "fused_word"), ("loss_batch_number", "loss_batch_word")):
        ra, rb = runs[a][0], runs[b][0]
        assert same_bits(ra["loss"], rb["loss"]), (a, b, "loss", float(ra["loss"]), float(rb["loss"]))
        for n, ga, gb in zip(st.names + ["frames"], ra["grads"] + [ra["dx"]], rb["grads"] + [rb["dx"]]):
            assert same_bits(ga, gb), (a, b, n)
