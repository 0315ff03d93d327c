"""One whole training step of a LatentDiffEqModel restated as the COMPOSITION of the CPU references, module by module — what
tests/test_gpu_composed_step.py and tests/test_gpu_step_models.py judge the product by, itself pinned without a GPU by
tests/test_step_ref.py (its gradients against central differences of its own loss):

    GOKU       x ─ feature extractor (chain) ─ three recurrent stacks ─ vcat ─ four latent_in heads ─ sample + β·KL
                 ─ latent_out (chain ×2) ─ solve(ẑ₀, θ̂) ─ reconstructor (chain) ─ reconstruction loss
    LatentODE  x ─ feature extractor (chain) ─ one recurrent stack ─ two latent_in heads ─ sample + β·KL
                 ─ identity ─ solve(ẑ₀; W) on D′ = D + augment_dim rows ─ reconstructor (chain, D′ inputs) ─ reconstruction loss

    [REF src/models/LatentDiffEqModel.jl:63-75, :101-113], [REF src/models/GOKU.jl:19-72, :83-91, :98-130, :148, :155-163],
    [REF src/models/LatentODE.jl:24-43, :53, :61-80], [REF examples/pendulum_friction-less/model_train.jl:225-238]

Building blocks: oracle.chain_*, rnn_*, sample_*, kl_*, mse_*, forward / adjoint (oracle/oracle.py: the C oracle, f64 or f32); tests/gru_ref.py
for GRU stacks (the C oracle has none); tests/lv_ref.py for Lotka–Volterra; tests/sde_ref.py for the stochastic pendulum at the
(seed, offset) the forward drew with. Every array is batch-major memory of the reference's column-major one: frames (T, B, pixels), stack
outputs (B, h), ẑ (T, B, D′). Everything is carried out in the oracle's precision: `Oracle("f64")` is the reference, `Oracle("f32")` the same
code restated in float32 — how far a CORRECT f32 step may sit from the reference (the tolerances of tests/test_gpu_step_models.py).

The frames' gradient is the encoder path's: the loss kernels take their target as data, (x − x̂)² sends no cotangent to x.

`fault=`: a deliberately wrong composition (tests/test_step_ref.py shows each moves the result by more than the GPU tolerance):
    "swap_heads"          μ and log σ² taken from each other's head
    "drop_second_source"  a stack output's gradient from the μ head only (the log σ² head's input gradient dropped)
    "rec_width_D"         the reconstructor reads ẑ rows with leading dimension D instead of D′ (LatentODE with augment_dim > 0)
    "theta_perm"          θ̂'s columns rotated by one (a parameter head wider than one)
"""
import numpy as np

from oracle import oracle as O
from tests import gru_ref, lv_ref, sde_ref

CELL_GRU = 3
FAULTS = ("swap_heads", "drop_second_source", "rec_width_D", "theta_perm")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _chain_spec(ch):
    return dict(kind="chain", sizes=list(ch.sizes), acts=list(ch.acts), skips=list(ch.skips))


def _rnn_spec(rec):
    return dict(kind="rnn", code=int(rec.code), sizes=list(rec.sizes), reverse=bool(rec.reverse))    # (lde_cell_kind: the same codes on both sides)


def _solve_spec(diffeq):
    """What the solve needs to know of a `diffeq` plug-in struct (api.py), read from its public fields."""
    name = type(diffeq).__name__
    kw = dict(diffeq.kwargs)
    sense = type(diffeq.sensealg).__name__
    s = dict(rhs={"Pendulum": "pendulum", "Pendulum_friction": "friction", "LotkaVolterra": "lv", "SPendulum": "sde", "NODE": "node"}[name],
             abstol=float(kw.get("abstol", 1e-6)), reltol=float(kw.get("reltol", 1e-3)), adaptive=bool(kw.get("adaptive", True)),
             dt=float(kw.get("dt", 0.0)), solver=type(diffeq.solver).__name__,
             discrete=sense in ("DiscreteSensitivity", "ForwardDiffSensitivity"), P=0)
    if s["rhs"] == "node":
        s.update(D=diffeq.latent_dim_in, augment=diffeq.augment_dim, layers=list(diffeq.layer_sizes), activation=kw.get("activation", "relu"),
                 batching={0: O.BATCH_PER_TRAJECTORY, 1: O.BATCH_COUPLED}[int(diffeq.batching)])
    else:
        s.update(D=2, augment=0, P=len(diffeq.prob.p))
    if s["rhs"] == "sde":
        s.update(seed=int(diffeq.seed), offset=int(diffeq.offset))
    return s


def spec_of(model):
    """(spec, names, weights): the model's structure, and per module of `model.modules()` its name and flat weights (float64 numpy,
    Flux.destructure order). Reads shapes and weights only — a model on the CPU serves."""
    e, d = model.encoder, model.decoder
    goku = isinstance(e.pattern_extractor, (tuple, list))
    pes = list(e.pattern_extractor) if goku else [e.pattern_extractor]
    los = list(d.latent_out) if isinstance(d.latent_out, (tuple, list)) else []
    spec = dict(goku=goku, fe=_chain_spec(e.feature_extractor), pe=[_rnn_spec(m) for m in pes], li=[_chain_spec(m) for m in e.latent_in],
                lo=[_chain_spec(m) for m in los], solve=_solve_spec(d.diffeq), rec=_chain_spec(d.reconstructor))
    if goku:
        names = ["feature_extractor", "pe_z0", "pe_th_fwd", "pe_th_bwd", "li_mu_z0", "li_ls_z0", "li_mu_th", "li_ls_th", "lo_z0", "lo_th"]
    else:
        names = ["feature_extractor", "pe", "li_mu", "li_ls"]
    mods = [e.feature_extractor, *pes, *e.latent_in, *los]
    if spec["solve"]["rhs"] == "node":
        names.append("node")
        mods.append(d.diffeq)
    names.append("reconstructor")
    mods.append(d.reconstructor)
    assert len(mods) == len(model.modules())
    return spec, names, [_np(m.flat_weights()) for m in mods]


def flat_grads(model):
    """The flat weight gradient of every module in `model.modules()` order, in flat_weights() order (float64 numpy). The NODE's `dudt` is a
    torch Sequential: per Linear vec(∂W) column-major [out × in], then ∂b (NODE.flat_weights)."""
    out = []
    for m in model.modules():
        if hasattr(m, "flat_weights"):
            out.append(_np(m.flat_weights().grad))
        else:
            out.append(np.concatenate([_np(q) for lin in m if hasattr(lin, "weight") for q in (lin.weight.grad.t().reshape(-1), lin.bias.grad)]))
    return out


# ---- the pieces, in the oracle's precision ----------------------------------------------------------------------------------------------
class _Ops:
    def __init__(self, orc):
        self.o, self.dt = orc, orc.dtype

    def fwd(self, s, W, x):
        if s["kind"] == "chain":
            return self.o.chain_forward(O.make_chain_desc(s["sizes"], s["acts"], s["skips"]), W, x)
        if s["code"] == CELL_GRU:
            return gru_ref.forward(s["sizes"], W, x, s["reverse"], self.dt)
        return self.o.rnn_forward(O.make_rnn_desc(s["code"], s["sizes"], reverse=s["reverse"]), W, x)

    def bwd(self, s, W, x, dy, need_dx=True):
        """(dx, dW)."""
        if s["kind"] == "chain":
            return self.o.chain_backward(O.make_chain_desc(s["sizes"], s["acts"], s["skips"]), W, x, dy, need_dx=need_dx)
        if s["code"] == CELL_GRU:
            return gru_ref.backward(s["sizes"], W, x, dy, s["reverse"], self.dt)
        return self.o.rnn_backward(O.make_rnn_desc(s["code"], s["sizes"], reverse=s["reverse"]), W, x, dy)


def _solve(s, z0, th, ts, orc, W=None, tol=None):
    """ẑ (T, B, D′) and its pullback dz ↦ (dẑ₀ (B, D), dθ̂ (B, P) or None, dW or None). `tol`: abstol = reltol override (the float64
    truth of a continuous adjoint). A `discrete` sensealg differentiates the solve on the steps it accepted; the others integrate the
    continuous adjoint backwards."""
    dt = orc.dtype
    abstol, reltol = (tol, tol) if tol is not None else (s["abstol"], s["reltol"])
    if s["rhs"] == "lv":
        z, J, ret, _ = lv_ref.solve(z0, th, ts, solver={"Tsit5": lv_ref.TSIT5, "RK4": lv_ref.RK4}[s["solver"]], adaptive=s["adaptive"], dt=s["dt"],
                                    dtype=dt, abstol=abstol, reltol=reltol)
        assert (ret == 0).all()
        return z, lambda dz: (*(g.astype(dt) for g in lv_ref.pullback(J, dz)), None)
    if s["rhs"] == "sde":
        z, J, ret = sde_ref.solve(z0, th, ts, s["dt"], solver={"EM": sde_ref.EM, "EulerHeun": sde_ref.EULER_HEUN}[s["solver"]], seed=s["seed"],
                                  offset=s["offset"], dtype=dt)
        assert (ret == 0).all()
        return z, lambda dz: (*(g.astype(dt) for g in sde_ref.pullback(J, dz)), None)
    kind = {"pendulum": O.RHS_PENDULUM, "friction": O.RHS_PENDULUM_FRICTION, "node": O.RHS_MLP}[s["rhs"]]
    node = s["rhs"] == "node"
    d = O.make_desc(rhs_kind=kind, state_dim=s["D"], param_dim=s["P"], augment_dim=s["augment"], layers=s["layers"] if node else (),
                    activation={"relu": O.ACT_RELU, "tanh": O.ACT_TANH}[s["activation"]] if node else O.ACT_RELU,
                    solver={"Tsit5": O.SOLVER_TSIT5, "RK4": O.SOLVER_RK4}[s["solver"]],
                    batching=s["batching"] if node else O.BATCH_PER_TRAJECTORY, adaptive=s["adaptive"], dt=s["dt"], abstol=abstol, reltol=reltol)
    if s["discrete"]:
        z, ret, rec, _ = orc.forward_steps(d, z0, th, ts, W=W)
        assert (ret == 0).all()
        return z, lambda dz: orc.adjoint_discrete(d, z, th, ts, dz, rec, W=W)[:3]
    z, ret, _ = orc.forward(d, z0, th, ts, W=W)
    assert (ret == 0).all()
    return z, lambda dz: orc.adjoint(d, z, th, ts, dz, W=W)[:3]


def evaluate(spec, weights, x_tbp, eps, beta, ts, orc, want_dx=False, fault=None, tol=None, discrete=None):
    """One step. x_tbp (T, B, pixels); eps: None (l̃ = μ, the non-variational step) or the ε arrays — (ε_z₀ (B, ·), ε_θ (B, ·)) for GOKU, one
    (B, ·) array for LatentODE; beta: the KL weight; ts: the save times; orc: Oracle("f64") or Oracle("f32"). `discrete`: overrides the
    plug-in's kind of sensitivity (True: the derivative of the discrete solve; False: the continuous adjoint).
    Returns dict(loss, z (T, B, D′), grads [flat ∂W per module, model.modules() order], dx (T, B, pixels) or None)."""
    assert fault is None or fault in FAULTS
    ops, dt = _Ops(orc), orc.dtype
    W = [np.asarray(w, dt) for w in weights]
    s = dict(spec["solve"])
    if discrete is not None:
        s["discrete"] = bool(discrete)
    goku = spec["goku"]
    T, B, NI = x_tbp.shape
    X = np.asarray(x_tbp, dt).reshape(T * B, NI)
    ts = np.asarray(ts, np.float64)
    npe, nli, nlo = len(spec["pe"]), len(spec["li"]), len(spec["lo"])
    i_pe, i_li, i_lo = 1, 1 + npe, 1 + npe + nli
    i_node = i_lo + nlo if s["rhs"] == "node" else None
    i_rec = len(W) - 1
    # ---- forward ------------------------------------------------------------------------------------------------------------------------
    fe3 = ops.fwd(spec["fe"], W[0], X).reshape(T, B, -1)
    ys = [ops.fwd(p, W[i_pe + i], fe3) for i, p in enumerate(spec["pe"])]
    # the inputs of the heads: GOKU (ẑ₀ stack; vcat(pe_forward, pe_backward) [REF GOKU.jl:47]), heads (μ_z₀, logσ²_z₀, μ_θ, logσ²_θ)
    parts = [ys[0], np.concatenate([ys[1], ys[2]], axis=1)] if goku else [ys[0]]
    hm, hl = (1, 0) if fault == "swap_heads" else (0, 1)        # which head of a part gives μ, which log σ²
    eps = (None,) * len(parts) if eps is None else (tuple(eps) if goku else (eps,))
    mus, lss, ls_, kl = [], [], [], 0.0
    for p, y in enumerate(parts):
        mu = ops.fwd(spec["li"][2 * p + hm], W[i_li + 2 * p + hm], y)
        lv = ops.fwd(spec["li"][2 * p + hl], W[i_li + 2 * p + hl], y)
        ls_.append(mu if eps[p] is None else orc.sample_forward(mu, lv, eps[p]))
        kl += orc.kl_forward(mu, lv, beta / B)
        mus.append(mu)
        lss.append(lv)
    if goku:
        z0h = ops.fwd(spec["lo"][0], W[i_lo], ls_[0])                 # (B, 2)
        thh = ops.fwd(spec["lo"][1], W[i_lo + 1], ls_[1])             # (B, P)
        if fault == "theta_perm":
            thh = np.roll(thh, 1, axis=1)
    else:
        z0h, thh = ls_[0], None                                       # latent_out is the identity [REF LatentODE.jl:142]
    z, pull = _solve(s, z0h, thh, ts, orc, W=None if i_node is None else W[i_node], tol=tol)
    z = np.asarray(z, dt)
    Dp = z.shape[2]
    if fault == "rec_width_D":
        zf, D = np.concatenate([z.reshape(-1), np.zeros(Dp, dt)]), s["D"]
        zin = np.stack([zf[r * D:r * D + Dp] for r in range(T * B)])
    else:
        zin = z.reshape(T * B, Dp)
    xh = ops.fwd(spec["rec"], W[i_rec], zin)
    scale = 1.0 / (B * T)
    loss = orc.mse_forward(X, xh, scale) + kl
    # ---- pullback -----------------------------------------------------------------------------------------------------------------------
    g = [None] * len(W)
    dxh = orc.mse_backward(X, xh, scale)
    dzin, g[i_rec] = ops.bwd(spec["rec"], W[i_rec], zin, dxh)
    if fault == "rec_width_D":
        dzf = np.zeros(T * B * Dp + Dp, dt)
        for r in range(T * B):
            dzf[r * D:r * D + Dp] += dzin[r]
        dz = dzf[:T * B * Dp].reshape(T, B, Dp)
    else:
        dz = dzin.reshape(T, B, Dp)
    dz0h, dthh, dWn = pull(dz)
    if i_node is not None:
        g[i_node] = np.asarray(dWn, dt)
    if goku:
        if fault == "theta_perm":
            dthh = np.roll(dthh, -1, axis=1)
        dl0, g[i_lo] = ops.bwd(spec["lo"][0], W[i_lo], ls_[0], dz0h)
        dl1, g[i_lo + 1] = ops.bwd(spec["lo"][1], W[i_lo + 1], ls_[1], dthh)
        dls = [dl0, dl1]
    else:
        dls = [np.asarray(dz0h, dt)]
    dys = []
    for p, y in enumerate(parts):
        dmu, dlv = orc.kl_backward(mus[p], lss[p], beta / B)
        if eps[p] is None:
            dmu = dmu + dls[p]
        else:
            a, b = orc.sample_backward(lss[p], eps[p], dls[p])
            dmu, dlv = dmu + a, dlv + b
        dy_mu, g[i_li + 2 * p + hm] = ops.bwd(spec["li"][2 * p + hm], W[i_li + 2 * p + hm], y, dmu)
        dy_lv, g[i_li + 2 * p + hl] = ops.bwd(spec["li"][2 * p + hl], W[i_li + 2 * p + hl], y, dlv)
        dys.append(dy_mu if fault == "drop_second_source" else dy_mu + dy_lv)      # a stack output feeds two heads: two gradient sources
    if goku:
        h = ys[1].shape[1]
        dys = [dys[0], np.ascontiguousarray(dys[1][:, :h]), np.ascontiguousarray(dys[1][:, h:])]
    dfe = None
    for i, p in enumerate(spec["pe"]):
        dxi, g[i_pe + i] = ops.bwd(p, W[i_pe + i], fe3, dys[i])
        dfe = dxi if dfe is None else dfe + dxi                                     # the features feed every stack
    dX, g[0] = ops.bwd(spec["fe"], W[0], X, dfe.reshape(T * B, -1), need_dx=want_dx)
    return dict(loss=float(loss), z=z, grads=[np.asarray(a, np.float64) for a in g], dx=None if dX is None else np.asarray(dX, np.float64).reshape(T, B, NI))


def rel_l2(a, b):
    """‖a − b‖ / ‖b‖."""
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))
