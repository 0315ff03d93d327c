"""Host-side training harness (scope row f-3): what the reference's example script wraps around the model. Pure host code —
the compute under `model(x, t)` and the loss terms is liblde.so (api.py, chain.py, recurrent.py, loss.py); this file launches
no kernel of its own.

    reference                                                                         here
    --------------------------------------------------------------------------------  -----------------------------
    LatentDiffEqModel(model_type, encoder_layers, decoder_layers); model(x, t, variational)
                                                      [REF src/models/LatentDiffEqModel.jl:6-37]      LatentDiffEqModel
    default_layers(model_type, input_dim, diffeq)     [REF src/models/GOKU.jl:201-273]               default_layers
    loss_batch(model, x, t, β, variational)           [REF examples/pendulum_friction-less/model_train.jl:225-238]   loss_batch
    kl, vector_kl                                     [REF src/utils/utils.jl:15-49]                  kl (elementwise), loss.vector_kl
    frange_cycle_linear(n_iter, start, stop, n_cycle, ratio)   [REF src/utils/utils.jl:53-66]         frange_cycle_linear
    normalize_to_unit_segment / denormalize_unit_segment       [REF src/utils/utils.jl:71-79]         same
    time_loader(x, full_seq_len, seq_len), rand_time  [REF src/utils/utils.jl:85-99]                  time_loader, rand_time
    the epoch loop: β schedule, progressive sequence length, ADAMW, per-minibatch validation loss, best weights
                                                      [REF model_train.jl:138-150, :172-218]          train
"""
from __future__ import annotations

import contextlib
import copy
import math
import os
from typing import Callable, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .api import Decoder
from .chain import decode, decode_loss, default_decoder_layers
from .loss import beta_kl, beta_word, reconstruction_loss, sample, sample_with_kl, vector_kl  # noqa: F401
from .loss import backward as _loss_backward
from .recurrent import Encoder, default_encoder_layers, encode


_FUSED_LOSS = True    # module-level switches (diagnostic: set the attribute before the call; nothing here reads the environment)
_NATIVE_ADAM = True   # FluxADAMW: the one-launch lde_adamw_flux_step   # loss_batch: sample + KL in one pass (diagnostic switch)


class LatentDiffEqModel:
    """LatentDiffEqModel(model_type, encoder_layers, decoder_layers); `model(x, t, variational)` → ((x̂, ẑ, l̂), μ, logσ²)."""

    def __init__(self, model_type, encoder_layers, decoder_layers):
        self.model_type = model_type
        self.encoder = Encoder(model_type, encoder_layers)
        self.decoder = Decoder(model_type, decoder_layers)

    def modules(self) -> List[torch.nn.Module]:
        e, d = self.encoder, self.decoder
        pe = list(e.pattern_extractor) if isinstance(e.pattern_extractor, tuple) else [e.pattern_extractor]
        lo = list(d.latent_out) if isinstance(d.latent_out, tuple) else []
        extra = [d.diffeq.dudt] if hasattr(d.diffeq, "dudt") else []   # the NODE's weights: trained here
        return [e.feature_extractor, *pe, *e.latent_in, *lo, *extra, d.reconstructor]

    def parameters(self) -> List[torch.nn.Parameter]:
        return [p for m in self.modules() for p in m.parameters()]

    def refresh_weights(self) -> int:
        """After an optimiser step: hand the new weights of every chain and recurrent stack to the library in ONE launch
        (lde_refresh_weights) instead of one per module at its next call. Optional — a module whose parameter changed without
        it re-uploads by itself."""
        from . import _lib as L
        return L.refresh_weights(self.modules())

    def __call__(self, x, t, variational: bool = False):
        mu, logvar = encode(self.encoder, x)
        l_tilde = sample(mu, logvar) if variational else mu                      # [REF LatentDiffEqModel.jl:31]
        return decode(self.decoder, l_tilde, t), mu, logvar


def default_layers(model_type, input_dim: int, diffeq, device=None, **kw):
    """(encoder_layers, decoder_layers)  [REF src/models/GOKU.jl:201-273], [REF src/models/LatentODE.jl:91-145]."""
    ekw = {k: v for k, v in kw.items() if k in ("hidden_dim_resnet", "rnn_input_dim", "rnn_output_dim", "latent_dim_z0", "latent_dim_theta")}
    dkw = {k: v for k, v in kw.items() if k in ("hidden_dim_resnet", "latent_dim_z0", "latent_dim_theta", "latent_to_diffeq_dim",
                                                "z0_activation", "theta_activation", "output_activation")}
    return (default_encoder_layers(model_type, input_dim, diffeq, device=device, **ekw),
            default_decoder_layers(model_type, input_dim, diffeq, device=device, **dkw))


def kl(mu, logvar):
    """kl(μ, logσ²) = (exp(logσ²) + μ² − logσ² − 1) / 2, elementwise  [REF src/utils/utils.jl:15]."""
    return (torch.exp(logvar) + mu ** 2 - logvar - 1) / 2


def loss_batch(model, x, t, beta: float, variational: bool, batch_size: Optional[int] = None):
    """reconstruction_loss + β·kl_loss with reconstruction_loss = sum(mean((x − x̂)², dims=(2,3)))  [REF model_train.jl:225-238].
    `batch_size`: the GLOBAL minibatch size when x is one rank's shard (the per-rank losses then add up to the reference's).
    `beta`: a number, or a β word — one float32 on the GPU that the loss kernels read at run time (loss.py), so that a captured step
    follows the β schedule; the non-variational loss is then reconstruction_loss(x, x̂, plus=beta_kl(μ, logσ², β))."""
    if variational and _FUSED_LOSS:
        # the same expression with the sample and the KL term read in one pass and the scalar additions folded into the
        # reductions (loss.sample_with_kl): encoder → (l̃, β·kl) → decoder → reconstruction_loss + β·kl
        mu, logvar = encode(model.encoder, x)
        l_tilde, bkl = sample_with_kl(mu, logvar, beta, batch_size)
        loss, _ = decode_loss(model.decoder, l_tilde, t, x, batch_size, plus=bkl, want_x_hat=False)   # (the reconstructor and the loss as one autograd node; x̂ is not kept)
        return loss
    (x_hat, _z, _l), mu, logvar = model(x, t, variational)
    if beta_word(beta)[0] is not None:
        return reconstruction_loss(x, x_hat, batch_size, plus=beta_kl(mu, logvar, beta, batch_size))
    return reconstruction_loss(x, x_hat, batch_size) + beta * vector_kl(mu, logvar, batch_size)


def frange_cycle_linear(n_iter: int, start: float = 0.0, stop: float = 1.0, n_cycle: int = 4, ratio: float = 0.5) -> np.ndarray:
    """Cyclical KL-annealing schedule, the reference's loop transcribed index for index (1-based `L[Int(round(i + c·period))]`
    with the strict `< n_iter` guard — so the last entry is never rewritten; Julia's `round` is round-half-even like Python's)
    [REF src/utils/utils.jl:53-66]."""
    L = np.ones(n_iter, dtype=np.float64) * stop
    period = n_iter / n_cycle
    step = np.float32((stop - start) / (period * ratio))
    for c in range(n_cycle):
        v, i = np.float32(start), 1
        while v <= stop and int(round(i + c * period)) < n_iter:
            L[int(round(i + c * period)) - 1] = v
            v = np.float32(v + step)
            i += 1
    return L.astype(np.float32)


def normalize_to_unit_segment(X):
    """[REF src/utils/utils.jl:71-77]."""
    lo, hi = X.min(), X.max()
    return (X - lo) / (hi - lo), lo, hi


def denormalize_unit_segment(Xh, lo, hi):
    """[REF src/utils/utils.jl:79]."""
    return Xh * (hi - lo) + lo


def rand_time(full_seq_len: int, seq_len: int, rng: Optional[np.random.Generator] = None):
    """start_time = rand(1:full_seq_len − seq_len); idxs = start:start+seq_len−1 (1-based, inclusive)  [REF utils.jl:95-99].
    Returned 0-based as a slice. (As in the reference the last possible window is never drawn.)"""
    rng = rng or np.random.default_rng()
    start = int(rng.integers(1, full_seq_len - seq_len + 1))      # 1 … full − seq, inclusive
    return slice(start - 1, start - 1 + seq_len)


def time_loader(x, full_seq_len: int, seq_len: int, rng: Optional[np.random.Generator] = None):
    """One random window of seq_len frames, the same for every sample of the minibatch: x [pixels, B, full] → [pixels, B, seq]
    [REF src/utils/utils.jl:85-93]."""
    return x[:, :, rand_time(full_seq_len, seq_len, rng)]


class _FluxNativeStep:
    """What FluxADAMW and FluxAdaBelief share: the one-launch native step in its four forms (host-counted, device-counted, guarded, clipped),
    the device words that go with them, and the surface around them — `grad_norms()`, `guard_state()`, `withheld()`, the `state_dict` round
    trip of the device step count. A mixin in front of a torch optimiser class; the rule's class says which entry points (`_ABI`), which
    state key holds the second state array (`_SECOND`), what goes between β₂ and the decay in the call (`_eps_args`) and its name in
    messages (`_NAME`)."""
    _NAME = "FluxADAMW"
    _ABI = "lde_adamw_flux_step"
    _SECOND = "exp_avg_sq"

    def _eps_args(self, group):
        return (group["eps"],)

    @classmethod
    def _check_options(cls, capturable, guard, clip_norm, clip_mode):
        if guard and not capturable:
            raise ValueError(f"{cls._NAME}(guard=True) needs capturable=True (the guard is part of the device-counted step)")
        if clip_mode not in L.CLIP_MODES:
            raise ValueError(f"{cls._NAME}(clip_mode={clip_mode!r}): one of {sorted(L.CLIP_MODES)}")
        if clip_norm is not None and not (math.isfinite(float(clip_norm)) and float(clip_norm) > 0.0):
            raise ValueError(f"{cls._NAME}(clip_norm=...) takes a finite threshold > 0 (None: no clipping)")

    def _setup_native(self, params, on_gpu, decay, native, capturable, guard, clip_norm, clip_mode):
        """Everything behind the base constructor: which path, and the device words of the capturable, guarded and clipped forms."""
        self.decay = float(decay)
        ok = on_gpu and all(p.dtype == torch.float32 and p.is_contiguous() for p in params)
        if native is None:
            native = ok and _NATIVE_ADAM
        if native and not ok:
            raise ValueError(f"{self._NAME}(native=True) needs contiguous float32 HIP parameters")
        self.native = bool(native)
        # capturable (native only): the step count lives in ONE device int64 shared by all arrays (lde_adamw_flux_step_dev), so that the
        # update can sit inside a captured hipGraph (train.GraphedStep); every array must then have a gradient at every step
        self.capturable = bool(capturable)
        if self.capturable and not self.native:
            raise ValueError(f"{self._NAME}(capturable=True) needs the native path")
        self._step_dev = torch.zeros((), dtype=torch.int64, device=params[0].device) if self.capturable else None
        if self.capturable:
            if len(self.param_groups) != 1:     # one device counter, bumped by every lde_adamw_flux_step_dev launch: one launch per step
                raise ValueError(f"{self._NAME}(capturable=True) takes ONE parameter group")
            self.set_noise_epoch()              # a captured step's ε is keyed by this counter: fresh noise at every replay (loss.randn)
        # guard: LDE_GUARD_WORDS device words (in flight, skipped, streak, last_bad_array), initialised once; the kernels keep them
        self.guard = bool(guard)
        self._guard_dev = None
        if self.guard:
            self._guard_dev = torch.empty(L.GUARD_WORDS, dtype=torch.int64, device=params[0].device)
            L.call("lde_guard_init", None, L.ptr(self._guard_dev), L.raw_stream(params[0].device.index))
        # clip: the workspace of the clipped step and its n + 1 norms, allocated ONCE — a captured step replays these addresses
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.clip_mode = clip_mode
        self._clip_ws = self._norms_dev = self._norms_host = None
        if self.clip_norm is not None and self.native:
            if not (self.capturable and self.guard):
                raise ValueError(f"{self._NAME}(clip_norm=...) on the native path needs capturable=True, guard=True "
                                 "(the clipped step is the guarded, device-counted step with a scale in front of it)")
            tab = (L.AdamTensor * len(params))()
            for i, p in enumerate(params):
                tab[i].n = p.numel()
            nbytes = int(L.load().lde_clip_ws_bytes(len(params), tab))
            self._clip_ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=params[0].device)
            self._norms_dev = torch.zeros(len(params) + 1, dtype=torch.float32, device=params[0].device)

    def set_noise_epoch(self):
        """Make this optimiser's device step count the noise epoch of a captured step's ε (loss.set_noise_epoch): the capturable form does
        it at construction; call it again after another optimiser took the role."""
        if not getattr(self, "capturable", False):
            raise ValueError(f"{self._NAME}.set_noise_epoch() needs capturable=True")
        from .loss import set_noise_epoch
        set_noise_epoch(self._step_dev)

    def grad_norms(self):
        """(per-array list, total) — the gradient norms of the most recent `step()`, before clipping, in the parameter group's order: what
        the clipped step measured (include/lde.h: "the clipped step"; an empty array reads 0, the total is the norm of all gradients
        together in either mode). ONE device→host copy: a synchronisation with the device; not for every step of a captured run."""
        if self.clip_norm is None:
            raise ValueError(f"{self._NAME}.grad_norms() needs clip_norm=")
        if self._norms_dev is not None:
            w = self._norms_dev.tolist()
        elif self._norms_host is not None:
            w = self._norms_host
        else:
            w = [0.0] * (sum(len(g["params"]) for g in self.param_groups) + 1)
        return [float(x) for x in w[:-1]], float(w[-1])

    @torch.no_grad()
    def _clip_with_torch(self):
        """Off the native path: the two rules of the clipped step with torch ops, on `p.grad` in place — norms in f64, rounded to f32, the
        scale formed in f32 (tests/clip_ref.py states the same). Arrays without a gradient count as empty."""
        ps = [p for g in self.param_groups for p in g["params"]]
        sq = [p.grad.detach().double().pow(2).sum() if p.grad is not None else torch.zeros((), dtype=torch.float64, device=p.device) for p in ps]
        per = [s.sqrt().float() for s in sq]
        total = torch.stack([s.cpu() for s in sq]).sum().sqrt().float() if sq else torch.zeros(())
        c = torch.tensor(self.clip_norm, dtype=torch.float32)
        one = torch.ones((), dtype=torch.float32)
        for p, ni in zip(ps, per):
            if p.grad is None:
                continue
            if self.clip_mode == "global":
                s = torch.minimum(one, c / (total + torch.tensor(1e-6, dtype=torch.float32)))
            else:
                s = c / ni.cpu() if float(ni) > float(c) else one
            if float(s) != 1.0:
                p.grad.mul_(s.to(p.grad.device, p.grad.dtype))
        self._norms_host = [float(x) for x in per] + [float(total)]

    def guard_state(self) -> dict:
        """dict(skipped, streak, last_bad_array) of the guarded step (include/lde.h: "the guarded step"): updates withheld so far,
        consecutive ones up to now, and the index — in the parameter group's order — of the lowest array with a non-finite gradient at the
        most recent withheld update (−1: never). Read-only. ONE device→host copy: a synchronisation with the device; not for every step
        (GraphedStep looks every `check_every` replays). The counters are not part of `state_dict()`."""
        if not self.guard:
            raise ValueError(f"{self._NAME}.guard_state() needs guard=True")
        w = self._guard_dev.tolist()
        return dict(skipped=int(w[1]), streak=int(w[2]), last_bad_array=int(w[3]))

    @contextlib.contextmanager
    def withheld(self):
        """Inside the block ONE `step()` of the guarded form is withheld whatever its gradients hold, and the counters are put back at the
        end: a whole training step can be run for what it does to the workspaces (GraphedStep.recover: the step record regrows) while the
        parameters, the moments, the step count and `guard_state()` stay what they were. Word [0] is raised by hand — the kernels see a
        scan that found something — and is −1 again after the step, as always."""
        if not self.guard:
            raise ValueError(f"{self._NAME}.withheld() needs guard=True")
        keep = self._guard_dev.clone()
        self._guard_dev[0:1].fill_(0)
        try:
            yield
        finally:
            self._guard_dev.copy_(keep)

    def add_param_group(self, param_group):
        if getattr(self, "capturable", False) and self.param_groups:
            raise ValueError(f"{self._NAME}(capturable=True) takes ONE parameter group")
        super().add_param_group(param_group)

    def state_dict(self):
        """The capturable form's step count lives on the device (`_step_dev`), not in `state`: a checkpoint carries it as every array's
        `step` (what the non-capturable and torch forms keep), so that a resumed run's bias corrections continue at t, not at 0."""
        sd = super().state_dict()
        if self.capturable:
            t = int(self._step_dev.item())
            sd["state"] = {k: dict(v, step=t) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self.capturable:
            steps = [int(st["step"]) for st in self.state.values() if "step" in st]
            if steps and min(steps) != max(steps):
                raise ValueError(f"{self._NAME}(capturable=True): the checkpoint's arrays have been updated unequally often")
            self._step_dev.fill_(steps[0] if steps else 0)
            for st in self.state.values():
                st.pop("step", None)

    @torch.no_grad()
    def _native_step(self):
        if self.capturable:
            for g in self.param_groups:
                ps = g["params"]
                if any(p.grad is None for p in ps):
                    raise RuntimeError(f"{self._NAME}(capturable=True): every parameter needs a gradient at every step")
                keep = []
                tab = (L.AdamTensor * len(ps))()
                for i, p in enumerate(ps):
                    st, gr = self.state[p], p.grad
                    if not st:
                        st["exp_avg"], st[self._SECOND] = torch.zeros_like(p), torch.zeros_like(p)
                    if gr.dtype != torch.float32 or not gr.is_contiguous():
                        gr = gr.float().contiguous()
                        keep.append(gr)
                    t = tab[i]
                    t.p, t.g, t.m, t.v, t.n = p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), st[self._SECOND].data_ptr(), p.numel()
                if self.clip_norm is not None:
                    L.call(self._ABI + "_clipped", None, len(ps), tab, g["lr"], g["betas"][0], g["betas"][1], *self._eps_args(g), self.decay,
                           self.clip_norm, L.CLIP_MODES[self.clip_mode], L.ptr(self._step_dev), L.ptr(self._guard_dev),
                           L.ptr(self._clip_ws), L.ptr(self._norms_dev), L.raw_stream(ps[0].device.index))
                elif self.guard:
                    L.call(self._ABI + "_guarded", None, len(ps), tab, g["lr"], g["betas"][0], g["betas"][1], *self._eps_args(g), self.decay,
                           L.ptr(self._step_dev), L.ptr(self._guard_dev), L.raw_stream(ps[0].device.index))
                else:
                    L.call(self._ABI + "_dev", None, len(ps), tab, g["lr"], g["betas"][0], g["betas"][1], *self._eps_args(g), self.decay,
                           L.ptr(self._step_dev), L.raw_stream(ps[0].device.index))
                torch.autograd.graph.increment_version(ps)
            return
        for g in self.param_groups:
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            keep, by_step = [], {}
            for p in ps:
                st = self.state[p]
                if not st:
                    st["step"], st["exp_avg"], st[self._SECOND] = 0, torch.zeros_like(p), torch.zeros_like(p)
                # a state loaded from a torch / fused Adam checkpoint carries `step` as a tensor: normalise to a Python int (the
                # native state is not resumable by torch's fused Adam, which wants tensor steps — documented in the class docstring)
                st["step"] = int(st["step"]) + 1
                by_step.setdefault(st["step"], []).append(p)
            # Flux keeps β₁ᵗ, β₂ᵗ per array: arrays that have been updated equally often share a launch (normally all of them)
            for t_step, group in by_step.items():
                tab = (L.AdamTensor * len(group))()
                for i, p in enumerate(group):
                    st, gr = self.state[p], p.grad
                    if gr.dtype != torch.float32 or not gr.is_contiguous():
                        gr = gr.float().contiguous()
                        keep.append(gr)
                    t = tab[i]
                    t.p, t.g, t.m, t.v, t.n = p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), st[self._SECOND].data_ptr(), p.numel()
                L.call(self._ABI, None, len(group), tab, g["lr"], g["betas"][0], g["betas"][1], *self._eps_args(g), self.decay, t_step,
                       L.raw_stream(group[0].device.index))
                # the kernel wrote through raw pointers: tell torch the parameters changed in place, so that `_lib.weights_key`
                # (data_ptr, _version) — which lets a module skip its weight upload — and autograd's saved-tensor checks see it
                torch.autograd.graph.increment_version(group)


class FluxADAMW(_FluxNativeStep, torch.optim.Adam):
    """`ADAMW(η, (β₁, β₂), decay)` of the pinned Flux 0.13.6 [REF Manifest.toml:452] = `Optimiser(ADAM(η, β), WeightDecay(decay))`
    [REF examples/pendulum_friction-less/model_train.jl:138]: Δ = η·m̂/(√v̂ + ε), then Δ += decay·x, then x −= Δ, i.e.
    x ← (1 − decay)·x − ADAM step — the decay is NOT multiplied by η (torch.optim.AdamW applies lr·weight_decay·x: 1000× weaker at
    the example's η = decay = 1e-3). ε = 1e-8 and the bias correction are Flux's = torch's.
    On the GPU (`native`, the default when every parameter is a contiguous f32 HIP tensor) the whole update is ONE liblde.so launch
    for all parameter arrays (lde_adamw_flux_step) — no per-step tensor grouping, step-counter kernels or separate decay pass;
    otherwise one multi-tensor scale of the parameters followed by torch's Adam update with the gradients taken at the un-decayed
    point (same arithmetic up to rounding; tests/test_gpu_optim.py compares the two). The native path bumps the parameters'
    version counters after its launch (it writes through raw pointers), so `refresh_weights()` is optional after it too. Its
    optimiser state keeps `step` as a Python int (a tensor step from a torch checkpoint is converted on entry); a native
    state_dict is therefore not resumable by torch's FUSED Adam, which expects tensor steps.
    `guard=True` (needs `capturable=True`): the step is lde_adamw_flux_step_guarded — every gradient is scanned on the device first, and
    if any element of any array is NaN or ±Inf the whole update is withheld: no parameter, no moment and not the step count change (the
    count is also the noise epoch of a captured step: the next replay draws the ε the withheld one drew). Otherwise the update is the
    unguarded one bit for bit. `guard_state()` reads the counters. Several GPUs: the gradient all-reduce sits before the optimiser half,
    and a sum with a NaN is NaN on every rank — all ranks withhold the same step; nothing is exchanged for it.
    `clip_norm=c` clips the gradients by norm in front of the update: `clip_mode="global"` is torch's `clip_grad_norm_` — one scale
    min(1, c/(‖g‖ + 1e-6)) from the norm of all gradients together; `"per_array"` is Flux's `Optimiser(ClipNorm(c), ADAMW(...))` — every
    array whose own norm exceeds c is scaled to norm c. On the native path it needs `capturable=True, guard=True`: the step is
    lde_adamw_flux_step_clipped (include/lde.h: "the clipped step") — the guard's scan also forms Σg², one small kernel turns the sums into
    norms and scales, the update scales g as it loads it; no launch per array, nothing read by the host, the gradients in memory stay as
    they were, and a norm that is not finite withholds the step like a NaN. Its workspace and the norms live at fixed addresses from
    construction on, so the step can be captured. Off the native path (CPU tensors, `native=False`) the same two rules are applied with
    torch ops in front of the step, to `p.grad` IN PLACE, as `clip_grad_norm_` does. `grad_norms()` reads the last step's norms."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), decay: float = 0.0, eps: float = 1e-8, fused=None, native=None,
                 capturable: bool = False, guard: bool = False, clip_norm: Optional[float] = None, clip_mode: str = "global"):
        self._check_options(capturable, guard, clip_norm, clip_mode)
        groups = list(params)
        params = [p for g in groups for p in (g["params"] if isinstance(g, dict) else [g])]     # (arrays, or torch's group dicts)
        on_gpu = bool(params) and all(p.is_cuda for p in params)
        if fused is None:
            fused = on_gpu
        self.capturable = False             # (add_param_group runs inside the base constructor)
        super().__init__(groups, lr=lr, betas=betas, eps=eps, weight_decay=0.0, fused=fused or None)
        self._setup_native(params, on_gpu, decay, native, capturable, guard, clip_norm, clip_mode)

    @torch.no_grad()
    def step(self, closure=None):
        if self.native:
            loss = None
            if closure is not None:
                with torch.enable_grad():
                    loss = closure()
            self._native_step()
            return loss
        loss = None
        if closure is not None:             # gradients at the UN-decayed point, as Flux's Optimiser(ADAM, WeightDecay) and the native path
            with torch.enable_grad():
                loss = closure()
        if self.clip_norm is not None:
            self._clip_with_torch()
        if self.decay:
            for g in self.param_groups:
                ps = [p for p in g["params"] if p.grad is not None]
                if ps:
                    torch._foreach_mul_(ps, 1.0 - self.decay)
        super().step()
        return loss


class FluxAdaBelief(_FluxNativeStep, torch.optim.Optimizer):
    """`AdaBelief(η, (β₁, β₂))` — the optimiser the reference's training scripts name as the alternative to ADAMW
    [REF examples/pendulum_friction-less/model_train.jl:136-138] — as `Optimiser(AdaBelief(η, β), WeightDecay(decay))`:
    m ← β₁m + (1−β₁)g; s ← β₂s + (1−β₂)(g − m)² + ε_var (the new m); Δ = η·m̂/(√ŝ + ε_den) + decay·x; x ← x − Δ (include/lde.h: "the
    AdaBelief step"; the decay is not scaled by η, as in FluxADAMW). `eps`: a number ε means ε_var = ε_den = ε² — Flux 0.13.6's placement
    AS RECALLED (its source is not available to this project: UNPINNED); a pair is (ε_var, ε_den) as given — the paper's placement is
    `eps=(1e-8, 1e-8)`, or whatever ε it is run with.
    Everything else is FluxADAMW's, with the same rules and messages under this class's name: `native` (the default when every parameter
    is a contiguous f32 HIP tensor) makes the whole update ONE liblde.so launch (lde_adabelief_flux_step); `capturable=True` keeps the step
    count on the device (…_step_dev) so that the update can sit in a captured step (GraphedStep); `guard=True` scans the gradients first
    and withholds the update when one is not finite (…_step_guarded; `guard_state()`, `withheld()`, and `GraphedStep(guard=opt)` takes
    it); `clip_norm=c` with `clip_mode` clips by norm in front of the update (…_step_clipped; `grad_norms()`). The scans are the ADAMW
    step's own kernels. State keys: `exp_avg`, `exp_avg_var`, `step`. Off the native path (CPU tensors, `native=False`) the rule is applied
    with torch ops — torch.optim has no AdaBelief — in the arithmetic of the parameters' dtype, the constants rounded to f32 the way the C
    ABI receives them; clipping then happens in front, on `p.grad` in place, as in FluxADAMW."""
    _NAME = "FluxAdaBelief"
    _ABI = "lde_adabelief_flux_step"
    _SECOND = "exp_avg_var"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps=1e-8, decay: float = 0.0, native=None, capturable: bool = False,
                 guard: bool = False, clip_norm: Optional[float] = None, clip_mode: str = "global"):
        self._check_options(capturable, guard, clip_norm, clip_mode)
        if not (float(lr) >= 0.0 and math.isfinite(float(lr))):
            raise ValueError(f"FluxAdaBelief(lr={lr!r}): a finite learning rate >= 0")
        if not (len(betas) == 2 and all(0.0 <= float(b) < 1.0 for b in betas)):
            raise ValueError(f"FluxAdaBelief(betas={betas!r}): two numbers in [0, 1)")
        self._split_eps(eps)
        groups = list(params)
        params = [p for g in groups for p in (g["params"] if isinstance(g, dict) else [g])]     # (arrays, or torch's group dicts)
        on_gpu = bool(params) and all(p.is_cuda for p in params)
        self.capturable = False             # (add_param_group runs inside the base constructor)
        super().__init__(groups, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=eps))
        self._setup_native(params, on_gpu, decay, native, capturable, guard, clip_norm, clip_mode)

    @staticmethod
    def _split_eps(eps):
        """(ε_var, ε_den) of `eps`: a number ε → (ε², ε²); a pair as given. Both finite and ≥ 0."""
        try:
            pair = tuple(float(e) for e in eps) if isinstance(eps, (tuple, list)) else (float(eps) ** 2,) * 2
            ok = len(pair) == 2 and all(math.isfinite(e) and e >= 0.0 for e in pair) and (isinstance(eps, (tuple, list)) or float(eps) >= 0.0)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"FluxAdaBelief(eps={eps!r}): a finite number >= 0, or a pair (eps_var, eps_den) of them")
        return pair

    def _eps_args(self, group):
        return self._split_eps(group["eps"])

    @torch.no_grad()
    def _torch_step(self):
        """The rule with torch ops, operation for operation what tests/belief_ref.py states (without the kernel's fused multiply-adds)."""
        f32 = np.float32
        for g in self.param_groups:
            b1, b2 = f32(g["betas"][0]), f32(g["betas"][1])
            omb1, omb2 = float(f32(1.0) - b1), float(f32(1.0) - b2)
            eps_var, eps_den = (float(f32(e)) for e in self._split_eps(g["eps"]))
            lr, decay = float(f32(g["lr"])), float(f32(self.decay))
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"], st["exp_avg"], st["exp_avg_var"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                st["step"] = t = int(st["step"]) + 1
                inv_bc1 = float(f32(1.0 / (1.0 - float(b1) ** t)))
                inv_bc2 = float(f32(1.0 / (1.0 - float(b2) ** t)))
                m, s, gr = st["exp_avg"], st["exp_avg_var"], p.grad.to(p.dtype)
                m.mul_(float(b1)).add_(gr * omb1)
                d = gr - m
                s.mul_(float(b2)).add_(d * omb2 * d).add_(eps_var)
                q = (m * inv_bc1) / ((s * inv_bc2).sqrt() + eps_den)
                p.sub_(q * lr + p * decay)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.native:
            self._native_step()
            return loss
        if self.clip_norm is not None:
            self._clip_with_torch()
        self._torch_step()
        return loss



class GraphedStep:
    """A whole training step — `fn()`: forward, loss, backward, `FluxADAMW(capturable=True).step()`, `refresh_weights` — captured ONCE
    in a hipGraph (torch.cuda.CUDAGraph) and replayed: the step is ≈ 80 small launches whose host enqueue time (≈ 1.5 ms) equals the
    device time; a replay is one submission  [REF examples/pendulum_friction-less/model_train.jl:186-204: the loop body this replaces].
    What the capture needs, and gets: every workspace sized before it (`warmup` eager steps on a side stream), the optimiser's step count
    in device memory (lde_adamw_flux_step_dev), gradients at fixed addresses (allocated from the graph's pool during capture), inputs
    copied INTO the captured tensors (`static_inputs`: tensors `fn` reads; `replay(*new)` copies into them), and a single stream — call
    with the encoder's branch streams off (`recurrent._BRANCH_STREAMS = False`: cross-stream capture of the recurrent stacks' side streams aborts
    inside the HIP runtime on ROCm 7.2). ε of `sample` comes from torch's generator, which is graph-safe (its offsets advance per replay).
    Several GPUs: the collective stays OUTSIDE the graphs — pass the step in two halves: `fn` = zero_grad, forward, loss, backward;
    `between` = the gradient all-reduce (dist.FlatGradAllReduce: eager, on the gradients' fixed addresses); `fn2` = the optimiser step and
    the weight hand-over, a second graph. A replay is then graph · all-reduce · graph (capture in `thread_local` error mode: torch's
    collective watchdog thread may query its events meanwhile).
    `guard` = the step's `FluxADAMW(capturable=True, guard=True)`: a captured step cannot look at its solve from the host (the eager
    step's look at the step record, api._SolveFn._record_that_holds, needs a synchronisation), so a replay whose minibatch is stiffer
    than the warm-up's can overflow the record and come back with NaN gradients — which the guarded update withholds on the device, at
    the cost of that step's own time. Every `check_every` replays `replay` reads `guard.guard_state()` (one synchronisation) and, if
    updates were withheld since its last look, calls `recover()`: ONE eager pass of the whole step on the current static inputs — outside
    capture, so the look at the record happens and the handle keeps the larger "record_capacity"; its own update is withheld
    (`FluxADAMW.withheld`), so the parameters, the step count and the counters are what the replays left — then the old graphs are
    dropped and the step is captured again as in the constructor. `recoveries` counts the calls. A cause that an eager pass does not
    cure (a trajectory that fails at maxiters, an overflow in a bf16 chain) keeps its steps withheld and costs a recovery per look that
    finds new ones: watch `guard_state()["streak"]`. Several GPUs: a sum with a NaN is NaN on every rank, so after the all-reduce every
    rank withholds the same step, looks at the same count and recovers at the same replay. `guard=None`: the class as it was."""

    def __init__(self, fn: Callable[[], torch.Tensor], static_inputs: Sequence[torch.Tensor] = (), warmup: int = 3,
                 between: Optional[Callable[[], None]] = None, fn2: Optional[Callable[[], None]] = None, guard=None,
                 check_every: int = 50):
        self.fn, self.static_inputs, self.between, self.fn2 = fn, list(static_inputs), between, fn2
        if guard is not None and not getattr(guard, "guard", False):
            raise ValueError("GraphedStep(guard=...) takes the step's FluxADAMW(capturable=True, guard=True)")
        if check_every < 1:
            raise ValueError("check_every must be at least 1")
        self.guard, self.check_every, self.recoveries = guard, int(check_every), 0
        self._replays, self._skipped_seen = 0, 0
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._whole()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if guard is not None:
            self._skipped_seen = guard.guard_state()["skipped"]
        self._capture()

    def _whole(self):
        out = self.fn()
        if self.between is not None:
            self.between()
        if self.fn2 is not None:
            self.fn2()
        return out

    def _capture(self):
        fn, between, fn2 = self.fn, self.between, self.fn2
        mode = dict(capture_error_mode="thread_local") if (between is not None or fn2 is not None) else {}
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, **mode):
            out = fn()
            self.loss = out.detach().clone() if isinstance(out, torch.Tensor) else None
        torch.cuda.synchronize()
        self.graph2 = None
        if fn2 is not None:
            if between is not None:
                between()                      # the gradients the second half is captured on are the reduced ones (shapes only matter)
            self.graph2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph2, **mode):
                fn2()
            torch.cuda.synchronize()

    def replay(self, *new_inputs) -> Optional[torch.Tensor]:
        for dst, src in zip(self.static_inputs, new_inputs):
            dst.copy_(src)
        self.graph.replay()
        if self.between is not None:
            self.between()
        if self.graph2 is not None:
            self.graph2.replay()
        if self.guard is not None:
            self._replays += 1
            if self._replays % self.check_every == 0:
                skipped = self.guard.guard_state()["skipped"]
                if skipped > self._skipped_seen:
                    self._skipped_seen = skipped
                    loss = self.loss.clone() if self.loss is not None else None   # this replay's loss: the new capture has a new tensor
                    self.recover()
                    return loss
        return self.loss

    def recover(self):
        """One eager pass of the whole step on the current static inputs with its update withheld (the workspaces — the step record —
        regrow; nothing the training run has computed changes), then a new capture in place of the old graphs. See the class docstring."""
        if self.guard is None:
            raise ValueError("GraphedStep.recover() needs guard=")
        self.recoveries += 1
        torch.cuda.synchronize()
        with self.guard.withheld():
            self._whole()
        torch.cuda.synchronize()
        self.graph = self.graph2 = None      # the old graphs and their memory pool go before the new capture
        self._capture()


def train(model: LatentDiffEqModel, loader_train: Iterable, val_set, dt: float, epochs: int, seq_len: int, full_seq_len: int,
          lr: float = 1e-3, decay: float = 1e-10, start_beta: float = 0.0, end_beta: float = 1.0, n_cycle: int = 3, ratio: float = 0.9,
          progressive_training: bool = False, prog_training_duration: int = 0, start_seq_len: int = 0, variational: bool = True,
          rng: Optional[np.random.Generator] = None, on_epoch: Optional[Callable] = None, grad_sync: Optional[Callable] = None,
          clip_norm: Optional[float] = None, clip_mode: str = "global", optimiser: str = "adamw", graphed: bool = False,
          check_every: int = 50):
    """The epoch loop of the example script  [REF examples/pendulum_friction-less/model_train.jl:138-218]: cyclical β, optional
    progressive sequence length, Flux-flavour ADAMW, validation loss after every minibatch, best weights kept. `loader_train` yields
    x [pixels, B, full_seq_len] tensors on the model's device; `grad_sync` is called between backward and the optimiser step
    (dist.FlatGradAllReduce for multi-GPU). `clip_norm` (with `clip_mode`, see FluxADAMW): the gradients are clipped by norm in front of
    every update — on the GPU the optimiser is then built in its capturable, guarded, clipped form (one submission per step, a step with
    non-finite gradients or norms is withheld) and is left in `model.optimizer`, where `grad_norms()` and `guard_state()` can be read;
    None: the loop as it was. `optimiser`: "adamw" (the scripts' choice) or "adabelief" — FluxAdaBelief, the alternative they name
    [REF model_train.jl:136-138], with the same η, β and decay. Returns (history, best_state).
    `graphed=True` (every parameter on a GPU): the loop on captured graphs. The optimiser is built capturable and guarded (clipped too with
    `clip_norm`) and left in `model.optimizer`; β lives in ONE device word that the host fills once per epoch and the loss kernels read
    (loss.py: the β word), so one capture serves the whole schedule; the training step AND the validation pass that follows it are one
    `GraphedStep(guard=opt, check_every=check_every)` whose static input is the minibatch window. A minibatch then costs the window copy,
    one graph launch and two scalar device-to-device copies into the epoch's history tensor; the host reads that tensor once per epoch —
    which is also when `val_loss < best` is decided, as in the reference [REF model_train.jl:212-217] — and otherwise synchronises only at
    the guard's look every `check_every` replays (a withheld step's loss is recorded as it came out). The encoder's branch streams
    (`recurrent._BRANCH_STREAMS`) are off for the call — a capture needs one stream — and put back at the end; with progressive training
    the epochs shorter than `seq_len` run the same step eagerly (same optimiser, same β word) and the capture happens at the first epoch
    that runs at `seq_len`: no graph per sequence length. `on_epoch` sees the epoch's history after the host has read it; if it solves
    with the model on another time grid it should do so on a decoder of its own (the captured solve reads the grid its handle holds). Not here: η on
    the device (the reference's η is constant), and the multi-GPU split — `grad_sync` with `graphed=True` is refused: the collective stays
    outside the graphs, which is `GraphedStep(between=, fn2=)` used directly."""
    if optimiser not in ("adamw", "adabelief"):
        raise ValueError(f"train(optimiser={optimiser!r}): 'adamw' or 'adabelief'")
    Opt = FluxADAMW if optimiser == "adamw" else FluxAdaBelief
    params = model.parameters()
    if graphed:
        if grad_sync is not None:
            raise ValueError("train(graphed=True) takes no grad_sync: the all-reduce stays outside the graphs — build the step as "
                             "GraphedStep(between=, fn2=) (the two-graph multi-GPU form is not inside train())")
        if not (params and all(p.is_cuda for p in params)):
            raise ValueError("train(graphed=True) needs every parameter on a GPU")
        if check_every < 1:
            raise ValueError("check_every must be at least 1")
        return _train_graphed(model, Opt, params, loader_train, val_set, dt, epochs, seq_len, full_seq_len, lr, decay, start_beta, end_beta,
                              n_cycle, ratio, progressive_training, prog_training_duration, start_seq_len, variational, rng, on_epoch,
                              clip_norm, clip_mode, int(check_every))
    if clip_norm is None:
        opt = Opt(params, lr=lr, betas=(0.9, 0.999), decay=decay)      # ADAMW(η, (0.9, 0.999), decay), Flux flavour
    else:
        on_gpu = bool(params) and all(p.is_cuda for p in params)
        opt = Opt(params, lr=lr, betas=(0.9, 0.999), decay=decay, capturable=on_gpu, guard=on_gpu, clip_norm=clip_norm, clip_mode=clip_mode)
        model.optimizer = opt
    schedule = frange_cycle_linear(epochs, start_beta, end_beta, n_cycle, ratio)
    if progressive_training:
        prog = np.rint(np.linspace(start_seq_len, seq_len, prog_training_duration)).astype(int)
    else:
        prog_training_duration = 0
    t_val = np.arange(val_set.shape[2]) * dt
    best, best_state, history = float("inf"), None, []
    val_loss = 0.0
    for epoch in range(1, epochs + 1):
        beta = float(schedule[epoch - 1])
        sl = int(prog[epoch - 1]) if epoch <= prog_training_duration else seq_len
        t = np.arange(sl) * dt
        for x in loader_train:
            xb = time_loader(x, full_seq_len, sl, rng)
            opt.zero_grad(set_to_none=True)
            loss = loss_batch(model, xb, t, beta, variational)
            _loss_backward(loss)
            L.join_weight_gradients()          # no-op unless _lib.set_async_weight_gradients(True)
            if grad_sync is not None:
                grad_sync()
            opt.step()
            model.refresh_weights()
            with torch.no_grad():
                val_loss = float(loss_batch(model, val_set, t_val, beta, False))
            history.append((epoch, float(loss.detach()), val_loss))
        if on_epoch is not None:
            on_epoch(epoch, history)
        if val_loss < best:
            best = val_loss
            best_state = [p.detach().clone() for p in params]
    return history, best_state


def _train_graphed(model, Opt, params, loader_train, val_set, dt, epochs, seq_len, full_seq_len, lr, decay, start_beta, end_beta, n_cycle, ratio,
                   progressive_training, prog_training_duration, start_seq_len, variational, rng, on_epoch, clip_norm, clip_mode, check_every):
    """train(graphed=True): see there. The step function is the eager loop's body with β read from the word and the two losses left on
    the device; `GraphedStep` replays it once an epoch runs at `seq_len`."""
    from . import recurrent as _rec
    dev = params[0].device
    opt = Opt(params, lr=lr, betas=(0.9, 0.999), decay=decay, capturable=True, guard=True, clip_norm=clip_norm, clip_mode=clip_mode)
    model.optimizer = opt
    schedule = frange_cycle_linear(epochs, start_beta, end_beta, n_cycle, ratio)
    if progressive_training:
        prog = np.rint(np.linspace(start_seq_len, seq_len, prog_training_duration)).astype(int)
    else:
        prog_training_duration = 0
    t_val = np.arange(val_set.shape[2]) * dt
    beta_w = torch.zeros(1, dtype=torch.float32, device=dev)         # the β word: written once per epoch, outside any graph
    val_static = torch.zeros((), dtype=torch.float32, device=dev)    # the validation loss of the last step
    # The validation pass solves on ITS OWN solver handle (a twin of the decoder's diffeq: same settings, same weights by reference): a
    # handle keeps ONE save-time grid on the device and restages it whenever a call brings another — with the training window's grid and
    # the validation set's alternating on one handle that upload would sit inside the graph, twice per replay, reading host staging
    # buffers that later eager calls reuse. With a handle per grid the warm-up leaves both grids in place and the graph uploads nothing.
    val_model = copy.copy(model)
    val_model.decoder = copy.copy(model.decoder)
    val_model.decoder.diffeq = copy.copy(model.decoder.diffeq)
    val_model.decoder.diffeq._handle = None
    window = [None]                                                  # the minibatch window the step reads (static once captured)
    t_now = [None]

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_batch(model, window[0], t_now[0], beta_w, variational)
        _loss_backward(loss)
        L.join_weight_gradients()
        opt.step()
        model.refresh_weights()
        with torch.no_grad():
            val_static.copy_(loss_batch(val_model, val_set, t_val, beta_w, False))
        return loss

    try:
        n_rows = max(int(len(loader_train)), 1)
    except TypeError:
        n_rows = 64
    rows = torch.zeros(n_rows, 2, dtype=torch.float32, device=dev)   # (loss, validation loss) per minibatch of the epoch
    best, best_state, history = float("inf"), None, []
    gs = None
    keep_branch = _rec._BRANCH_STREAMS
    _rec._BRANCH_STREAMS = False
    try:
        for epoch in range(1, epochs + 1):
            beta_w.fill_(float(schedule[epoch - 1]))
            sl = int(prog[epoch - 1]) if epoch <= prog_training_duration else seq_len
            t_now[0] = np.arange(sl) * dt
            k = 0
            for x in loader_train:
                xb = time_loader(x, full_seq_len, sl, rng)
                if k == rows.shape[0]:                                # a loader without a length that outgrew the guess
                    rows = torch.cat([rows, torch.zeros_like(rows)])
                if sl != seq_len:                                     # progressive training: not yet the captured length — eager
                    window[0] = xb
                    loss = step().detach()
                elif gs is None:
                    # the first minibatch at seq_len: size every workspace with eager passes whose update is withheld (the parameters, the
                    # moments, the step count and the guard's counters stay what they were), capture, then replay for the real step
                    window[0] = xb.detach().clone().contiguous()
                    side = torch.cuda.Stream(dev)
                    side.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(side):
                        for _ in range(2):
                            with opt.withheld():
                                step()
                    torch.cuda.current_stream(dev).wait_stream(side)
                    gs = GraphedStep(step, static_inputs=[window[0]], warmup=0, guard=opt, check_every=check_every)
                    loss = gs.replay(xb)
                else:
                    loss = gs.replay(xb)
                rows[k, 0].copy_(loss)
                rows[k, 1].copy_(val_static)
                k += 1
            got = rows[:k].tolist()                                   # the epoch's one read
            history.extend((epoch, float(a), float(b)) for a, b in got)
            if on_epoch is not None:
                on_epoch(epoch, history)
            if got and got[-1][1] < best:
                best = got[-1][1]
                best_state = [p.detach().clone() for p in params]
    finally:
        _rec._BRANCH_STREAMS = keep_branch
    model.graphed_step, model.beta_word = gs, beta_w              # (left for inspection, like model.optimizer)
    return history, best_state
