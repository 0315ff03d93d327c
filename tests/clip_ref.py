"""Restatement (numpy) of the clipped step (include/lde.h: "the clipped step"; lde_adamw_flux_step_clipped, `FluxADAMW(clip_norm=…)`):
the norms in f64, the two scale rules with the norm ROUNDED TO f32 and the scale formed in f32 (the contract), and Flux-flavour ADAMW on s·g
in f32 — m ← β₁m + (1−β₁)g; v ← β₂v + (1−β₂)g²; Δ = m/(1−β₁ᵗ)/(√(v/(1−β₂ᵗ)) + ε)·η + decay·x; x ← x − Δ (the decay is not scaled by η).
The bias corrections are formed as the kernels form them: 1/(1 − βᵗ) in f64 from the f32 β, rounded to f32."""
import numpy as np

GLOBAL, PER_ARRAY = 0, 1
MODES = {"global": GLOBAL, "per_array": PER_ARRAY}
f32 = np.float32


def norms(grads):
    """(per-array norms, total norm) in f64 of a list of arrays (an empty array has norm 0)."""
    sq = [float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads]
    return [float(np.sqrt(s)) for s in sq], float(np.sqrt(np.sum(np.asarray(sq, np.float64))))


def scales(per, total, c, mode):
    """The f32 scale of every array from the f64 norms: the norm is rounded to f32 first, everything after it is f32 arithmetic."""
    c = f32(c)
    if mode == GLOBAL:
        s = min(f32(1.0), f32(c / f32(f32(total) + f32(1e-6))))
        return [f32(s) for _ in per]
    assert mode == PER_ARRAY
    return [f32(c / f32(n)) if f32(n) > c else f32(1.0) for n in per]


def adamw(p, g, m, v, t, lr, b1, b2, eps, decay, one_minus_beta_in_f64=False):
    """One Flux-flavour ADAMW step on f32 arrays at step count t ≥ 1 (f32 arithmetic, one rounding per operation); returns new (p, m, v).
    The kernels receive β as f32 and form 1 − β in f32 (1 − 0.999f = 1.0000467e-3); torch's Adam — the non-native path of FluxADAMW — forms
    it from the Python float (1e-3): `one_minus_beta_in_f64` restates that, the one place where the two paths differ by more than rounding."""
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    omb1, omb2 = (f32(1.0 - b1), f32(1.0 - b2)) if one_minus_beta_in_f64 else (f32(1.0) - f32(b1), f32(1.0) - f32(b2))
    bc1, bc2 = ((1.0 - float(b) ** t) if one_minus_beta_in_f64 else (1.0 - float(f32(b)) ** t) for b in (b1, b2))
    bc1, bc2 = f32(1.0 / bc1), f32(1.0 / bc2)
    b1, b2, lr, eps, decay = f32(b1), f32(b2), f32(lr), f32(eps), f32(decay)
    m = b1 * m + omb1 * g
    v = b2 * v + omb2 * g * g
    d = (m * bc1) / (np.sqrt(v * bc2) + eps) * lr + decay * p
    return (p - d).astype(f32), m.astype(f32), v.astype(f32)


def clipped_step(ps, gs, ms, vs, t, hp, c, mode, **kw):
    """The clipped step on lists of arrays: hp = (η, β₁, β₂, ε, decay). Returns (ps, ms, vs, per-array f64 norms, total f64 norm, scales).
    `c = None`: no clipping (every scale 1) — the control of the tests."""
    per, total = norms(gs)
    s = scales(per, total, c, mode) if c is not None else [f32(1.0) for _ in per]
    out = [adamw(p, f32(si) * np.asarray(g, f32), m, v, t, *hp, **kw) for p, g, m, v, si in zip(ps, gs, ms, vs, s)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], per, total, s
