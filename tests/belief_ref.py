"""Restatement (numpy) of the AdaBelief step (include/lde.h: "the AdaBelief step"; lde_adabelief_flux_step*, `FluxAdaBelief`):
    m ← β₁·m + (1 − β₁)·g;   s ← β₂·s + (1 − β₂)·(g − m)² + ε_var  (the NEW m);   Δ = η·(m/(1 − β₁ᵗ))/(√(s/(1 − β₂ᵗ)) + ε_den) + decay·x;   x ← x − Δ
in two modes. `f64`: the arithmetic in f64 on the f32 values the C ABI receives — η, β, ε, decay and the gradients rounded to f32 first,
1 − β formed from the f32 β, the state carried in f64 from step to step: THE REFERENCE. `f32`: the same operations in the same order, one
f32 rounding per operation (no fused multiply-add), the bias corrections as the kernels form them (1/(1 − βᵗ) in f64 from the f32 β,
rounded to f32), the state carried in f32. The distance between the two on a test's own inputs is the FLOOR of that test: what f32
arithmetic in this order costs, measured and not guessed; a kernel may contract a·b + c·d to a fused multiply-add and order its
operations differently, each such difference a rounding of the floor's size — the tests allow BOUND_FACTOR = 4 floors.
hp = (η, β₁, β₂, ε_var, ε_den, decay). The clipped form takes its norms and scales from tests/clip_ref.py (the scan is the same code)."""
import numpy as np

from tests import clip_ref as C

f32, f64 = np.float32, np.float64
BOUND_FACTOR = 4.0
HP = (1e-3, 0.9, 0.999, 1e-16, 1e-16, 1e-3)      # η, β₁, β₂, ε_var, ε_den, decay: FluxAdaBelief's defaults (ε = 1e-8 → ε²) with a decay that shows


def _many():
    """49 non-empty arrays with empty ones in the middle: one more than a launch's table holds (csrc/lde_host.h: OPT_MAXT = 48)."""
    pool, out, i = [1, 3, 5, 0, 17, 300, 2049, 0, 64], [], 0
    while sum(1 for n in out if n) < 49:
        out.append(pool[i % len(pool)])
        i += 1
    return out


# the inputs of tests/test_gpu_belief.py, made here so that tests/test_belief_host.py measures the floor on the very same numbers:
# sizes around the update's slice of 2048 elements, one array whose four views start one float past a 16-byte boundary, and the long table
CASES = {"paths": dict(sizes=[1, 0, 5, 2047, 2048, 2049, 8193, 3 * 2048 + 7, 2051], unaligned=(8,), steps=4, seed=101),
         "49 arrays": dict(sizes=_many(), unaligned=(), steps=3, seed=202)}
_INPUTS = {}


def inputs(name):
    """(sizes, unaligned, ps, grads) of a case: x ~ N(0, 1), a FRESH gradient ~ N(0, 0.1²) for every step (with a repeated gradient g − m
    cancels and s collapses to ε_var: the rule's own behaviour, not the kernel's); m = s = 0 before the first step. Read-only, made once."""
    if name not in _INPUTS:
        c = CASES[name]
        rng = np.random.default_rng(c["seed"])
        ps = [rng.standard_normal(n).astype(f32) for n in c["sizes"]]
        grads = [[(rng.standard_normal(n) * 0.1).astype(f32) for n in c["sizes"]] for _ in range(c["steps"])]
        for a in ps + [g for gs in grads for g in gs]:
            a.setflags(write=False)
        _INPUTS[name] = (list(c["sizes"]), tuple(c["unaligned"]), ps, grads)
    return _INPUTS[name]


def zeros(ps):
    return [np.zeros_like(p) for p in ps]


def step(p, g, m, s, t, hp, mode="f64"):
    """One step at count t ≥ 1 on arrays; returns new (p, m, s, Δ) in the mode's precision."""
    lr, b1, b2, eps_var, eps_den, decay = (f32(h) for h in hp)
    g = np.asarray(g, f32)
    if mode == "f64":
        T = f64
        p, g, m, s = (np.asarray(a, f64) for a in (p, g, m, s))
        lr, b1, b2, eps_var, eps_den, decay = (f64(h) for h in (lr, b1, b2, eps_var, eps_den, decay))
        omb1, omb2 = 1.0 - b1, 1.0 - b2
        inv_bc1, inv_bc2 = 1.0 / (1.0 - b1 ** t), 1.0 / (1.0 - b2 ** t)
    else:
        assert mode == "f32"
        T = f32
        p, m, s = (np.asarray(a, f32) for a in (p, m, s))
        omb1, omb2 = f32(1.0) - b1, f32(1.0) - b2
        inv_bc1, inv_bc2 = f32(1.0 / (1.0 - float(b1) ** t)), f32(1.0 / (1.0 - float(b2) ** t))
    with np.errstate(invalid="raise", divide="raise"):
        m = b1 * m + omb1 * g
        d = g - m
        s = b2 * s + omb2 * d * d + eps_var
        delta = (m * inv_bc1) / (np.sqrt(s * inv_bc2) + eps_den) * lr + decay * p
        p = p - delta
    return p.astype(T), m.astype(T), s.astype(T), delta.astype(T)


def steps(ps, grads, ms, ss, hp, mode="f64", t0=0, scales=None):
    """Consecutive steps on lists of arrays: `grads[k]` is step t0 + k + 1's list of gradients, `scales[k]` (optional) its f32 scale per array
    (the clipped form: g ← s·g in f32 in front of the moments). Returns a list with one (ps, ms, ss) per step."""
    out = []
    for k, gs in enumerate(grads):
        sc = scales[k] if scales is not None else [f32(1.0)] * len(gs)
        new = [step(p, f32(c) * np.asarray(g, f32), m, s, t0 + k + 1, hp, mode)[:3] for p, g, m, s, c in zip(ps, gs, ms, ss, sc)]
        ps, ms, ss = [n[0] for n in new], [n[1] for n in new], [n[2] for n in new]
        out.append((ps, ms, ss))
    return out


def clip_scales(grads, c, mode):
    """The clipped step's f32 scales for one step's gradients: f64 norms rounded to f32, the scale formed in f32 (tests/clip_ref.py)."""
    per, total = C.norms(grads)
    return C.scales(per, total, c, mode), per, total


def errors(got, ref, lr):
    """(ex, em, es) of one step's (ps, ms, ss) against the f64 reference's, the worst over all arrays:
    em, es — |m − m_ref| and |s − s_ref| relative to the reference's largest |m|, |s| over all arrays of the step;
    ex — |x − x_ref| in units of 2⁻²⁴·(|x_ref| + η): half an ulp of x where x is large, and a 2⁻²⁴ of the step's own size η where x is small
    (Δ is of the order of η whatever the gradient's scale, and its relative error is what f32 gives)."""
    (gp, gm, gs), (rp, rm, rs) = got, ref
    big = lambda arrs: max((float(np.abs(a).max()) for a in arrs if a.size), default=0.0)
    mm, sm = big(rm), big(rs)
    ex = em = es = 0.0
    for a, b, c, d, e, f in zip(gp, rp, gm, rm, gs, rs):
        if not np.size(b):
            continue
        b, d, f = (np.asarray(v, f64) for v in (b, d, f))
        ex = max(ex, float((np.abs(np.asarray(a, f64) - b) / (2.0 ** -24 * (np.abs(b) + float(f32(lr))))).max()))
        em = max(em, float(np.abs(np.asarray(c, f64) - d).max()) / mm)
        es = max(es, float(np.abs(np.asarray(e, f64) - f).max()) / sm)
    return ex, em, es


def floors(ps, grads, ms, ss, hp, t0=0, scales=None):
    """Per step (ex, em, es) of the f32 mode against the f64 mode on these very inputs, and the f64 mode's states (the reference)."""
    ref = steps(ps, grads, ms, ss, hp, "f64", t0, scales)
    low = steps(ps, grads, ms, ss, hp, "f32", t0, scales)
    return [errors(a, b, hp[0]) for a, b in zip(low, ref)], ref
