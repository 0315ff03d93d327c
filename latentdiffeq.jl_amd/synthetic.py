"""Synthetic inputs of the hot path: shared by bench.py, the tests and golden generation.
Pure numpy; array *memory* is the reference's column-major layout: z0 (B,D) == [D×B], ẑ (T,B,D') == [D'×B×T]."""
import numpy as np

def pendulum_inputs(B: int, seed: int = 1, dtype=np.float32):
    """θ₀~U(±π/6), ω₀~U(±π/3), L~U(1,2)  [REF examples/pendulum_friction-less/create_data.jl:19-22]."""
    rng = np.random.default_rng(seed)
    z0 = np.stack([rng.uniform(-np.pi / 6, np.pi / 6, B), rng.uniform(-np.pi / 3, np.pi / 3, B)], axis=1)
    L = rng.uniform(1.0, 2.0, (B, 1))
    return z0.astype(dtype), L.astype(dtype)


def time_grid(T: int = 50, dt: float = 0.05, t0: float = 0.0):
    """t = range(0, step=0.05, length=50), Float64  [REF examples/pendulum_friction-less/model_train.jl:40,44,181]."""
    return t0 + dt * np.arange(T, dtype=np.float64)


def shifted_grids(T: int = 33, spacing: float = 1.0 / 16.0):
    """The time-translation known answer's grids: base = (0 … T−1)·spacing (a power of two: 1/16) and base + c for c = ±1024, +2²⁰, −base[−1] (ends exactly at 0) and
    −base[T//2] (contains 0), as an ordered dict name → grid with "base" first. Every entry and every sum is a dyadic rational well inside
    53 bits, so each shifted grid has bit-identical differences (asserted) and, with a dyadic dt, every time a stepping loop forms is exact:
    an autonomous right-hand side must then give bit-identical results on every grid."""
    assert np.frexp(spacing)[0] == 0.5 and spacing <= 1.0, "a power of two"
    base = np.arange(T, dtype=np.float64) * spacing
    shifts = {"base": 0.0, "plus_1024": 1024.0, "minus_1024": -1024.0, "plus_2p20": float(2 ** 20), "ends_at_0": -base[-1],
              "contains_0": -base[T // 2]}
    grids = {name: base + c for name, c in shifts.items()}
    for name, g in grids.items():
        assert np.array_equal(np.diff(g), np.diff(base)) and np.array_equal(g - shifts[name], base), name
    assert grids["ends_at_0"][-1] == 0.0 and grids["contains_0"][T // 2] == 0.0
    return grids


def cotangent(T: int, B: int, Dp: int, seed: int = 2, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, B, Dp)) / (B * T)).astype(dtype)


def mlp_weights(layers, seed: int = 3, scale: float = 1.0, dtype=np.float32):
    """Flat Flux.destructure-order weights, U(±1/√fan_in)·scale, biases U(±1/√fan_in)·scale."""
    rng = np.random.default_rng(seed)
    parts = []
    for i in range(len(layers) - 1):
        fan_in, out = layers[i], layers[i + 1]
        bound = scale / np.sqrt(fan_in)
        Wl = rng.uniform(-bound, bound, (out, fan_in))
        bl = rng.uniform(-bound, bound, out)
        parts.append(Wl.flatten(order="F"))  # vec(W), column-major [out×in]
        parts.append(bl)
    return np.concatenate(parts).astype(dtype)
