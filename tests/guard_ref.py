"""The inputs of the guarded captured step's end-to-end test (tests/test_gpu_guard.py, case 6), shared with the CPU test that pins how many
steps they take (tests/test_guard_host.py): B = 8 frictionless pendulums over T = 8 save times 0.25 apart, Tsit5 at the default tolerances
(1e-6 / 1e-3). "mild": long pendulums at small angles — the oracle accepts 10 … 13 steps; "harsh": lengths of 2 … 3 cm from an angle of
1 … 1.5 rad — 41 … 50 steps. CAP = 20 is the "record_capacity" the test starts from: every mild trajectory stays at or below CAP − 2, every
harsh one reaches at least CAP + 2 (the kernel's controller takes about 3 % fewer or more steps than the oracle's)."""
import numpy as np

B, T, DT, CAP = 8, 8, 0.25, 20
MILD_STEPS = (10, 13)       # the oracle's fewest and most accepted steps over the B trajectories (f32 oracle, tests/test_guard_host.py)
HARSH_STEPS = (41, 50)


def grid():
    return np.arange(T) * DT


def inputs(kind: str):
    """(z0 [B, 2], θ [B, 1]) float32, batch-major."""
    rng = np.random.default_rng(dict(mild=3, harsh=4)[kind])
    (alo, ahi), (llo, lhi) = dict(mild=((0.2, 0.6), (1.5, 2.0)), harsh=((1.0, 1.5), (0.02, 0.03)))[kind]
    z0 = np.stack([rng.uniform(alo, ahi, B), rng.uniform(-0.3, 0.3, B)], axis=1).astype(np.float32)
    th = rng.uniform(llo, lhi, (B, 1)).astype(np.float32)
    return z0, th
