"""GPU: HIP path (through the C ABI) against the committed golden fixtures of tests/golden/ — the data that is
guaranteed identical on the build container and on the GPU box.

Tolerances: tight-tolerance / fixed-step fixtures ≤ 2e-5 on ẑ (fp32 round-off through ≤ 200 RHS evaluations);
default-tolerance fixtures: worst column within 3× max(3e-4, the fixture's own float64 error), median within
max(1e-4, half of it), and no farther from the stored float64 truth than 2.5× the fixture's own error + 1e-5.
Gradients: a per-fixture relative gate against the fixture (GRAD_LIM), set at ≈ 3–10× the margin measured on MI355X
(abl/golden_margins.py, round 2; "own" = the fixture's own distance from its float64 adjoint):

    fixture                              |Δẑ|      dẑ₀       dθ̂        dW        own dẑ₀ / dθ̂ / dW
    c1_goku_pendulum_b64                 5.3e-5    4.7e-7    1.0e-6    –         2.4e-6 / 2.7e-5 / –
    metric_goku_pendulum_b256            2.6e-5    6.7e-7    1.8e-6    –         3.9e-6 / 1.5e-5 / –
    metric_goku_pendulum_b256_tight      1.2e-6    2.5e-7    3.2e-7    –         3.0e-7 / 4.8e-7 / –
    goku_pendulum_friction_b32           2.3e-5    2.8e-7    6.0e-7    –         4.6e-7 / 1.8e-5 / –
    c2_latentode_rk4_d8_h200_b16         1.2e-7    1.4e-7    –         1.2e-7    3.4e-4 / – / 4.0e-4   (own: RK4 dt=0.05 truncation)
    latentode_aug_tanh_d6a2_b16          3.8e-7    2.3e-7    –         2.2e-7    2.5e-7 / – / 1.4e-7
    c4_latentode_tsit5_d32_h128_b16      3.2e-5    (gradients: tests/test_gpu_same_steps.py, 1e-4 on the same steps)
    c3_pendulum_plus_mlp_b32             1.3e-3    (   "   )
    latentode_ref_tsit5_d16_h200_b16     …         (   "   )

The analytic right-hand sides and the smooth / fixed-step networks reproduce the fixture's gradients to ~1e-6 (the
time-parallel adjoint takes the same single step per save interval as the oracle). Where a relu network meets the adaptive
controller at reltol = 1e-3, two correct f32 solves — two free-running controllers — differ by about the solver's own error
(rounds 1–4 gated those three fixtures' gradients at 3e-3 … 2.5e-2 here: a number that says nothing about arithmetic). Since
round 5 their gradients are held where they can be held tightly: kernel and oracle on the SAME recorded steps, every gradient
≤ 1e-4 (tests/test_gpu_same_steps.py, continuous adjoint; tests/test_gpu_discrete.py, LDE_SENSE_DISCRETE) — so this file keeps
their forward gate and a bound against the FLOAT64 adjoint of the size of the fixture's own float64 distance, and no loose
fixture-relative gate. Against the float64 adjoint: ≤ 3.5× the fixture's own distance + 1e-3."""
import glob
import os

import numpy as np
import pytest

from tests.golden import make_golden as G

pytestmark = pytest.mark.gpu
# relative gradient gates against the fixture: (dẑ₀ and dθ̂, dW)
GRAD_LIM = {
    "c1_goku_pendulum_b64": (1e-5, None), "metric_goku_pendulum_b256": (1e-5, None), "metric_goku_pendulum_b256_tight": (5e-6, None),
    "goku_pendulum_friction_b32": (1e-5, None), "c2_latentode_rk4_d8_h200_b16": (5e-6, 5e-6), "latentode_aug_tanh_d6a2_b16": (5e-6, 5e-6),
}
# relu network + adaptive control at reltol 1e-3: no fixture-relative gradient gate here (two free-running controllers) — their gradients are
# held to 1e-4 on the same steps in tests/test_gpu_same_steps.py / tests/test_gpu_discrete.py
SAME_STEPS_ONLY = {"c4_latentode_tsit5_d32_h128_b16", "c3_pendulum_plus_mlp_b32", "latentode_ref_tsit5_d16_h200_b16"}
FIX = sorted(f for f in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))
             if not os.path.basename(f).startswith(("chain_", "dual_parent_bits")))   # chain fixtures: tests/test_oracle_chain.py; the dual
#                                                                                      kernels' recorded bits: tests/test_gpu_dual_bits.py


@pytest.mark.parametrize("path", FIX, ids=[os.path.basename(f)[:-4] for f in FIX])
def test_hip_matches_golden_fixture(path):
    import ctypes as C
    from tests.gpu_util import Native
    from latentdiffeq_amd import _lib as L
    name = os.path.basename(path)[:-4]
    cfg = G.CONFIGS[name]
    fx = np.load(path)
    ts, z0, theta, W, dz = G.inputs(cfg)
    k = cfg["keep"]
    od = G.desc(cfg)
    d = L.ProblemDesc()
    C.memmove(C.byref(d), C.byref(od), C.sizeof(d))
    nat = Native(d)
    if W is not None:
        nat.set_weights(W)
    z, ret, st = nat.forward(z0, theta, ts)
    assert np.array_equal(ret[:k], fx["retcode"]) and (ret == 0).all()
    tight = cfg.get("reltol", 1e-3) < 1e-4 or not cfg.get("adaptive", True)
    per = np.abs(z[:, :k] - fx["z"]).max(axis=(0, 2))
    e_k, e_o = np.abs(z[:, :k] - fx["z64"]).max(), np.abs(fx["z"] - fx["z64"]).max()
    if tight:
        assert per.max() <= 2e-5
    else:
        # two correct fp32 solves differ by at most about the solver's own error at this tolerance
        # (relu right-hand sides are the worst case: a kink crossed at a slightly different step size moves a
        #  trajectory by a multiple of the local error — hence the factor on the worst column, with the bulk bounded)
        assert per.max() <= 3 * max(3e-4, e_o) and np.median(per) <= max(1e-4, 0.5 * e_o)
        assert e_k <= 2.5 * e_o + 1e-5
    assert abs(st["naccept"] - fx["fwd_stats"][1]) <= 0.10 * fx["fwd_stats"][1] + 2
    g0, gth, gW, sb = nat.adjoint(z, theta, ts, dz)
    lim, limW = GRAD_LIM.get(name, (1e-3 if tight else 1e-2, 1e-3 if tight else 1e-2))   # (a new fixture starts at the round-1 gates)
    s0 = np.abs(fx["dz0"]).max()

    def close(g, ref, ref64, lim=lim):   # within the fixture's measured-margin gate (module docstring)
        return name in SAME_STEPS_ONLY or np.abs(g - ref).max() <= lim * np.abs(ref).max()
    assert close(g0[:k], fx["dz0"], fx["dz0_64"])
    assert np.abs(g0[:k] - fx["dz0_64"]).max() <= 3.5 * np.abs(fx["dz0"] - fx["dz0_64"]).max() + 1e-3 * s0
    if theta is not None:
        assert close(gth[:k], fx["dtheta"], fx["dtheta_64"])
    if W is not None:
        sw = np.abs(fx["dW"]).max()
        assert close(gW[fx["dW_idx"]], fx["dW"], fx["dW_64"], limW)
        assert name in SAME_STEPS_ONLY or abs(np.linalg.norm(gW.astype(np.float64)) - fx["dW_norm"][0]) <= 4 * limW * fx["dW_norm"][0]
        assert np.abs(gW[fx["dW_idx"]] - fx["dW_64"]).max() <= 3.5 * np.abs(fx["dW"] - fx["dW_64"]).max() + 1e-3 * sw
