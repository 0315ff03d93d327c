"""GPU: every path through k_pend_adjoint_disc_tp's entry and save-time phase (csrc/lde_pendulum.hip), at the smallest shape that reaches it.

The entry issues its first round of global loads unconditionally at clamped indices (min(lane, T − 1), min(sl, cap − 1), min(sl + 1, cap − 1))
and applies the guards as selects; the save-time phase is straight-line for one trip of four save times per lane, with the ragged-grid
re-fetch and the further trips behind wave votes. Each case below names the path it is there for. All of them go through
tests/test_gpu_discrete.py's `_check` — the oracle's `adjoint_discrete` on the kernel's own record, f32 and f64, |Δẑ| ≤ 2e-5, gradients ≤ 1e-4
— and assert the pullback's statistics (accepted steps = the record's, 2S + 1 evaluations per step and one for k₁ of the first).

The inputs are such that the f32 and the f64 oracle, each differentiating the f32 oracle's own record of them, agree within half of the
gradient gate (largest relative difference over all cases 6e-6: checked on the CPU), so the gate is the kernel's to miss.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import test_gpu_discrete as D

pytestmark = pytest.mark.gpu
_native, _check = D._native, D._check


@pytest.fixture(autouse=True)
def _at_most_16_oracle_threads(monkeypatch):
    monkeypatch.setattr(D, "NT", min(D.NT, 16))


def _uniform(T, t_end=2.45):
    return np.arange(T) * (t_end / (T - 1))


def _geometric(T=17, t_end=2.45, r=1.3):
    """Spacings that grow by 30 % from one save time to the next: the uniform-grid guess of a step's last save time is wrong nearly everywhere."""
    return t_end * (r ** np.arange(T) - 1.0) / (r ** (T - 1) - 1.0)


# name → (B, save grid, descriptor fields, seed)
CASES = {
    "one_step_one_save_time": (1, O.time_grid(2), {}, 21),                  # grid padded to 8 workgroups, every first-round index clamped
    "metric_path_two_xcd_columns": (9, O.time_grid(50), {}, 22),            # one trip per lane, workgroups b = 8 on a second XCD column
    "more_save_times_than_lanes_65": (3, _uniform(65), {}, 23),             # the staging loop runs for one lane
    "more_save_times_than_lanes_130": (3, _uniform(130), {}, 24),           # … twice for most, three times for two lanes
    "geometric_grid_ragged_path": (5, _geometric(), {}, 25),
    "many_save_times_per_step_extra_trips": (4, np.arange(200) / 199.0, dict(reltol=1e-2), 26),
    "more_than_21_steps_later_rounds": (4, _uniform(5, 1.2), dict(abstol=1e-9, reltol=1e-7), 27),
    "friction": (5, O.time_grid(50), dict(rhs_kind=O.RHS_PENDULUM_FRICTION), 28),
    "rk4_fixed_step": (5, O.time_grid(50), dict(solver=O.SOLVER_RK4, adaptive=0, dt=0.13), 29),
}


def case_inputs(name):
    B, ts, kw, seed = CASES[name]
    z0, L = O.pendulum_inputs(B, seed=seed)
    T = len(ts)
    return z0, L, np.ascontiguousarray(ts, np.float64), O.cotangent(T, B, 2, seed=seed + 100), kw


def _stages(kw):
    return 4 if kw.get("solver") == O.SOLVER_RK4 else 6


def _assert_pullback_statistics(rec, sb, S):
    n = rec["n"].astype(np.int64)
    assert sb["nfailed"] == 0 and sb["nreject"] == 0
    assert sb["naccept"] == int(n.sum()) and sb["max_steps"] == int(n.max())
    assert sb["nfe"] == int((n * (2 * S + 1) + 1).sum())


def _run(name, o32, o64, options=()):
    z0, L, ts, dz, kw = case_inputs(name)
    nat, od = _native(None, **kw)
    for k, v in options:
        nat.set_option(k, v)
    z, rec, g, st, sb = _check(nat, od, o32, o64, z0, L, ts, dz, None)
    _assert_pullback_statistics(rec, sb, _stages(kw))
    return nat, z, rec, g


@pytest.mark.parametrize("name", list(CASES))
def test_disc_tp_path_matches_oracle_on_the_same_steps(o32, o64, name):
    _, z, rec, _ = _run(name, o32, o64)
    n, ts = rec["n"], CASES[name][1]
    if name == "one_step_one_save_time":
        assert int(n[0]) == 1
    if name == "many_save_times_per_step_extra_trips":   # a lane's share of the longest step: more than the four save times of one trip
        assert (len(ts) - 1) / int(n.max()) > 12
    if name == "more_than_21_steps_later_rounds":
        assert int(n.min()) > 21
    if name == "geometric_grid_ragged_path":             # several steps between the late save times, several early save times inside the first step
        assert int(n.max()) >= 4 and ts[2] < rec["dt"][:, 0].min()


def test_disc_tp_non_finite_row_gets_zero_and_leaves_the_others_alone(o32, o64):
    name = "metric_path_two_xcd_columns"
    z0, L, ts, dz, kw = case_inputs(name)
    z0, L, dz = z0[:6], L[:6], np.ascontiguousarray(dz[:, :6])
    nat, od = _native(None, **kw)
    z, rec, (g0, gth, _), _, sb = _check(nat, od, o32, o64, z0, L, ts, dz, None)
    _assert_pullback_statistics(rec, sb, 6)
    zb = z0.copy()
    zb[2, 0] = np.inf
    z2, ret2, st2 = nat.forward(zb, L, ts)
    assert ret2[2] != 0 and (np.delete(ret2, 2) == 0).all() and np.isnan(z2[1:, 2]).all()
    h0, hth, _, sb2 = nat.adjoint(z2, L, ts, dz)
    assert sb2["nfailed"] == 1 and (h0[2] == 0).all() and hth[2, 0] == 0
    keep = np.arange(6) != 2
    assert np.array_equal(h0[keep], g0[keep]) and np.array_equal(hth[keep], gth[keep])
    assert sb2["naccept"] == int(np.delete(rec["n"], 2).sum())


def test_disc_tp_record_overflow_is_nan_never_a_truncated_sweep(o32, o64):
    name = "metric_path_two_xcd_columns"
    z0, L, ts, dz, kw = case_inputs(name)
    nat, od = _native(None, **kw)
    nat.set_option("record_capacity", 3)
    z, ret, st = nat.forward(z0, L, ts)
    assert (ret == 0).all() and st["max_steps"] > 3
    g0, gth, _, sb = nat.adjoint(z, L, ts, dz)
    assert sb["nfailed"] == len(z0) and np.isnan(g0).all() and np.isnan(gth).all() and sb["naccept"] == 0
    nat.set_option("record_capacity", 512)
    z2, rec, _, _, sb = _check(nat, od, o32, o64, z0, L, ts, dz, None)
    assert np.array_equal(z2, z)
    _assert_pullback_statistics(rec, sb, 6)
