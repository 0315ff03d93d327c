"""GPU: k_pend_adjoint_disc_tp (csrc/lde_pendulum.hip) after its save-time trip came to run speculatively on the guessed index, in front of
ONE wave vote (a lane whose guess was wrong drops its sums and runs the trip again), and its entry and round top were lightened.

1. The parent's bits. tests/golden/bits/disc_tp_parent_bits.npz was recorded on an MI355X from a build of the commit named in its
   `parent_commit` entry (the last one with a vote in front of the trip and one behind it), by `record()` below; `hipcc_version` is the compiler of that build. Every
   array is compared as raw bytes, no tolerance: ẑ, the return codes, dz0, dθ and the four statistics of the pullback. A difference is a finding
   about the kernel's arithmetic (a multiply and an add that now share a block and were fused), not a reason for a bound. Cases: every entry of
   tests/test_gpu_disc_tp_paths.py's CASES, its non-finite-row and record-overflow setups, the metric's own inputs, and the three grids of 2.

2. The paths the speculative trip creates: a lane whose guess of the step's last save time is wrong (its speculative trip is discarded, the
   index walked to, the trip run again) AND whose step holds more than the twelve save times of one trip of its three lanes (the redone trip
   continues into the extra trips) — with T > 64 and, at tight tolerances, in rounds r > 0 of records longer than 42 steps. Each goes through
   tests/test_gpu_discrete.py's `_check` (the oracle's sweep on the kernel's own record, f32 and f64, |Δẑ| ≤ 2e-5, gradients ≤ 1e-4) and
   asserts the pullback's statistics; that the record has such steps is asserted from the record itself. On the CPU, with the f32 oracle's
   record, the f32 and the f64 oracle agree on these inputs within 2.0e-6 / 2.8e-7 / 1.0e-6 (relative, largest gradient entry): the 1e-4 gate
   is the kernel's to miss.

3. One of them through the lane-per-trajectory kernel (option "pend_disc_tp_max_b" = 0): the two mappings within 1e-5 of each other.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import test_gpu_discrete as D
from tests import test_gpu_disc_tp_paths as P

pytestmark = pytest.mark.gpu

# (in a folder of its own: tests/test_golden.py and tests/test_gpu_golden.py take every tests/golden/*.npz for an oracle fixture)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bits", "disc_tp_parent_bits.npz")
STAT_KEYS = ("nfe", "naccept", "nreject", "nfailed")


@pytest.fixture(autouse=True)
def _at_most_16_oracle_threads(monkeypatch):
    monkeypatch.setattr(D, "NT", min(D.NT, 16))


def _cubic121():
    return 2.45 * np.linspace(0, 1, 121) ** 3


def _dense_head_then_quadratic():
    return np.concatenate([np.linspace(0, 0.04, 30, endpoint=False), 0.04 + 2.41 * np.linspace(0, 1, 20) ** 2])


# name → (B, save grid, descriptor fields, seed)
GRIDS = {
    "cubic121": (4, _cubic121(), {}, 31),
    "cubic121_tight": (4, _cubic121(), dict(abstol=1e-9, reltol=1e-7), 32),
    "dense_head_then_quadratic": (4, _dense_head_then_quadratic(), {}, 33),
}
BIT_CASES = list(P.CASES) + ["non_finite_row", "record_overflow", "metric"] + list(GRIDS)


def grid_inputs(name):
    B, ts, kw, seed = GRIDS[name]
    z0, L = O.pendulum_inputs(B, seed=seed)
    T = len(ts)
    return z0, L, np.ascontiguousarray(ts, np.float64), O.cotangent(T, B, 2, seed=seed + 100), kw


def _arrays(z, ret, g0, gth, sb):
    return dict(z=z, retcode=ret, dz0=g0, dtheta=gth, pullback_stats=np.array([sb[k] for k in STAT_KEYS], np.int64))


def compute(case):
    """The arrays of one case, from whatever build of the library is loaded."""
    options = ()
    if case == "metric":
        z0, L = O.pendulum_inputs(256, seed=1)
        ts, dz, kw = O.time_grid(50), O.cotangent(50, 256, 2, seed=2), {}
    elif case in GRIDS:
        z0, L, ts, dz, kw = grid_inputs(case)
    else:
        z0, L, ts, dz, kw = P.case_inputs("metric_path_two_xcd_columns" if case in ("non_finite_row", "record_overflow") else case)
    if case == "non_finite_row":
        z0, L, dz = z0[:6].copy(), L[:6], np.ascontiguousarray(dz[:, :6])
        z0[2, 0] = np.inf
    if case == "record_overflow":
        options = (("record_capacity", 3),)
    nat, _ = D._native(None, **kw)
    for k, v in options:
        nat.set_option(k, v)
    z, ret, _ = nat.forward(z0, L, ts)
    g0, gth, _, sb = nat.adjoint(z, L, ts, dz)
    return _arrays(z, ret, g0, gth, sb)


def record(path, parent_commit, hipcc_version):
    """Write the golden file from the loaded build (run once, on the build of the commit before the trip became speculative)."""
    arrays = {"parent_commit": np.array(parent_commit), "hipcc_version": np.array(hipcc_version)}
    for case in BIT_CASES:
        for k, v in compute(case).items():
            arrays[f"{case}/{k}"] = v
    np.savez_compressed(path, **arrays)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("case", BIT_CASES)
def test_the_parents_bits(case):
    gold = _golden()
    got = compute(case)
    want = {k.split("/", 1)[1]: v for k, v in gold.items() if k.startswith(case + "/")}
    assert set(want) == set(got) and len(want) == 5
    nfailed = int(got["pullback_stats"][3])
    if case == "non_finite_row":
        assert nfailed == 1 and got["retcode"][2] != 0 and (got["dz0"][2] == 0).all() and got["dtheta"][2, 0] == 0
        assert np.abs(np.delete(got["dtheta"], 2, axis=0)).min() > 0
    elif case == "record_overflow":
        assert nfailed == len(got["dz0"]) and np.isnan(got["dz0"]).all() and np.isnan(got["dtheta"]).all()
    else:
        assert nfailed == 0 and (got["retcode"] == 0).all() and np.isfinite(got["dz0"]).all() and np.abs(got["dtheta"]).max() > 0
    bad = [k for k in sorted(want) if not _same_bytes(want[k], got[k])]
    assert not bad, f"{case}: {bad} differ from the bits of {gold['parent_commit']}"


def _ragged_steps_with_extra_trips(rec, ts):
    """Per trajectory, the steps of the kernel's record that hold more than twelve save times AND whose last save time is not where a
    uniform grid would have it (the kernel's own guess: csrc/lde_pendulum.hip, `jscale`)."""
    T = len(ts)
    jscale = float(T - 1) / (ts[-1] - ts[0])
    found = []
    for b, n in enumerate(rec["n"]):
        n = int(n)
        t = rec["t"][b, :n]
        tnew = np.append(t[1:], ts[-1])
        hits = []
        for s in range(n):
            true = T - 1 if s == n - 1 else int(np.searchsorted(ts, tnew[s], side="right")) - 1
            below = int(np.searchsorted(ts, t[s], side="right")) - 1          # the last save time ≤ t: not the step's
            guess = min(max(int((tnew[s] - ts[0]) * jscale + 1e-6), 0), T - 1)
            if true - below > 12 and guess != true:
                hits.append(s)
        found.append(hits)
    return found


def _run_grid(name, o32, o64, options=()):
    z0, L, ts, dz, kw = grid_inputs(name)
    nat, od = D._native(None, **kw)
    for k, v in options:
        nat.set_option(k, v)
    z, rec, g, st, sb = D._check(nat, od, o32, o64, z0, L, ts, dz, None)
    P._assert_pullback_statistics(rec, sb, 6)
    return rec, g, ts


@pytest.mark.parametrize("name", list(GRIDS))
def test_discarded_speculative_trip_redone_and_continued(o32, o64, name):
    rec, _, ts = _run_grid(name, o32, o64)
    hits = _ragged_steps_with_extra_trips(rec, ts)
    print(name, "steps per trajectory", rec["n"], "ragged steps with more than 12 save times", hits)
    assert sum(len(h) for h in hits) >= 1, hits
    if name != "dense_head_then_quadratic":
        assert len(ts) > 64
    if name == "cubic121_tight":       # three rounds of 21 steps: the paths above in rounds r > 0
        assert int(rec["n"].min()) > 42


def test_the_two_mappings_agree_on_such_a_grid(o32, o64):
    _, tp, _ = _run_grid("cubic121", o32, o64)
    _, lane, _ = _run_grid("cubic121", o32, o64, options=(("pend_disc_tp_max_b", 0),))
    assert D._rel(tp[0], lane[0]) <= 1e-5 and D._rel(tp[1], lane[1]) <= 1e-5, (D._rel(tp[0], lane[0]), D._rel(tp[1], lane[1]))
