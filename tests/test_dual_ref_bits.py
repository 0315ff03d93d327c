"""CPU: the numpy references of the dual-number solves (tests/lv_ref.py, tests/kuramoto_ref.py, tests/dpend_ref.py — thin wrappers over the one
solve of tests/dual_ref.py) return the BITS that the three modules returned when each carried its own copy of the stepping loop.

tests/golden/dual_parent_bits_ref.npz was recorded by `record()` below from the modules of the commit named in its `parent_commit` entry.
Every array is compared as raw bytes, no tolerance: ẑ, the row of J named in J_ROWS (the file is kept to a few tens of kB; the gradients,
which sum over every row, are whole), the return codes, the three counts of `info`, every trajectory's accepted `t` / `dt` (concatenated,
with their lengths), dz0 and dθ of `pullback`. A difference is a finding about the order of numpy operations in tests/dual_ref.py.

Cases: {lv, Kuramoto at N = 2, 3, 7, the double pendulum} × {float64, float32} × {Tsit5 adaptive, Tsit5 at dt = 0.05, RK4 at dt = 0.05} on
B = 3 and the nine-point ragged grid; per module (Kuramoto at N = 3) and precision one replay of the adaptive solve's steps (`steps=`) and
one failing solve (maxiters = 3)."""
import functools
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dual_parent_bits_ref.npz")
B = 3
J_ROWS = [8]                    # of the nine: the last
SIZE_LIMIT = 80_000
RET_MAXITERS = 1

SYSTEMS = ("lv", "n2", "n3", "n7", "dp")
SOLVES = {"tsit5_adaptive": dict(), "tsit5_fixed": dict(adaptive=False, dt=0.05), "rk4_fixed": dict(solver=1, adaptive=False, dt=0.05)}
DTYPES = {"f64": np.float64, "f32": np.float32}
CASES = ([f"{s}-{v}-{d}" for s in SYSTEMS for v in SOLVES for d in DTYPES]
         + [f"{s}-{v}-{d}" for s in ("lv", "n3", "dp") for v in ("replay", "fails") for d in DTYPES])


def _system(name):
    """(module, inputs(B), cotangent(T, B)) of a case's system."""
    if name == "lv":
        from tests import lv_ref as R
        return R, lambda: R.inputs(B, seed=9), lambda T: R.cotangent(T, B)
    if name == "dp":
        from tests import dpend_ref as R
        return R, lambda: R.inputs(B, seed=R.RAGGED_SEED), lambda T: R.cotangent(T, B)
    from tests import kuramoto_ref as R
    N = int(name[1:])
    return R, lambda: R.inputs(B, N, seed=9 + N), lambda T: R.cotangent(T, B, N)


def compute(case):
    """The arrays of one case, from whatever reference modules are importable."""
    from tests.lv_ref import ragged_grid
    name, what, prec = case.split("-")
    R, inputs, cotangent = _system(name)
    dtype = DTYPES[prec]
    ts = ragged_grid()
    z0, th = inputs()
    if what == "replay":
        info = R.solve(z0, th, ts, dtype=dtype)[3]
        kw = dict(steps=(info["t"], info["dt"]))
    else:
        kw = dict(maxiters=3) if what == "fails" else SOLVES[what]
    z, J, ret, info = R.solve(z0, th, ts, dtype=dtype, **kw)
    dz0, dth = R.pullback(J, cotangent(len(ts)))
    return dict(z=z, J=J[J_ROWS], ret=ret, counts=np.array([info[k] for k in ("nfe", "naccept", "nreject")], np.int64),
                steps_n=np.array([len(t) for t in info["t"]], np.int64), steps_t=np.concatenate(info["t"]).astype(np.float64),
                steps_dt=np.concatenate(info["dt"]).astype(np.float64), dz0=dz0, dtheta=dth)


def record(path, parent_commit):
    """Write the golden file from the importable modules (run once, on the commit before the three loops became one)."""
    arrays = {"parent_commit": np.array(parent_commit)}
    for case in CASES:
        arrays[case] = _pack(compute(case))
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= SIZE_LIMIT, os.path.getsize(path)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _pack(arrays):
    """A case's arrays as ONE entry of the file (an entry of an .npz costs more than most of these arrays hold): a line that names every
    array's dtype and shape, then their bytes in that order."""
    items = [(k, np.ascontiguousarray(arrays[k])) for k in sorted(arrays)]
    head = ";".join(f"{k}:{v.dtype.str}:{v.shape}" for k, v in items) + "\n"
    return np.frombuffer(head.encode() + b"".join(v.tobytes() for _, v in items), np.uint8)


def _differing(want, arrays):
    """The names of the arrays whose dtype, shape or bytes are not the packed `want`'s."""
    raw = want.tobytes()
    head, body = raw.split(b"\n", 1)
    bad, off = [], 0
    for entry in head.decode().split(";"):
        k, dt, shape = entry.split(":")
        v = np.ascontiguousarray(arrays[k])
        n = int(np.prod(eval(shape), dtype=np.int64)) * np.dtype(dt).itemsize
        if v.dtype.str != dt or str(v.shape) != shape or v.tobytes() != body[off:off + n]:
            bad.append(k)
        off += n
    return bad


def test_the_file_is_small_and_names_its_commit():
    assert os.path.getsize(GOLDEN) <= SIZE_LIMIT and str(_golden()["parent_commit"])


@pytest.mark.parametrize("case", CASES)
def test_the_parents_bits(case):
    gold = _golden()
    got = compute(case)
    assert len(got) == 9
    name, what, prec = case.split("-")
    assert got["z"].dtype == DTYPES[prec] and got["J"].dtype == DTYPES[prec]
    if what == "fails":
        assert (got["ret"] == RET_MAXITERS).all() and np.isnan(got["z"]).all() and (got["J"] == 0).all() and (got["dz0"] == 0).all()
    else:
        assert (got["ret"] == 0).all() and np.isfinite(got["z"]).all() and np.abs(got["J"]).max() > 0 and got["steps_n"].min() >= 2
    bad = [] if np.array_equal(gold[case], _pack(got)) else _differing(gold[case], got) or ["the names of the arrays"]
    assert not bad, f"{case}: {bad} differ from the bits of {gold['parent_commit']}"
