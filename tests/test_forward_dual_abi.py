"""CPU: the C ABI and the Python tags of LDE_SENSE_FORWARD_DUAL — the dual-number solve that gives the reference's training-time answer
(include/lde.h). Where it is served, lde_create accepts it (LDE_OK on a GPU box, LDE_ERR_NO_DEVICE without one — never an invalid
argument); elsewhere it is LDE_ERR_UNSUPPORTED with a text that names the missing piece. The default mappings stay LDE_SENSE_DISCRETE."""
import ctypes as C

import pytest


def _desc(**kw):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    d.sensealg = L.SENSE_FORWARD_DUAL
    layers = kw.pop("layers", ())
    d.n_layers = max(len(layers) - 1, 0)
    for i, s in enumerate(layers):
        d.layer_sizes[i] = s
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _create(d):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    h = C.c_void_p()
    rc = lib.lde_create(C.byref(d), C.byref(h))
    if h.value:
        lib.lde_destroy(h)
    assert rc != 0 or h.value, "LDE_OK must come with a handle"
    return rc


@pytest.mark.parametrize("case", ["pendulum", "friction", "rk4_fixed", "tsit5_fixed"])
def test_served_descriptions_are_accepted(case):
    from latentdiffeq_amd import _lib as L
    kw = {"pendulum": {}, "friction": dict(rhs_kind=L.RHS_PENDULUM_FRICTION),
          "rk4_fixed": dict(solver=L.SOLVER_RK4, adaptive=0, dt=0.013), "tsit5_fixed": dict(adaptive=0, dt=0.02)}[case]
    d = _desc(**kw)
    assert L.load().lde_desc_error(C.byref(d)) == b""
    assert _create(d) in (0, -3)          # LDE_OK (GPU box) or LDE_ERR_NO_DEVICE (CPU box); never LDE_ERR_INVALID_ARG


@pytest.mark.parametrize("case", ["mlp", "pendulum_plus_mlp", "coupled", "mlp_per_trajectory"])
def test_unserved_descriptions_are_unsupported_and_say_why(case):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    mlp = dict(rhs_kind=L.RHS_MLP, state_dim=4, param_dim=0, layers=(4, 16, 4), batching=L.BATCH_COUPLED)
    kw = {"mlp": mlp,
          "mlp_per_trajectory": dict(mlp, batching=L.BATCH_PER_TRAJECTORY),
          "pendulum_plus_mlp": dict(rhs_kind=L.RHS_PENDULUM_PLUS_MLP, layers=(2, 16, 2)),
          "coupled": dict(batching=L.BATCH_COUPLED)}[case]
    d = _desc(**kw)
    assert _create(d) == -2               # LDE_ERR_UNSUPPORTED
    why = lib.lde_desc_error(C.byref(d)).decode()
    assert "LDE_SENSE_FORWARD_DUAL" in why
    assert ("MLP" in why) if "mlp" in case else ("LDE_BATCH_PER_TRAJECTORY" in why), why


def test_sensealg_range_and_default_unchanged():
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = _desc(sensealg=5)
    assert _create(d) == -1 and lib.lde_desc_error(C.byref(d)) == b"unknown sensealg"
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    assert d.sensealg == L.SENSE_DISCRETE == 3 and L.SENSE_FORWARD_DUAL == 4
    assert lib.lde_desc_error(C.byref(d)) == b""


def test_python_tags():
    import latentdiffeq_amd as la
    assert la.ForwardDiffSensitivity(dual_norm=True).code == 4
    assert la.ForwardDiffSensitivity().code == 3 and la.ForwardDiffSensitivity(dual_norm=False).code == 3
    assert la.Pendulum().sensealg.code == 3 and la.Pendulum_friction().sensealg.code == 3
    p = la.Pendulum(sensealg=la.ForwardDiffSensitivity(dual_norm=True))
    assert p.sensealg.code == 4 and p.sensealg.dual_norm


def test_node_with_the_dual_sensealg_raises_at_handle_creation_with_the_librarys_text():
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    n = la.NODE(4, hidden_dim=8, sensealg=la.ForwardDiffSensitivity(dual_norm=True))
    with pytest.raises(L.LdeError, match=r"LDE_ERR_UNSUPPORTED: LDE_SENSE_FORWARD_DUAL: no MLP right-hand side"):
        n._native()
    pn = la.PendulumNODE(hidden_dim=8, sensealg=la.ForwardDiffSensitivity(dual_norm=True))
    with pytest.raises(L.LdeError, match=r"LDE_SENSE_FORWARD_DUAL"):
        pn._native()
