"""CPU: the exact-input cases of tests/test_gpu_chain_exact.py are fair and not vacuous — on the float64 restatement alone
(tests/chain_exact_ref.py), no GPU. Every case of the table holds every condition: no skip, no expected failure, no share of exempt
cases. A (k, seed) pair that fails is replaced in the table."""
import numpy as np
import pytest

from tests import chain_exact_ref as E


def test_the_table_holds_every_case_the_gpu_legs_ask_for():
    want = [("edge", s, N) for s in E.SPECS for N in E.EDGE_N]
    want += [("switch", s, N) for s in ("reconstructor", "feature_extractor") for N in E.SWITCH_N]
    want += [("switch", "one", N) for N in (12224, 12225)]
    want += [("walk", s, N) for s in E.WALK_SPECS for N in E.WALK_N]
    assert sorted(want) == sorted((c.leg, c.spec, c.N) for c in E.TABLE)
    for s in E.WALK_SPECS:                                   # a different draw per call of the walk
        seeds = [c.seed for c in E.cases("walk", s)]
        assert len(set(seeds)) == len(E.WALK_N)
    for sizes, acts, skips in E.SPECS.values():
        assert set(acts) <= {E.R, E.I} and len(acts) == len(skips) == len(sizes) - 1


@pytest.mark.parametrize("case", E.TABLE, ids=lambda c: f"{c.leg}-{c.spec}-{c.N}")
def test_case_holds_its_conditions(case):
    got = E.conditions(case)
    assert got == dict(exact=True, order_free=True, storable=True, contributes=True), (case, got)


@pytest.mark.parametrize("spec", sorted(E.SPECS))
def test_accumulating_onto_small_integers_stays_exact(spec):
    """Leg (d) of the GPU file: dW0 + dW is exact in f32 in any order of its partial sums."""
    for N in (17, 129):
        case = E.case("edge", spec, N)
        dW0 = E.accumulation_base(case)
        assert E.accumulation_is_exact(case) and np.abs(dW0).max() <= E.ACC_MAX and np.array_equal(dW0, np.rint(dW0)) and dW0.size == E.reference(case)[2].size


def test_generator_draws_what_it_says():
    sizes = (40, 100, 100, 12)
    W, x, dy = E.exact_inputs(sizes, 33, 5, 3)
    for Wl, b in E._split(sizes, W):
        assert ((Wl != 0).sum(axis=1) == 3).all() and set(np.unique(Wl)) <= {-1.0, -0.5, 0.0, 0.5, 1.0} and set(np.unique(b)) <= {-1.0, 0.0, 1.0}
    assert set(np.unique(x)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(np.unique(dy * 2.0 ** 10)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert x.any(axis=1).all() and dy.any(axis=1).all()
    W2, x2, _ = E.exact_inputs(sizes, 17, 5, 3)              # the weights do not depend on N, the data do
    assert np.array_equal(W, W2) and not np.array_equal(x[:17], x2)
    Wn, _, _ = E.exact_inputs((2, 200, 784), 4, 1, 3)        # narrower than k: every entry of the row
    assert ((E._split((2, 200, 784), Wn)[0][0] != 0).sum(axis=1) == 2).all()


def test_bf16_rounding_and_the_grain():
    a = np.array([1.0, 1.00390625, 1.01171875, 255.0, 257.0, -0.75, 3.0 * 2.0 ** -14], np.float32)   # 1 + 2⁻⁸ ties to even (down), 1 + 3·2⁻⁸ up
    assert np.array_equal(E.bf16r(a), np.array([1.0, 1.0, 1.015625, 255.0, 256.0, -0.75, 3.0 * 2.0 ** -14], np.float32))
    assert E._grain(np.array([0.0, 1.5, -0.25, 6.0])) == 0.25 and E._grain(np.zeros(3)) == 1.0


def _differs(case, fault, what):
    sizes, acts, skips, W, x, dy = E.case_inputs(case)
    bad = E.chain_ref_full(sizes, acts, skips, W, x, dy, E.identity, fault=fault)
    ref = dict(zip(("y", "dx", "dW"), E.reference(case)))
    return not np.array_equal(bad[what].astype(np.float32), ref[what])


@pytest.mark.parametrize("spec", sorted(E.SPECS))
@pytest.mark.parametrize("N", [1, 65, 129])
def test_a_dropped_row_of_any_weight_gradient_product_changes_a_compared_bit(spec, N):
    """Leg (a) compares dW bit for bit: the product of ANY layer without its last row n (a ragged chunk's tail, the last part) is seen."""
    case = E.case("edge", spec, N)
    for l in range(len(E.SPECS[spec][0]) - 1):
        assert _differs(case, ("dw_row", l), "dW"), (spec, N, l)


def test_a_dropped_k_group_of_the_784_wide_layer_changes_a_compared_bit():
    """784 = 24·32 + 16: the feature extractor's first product (y, and everything behind it) and the reconstructor's last
    input-gradient product (dx) without the ragged K-group."""
    for N in (1, 17, 64):
        assert _differs(E.case("edge", "feature_extractor", N), ("kgroup",), "y")
        assert _differs(E.case("edge", "feature_extractor", N), ("kgroup",), "dW")
        assert _differs(E.case("edge", "reconstructor", N), ("kgroup",), "dx")
    assert _differs(E.case("switch", "feature_extractor", 6113), ("kgroup",), "y")


@pytest.mark.parametrize("spec", sorted(E.SPECS))
def test_a_zeroed_last_column_of_dx_changes_a_compared_bit(spec):
    for N in (1, 17, 33, 129):
        assert _differs(E.case("edge", spec, N), ("dx_col",), "dx"), (spec, N)     # (at every other N too: `contributes` says row N − 1 of dx is not zero)
