"""CPU: tests/_general_bounds.py pinned against HiGHS alone, so that the device tests of K16s at general bounds
(tests/test_gpu_crossover_band_bounds.py) and the sharded re-solve's (tests/test_dist_gloo.py) never stand on an
unchecked transformation."""
import numpy as np
import pytest

import workloads
from _general_bounds import affine_image, column_kinds, free_some, highs, map_basis, map_vertex

OPT = -575.0012961276          # HiGHS on netlib_lp(400, 1600, seed=11)


@pytest.fixture(scope="module")
def base():
    inst = workloads.netlib_lp(400, 1600, seed=11)
    ref = highs(inst)
    assert ref.status == 0 and ref.fun == pytest.approx(OPT, rel=1e-10)
    return inst, ref


def test_image_has_the_optimum_of_the_original_and_every_kind_of_column(base):
    inst, ref = base
    image, d, t, const = affine_image(inst, 12)
    assert np.array_equal(image.A.indptr, inst.A.indptr) and np.array_equal(image.A.indices, inst.A.indices)   # same pattern
    assert image.A.has_sorted_indices
    kinds = column_kinds(image)
    assert kinds == {"lower_only": 581, "upper_only": 614, "boxed": 405, "free": 0, "nonzero_lower": 591}
    assert np.count_nonzero((image.l < 0) & (image.u > 0) & np.isfinite(image.l) & np.isfinite(image.u)) > 0    # boxes that straddle 0
    got = highs(image)
    assert got.status == 0
    assert got.fun + const == pytest.approx(ref.fun, rel=1e-9)
    np.testing.assert_allclose(map_vertex(ref.x, d, t), got.x, rtol=1e-6, atol=1e-7)
    # the vertex mapped back and forth
    np.testing.assert_allclose(d * got.x + t, ref.x, rtol=1e-6, atol=1e-7)


def test_mapped_point_is_a_complementary_pair_of_the_image(base):
    """(x', y') = (d * (x - t), y): feasible and complementary for the image to the generator's 1e-9."""
    inst, _ = base
    image, d, t, const = affine_image(inst, 12)
    x, y = image.x, image.y
    lt = image.sense == "<"
    s = image.b - image.A @ x
    assert np.abs(s[~lt]).max() <= 1e-9 and s[lt].min() >= -1e-9
    assert np.all(x >= image.l) and np.all(x <= image.u)
    assert np.all(y[lt] <= 1e-9) and np.abs(s * y).max() <= 1e-9                      # rows
    rc = image.c - image.A.T @ y
    to_l, to_u = x - image.l, image.u - x                                            # (inf where there is no bound)
    assert np.all(to_l[rc > 1e-9] <= 1e-9 * (1 + 1e-6)) and np.all(to_u[rc < -1e-9] <= 1e-9 * (1 + 1e-6))
    assert float(image.c @ x) + const == pytest.approx(float(inst.c @ inst.x), rel=1e-12)
    # codes: a mirrored column swaps 'at lower' and 'at upper'
    vb = np.array([-1, -2, 0, -1, -2, 0], dtype=np.int8)
    dd = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])
    assert map_basis(vb, dd).tolist() == [-1, -2, 0, -2, -1, 0]


@pytest.mark.parametrize("col,want", [(439, -702.0472810), (500, -603.1253830), (1001, None)])
def test_a_freed_non_basic_column_with_positive_reduced_cost_improves_the_optimum(base, col, want):
    """The three columns sit at l = 0 with reduced cost +1.37 / +0.66 / +0.62 at the optimum: with the lower bound gone
    they move DOWN -- a solver that prices free columns in one direction only keeps -575.00."""
    inst, ref = base
    lt = inst.sense == "<"
    y = np.zeros(lt.size)
    y[lt], y[~lt] = ref.ineqlin.marginals, ref.eqlin.marginals
    rc = inst.c - inst.A.T @ y
    assert ref.x[col] == 0.0 and rc[col] > 0.6
    got = highs(free_some(inst, [col]))
    if want is None:
        assert got.status == 3                                                        # unbounded
    else:
        assert got.status == 0 and got.fun == pytest.approx(want, rel=1e-9) and got.fun < ref.fun - 1.0


def test_freeing_basic_columns_leaves_the_optimum_where_it_is(base):
    inst, ref = base
    m = inst.A.shape[0]
    basic = np.flatnonzero((ref.x > inst.l + 1e-7) & (ref.x < inst.u - 1e-7))
    cols = np.random.default_rng(3).choice(basic, m // 50, replace=False)
    got = highs(free_some(inst, cols))
    assert got.status == 0 and got.fun == pytest.approx(ref.fun, rel=1e-9)
