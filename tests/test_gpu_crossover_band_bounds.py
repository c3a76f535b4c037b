"""GPU: the sparse crossover (K16s, csrc/sx_crossover_band.hip) at GENERAL column bounds.  Every generator of workloads.py
draws l = 0 with u = inf or a positive finite u, so tests/test_gpu_crossover_band.py never reaches the 'at upper' branches,
the placement of a non-basic column without the bound its code names, right-hand sides b - A_N x_N with x_N != 0, columns
fixed at a non-zero value, or free columns.  Here the same LPs are seen through x = d * x' + t (tests/_general_bounds.py,
pinned against HiGHS alone by tests/test_general_bounds_cpu.py), with columns fixed and freed on top.  The reference
everywhere is HiGHS (scipy.optimize.linprog) on the very LP handed to the device, objectives at rel = abs = 1e-8 (the
figure of tests/test_gpu_crossover_band.py), plus a certificate that knows the four kinds of bounds.

Conventions pinned (include/sxhip.h): a non-basic column rests at the bound its code names
(-1 lower, -2 upper), at the other one when that bound is infinite, at 0 when both are; a non-basic free column is
REPORTED as -3 (at 0, reduced cost 0 within the tolerance) and prices in both directions."""
import dataclasses
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import workloads
from _general_bounds import affine_image, column_kinds, fix_some, free_some, highs, map_basis, map_vertex

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_crossover_band import direct, perturbed_sub_problem, resolve   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from smart_crossover.hip import default_context
    return default_context()


def general_certificate(lp, x, y, vb, cb, tol=1e-6):
    """Optimality of (x, y, basis) for min c x, A x (= | <=) b, l <= x <= u with any mix of finite and infinite bounds."""
    A, b, c, l, u = lp.A, lp.b, lp.c, lp.l, lp.u
    lt = np.asarray(lp.sense) == "<"
    vb, cb = np.asarray(vb).astype(int), np.asarray(cb).astype(int)
    m = A.shape[0]
    s_p = b - A @ x
    assert np.abs(s_p[~lt]).max(initial=0.0) <= tol and s_p[lt].min(initial=0.0) >= -tol
    assert np.all(x >= l - 1e-9) and np.all(x <= u + 1e-9)
    lo, up, sup = vb == -1, vb == -2, vb == -3
    assert np.all((vb == 0) | lo | up | sup)
    assert np.all(np.isfinite(l[lo])) and np.all(np.isfinite(u[up])), "a column reported at an infinite bound"
    assert np.all(x[lo] == l[lo]) and np.all(x[up] == u[up])                      # non-basic: AT the bound, exactly
    free = np.isinf(l) & np.isinf(u)
    assert not np.any(sup & ~free), "-3 on a column that has a bound"
    assert np.all(x[sup] == 0.0)
    rc = c - A.T @ y
    fixed = l == u                                                                # (a fixed column prices at any sign)
    assert np.all(rc[lo & ~fixed] >= -tol) and np.all(rc[up & ~fixed] <= tol)
    assert np.abs(rc[vb == 0]).max(initial=0.0) <= tol and np.abs(rc[sup]).max(initial=0.0) <= tol
    assert np.all(y[lt & (cb == -1)] <= tol) and np.abs(y[cb == 0]).max(initial=0.0) <= tol
    assert int(np.count_nonzero(vb == 0) + np.count_nonzero(cb == 0)) == m


def call(ctx, lp, x_start, vb=None, cb=None, c=None):
    lt = np.asarray(lp.sense) == "<"
    return direct(ctx, lp.A, lp.b, lp.c if c is None else c, lp.l, lp.u, lt, x_start, vb, cb)


def optimum(lp):
    ref = highs(lp)
    assert ref.status == 0
    return ref


def duals(lp, ref):
    lt = np.asarray(lp.sense) == "<"
    y = np.zeros(lt.size)
    y[lt], y[~lt] = ref.ineqlin.marginals, ref.eqlin.marginals
    return y


# ---------------------------------------------------------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def small():
    """netlib_lp(400, 1600, seed=11), its image (kinds from seed 12) and HiGHS on both."""
    inst = workloads.netlib_lp(400, 1600, seed=11)
    image, d, t, const = affine_image(inst, 12)
    kinds = column_kinds(image)
    assert kinds["upper_only"] > 500 and kinds["nonzero_lower"] > 500 and kinds["boxed"] > 300
    ref, ref_image = optimum(inst), optimum(image)
    assert ref_image.fun + const == pytest.approx(ref.fun, rel=1e-9)
    return dict(inst=inst, image=image, d=d, t=t, ref=ref, ref_image=ref_image)


@pytest.fixture(scope="module")
def small_image_vertex(ctx, small):
    """Case 1's run, shared: the image from its mapped interior point (guessed entry)."""
    image = small["image"]
    return call(ctx, image, image.x)


@pytest.fixture(scope="module")
def small_vertex(ctx, small):
    """The ORIGINAL 400 x 1,600 LP from its interior point: the optimal basis case 6 starts from."""
    inst = small["inst"]
    return call(ctx, inst, inst.x)


# ------------------------------------------------------------------------------------------------------------ 1, 2: guessed
def test_guessed_start_on_the_image_reaches_highs_optimum(small, small_image_vertex):
    """The mirrored twin of test_direct_call_from_a_poor_start_reaches_highs_optimum: 614 upper-only columns, 591 non-zero
    lower bounds -- phase 1 and the pushes of the superbasic columns run mostly through the 'at upper' branches."""
    image = small["image"]
    res, x, y, vb, cb = small_image_vertex
    assert int(res.status) == 0
    assert float(image.c @ x) == pytest.approx(small["ref_image"].fun, rel=1e-8, abs=1e-8)
    general_certificate(image, x, y, vb, cb)
    assert np.count_nonzero(vb == -2) > 100 and np.count_nonzero(vb == -1) > 100


@pytest.mark.parametrize("seed,scale", [(4, 0.3), (5, 1.0)])
def test_another_cost_on_the_image_brings_columns_in_from_both_bounds(ctx, small, seed, scale):
    """The twin of test_another_cost_brings_columns_in_by_pricing, u = 30 applied BEFORE the map: every column is a box at
    shifted bounds, and the columns the new optimum needs rest at their lower AND at their upper bounds at the start."""
    inst = small["inst"]
    rng = np.random.default_rng(seed)
    c = inst.c + scale * rng.standard_normal(inst.c.size)
    u = np.where(np.isinf(inst.u), 30.0, inst.u)
    boxed = dataclasses.replace(inst, c=c, u=u, x=np.clip(inst.x, inst.l, u))
    image, d, t, const = affine_image(boxed, 12)
    assert column_kinds(image)["boxed"] == c.size
    start = image.x
    res, x, y, vb, cb = call(ctx, image, start)
    assert int(res.status) == 0
    assert int(res.phase1_iters) > 0        # (the field counts the columns that pricing brought into the tableau)
    was_low, was_up = np.abs(start - image.l) <= 1e-6, np.abs(image.u - start) <= 1e-6
    assert np.count_nonzero(was_low & (x > image.l + 1e-6)) > 0 and np.count_nonzero(was_up & (x < image.u - 1e-6)) > 0
    assert float(image.c @ x) == pytest.approx(optimum(image).fun, rel=1e-8, abs=1e-8)
    general_certificate(image, x, y, vb, cb)


# -------------------------------------------------------------------------------------------------------- 3: given basis
def test_a_given_optimal_basis_mapped_to_the_image_needs_no_pivot(ctx):
    """The optimal basis of the ORIGINAL 1,200 x 6,000 LP mapped through (d, t) and handed to sx_crossover_band_basis_dev on
    the image: the right-hand side of the basic solution is b' - A'_N x'_N with x'_N != 0 almost everywhere, and a code
    names the bound of a column that has only the other one never (the map swaps -1 / -2 on mirrored columns) -- 0
    iterations, the same codes, x' = d * (x0 - t).  Then members swapped (declared at lower: on upper-only columns that
    is the bound they do not have) and members missing: a few pivots back to HiGHS' optimum of the image."""
    inst = workloads.netlib_lp(1200, 6000, seed=21)
    image, d, t, const = affine_image(inst, 22)
    first = call(ctx, inst, inst.x)
    assert int(first[0].status) == 0 and int(first[0].iters) > 0
    _, x0, y0, vb0, cb0 = first
    xm, vbm = map_vertex(x0, d, t), map_basis(vb0, d)
    res, x, y, vb, cb = call(ctx, image, xm, vbm, cb0)
    assert int(res.status) == 0 and int(res.iters) == 0 and int(res.warm_start_used) == 1
    assert np.array_equal(vb, vbm) and np.array_equal(cb, cb0)
    np.testing.assert_allclose(x, xm, rtol=1e-9, atol=1e-9)
    general_certificate(image, x, y, vb, cb)
    want = optimum(image).fun
    assert float(image.c @ x) == pytest.approx(want, rel=1e-8, abs=1e-8)
    rng = np.random.default_rng(4)
    # (a) members swapped: 15 basic columns declared non-basic at their lower bound, 15 non-basic ones declared basic
    vb1 = vbm.copy()
    out_ = rng.choice(np.flatnonzero(vbm == 0), 15, replace=False)
    in_ = rng.choice(np.flatnonzero(vbm != 0), 15, replace=False)
    assert np.count_nonzero(np.isinf(image.l[out_])) > 0          # 'at lower' of a column without a lower bound: placed at u
    vb1[out_], vb1[in_] = -1, 0
    res, x, y, vb, cb = call(ctx, image, xm, vb1, cb0)
    assert int(res.status) == 0 and int(res.iters) > 0
    assert float(image.c @ x) == pytest.approx(want, rel=1e-8, abs=1e-8)
    general_certificate(image, x, y, vb, cb)
    # (b) members missing: 25 basic columns dropped and nothing put in their place
    vb2 = vbm.copy()
    vb2[rng.choice(np.flatnonzero(vbm == 0), 25, replace=False)] = -2
    res, x, y, vb, cb = call(ctx, image, xm, vb2, cb0)
    assert int(res.status) == 0
    assert float(image.c @ x) == pytest.approx(want, rel=1e-8, abs=1e-8)
    general_certificate(image, x, y, vb, cb)


# ------------------------------------------------------------------------------------------------------- 4: fixed columns
@pytest.mark.parametrize("entry", ["guessed", "given"])
def test_columns_fixed_at_non_zero_values_stay_there(ctx, small, small_image_vertex, entry):
    """5 % of the columns, all non-basic at a NON-ZERO bound of the image (reduced cost well away from 0, so in every
    optimal basis), get l = u at that value: the same optimum, the fixed columns keep their value exactly and are never
    basic."""
    image, ref = small["image"], small["ref_image"]
    rc = image.c - image.A.T @ duals(image, ref)
    at_l = (np.abs(ref.x - image.l) <= 1e-9) & (image.l != 0) & (rc > 1e-2)
    at_u = (np.abs(image.u - ref.x) <= 1e-9) & (image.u != 0) & (rc < -1e-2)
    assert np.count_nonzero(at_l) > 100 and np.count_nonzero(at_u) > 100
    cols = np.sort(np.random.default_rng(6).choice(np.flatnonzero(at_l | at_u), image.c.size // 20, replace=False))
    assert np.count_nonzero(at_l[cols]) > 10 and np.count_nonzero(at_u[cols]) > 10
    fixed = fix_some(image, cols, ref.x)
    assert np.all(fixed.l[cols] == fixed.u[cols]) and np.all(fixed.l[cols] != 0)
    want = optimum(fixed).fun
    assert want == pytest.approx(ref.fun, rel=1e-9)
    if entry == "guessed":
        res, x, y, vb, cb = call(ctx, fixed, np.clip(image.x, fixed.l, fixed.u))
    else:
        r0, x0, y0, vb0, cb0 = small_image_vertex
        assert int(r0.status) == 0
        res, x, y, vb, cb = call(ctx, fixed, x0, vb0, cb0)
        assert int(res.warm_start_used) == 1
    assert int(res.status) == 0
    assert float(fixed.c @ x) == pytest.approx(want, rel=1e-8, abs=1e-8)
    assert np.all(x[cols] == fixed.l[cols]) and not np.any(vb[cols] == 0)
    general_certificate(fixed, x, y, vb, cb)


# --------------------------------------------------------------------------------------------------------- 5, 6: free columns
def test_freed_basic_columns_end_basic_at_the_same_optimum(ctx, small):
    image, ref = small["image"], small["ref_image"]
    m = image.A.shape[0]
    basic = np.flatnonzero((ref.x > image.l + 1e-7) & (ref.x < image.u - 1e-7))
    cols = np.random.default_rng(3).choice(basic, m // 50, replace=False)
    freed = free_some(image, cols)
    want = optimum(freed).fun
    assert want == pytest.approx(ref.fun, rel=1e-9)
    res, x, y, vb, cb = call(ctx, freed, image.x)
    assert int(res.status) == 0
    assert float(freed.c @ x) == pytest.approx(want, rel=1e-8, abs=1e-8)
    assert np.all(vb[cols] == 0)
    general_certificate(freed, x, y, vb, cb)


# column, code it has in the optimal basis of the original LP, HiGHS' optimal value once it is free (None: unbounded).
# 439 / 500 / 1001 rest at l = 0 with reduced costs +1.37 / +0.66 / +0.62; 81 rests at u = 5.86 with reduced cost -0.59
FREED = [(439, -1, -702.0472810), (500, -1, -603.1253830), (1001, -1, None), (81, -2, -646.5444022)]


@pytest.mark.parametrize("col,code,want", FREED)
def test_a_free_non_basic_column_enters_in_the_direction_its_reduced_cost_names(ctx, small, small_vertex, col, code, want):
    """The optimal basis of the original LP handed back with ONE non-basic column freed, its code unchanged.  A free column
    rests at 0 whatever its code says and moves either way: 439, 500 and 1001 have to move DOWN from where their lower
    bound was (reduced cost > 0 -- a pricing that reads 'at lower: only d < 0 may enter' returns the old vertex, -575.00,
    as optimal), 81 UP past where its upper bound was (8 columns away the LP is unbounded: 1001)."""
    inst, ref = small["inst"], small["ref"]
    r0, x0, y0, vb0, cb0 = small_vertex
    assert int(r0.status) == 0 and float(inst.c @ x0) == pytest.approx(ref.fun, rel=1e-8, abs=1e-8)
    # the basis is the optimum's: the duals are HiGHS' (they are unique: its vertex is not degenerate), hence the signs
    np.testing.assert_allclose(y0, duals(inst, ref), rtol=1e-6, atol=1e-7)
    rc = inst.c - inst.A.T @ y0
    assert vb0[col] == code and (rc[col] > 0.6 if code == -1 else rc[col] < -0.3)
    freed = free_some(inst, [col])
    got = highs(freed)
    res, x, y, vb, cb = call(ctx, freed, x0, vb0, cb0)
    if want is None:
        assert got.status == 3 and int(res.status) == 2             # unbounded, both
        return
    assert got.status == 0 and got.fun == pytest.approx(want, rel=1e-9) and got.fun < ref.fun - 1.0
    assert int(res.status) == 0 and int(res.iters) > 0
    assert float(freed.c @ x) == pytest.approx(got.fun, rel=1e-8, abs=1e-8)
    general_certificate(freed, x, y, vb, cb)


def test_the_first_run_ends_on_highs_duals(small, small_vertex):
    """What the freed-column cases stand on: the basis they start from is optimal and its reduced costs are HiGHS'.
    (Not its vertex: the generator gives the m columns of its basis reduced costs of 1e-10, below any solver's
    tolerance, so the LP has a face of vertices that are optimal to 1e-7 -- measured: 353 of 1,600 entries of the device's
    vertex differ from HiGHS', by up to 10.2, at objectives equal to 1e-8.  HiGHS' vertex is not degenerate, so the duals
    are unique, and the reduced costs of the columns outside the face are the same at every one of those vertices.)"""
    inst, ref = small["inst"], small["ref"]
    r0, x0, y0, vb0, cb0 = small_vertex
    assert int(r0.status) == 0
    general_certificate(inst, x0, y0, vb0, cb0)
    assert float(inst.c @ x0) == pytest.approx(ref.fun, rel=1e-8, abs=1e-8)
    y_ref = duals(inst, ref)
    np.testing.assert_allclose(y0, y_ref, rtol=1e-6, atol=1e-7)
    rc, rc_ref = inst.c - inst.A.T @ y0, inst.c - inst.A.T @ y_ref
    away = np.abs(rc_ref) > 1e-3                      # the columns outside the optimal face: at the same bound in both
    assert np.count_nonzero(away) > 1000
    np.testing.assert_allclose(x0[away], ref.x[away], rtol=0, atol=1e-9)
    np.testing.assert_allclose(rc[away], rc_ref[away], rtol=1e-6, atol=1e-7)


def test_a_free_column_that_stays_out_is_reported_superbasic_at_zero(ctx, small, small_vertex):
    """A non-basic column whose reduced cost is 0 within the tolerance stays where it is when it is freed -- nothing to
    gain either way -- and comes back as -3 at x = 0.0: no bound to be 'at'."""
    inst, ref = small["inst"], small["ref"]
    r0, x0, y0, vb0, cb0 = small_vertex
    rc = inst.c - inst.A.T @ y0
    cand = np.flatnonzero((vb0 == -1) & (np.abs(rc) <= 1e-8) & (x0 == 0.0))
    assert cand.size > 0
    col = int(cand[0])
    freed = free_some(inst, [col])
    res, x, y, vb, cb = call(ctx, freed, x0, vb0, cb0)
    assert int(res.status) == 0 and int(res.iters) == 0
    assert vb[col] == -3 and x[col] == 0.0
    assert float(freed.c @ x) == pytest.approx(optimum(freed).fun, rel=1e-8, abs=1e-8)
    general_certificate(freed, x, y, vb, cb)


# ---------------------------------------------------------------------------------------------------------- 7: product path
@pytest.mark.parametrize("m,n,seed", [(300, 3000, 1), (3000, 30000, 2)])
def test_product_path_on_the_image(ctx, monkeypatch, m, n, seed):
    """get_perturb_problem, K16p and K16s as solve_lp runs them (the twin of test_band_crossover_reaches_the_vertex)."""
    from smart_crossover.lp_methods import algorithms as alg
    image, d, t, const = affine_image(workloads.netlib_lp(m, n, seed=seed), seed + 100)
    kinds = column_kinds(image)
    assert kinds["upper_only"] > n // 10 and kinds["nonzero_lower"] > n // 10
    lp, mgr = perturbed_sub_problem(image)
    caller, out = resolve(mgr, image, monkeypatch, "band")
    assert caller.solved_by == "crossover_band" and out.status == "OPTIMAL"
    sub = mgr.lp_sub
    general_certificate(sub, out.x, out.y, out.basis.vbasis, out.basis.cbasis)
    assert float(sub.c @ out.x) == pytest.approx(optimum(sub).fun, rel=1e-8, abs=1e-8)
    with redirect_stdout(io.StringIO()):
        assert alg.check_perturb_output_precision(mgr, out.x, lp.c, float(lp.c @ image.x)) is True   # gap < 1e-8
