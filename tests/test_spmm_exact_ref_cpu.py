"""The references of tests/spmm_exact_ref.py checked on the host: the dyadic case really is exact in any order (magnitudes below
2**53 grid units; numpy's and the oracle's f64 products equal the integer reference bit for bit; sample elements again in Python
integers), the bounded case has a 64-bit significand and bounds the oracle's own sequential sums, the hostile cases carry infinite
factors and the oracle's results for them are finite, and a non-finite panel row reaches exactly the vectors the reference says."""
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import scanrs_oracle as so  # noqa: E402
import spmm_exact_ref as er  # noqa: E402


@pytest.mark.parametrize("shape_i", range(len(er.WIDE_SHAPES)))
def test_dyadic_case_is_exact_in_any_order(shape_i):
    rows, cols, fill = er.WIDE_SHAPES[shape_i]
    case = er.dyadic_case(rows, cols, fill, 100 + shape_i)
    assert set(np.unique(case.dense[case.dense > 0]).tolist()) <= set(er.COUNT_SET)
    if rows * cols * fill > 2000:
        assert {8, 9, 15, 16, 255, 256, 300} <= set(np.unique(case.dense).tolist())
    rng = np.random.default_rng(shape_i)
    for name in er.DYADIC_MAPS:
        tf = np.ldexp(er.dyadic_terms(case, name).toarray().astype(np.float64), -er.GRID)
        o = er.dyadic_oracle(case, name)
        assert np.array_equal(o.to_dense(), tf), name  # the map built on a handle is the map of the integer terms
        for offset in (False, True):
            for side in ("dot", "rdot"):
                ref = er.dyadic_ref(case, name, side, max(er.WIDE_L), offset)
                assert int(ref.mag.max()) < 2 ** 53, (name, side, offset, int(ref.mag.max()).bit_length())
                if side == "dot":
                    full = tf @ case.x + ((case.u @ (case.v @ case.x)) if offset else 0.0)
                    perm = rng.permutation(cols)  # another order of the same sum
                    again = tf[:, perm] @ case.x[perm] + ((case.u @ (case.v[:, perm] @ case.x[perm])) if offset else 0.0)
                    orc = o.dot(case.x) + ((case.u @ (case.v @ case.x)) if offset else 0.0)
                else:
                    full = case.xl @ tf + (((case.xl @ case.u) @ case.v) if offset else 0.0)
                    perm = rng.permutation(rows)
                    again = case.xl[:, perm] @ tf[perm] + (((case.xl[:, perm] @ case.u[perm]) @ case.v) if offset else 0.0)
                    orc = o.rdot(case.xl) + (((case.xl @ case.u) @ case.v) if offset else 0.0)
                for got in (full, again, orc):
                    assert np.array_equal(er.bits(got), er.bits(ref.want)), (name, side, offset)
                for l in er.WIDE_L:  # a narrower panel is a slice of the same reference
                    part = er.dyadic_ref(case, name, side, l, offset).want
                    assert np.array_equal(part, ref.want[:, :l] if side == "dot" else ref.want[:l])
    # Python integers, sample elements
    small = er.dyadic_case(33, 97, 0.5, 100)
    for name in er.DYADIC_MAPS:
        for side, (i, k) in (("dot", (0, 3)), ("dot", (32, 104)), ("rdot", (5, 96)), ("rdot", (104, 0))):
            ref = er.dyadic_ref(small, name, side, 105, True)
            assert float(ref.want[i, k]) * 2.0 ** er.GRID == er.dyadic_ref_python(small, name, side, 105, True, i, k)


def _bounded_maps(dense, rng):
    rows, cols = dense.shape
    o = so.AdaptiveMat.from_dense(dense, so.CSR)
    fr, fc = rng.random(rows) + 0.5, rng.random(cols) + 0.5
    return {
        "log_normalize": so.log_normalize(o, None, so.LOG_TWO).ops,
        "cellranger": so.normalize(o, "cellranger").inner_sparse().ops,
        "scale0_log2_scale1": o.compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=0, a=fr)).apply(so.OP_LOG2_1P).compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=1, a=fc)).ops,
        "scale1_log2_scale0": o.compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=1, a=fc)).apply(so.OP_LOG2_1P).compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=0, a=fr)).ops,
    }


def test_bounded_reference_has_a_64_bit_significand_and_bounds_the_oracle():
    assert np.finfo(np.longdouble).nmant == 63
    rng = np.random.default_rng(7)
    for rows, cols, fill in er.WIDE_SHAPES[:2]:
        dense = er.real_counts(rng, rows, cols, fill)
        x, xl = rng.standard_normal((cols, 50)), rng.standard_normal((50, rows))
        for name, ops in _bounded_maps(dense, rng).items():
            o = so.AdaptiveMat.from_dense(dense, so.CSR).set_map(ops)
            ref = er.bounded_ref(dense, ops, x)
            assert ref.exact.dtype == np.longdouble and np.all(ref.bound[ref.n > 0] > 0)
            rb, ru = er.error_ratios(o.dot(x), ref)
            assert rb <= 1.0, (name, rb, ru)
            ref = er.transposed(er.bounded_ref(dense.T, er.flip_ops(ops), xl.T))
            rb, ru = er.error_ratios(o.rdot(xl), ref)
            assert rb <= 1.0, (name, rb, ru)
            # the bound is not slack by orders of magnitude: a relative error of 1e-12 in one weight class breaks it
            ri, ci = np.nonzero(dense)
            t = er.chain_terms(ops, ri, ci, dense[ri, ci])
            t = np.where(dense[ri, ci] == 2, t * (1 + np.longdouble(1e-12)), t)
            import scipy.sparse as sp

            wrong = sp.csr_matrix((t.astype(np.float64), (ri, ci)), shape=dense.shape) @ x
            assert er.error_ratios(wrong, er.bounded_ref(dense, ops, x))[0] > 1.0, name


def test_hostile_cases_have_infinite_factors_and_finite_results():
    rng = np.random.default_rng(11)
    dense = er.hostile_counts(rng, 300, 401, 0.3)
    er_, ec_ = er.empty_positions(300), er.empty_positions(401)
    assert {0, 48, 96, 299} <= set(er_) and {0, 7, 40, 80, 192, 400} <= set(ec_)
    assert not dense[er_].any() and not dense[:, ec_].any() and dense.any()
    o = so.AdaptiveMat.from_dense(dense, so.CSR)
    x, xl = rng.standard_normal((401, 50)), rng.standard_normal((50, 300))
    ln = so.log_normalize(o, None, so.LOG_TWO)
    assert np.isinf(ln.ops[-2].a[ec_]).all() and np.isfinite(np.delete(ln.ops[-2].a, ec_)).all()
    cr = so.normalize(o, "cellranger")
    fa, fb = er.inf_at_empty(rng, 300, er_), er.inf_at_empty(rng, 401, ec_)
    ex0 = o.compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=0, a=fa)).apply(so.OP_LOG2_1P).compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=1, a=fb))
    ex1 = o.compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=1, a=fb)).apply(so.OP_LOG2_1P).compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=0, a=fa))
    for m in (ln, cr, ex0, ex1):
        assert np.isfinite(m.dot(x)).all() and np.isfinite(m.rdot(xl)).all()
        assert np.isfinite(m.t().dot(xl.T)).all()
    for m in (ln, cr.inner_sparse(), ex0, ex1):
        ref = er.bounded_ref(dense, m.ops, x)
        assert np.isfinite(ref.exact.astype(np.float64)).all() and np.all(ref.exact[er_] == 0)
        assert er.error_ratios(m.dot(x), ref)[0] <= 1.0


@pytest.mark.parametrize("values", [[np.nan], [np.inf], [np.nan, np.inf, -np.inf, 1.0]])
def test_a_non_finite_panel_row_reaches_only_the_vectors_that_store_it(values):
    rng = np.random.default_rng(12)
    dense = er.hostile_counts(rng, 300, 401, 0.3)
    o = so.log_normalize(so.AdaptiveMat.from_dense(dense, so.CSR), None, so.LOG_TWO)
    x = rng.standard_normal((401, 50))
    for r in (144, 101, 96):  # row 0 of a tile of 48 that some vectors hold; mid-tile; an empty inner position
        bad, zeroed, hit = er.nonfinite_panel_case(dense, x, r, values)
        assert (len(hit) == 0) == (r == 96) and len(hit) < 300
        got, clean = o.dot(bad), o.dot(zeroed)
        finite = np.isfinite(got)
        if values != [np.nan, np.inf, -np.inf, 1.0]:
            assert not finite[hit].any()
        else:
            assert not finite[hit][:, :3].any() and finite[hit][:, 3].all()  # the finite entry of a mixed row stays finite
        rest = np.setdiff1d(np.arange(300), hit)
        assert np.array_equal(er.bits(got[rest]), er.bits(clean[rest]))
