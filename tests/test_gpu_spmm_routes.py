"""Every route of the sparse product (launch_spmm_f64 in kernels.hip; the hybrid tile product in tiles.hip / tiles_dense.inc), forced
through handle options, against the references of tests/spmm_exact_ref.py: bit for bit on dyadic inputs, within the derived bound
B = (n + 32) 2**-53 sum|t||x| on logarithm maps, on matrices with empty vectors whose scale factors are infinite, on panels with one
non-finite row, and with NaN in the slack behind the tile kernel's panel copy (handle option "tile_poison_slack").

Every test first proves its route: the profile must hold the route's kernel (and none of another product route's), a tile
route's layout must have served nonzeros (counter "tile_served_nonzeros"), and the record the library keeps of its last product
(counters "spmm_route" / "spmm_form" / "spmm_chunks", csrc/spmm_route.hpp) must name the route's kernel family, the FORM this table
claims for the (route, map, side) and the number of column chunks. The expected forms are written out below (Route.forms,
MAP_SCALE_AXIS, the *_FORM tables), not asked of the library's host function.

route (id)            options                                                    profile name that proves it
gather1               spmm_path 1                                                spmm_gather_kernel<double, N>
gather2               spmm_path 2                                                spmm_gather2d_kernel<1>/...
gather2_f32           spmm_path 2, panel precision 1 (exact test only)           spmm_gather2d_f32_kernel/...
r4_2_32_48_4 ...      spmm_path 3, tile_dense 0, tile_ku 0, tile_k/s/t/b:        spmm_tile_kernel/...   (+ spmm_gather2d_ov/... overflow)
  r4_2_28_48_4, r4_3_32_64_3, r4_4_32_96_2, r4_4_28_40_3                         fixed positions, a weight per position
r4_unit               spmm_path 3, tile_dense 0, tile_ku 1                       spmm_tile_kernel/...   unit positions under a separable
                                                                                 map (raw, sq_axis0/1, the logarithm maps); the weighted
                                                                                 kernel on the same layout under sq_both (not separable)
dense_tab             spmm_path 3 (dense records, the default)                   spmm_tile_kernel/...   table by place ("tabo") when the
                                                                                 product's outer side owns the nonlinear link AND under
                                                                                 raw counts (no nonlinear link: the place table holds the
                                                                                 counts, on either side), by inner position ("tabi")
                                                                                 otherwise: map x dot/rdot gives both; weight stream,
                                                                                 nothing folded, under sq_both
dense_stream          spmm_path 3, tile_wtab 0                                   spmm_tile_kernel/...   weight stream, the factor of the side
                                                                                 without the nonlinear link folded out (inner: in the
                                                                                 panel, outer: on the sums); nothing folded under sq_both
dense_unfolded        spmm_path 3, tile_fold 0                                   spmm_tile_kernel/...   both factors in every weight
gather2_3_to_15       spmm_path 3, l in 3, 8, 15                                 spmm_gather2d_kernel<1>/...
gather1_3_to_15       spmm_path 0, l in 3, 8, 15                                 spmm_gather_kernel<double, N>
spmv_small            spmm_path 0, l in 1, 2                                     spmv_kernel/...
slice_walk            48 x 2**19+1, l 1                                          slice_walk_spmv/short-outer
spmv2d                same, slice_walk 0 (l 1) or l 2                            spmv2d_kernel/short-outer   l 1 under a chain that starts with the
                                                                                 inner side's scale: the scale interleaved with the vector;
                                                                                 this route never reads materialized values
spmv_big_long         same matrix, rdot (outer 2**19+1)                          spmv_kernel/long-outer
spmv_lds              2**16 x 18433, l 1, two parts; forms: 0 raw / inner-indexed map evaluated per nonzero, 2 row table (outer-only
                      chain), 1 materialized values (logarithm chain, bounded test) spmv_lds_kernel/long-outer

What is asserted about the form, after every product: which spmv_lds form ran, table by place / by inner position / weight stream
(TileLayout::wsrc), unit mode against the weighted kernel, folded against unfolded factors, materialized values and the staged /
interleaved scale of slice_walk and spmv2d, and the column chunks of a wide panel (105 columns: 2). What still is not: the number
of parts of a layout and the rounds of a visit follow from the shapes alone and have no counter. Two claims an earlier version of
this text made did not survive the assertions' table: under raw counts dense_tab runs the table by place on BOTH sides (it said
"by inner position otherwise"), and spmv2d has no materialized-values form at all, so "spmv2d_unmaterialized" below runs exactly
what "spmv2d" runs (the text said "the same without materialized values"). The exact, bounded, infinite-scale and non-finite-row
checks run on every route above, the narrow ones included (the two large matrices have empty rows and columns, infinite factors
there, and NaN / inf vector entries).

Measured on an MI355X: worst |err| / B, and worst |err| / (2**-53 S) in brackets, over all shapes, storages, widths and sides
(printed by the tests, run with -s). No ratio is above 1; the largest, 0.34, is under normalize(CellRanger), whose gene scales the
library makes from its own moment sums while the reference's chain carries the oracle's (most likely a few ulps apart; not examined).
route            log_normalize  cellranger     scale0_log2_scale1  scale1_log2_scale0 | hostile: log_normalize cellranger inf0_log2_inf1 inf1_log2_inf0
gather1, gather2 0.149 (5.35)   0.319 (10.86)  0.115 (3.89)        0.128 (4.21)       | 0.027 (4.12)  0.028 (3.80)  0.030 (4.22)  0.025 (3.69)
r4_2_32_48_4     0.149 (5.35)   0.319 (10.86)  0.115 (4.25)        0.128 (4.21)       | 0.010 (1.19)  0.019 (2.66)  0.013 (1.62)  0.011 (1.23)
r4_2_28_48_4     0.149 (5.35)   0.319 (10.86)  0.115 (3.89)        0.128 (4.21)       | 0.022 (2.51)  0.027 (3.72)  0.023 (2.75)  0.021 (2.86)
r4_3_32_64_3     0.149 (5.35)   0.319 (10.86)  0.115 (3.89)        0.128 (4.21)       | 0.023 (2.54)  0.024 (3.37)  0.024 (2.68)  0.031 (4.37)
r4_4_32_96_2     0.149 (5.35)   0.319 (10.86)  0.115 (3.89)        0.128 (4.21)       | 0.027 (4.12)  0.025 (3.53)  0.027 (3.03)  0.025 (3.15)
r4_4_28_40_3     0.149 (5.35)   0.319 (10.86)  0.115 (3.89)        0.128 (4.21)       | 0.017 (2.00)  0.024 (3.37)  0.017 (2.08)  0.018 (2.21)
r4_unit          0.174 (5.91)   0.336 (11.41)  0.115 (3.87)        0.128 (4.21)       | 0.011 (1.41)  0.024 (3.37)  0.010 (1.19)  0.011 (1.28)
dense_tab        0.149 (5.35)   0.319 (10.86)  0.115 (3.88)        0.128 (4.21)       | 0.010 (1.19)  0.018 (2.60)  0.013 (1.56)  0.011 (1.19)
dense_stream     0.149 (5.35)   0.319 (10.86)  0.115 (3.88)        0.128 (4.21)       | 0.010 (1.19)  0.018 (2.60)  0.013 (1.56)  0.011 (1.19)
dense_unfolded   0.149 (5.35)   0.319 (10.86)  0.118 (4.24)        0.128 (4.21)       | 0.010 (1.19)  0.019 (2.66)  0.013 (1.62)  0.011 (1.23)
(equal figures across routes: most likely rows of one or two stored terms, where the error is the term's own, the same logarithm on every route)
gather2_3_to_15  0.130 (4.40)   0.303 (10.21)  0.112 (3.71)        0.128 (4.21)       | 0.025 (3.99)  0.024 (3.53)  0.030 (4.22)  0.025 (3.20)
gather1_3_to_15  0.130 (4.40)   0.303 (10.21)  0.112 (3.71)        0.128 (4.21)       | 0.025 (3.99)  0.024 (3.53)  0.030 (4.22)  0.025 (3.20)
spmv_small       0.130 (4.40)   0.299 (10.17)  0.106 (3.49)        0.110 (3.62)       | 0.007 (0.71)  0.018 (2.54)  0.005 (0.66)  0.006 (0.71)
Large matrices (infinite factors at their empty rows and columns): slice_walk 0.000 (0.03), spmv2d 0.000 (0.07; the same form
with "materialize" 0), spmv_big_long 0.089 (3.28), spmv_lds forms 0 and 1 0.013 (1.18), form 2 0.016 (1.23).
Run time of the file on an MI355X: 62 s for its 101 tests (the slowest call under 3 s, the two large matrices 4 s of fixture set-up each)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import scanrs_oracle as so  # noqa: E402
import spmm_exact_ref as er  # noqa: E402

TILE, OV = "spmm_tile_kernel/", "spmm_gather2d_ov/"
PRODUCT_KERNELS = ("spmm_gather_kernel<", "spmm_gather2d_kernel<1>/", "spmm_gather2d_f32_kernel/", TILE, "spmv_kernel/", "spmv2d_kernel/",
                   "spmv_lds_kernel/", "slice_walk_spmv/")


# kernel family (counter "spmm_route", SCANRS_SPMM_* of scanrs_amd.h) by the profile name that proves the route
FAMILY = {TILE: 1, "spmm_gather2d_kernel<1>/": 2, "spmm_gather2d_f32_kernel/": 3, "slice_walk_spmv/": 4, "spmv2d_kernel/": 5, "spmv_lds_kernel/": 6,
          "spmv_kernel/": 7, "spmm_gather_kernel<": 8}
# The axis of the scale in front of a map's nonlinear link (None: no link at all, "N": scales of both axes in front of it - the map
# does not separate). A product walks the copy whose outer vectors are the rows (dot: axis 0) or the columns (rdot, the transposed
# view: axis 1); the map is class "O" when that axis owns the nonlinear link or there is none, "I" when the other one does.
MAP_SCALE_AXIS = {"raw": None, "sq_axis0": 0, "sq_axis1": 1, "sq_both": "N", "log_normalize": 1, "cellranger": 1, "scale0_log2_scale1": 0,
                  "scale1_log2_scale0": 1, "inf0_log2_inf1": 0, "inf1_log2_inf0": 1}
# counter "spmm_form" of a tile product: bit 0 dense records, bit 1 unit mode, bits 2-3 the weight's source (0 stream, 1 table by
# place, 2 table by inner position), bits 4-5 the factor folded out (0 none, 1 the inner side's, 2 the outer side's)
FIXED_FORMS = {"O": 0, "I": 0, "N": 0}                       # fixed positions, a weight per position
UNIT_FORMS = {"O": 2, "I": 2, "N": 0}                        # unit mode under a separable map, the weighted kernel otherwise
TAB_FORMS = {"O": 1 | 1 << 2 | 1 << 4, "I": 1 | 2 << 2 | 2 << 4, "N": 1}   # tabo + the inner factor in the panel, tabi + the outer factor on the sums, the stream
STREAM_FORMS = {"O": 1 | 1 << 4, "I": 1 | 2 << 4, "N": 1}    # the weight stream, folded
UNFOLDED_FORMS = {"O": 1, "I": 1, "N": 1}                    # the weight stream, both factors in every weight


def map_class(name, side):
    axis = MAP_SCALE_AXIS[name]
    if axis is None or axis == "N":
        return "O" if axis is None else "N"
    return "O" if axis == (0 if side == "dot" else 1) else "I"


class Route:
    def __init__(self, name, path, prof, opts=(), precision=0, tile_t=0, ls=None, forms=None, form=0):
        self.name, self.path, self.prof, self.opts, self.precision, self.tile_t = name, path, prof, tuple(opts), precision, tile_t
        self.ls = ls  # panel widths of a route that serves narrow panels only (None: the wide widths of the test)
        self.family = next(v for k, v in FAMILY.items() if prof.startswith(k))
        self.forms, self.form = forms, form  # a tile route: the form by map class; another one: its one form
        assert self.tile == (forms is not None)

    def check_form(self, g, name=None, side="dot", l=1):
        """the last product on g: this route's family, the form claimed for (map, side), the column chunks of an l-wide panel"""
        want = (self.family, self.forms[map_class(name, side)] if self.tile else self.form, (l + 103) // 104 if self.tile else 1)
        got = (g.counter("spmm_route"), g.counter("spmm_form"), g.counter("spmm_chunks"))
        assert got == want, (self.name, name, side, l, got, want)

    @property
    def tile(self):
        return self.prof == TILE

    def configure(self, g):
        g.set_spmm_path(self.path)
        for k, v in self.opts:
            g.set_option(k, v)
        if self.precision:
            g.set_panel_precision(self.precision)
        g.profile_enable(True)
        return g

    def check_ran(self, g):
        """the route's kernel ran, no other product kernel did, and (tiles) every layout built so far served nonzeros"""
        names = list(g.profile_get())
        assert g.counter("spmm_route") == self.family, (self.name, g.counter("spmm_route"))
        assert any(n.startswith(self.prof) for n in names), (self.name, names)
        others = [n for n in names if any(n.startswith(p) for p in PRODUCT_KERNELS) and not n.startswith(self.prof)]
        assert not others, (self.name, others)
        if self.tile:
            served = g.counter("tile_served_nonzeros")
            assert served > 0, self.name
            return served, g.counter("tile_overflow_nonzeros")
        return 0, 0


def _r4(k, s, t, b):
    return Route(f"r4_{k}_{s}_{t}_{b}", 3, TILE, (("tile_dense", 0), ("tile_ku", 0), ("tile_k", k), ("tile_s", s), ("tile_t", t), ("tile_b", b)), tile_t=t, forms=FIXED_FORMS)


GATHER_ROUTES = [Route("gather1", 1, "spmm_gather_kernel<double"), Route("gather2", 2, "spmm_gather2d_kernel<1>/")]
F32_ROUTE = Route("gather2_f32", 2, "spmm_gather2d_f32_kernel/", precision=1)
TILE_ROUTES = [_r4(2, 32, 48, 4), _r4(2, 28, 48, 4), _r4(3, 32, 64, 3), _r4(4, 32, 96, 2), _r4(4, 28, 40, 3),
               Route("r4_unit", 3, TILE, (("tile_dense", 0), ("tile_ku", 1)), tile_t=48, forms=UNIT_FORMS),
               Route("dense_tab", 3, TILE, (), tile_t=48, forms=TAB_FORMS),
               Route("dense_stream", 3, TILE, (("tile_wtab", 0),), tile_t=48, forms=STREAM_FORMS),
               Route("dense_unfolded", 3, TILE, (("tile_fold", 0),), tile_t=48, forms=UNFOLDED_FORMS)]
F64_ROUTES = GATHER_ROUTES + TILE_ROUTES
# panels under 16 columns on small matrices: the blocked gather (asked for), the plain gather and spmv_kernel (auto path)
SMALL_L_ROUTES = [Route("gather2_3_to_15", 3, "spmm_gather2d_kernel<1>/", ls=(3, 8, 15)), Route("gather1_3_to_15", 0, "spmm_gather_kernel<double", ls=(3, 8, 15)),
                  Route("spmv_small", 0, "spmv_kernel/", ls=(1, 2))]
ids = lambda r: r.name  # noqa: E731


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gfx950 device required for -m gpu tests (no CPU fallback exists)")
    return scanrs_amd


def _no_offset(g):
    r, c = g.shape()
    return g.set_offset(np.zeros((r, 0)), np.zeros((0, c)))


# ---- shared inputs and references (computed once) -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dyadic_cases():
    out = []
    for i, (rows, cols, fill) in enumerate(er.WIDE_SHAPES):
        case = er.dyadic_case(rows, cols, fill, 100 + i)
        refs = {}
        for name in er.DYADIC_MAPS:
            for side in ("dot", "rdot"):
                for offset in (False, True):
                    ref = er.dyadic_ref(case, name, side, max(er.WIDE_L), offset)
                    assert int(ref.mag.max()) < 2 ** 53
                    ref.want.setflags(write=False)
                    refs[name, side, offset] = ref.want
        out.append((case, refs))
    return out


def _log_maps(sa, dense, seed):
    """name -> (apply to a library handle, oracle chain)"""
    rows, cols = dense.shape
    rng = np.random.default_rng(seed)
    fr, fc = rng.random(rows) + 0.5, rng.random(cols) + 0.5
    o = so.AdaptiveMat.from_dense(dense, so.CSR)
    sc = lambda ax, f: so.MapOp(so.OP_SCALE_AXIS, axis=ax, a=f)  # noqa: E731
    return {
        "log_normalize": (lambda g: sa.log_normalize_with_size_factor(g, None, sa.FN_LOG2_1P), so.log_normalize(o, None, so.LOG_TWO).ops),
        "cellranger": (lambda g: _no_offset(sa.normalize(g, sa.Normalization.CellRanger)), so.normalize(o, "cellranger").inner_sparse().ops),
        "scale0_log2_scale1": (lambda g: g.compose_scale_axis(0, fr).apply(sa.FN_LOG2_1P).compose_scale_axis(1, fc),
                               o.compose_map(sc(0, fr)).apply(so.OP_LOG2_1P).compose_map(sc(1, fc)).ops),
        "scale1_log2_scale0": (lambda g: g.compose_scale_axis(1, fc).apply(sa.FN_LOG2_1P).compose_scale_axis(0, fr),
                               o.compose_map(sc(1, fc)).apply(so.OP_LOG2_1P).compose_map(sc(0, fr)).ops),
    }


def _bounded_refs(dense, maps, x, xl):
    refs = {}
    for name, (_, ops) in maps.items():
        refs[name, "dot"] = er.bounded_ref(dense, ops, x)
        refs[name, "rdot"] = er.transposed(er.bounded_ref(dense.T, er.flip_ops(ops), xl.T))
    return refs


def _cut(ref, side, l):
    return ref.cut(cols=slice(0, l)) if side == "dot" else ref.cut(rows=slice(0, l))


@pytest.fixture(scope="module")
def bounded_cases(sa):
    out = []
    for i, (rows, cols, fill) in enumerate(er.WIDE_SHAPES):
        rng = np.random.default_rng(200 + i)
        dense = er.real_counts(rng, rows, cols, fill)
        x, xl = rng.standard_normal((cols, max(er.WIDE_L))), rng.standard_normal((max(er.WIDE_L), rows))
        maps = _log_maps(sa, dense, 300 + i)
        out.append((dense, x, xl, maps, _bounded_refs(dense, maps, x, xl)))
    return out


HOSTILE_SHAPE = (300, 401)
HOSTILE_L = (16, 50)


@pytest.fixture(scope="module")
def hostile_case(sa):
    rows, cols = HOSTILE_SHAPE
    rng = np.random.default_rng(11)
    dense = er.hostile_counts(rng, rows, cols, 0.3)
    e_r, e_c = er.empty_positions(rows), er.empty_positions(cols)
    fa, fb = er.inf_at_empty(rng, rows, e_r), er.inf_at_empty(rng, cols, e_c)
    o = so.AdaptiveMat.from_dense(dense, so.CSR)
    sc = lambda ax, f: so.MapOp(so.OP_SCALE_AXIS, axis=ax, a=f)  # noqa: E731
    maps = _log_maps(sa, dense, 1)
    maps = {"log_normalize": maps["log_normalize"], "cellranger": maps["cellranger"],
            "inf0_log2_inf1": (lambda g: g.compose_scale_axis(0, fa).apply(sa.FN_LOG2_1P).compose_scale_axis(1, fb),
                               o.compose_map(sc(0, fa)).apply(so.OP_LOG2_1P).compose_map(sc(1, fb)).ops),
            "inf1_log2_inf0": (lambda g: g.compose_scale_axis(1, fb).apply(sa.FN_LOG2_1P).compose_scale_axis(0, fa),
                               o.compose_map(sc(1, fb)).apply(so.OP_LOG2_1P).compose_map(sc(0, fa)).ops)}
    x, xl = rng.standard_normal((cols, max(HOSTILE_L))), rng.standard_normal((max(HOSTILE_L), rows))
    refs = _bounded_refs(dense, maps, x, xl)
    for ref in refs.values():
        assert np.isfinite(ref.exact.astype(np.float64)).all()
    return dense, x, xl, maps, refs


WORST = {}


def _note(route, name, rb, ru):
    a, b = WORST.get((route.name, name), (0.0, 0.0))
    WORST[route.name, name] = (max(a, rb), max(b, ru))


# ---- exact -----------------------------------------------------------------------------------------------------------------------
def _exact_products(sa, route, dyadic_cases, ls):
    for case, refs in dyadic_cases:
        for storage in (sa.CSR, sa.CSC):
            for name in er.DYADIC_MAPS:
                g = route.configure(er.dyadic_gpu(sa, sa.AdaptiveMat.from_dense(case.dense, storage), case, name))
                for offset in (False, True):
                    if offset:
                        g.set_offset(case.u, case.v)
                    for l in ls:
                        where = (route.name, case.shape, storage, name, offset, l)
                        got = g.dot(case.x[:, :l])
                        route.check_form(g, name, "dot", l)
                        assert np.array_equal(er.bits(got), er.bits(refs[name, "dot", offset][:, :l])), where
                        if l == ls[0] and not offset:
                            first = route.check_ran(g)
                        got = g.rdot(case.xl[:l])
                        route.check_form(g, name, "rdot", l)
                        assert np.array_equal(er.bits(got), er.bits(refs[name, "rdot", offset][:l])), where
                        if l == ls[0] and not offset and route.tile:
                            assert route.check_ran(g)[0] > first[0], where  # the second orientation's layout served nonzeros too
                route.check_ran(g)


@pytest.mark.parametrize("route", F64_ROUTES + [F32_ROUTE], ids=ids)
def test_dyadic_products_are_exact(sa, route, dyadic_cases):
    _exact_products(sa, route, dyadic_cases, er.WIDE_L)


@pytest.mark.parametrize("route", SMALL_L_ROUTES, ids=ids)
def test_dyadic_products_of_narrow_panels_are_exact(sa, route, dyadic_cases):
    _exact_products(sa, route, dyadic_cases, route.ls)


# ---- bounded ---------------------------------------------------------------------------------------------------------------------
def _bounded_products(sa, route, cases, ls, storages=None, tag=""):
    for dense, x, xl, maps, refs in cases:
        for storage in storages or (sa.CSR, sa.CSC):
            for name, (apply, _) in maps.items():
                g = route.configure(sa.AdaptiveMat.from_dense(dense, storage))
                apply(g)
                g.profile_reset()  # (a normalisation's own passes are not the subject)
                for l in ls:
                    sides = [("dot", lambda: g.dot(x[:, :l])), ("rdot", lambda: g.rdot(xl[:l]))]
                    if l == ls[0]:  # the transposed view
                        sides.append(("t", lambda: g.t().dot(xl[:l].T.copy()).T))
                    for side, product in sides:
                        got = product()
                        route.check_form(g, name, side, l)
                        rb, ru = er.error_ratios(got, _cut(refs[name, "dot" if side == "dot" else "rdot"], "dot" if side == "dot" else "rdot", l))
                        _note(route, tag + name, rb, ru)
                        assert np.isfinite(got).all() and rb <= 1.0, (route.name, dense.shape, storage, name, side, l, rb, ru)
                route.check_ran(g)
    print(f"\n{route.name}: worst |err|/B, |err|/(2^-53 S): " + "; ".join(f"{n} {WORST[route.name, tag + n][0]:.3f}, {WORST[route.name, tag + n][1]:.2f}" for n in cases[0][3]))


@pytest.mark.parametrize("route", F64_ROUTES + SMALL_L_ROUTES, ids=ids)
def test_logarithm_maps_within_the_derived_bound(sa, route, bounded_cases):
    _bounded_products(sa, route, bounded_cases, route.ls or er.WIDE_L)


@pytest.mark.parametrize("route", F64_ROUTES + SMALL_L_ROUTES, ids=ids)
def test_empty_vectors_with_infinite_scales_give_the_reference_s_finite_results(sa, route, hostile_case):
    ls = route.ls or HOSTILE_L
    _bounded_products(sa, route, [hostile_case], ls, tag="hostile ")
    # With the centring offset of the normalisation on, the point is that the results are FINITE. The comparison with the f64 oracle
    # behind it is a plausibility check only (the offset term is a dense product with tests of its own, tests/test_gpu_dense.py):
    # at 1e-10 it cannot tell rounding from a small systematic error, which the bounded check above does for the sparse part.
    dense, x, xl, _, _ = hostile_case
    for storage in (sa.CSR, sa.CSC):
        g = sa.normalize(route.configure(sa.AdaptiveMat.from_dense(dense, storage)), sa.Normalization.CellRanger)
        o = so.normalize(so.AdaptiveMat.from_dense(dense, storage), "cellranger")
        for got, want in ((g.dot(x[:, :ls[-1]]), o.dot(x[:, :ls[-1]])), (g.rdot(xl[:ls[-1]]), o.rdot(xl[:ls[-1]]))):
            assert np.isfinite(got).all(), (route.name, storage)
            assert np.all(np.abs(got - want) <= 1e-10 * np.max(np.abs(want))), (route.name, storage)


def _first_live_multiple(t, n, empties):
    r = -(-100 // t) * t
    while r in empties:
        r += t
    assert r < n - 6
    return r


@pytest.mark.parametrize("values", [[np.nan], [np.inf], [np.nan, np.inf, -np.inf, 1.0]], ids=["nan", "inf", "mixed"])
@pytest.mark.parametrize("route", F64_ROUTES + [F32_ROUTE] + SMALL_L_ROUTES, ids=ids)
def test_a_non_finite_panel_row_stays_in_the_vectors_that_store_it(sa, route, values, hostile_case):
    dense, x, xl, maps, _ = hostile_case
    t = route.tile_t or 48
    for storage in (sa.CSR, sa.CSC):
        g = route.configure(sa.AdaptiveMat.from_dense(dense, storage))
        maps["log_normalize"][0](g)
        g.profile_reset()
        for l, side, d, panel in [(l, side, d, panel) for l in (route.ls or (50,)) for side, d, panel in (("dot", dense, x[:, :l]), ("rdot", dense.T, xl[:l].T))]:
            n = d.shape[1]
            r0 = _first_live_multiple(t, n, er.empty_positions(n))
            for r in (r0, r0 + 5, t, 7):  # a tile's row 0 that some vectors hold, mid-tile, empty inner positions (a tile's row 0, mid-tile)
                bad, zeroed, hit = er.nonfinite_panel_case(d, panel, r, values)
                assert (len(hit) == 0) == (r in (t, 7)) and len(hit) < d.shape[0]
                if side == "dot":
                    got, clean = g.dot(bad), g.dot(zeroed)
                else:
                    got, clean = g.rdot(bad.T.copy()).T, g.rdot(zeroed.T.copy()).T
                route.check_form(g, "log_normalize", side, l)
                where = (route.name, storage, side, r)
                nf_cols = ~np.isfinite(bad[r])
                assert not np.isfinite(got[np.ix_(hit, nf_cols)]).any(), where
                assert np.isfinite(got[np.ix_(hit, ~nf_cols)]).all(), where
                rest = np.setdiff1d(np.arange(d.shape[0]), hit)
                assert np.array_equal(er.bits(got[rest]), er.bits(clean[rest])), (where, int((er.bits(got[rest]) != er.bits(clean[rest])).any(axis=1).sum()))
        route.check_ran(g)


# ---- the slack behind the tile kernel's panel copy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [TILE_ROUTES[0], TILE_ROUTES[5], TILE_ROUTES[6], TILE_ROUTES[7]], ids=ids)
def test_poisoned_panel_slack_changes_nothing(sa, route):
    """n_inner on and off a multiple of the tile (48 rows), one part and several. Scale exponents in [-2, 2] here: one term of the
    full range can reach 2**50.5 grid units, which leaves other seeds and shapes than WIDE_SHAPES' no certain room below 2**53
    (largest term here: 2**42.5; the test asserts the sums)."""
    for rows, cols, fill in ((33, 96, 0.5), (33, 97, 0.5), (97, 19968, 0.01), (97, 20000, 0.01), (2000, 193, 0.1), (1920, 193, 0.1)):
        case = er.dyadic_case(rows, cols, fill, 400 + cols, emax=2)
        for name in ("raw", "sq_axis1", "sq_both"):
            g = route.configure(er.dyadic_gpu(sa, sa.AdaptiveMat.from_dense(case.dense, sa.CSR), case, name))
            for l in (16, 104):
                outs = []
                for poison in (0, 1, 0):
                    g.set_option("tile_poison_slack", poison)
                    g.profile_reset()
                    outs.append((g.dot(case.x[:, :l]), g.rdot(case.xl[:l])))
                    route.check_form(g, name, "rdot", l)
                    assert ("tile_poison_slack" in g.profile_get()) == bool(poison)  # the hook's kernel ran, and only when asked
                refs = er.dyadic_ref(case, name, "dot", l, False), er.dyadic_ref(case, name, "rdot", l, False)
                assert max(int(r.mag.max()) for r in refs) < 2 ** 53
                want = refs[0].want, refs[1].want
                for o in outs:
                    assert np.array_equal(er.bits(o[0]), er.bits(want[0])) and np.array_equal(er.bits(o[1]), er.bits(want[1])), (route.name, rows, cols, name, l)
            route.check_ran(g)


def test_the_layouts_cover_both_sides_of_the_overflow(sa, bounded_cases, dyadic_cases):
    """a layout whose records serve every nonzero and one that leaves some to the overflow gather"""
    dense = bounded_cases[0][0]  # 33 x 97, counts below 9: the dense records take all of it
    g = TILE_ROUTES[6].configure(sa.AdaptiveMat.from_dense(dense, sa.CSR))
    g.dot(bounded_cases[0][1][:, :16])
    served, over = TILE_ROUTES[6].check_ran(g)
    assert served == int(np.count_nonzero(dense)) and over == 0
    case = dyadic_cases[0][0]    # counts above 255 and more nonzeros per tile than two positions per visit hold
    g = TILE_ROUTES[0].configure(sa.AdaptiveMat.from_dense(case.dense, sa.CSR))
    g.dot(case.x[:, :16])
    served, over = TILE_ROUTES[0].check_ran(g)
    # (for this layout the served count is the difference of the two totals - tile_layout_stats - so the sum says nothing; over > 0 does)
    assert over > 0 and served + over == int(np.count_nonzero(case.dense))
    assert any(n.startswith(OV) for n in g.profile_get())


# ---- Ix1 and Ix2 products of large matrices ------------------------------------------------------------------------------------------
def _from_scipy_counts(sa, m):
    return sa.AdaptiveMat.from_csmat(m.shape[0], m.shape[1], sa.CSR, m.indptr.astype(np.uint64), m.indices.astype(np.uint32), m.data.astype(np.uint32))


SHORT_EMPTY_ROWS, SHORT_EMPTY_COLS = (5, 47), (0, 7, 1024, 2048, 1 << 19)           # slice edges (1024 positions), both ends, mid-slice
LONG_EMPTY_ROWS, LONG_EMPTY_COLS = (0, 15, 16, (1 << 16) - 1), (0, 7, 1024, 10240, 18432)  # 10240: first position of the second LDS part


def _large_case(rows, cols, seed, heavy, empty_rows, empty_cols):
    m = er.narrow_counts(np.random.default_rng(seed), rows, cols, 1 << 22, heavy, empty_rows, empty_cols)
    case = er.dyadic_case(rows, cols, 0.0, seed + 1, csr=m, emax=1, lmax=2)
    case.empty_rows, case.empty_cols = empty_rows, empty_cols
    return case


@pytest.fixture(scope="module")
def short_outer_case():
    """48 x 2**19+1, just over 2**22 nonzeros, an eighth of them in row 0 (every column that is not empty); empty rows and columns"""
    return _large_case(48, (1 << 19) + 1, 500, 0.125, SHORT_EMPTY_ROWS, SHORT_EMPTY_COLS)


@pytest.fixture(scope="module")
def long_outer_case():
    """2**16 x 18433, just over 2**22 nonzeros: two LDS parts of the vector; empty rows and columns"""
    return _large_case(1 << 16, 18433, 510, 0.0, LONG_EMPTY_ROWS, LONG_EMPTY_COLS)


def _narrow_exact(sa, case, route, name, side, l, refs):
    g = route.configure(er.dyadic_gpu(sa, _from_scipy_counts(sa, case.csr), case, name))
    for offset in (False, True):
        if offset:
            g.set_offset(case.u, case.v)
        key = (name, side, l, offset)
        if key not in refs:
            ref = er.dyadic_ref(case, name, side, l, offset)
            assert int(ref.mag.max()) < 2 ** 53, key
            refs[key] = ref.want
        got = g.dot(case.x[:, :l]) if side == "dot" else g.rdot(case.xl[:l])
        route.check_form(g)
        assert np.array_equal(er.bits(got), er.bits(refs[key])), (route.name, key)
    route.check_ran(g)
    return g


NARROW_REFS = {}
SLICE_WALK_FORM = {"raw": 0, "sq_axis1": 1, "sq_axis0": 0}
SPMV2D_L1_FORM = {"raw": 0, "sq_axis1": 2, "sq_axis0": 0}
SPMV_LDS_FORM = {"raw": 0, "sq_axis1": 0, "sq_only0": 2}


@pytest.mark.parametrize("name", ["raw", "sq_axis1", "sq_axis0"])
def test_dyadic_slice_walk_and_spmv2d(sa, short_outer_case, name):
    refs = NARROW_REFS.setdefault("short", {})
    # sq_axis1 starts with the inner side's scale: slice_walk reads materialized values (bit 0), spmv2d interleaves the scale (bit 1)
    _narrow_exact(sa, short_outer_case, Route("slice_walk", 0, "slice_walk_spmv/", form=SLICE_WALK_FORM[name]), name, "dot", 1, refs)
    _narrow_exact(sa, short_outer_case, Route("spmv2d", 0, "spmv2d_kernel/short-outer", (("slice_walk", 0),), form=SPMV2D_L1_FORM[name]), name, "dot", 1, refs)
    _narrow_exact(sa, short_outer_case, Route("spmv2d", 0, "spmv2d_kernel/short-outer"), name, "dot", 2, refs)
    _narrow_exact(sa, short_outer_case, Route("spmv_big_long", 0, "spmv_kernel/long-outer"), name, "rdot", 1, refs)


@pytest.mark.parametrize("name", ["raw", "sq_axis1", "sq_only0"])  # forms 0, 0 (inner-indexed link per nonzero), 2 (row table)
def test_dyadic_spmv_lds(sa, long_outer_case, name):
    _narrow_exact(sa, long_outer_case, Route("spmv_lds", 0, "spmv_lds_kernel/", form=SPMV_LDS_FORM[name]), name, "dot", 1, NARROW_REFS.setdefault("long", {}))


def _narrow_bounded(sa, case, route, side, l, chain):
    """A large case under a logarithm chain with real factors that are INFINITE at the empty rows and columns (never applied by
    the reference, which sums stored terms): chain "inner": Scale(inner side) -> LOG2_1P, "inner_outer": ... -> Scale(outer side),
    "outer": Scale(outer side) -> LOG2_1P. Every element within B of the longdouble reference (so finite, and exactly 0 for an empty
    vector); then one vector entry set to NaN / inf - at an empty inner position and at a stored one - must reach the outer vectors
    that store it and leave every other element bit for bit what the zeroed entry gives."""
    rng = np.random.default_rng(520)
    rows, cols = case.shape
    fr, fc = rng.random(rows) + 0.5, rng.random(cols) + 0.5
    fr[list(case.empty_rows)] = np.inf
    fc[list(case.empty_cols)] = np.inf
    inner_axis = 1 if side == "dot" else 0
    f_inner, f_outer = (fc, fr) if inner_axis else (fr, fc)
    g = route.configure(_from_scipy_counts(sa, case.csr))
    ops = []
    if chain != "outer":
        g.compose_scale_axis(inner_axis, f_inner)
        ops.append(so.MapOp(so.OP_SCALE_AXIS, axis=inner_axis, a=f_inner))
    else:
        g.compose_scale_axis(1 - inner_axis, f_outer)
        ops.append(so.MapOp(so.OP_SCALE_AXIS, axis=1 - inner_axis, a=f_outer))
    g.apply(sa.FN_LOG2_1P)
    ops.append(so.MapOp(so.OP_LOG2_1P))
    if chain == "inner_outer":
        g.compose_scale_axis(1 - inner_axis, f_outer)
        ops.append(so.MapOp(so.OP_SCALE_AXIS, axis=1 - inner_axis, a=f_outer))
    ri, ci, c = case.coo()
    t = er.chain_terms(ops, ri, ci, c)
    assert np.isfinite(t.astype(np.float64)).all()
    x = rng.standard_normal((cols if side == "dot" else rows, l))
    if side == "rdot":
        order = np.lexsort((ri, ci))
        ri, ci, t = ci[order], ri[order], t[order]
    counts = np.bincount(ri, minlength=rows if side == "dot" else cols)
    assert (counts == 0).any()  # empty outer vectors
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    prod = t[:, None] * x.astype(np.longdouble)[ci]
    ref = er.BoundedRef(er.row_sums(prod, starts, counts), er.row_sums(np.abs(prod), starts, counts),
                        np.broadcast_to(counts[:, None].astype(np.float64), (counts.shape[0], l)))
    product = (lambda v: g.dot(v)) if side == "dot" else (lambda v: g.rdot(v.T.copy()).T)
    got = product(x)
    route.check_form(g)
    rb, ru = er.error_ratios(got, ref)
    print(f"\n{route.name} l={l} {chain}: worst |err|/B {rb:.3f}, worst |err|/(2^-53 S) {ru:.2f}")
    assert np.isfinite(got).all() and rb <= 1.0, (route.name, side, l, chain, rb, ru)
    empty_inner = case.empty_cols if inner_axis else case.empty_rows
    r_empty = empty_inner[min(2, len(empty_inner) - 1)]  # (columns: 1024, a slice / base-tile edge)
    for r in (r_empty, r_empty + 1 if r_empty + 1 < x.shape[0] else r_empty - 1):
        hit = np.unique(ri[ci == r])
        assert (hit.size == 0) == (r == r_empty) and hit.size < counts.shape[0]
        bad, zeroed = x.copy(), x.copy()
        bad[r], zeroed[r] = np.resize([np.nan, np.inf], l), 0.0
        got, clean = product(bad), product(zeroed)
        assert not np.isfinite(got[hit]).any(), (route.name, side, l, chain, r)
        rest = np.setdiff1d(np.arange(counts.shape[0]), hit)
        assert np.array_equal(er.bits(got[rest]), er.bits(clean[rest])), (route.name, side, l, chain, r)
    route.check_ran(g)


def test_logarithm_maps_slice_walk_and_spmv2d_within_the_bound(sa, short_outer_case):
    for chain in ("inner", "inner_outer"):
        _narrow_bounded(sa, short_outer_case, Route("slice_walk", 0, "slice_walk_spmv/", form=1), "dot", 1, chain)  # materialized values
        _narrow_bounded(sa, short_outer_case, Route("spmv2d", 0, "spmv2d_kernel/short-outer", (("slice_walk", 0),), form=2), "dot", 1, chain)  # (the scale fused into the vector's slots)
        _narrow_bounded(sa, short_outer_case, Route("spmv2d_unmaterialized", 0, "spmv2d_kernel/short-outer", (("slice_walk", 0), ("materialize", 0)), form=2), "dot", 1, chain)  # (the same form: spmv2d reads no materialized values)
        _narrow_bounded(sa, short_outer_case, Route("spmv2d", 0, "spmv2d_kernel/short-outer"), "dot", 2, chain)
    _narrow_bounded(sa, short_outer_case, Route("spmv_big_long", 0, "spmv_kernel/long-outer"), "rdot", 1, "inner_outer")


def test_logarithm_maps_spmv_lds_within_the_bound(sa, long_outer_case):
    _narrow_bounded(sa, long_outer_case, Route("spmv_lds_values", 0, "spmv_lds_kernel/", form=1), "dot", 1, "inner_outer")
    _narrow_bounded(sa, long_outer_case, Route("spmv_lds_lazy", 0, "spmv_lds_kernel/", (("materialize", 0),), form=0), "dot", 1, "inner_outer")
    _narrow_bounded(sa, long_outer_case, Route("spmv_lds_row_table", 0, "spmv_lds_kernel/", form=2), "dot", 1, "outer")
