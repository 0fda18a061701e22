"""The route of a sparse product as a table of literal cases through `host_spmm_route` (scanrs_host_spmm_route; the pure part of
scan-rs_amd/csrc/spmm_route.hpp, the source launch_spmm_f64 decides by). Every expectation was READ from the code of the commit
before the decision was gathered into that header, never taken from the function under test; the last column of a row names the
line it was read from: k = kernels.hip, t = tiles.hip, d = tiles_dense.inc of that commit (4622fa9).

A row: (id, sizes (n_outer, n_inner, nnz), l, ldx, links, options and flags, expected, source). `expected` holds family, form and
chunks, optionally width (the tile chunk width), even (the family refuses odd leading dimensions: that commit's error) and cand
(tiles_static_candidate). Links are (kind, a_outer) as the walked copy sees them, after mat_apply has folded a trailing
inner-indexed ScaleAxis into the panel. Forms as include/scanrs_amd.h packs them.

The sliver branch of the tile route (a last chunk under 16 columns goes to the plain gather) is NOT dead: the narrowest panel that
reaches it is 4591 columns (45 chunks of 104, the last one 15), found by walking the chunk rule over every width; no solver makes
such a panel, and no GPU test does."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILES, GATHER2D, GATHER2D_F32, SLICE_WALK, SPMV2D, SPMV_LDS, SPMV, GATHER = 1, 2, 3, 4, 5, 6, 7, 8
SLIVER = 1 << 16
SCALE, LN, LOG2, LOG10, SQUARE, BINOM_DEV, BINOM_PEARSON = 1, 2, 3, 4, 5, 6, 7
OUTER, INNER = 1, 0

SMALL = (1000, 1000, 10 ** 5)            # below blocked_min_nnz (2**22)
MID = (1000, 1000, 1 << 22)              # at blocked_min_nnz, below the auto tile threshold (2**24)
BIG = (10 ** 6, 33000, 1 << 24)          # at the auto tile threshold
SHORT = (48, (1 << 19) + 1, (1 << 22) + 1)    # few long vectors against a vector beyond L2
LONG = (1 << 16, 18433, (1 << 22) + 1)        # many vectors against a vector of two LDS parts
AVAIL = {"tiles_available": True}


def E(family, form=0, chunks=1, **more):
    return dict(family=family, form=form, chunks=chunks, **more)


def tform(dense=0, unit=0, wsrc=0, fold=0):
    """fold: 0 none, 1 the inner side's factor, 2 the outer side's"""
    return dense | unit << 1 | wsrc << 2 | fold << 4


RAW = ()
SQ_OUTER = ((SCALE, OUTER), (SQUARE, 0))                   # sq_axis0 under dot / sq_axis1 under rdot (the trailing inner scale rides in the panel)
SQ_INNER = ((SCALE, INNER), (SQUARE, 0), (SCALE, OUTER))   # sq_axis1 under dot / sq_axis0 under rdot
LOG_OUTER = ((SCALE, OUTER), (LOG2, 0))
LOG_INNER = ((SCALE, INNER), (LOG2, 0), (SCALE, OUTER))
SQ_BOTH = ((SCALE, OUTER), (SCALE, INNER), (SQUARE, 0))
DEV, PEARSON = ((BINOM_DEV, OUTER),), ((BINOM_PEARSON, INNER),)

ROWS = [
    # ---- every path, f64 and f32 panels, a 100-column panel ---------------------------------------------------------------------
    ("p0_f64_small", SMALL, 100, 100, RAW, {}, E(GATHER, cand=0), "k:1965 (auto: t:1594 nnz), k:1977 nnz < blocked_min_nnz, k:2080"),
    ("p0_f32_small", SMALL, 100, 100, RAW, {"panel_precision": 1}, E(GATHER), "k:1977, k:2080"),
    ("p1_f64", MID, 100, 100, RAW, {"spmm_path": 1}, E(GATHER, even=0), "k:1977 path 1 wants no 2d, k:2080"),
    ("p1_f32", MID, 100, 100, RAW, {"spmm_path": 1, "panel_precision": 1}, E(GATHER), "k:1977, k:2080"),
    ("p2_f64", SMALL, 100, 100, RAW, {"spmm_path": 2}, E(GATHER2D, even=1, cand=0), "k:1965 path 2 never tiles, k:1977-1982"),
    ("p2_f32", SMALL, 100, 100, RAW, {"spmm_path": 2, "panel_precision": 1}, E(GATHER2D_F32, even=0), "k:1979-1980"),
    ("p3_f64", SMALL, 100, 100, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), width=100, cand=1), "k:1964-1965; form d:1075-1085"),
    ("p3_f32", SMALL, 100, 100, RAW, {"spmm_path": 3, "panel_precision": 1, **AVAIL}, E(TILES, tform(1, 0, 1, 1), cand=1), "k:1965: a forced path 3 ignores the precision"),
    ("p3_no_layout", SMALL, 100, 100, RAW, {"spmm_path": 3}, E(GATHER2D, cand=1), "k:1977 (the flag off: what is below the tile attempt)"),
    ("p0_big_layout", BIG, 100, 100, RAW, AVAIL, E(TILES, tform(1, 0, 1, 1), cand=1), "k:1965, t:1593-1598"),
    ("p0_big_no_layout", BIG, 100, 100, RAW, {}, E(GATHER2D, cand=1), "k:1965 spmm_tiles_auto false, k:1977"),
    ("p0_big_f32", BIG, 100, 100, RAW, {"panel_precision": 1, **AVAIL}, E(GATHER2D_F32, cand=0), "k:1965 f64 panels on the auto path, k:1979"),
    # ---- widths ----------------------------------------------------------------------------------------------------------------
    ("p3_l1", SMALL, 1, 2, RAW, {"spmm_path": 3, **AVAIL}, E(GATHER2D, cand=0), "k:1964 l >= 16, k:1977: path 3 wants 2d before the narrow routes"),
    ("p3_l2", SMALL, 2, 2, RAW, {"spmm_path": 3, **AVAIL}, E(GATHER2D), "k:1977"),
    ("p3_l3", SMALL, 3, 4, RAW, {"spmm_path": 3, **AVAIL}, E(GATHER2D), "k:1977"),
    ("p3_l15", SMALL, 15, 16, RAW, {"spmm_path": 3, **AVAIL}, E(GATHER2D, cand=0), "k:1964"),
    ("p3_l16", SMALL, 16, 16, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), 1, width=16), "k:1962-1964"),
    ("p3_l104", SMALL, 104, 104, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), 1, width=104), "k:1962-1963"),
    ("p3_l106", SMALL, 106, 106, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), 2, width=54), "k:1962-1963: 2 x 54 (54 + 52), no sliver"),
    ("p3_l200", SMALL, 200, 200, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), 2, width=100), "k:1959-1963"),
    ("p3_l500", SMALL, 500, 500, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), 5, width=100), "k:1959-1963"),
    ("p3_l4591_sliver", SMALL, 4591, 4592, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), 45 | SLIVER, width=104), "k:1966-1971: 44 x 104 + 15"),
    ("p3_l4590_no_sliver", SMALL, 4590, 4590, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), 45, width=102), "k:1962-1963"),
    ("p0_l1", SMALL, 1, 2, RAW, {}, E(SPMV, even=1), "k:1985, k:2066-2078"),
    ("p0_l2", SMALL, 2, 2, RAW, {}, E(SPMV, even=1), "k:1985"),
    ("p0_l3", SMALL, 3, 4, RAW, {}, E(GATHER, even=0), "k:1985 l <= 2, k:2080"),
    ("p0_mid_l15", MID, 15, 16, RAW, {}, E(GATHER), "k:1977 l >= 16"),
    ("p0_mid_l16", MID, 16, 16, RAW, {}, E(GATHER2D, cand=0), "k:1977; t:1594: below 2**24 no tiles"),
    # ---- the narrow routes' thresholds, one below and at -----------------------------------------------------------------------------
    ("sw_inner_below", (48, (1 << 19) - 1, (1 << 22) + 1), 1, 2, RAW, {}, E(SPMV), "k:1988 / 2001 n_inner >= 2**19; k:2028 n_outer"),
    ("sw_inner_at", (48, 1 << 19, (1 << 22) + 1), 1, 2, RAW, {}, E(SLICE_WALK, 0, even=1), "k:1988-1998"),
    ("sw_l2", (48, 1 << 19, (1 << 22) + 1), 2, 2, RAW, {}, E(SPMV2D, 0), "k:1988 l == 1, k:2001"),
    ("sw_nnz_below", (48, 1 << 19, (1 << 22) - 1), 1, 2, RAW, {}, E(SPMV), "k:1988 / 2001 / 2028 nnz >= blocked_min_nnz"),
    ("sw_nnz_at", (48, 1 << 19, 1 << 22), 1, 2, RAW, {}, E(SLICE_WALK), "k:1988"),
    ("sw_long_outer", ((1 << 19) + 1, 1 << 19, (1 << 22) + 1), 1, 2, RAW, {}, E(SPMV2D), "k:1988 !long_outer, k:2001"),
    ("lds_outer_below", ((1 << 16) - 1, 18433, (1 << 22) + 1), 1, 2, RAW, {}, E(SPMV), "k:2028 n_outer >= 2**16"),
    ("lds_outer_at", LONG, 1, 2, RAW, {}, E(SPMV_LDS, 0, even=1), "k:2028, k:2044-2061: no link, no row table"),
    ("lds_l2", LONG, 2, 2, RAW, {}, E(SPMV), "k:2028 l == 1"),
    ("lds_inner_8191", (1 << 16, 8191, (1 << 22) + 1), 1, 2, RAW, {}, E(SPMV), "k:2028 n_inner >= 8192"),
    ("lds_inner_8192", (1 << 16, 8192, (1 << 22) + 1), 1, 2, RAW, {}, E(SPMV_LDS), "k:2028"),
    ("lds_inner_top", (1 << 16, 8 * 18432, (1 << 22) + 1), 1, 2, RAW, {}, E(SPMV_LDS), "k:2029 n_inner <= 8 * 18432"),
    ("lds_inner_over", (1 << 16, 8 * 18432 + 1, (1 << 22) + 1), 1, 2, RAW, {}, E(SPMV), "k:2029"),
    ("lds_nnz_below", (1 << 16, 18433, (1 << 22) - 1), 1, 2, RAW, {}, E(SPMV), "k:2028"),
    ("auto_nnz_below", (10 ** 6, 33000, (1 << 24) - 1), 100, 100, RAW, AVAIL, E(GATHER2D, cand=0), "t:1594"),
    ("auto_nnz_at", BIG, 100, 100, RAW, AVAIL, E(TILES, tform(1, 0, 1, 1), cand=1), "t:1594"),
    ("auto_min_nnz_below", (10 ** 6, 33000, (1 << 25) - 1), 100, 100, RAW, {"blocked_min_nnz": 1 << 25, **AVAIL}, E(GATHER, cand=0), "t:1594 max(blocked_min_nnz, 2**24), k:1977"),
    ("auto_min_nnz_at", (10 ** 6, 33000, 1 << 25), 100, 100, RAW, {"blocked_min_nnz": 1 << 25, **AVAIL}, E(TILES, tform(1, 0, 1, 1), cand=1), "t:1594"),
    ("visits_fit", (32 << 16, 48 * ((1 << 16) - 1), 1 << 24), 100, 100, RAW, AVAIL, E(TILES, tform(1, 0, 1, 1), cand=1), "t:1596: 2**16 x (2**16 - 1) visits"),
    ("visits_over", (32 << 16, 48 << 16, 1 << 24), 100, 100, RAW, AVAIL, E(GATHER2D, cand=0), "t:1596: 2**32 visits"),
    ("visits_over_forced", (32 << 16, 48 << 16, 1 << 24), 100, 100, RAW, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1), cand=1), "k:1965: the forced path asks no visit index"),
    # ---- switches off -----------------------------------------------------------------------------------------------------------------
    ("slice_walk_off", SHORT, 1, 2, RAW, {"slice_walk": 0}, E(SPMV2D, 0), "k:1988, k:2001"),
    ("slice_walk_off_fused", SHORT, 1, 2, LOG_INNER, {"slice_walk": 0}, E(SPMV2D, 2), "k:2011: the first link's inner scale interleaved; no materialized values on this route"),
    ("spmv2d_ld4_not_fused", SHORT, 1, 4, LOG_INNER, {"slice_walk": 0}, E(SPMV2D, 0), "k:2011 ldx == 2"),
    ("spmv_lds_off", LONG, 1, 2, RAW, {"spmv_lds": 0}, E(SPMV), "k:2028"),
    ("row_table", LONG, 1, 2, LOG_OUTER, {}, E(SPMV_LDS, 2), "k:2044-2045, k:2056"),
    ("row_table_off", LONG, 1, 2, LOG_OUTER, {"spmv_row_table": 0}, E(SPMV_LDS, 1), "k:2044, k:2046 (a logarithm: values for the ALU's sake, k:1619-1631)"),
    ("row_table_off_square", LONG, 1, 2, SQ_OUTER, {"spmv_row_table": 0}, E(SPMV_LDS, 0), "k:1624: a square is not heavy"),
    ("lds_values", LONG, 1, 2, LOG_INNER, {}, E(SPMV_LDS, 1), "k:2045 an inner-indexed scale, k:2046"),
    ("lds_values_off", LONG, 1, 2, LOG_INNER, {"materialize": 0}, E(SPMV_LDS, 0), "k:1620"),
    ("lds_values_no_room", LONG, 1, 2, LOG_INNER, {"values_room": False}, E(SPMV_LDS, 0), "k:1627-1630"),
    ("lds_binomial", LONG, 1, 2, DEV, {}, E(SPMV_LDS, 1), "k:2044 map_is_simple, k:1624"),
    ("tile_auto_off", BIG, 100, 100, RAW, {"tile_auto": 0, **AVAIL}, E(GATHER2D, cand=0), "t:1594"),
    ("p1_short", SHORT, 1, 2, RAW, {"spmm_path": 1}, E(SPMV, even=1), "k:1988 / 2001 spmm_path != 1"),
    ("p1_long", LONG, 1, 2, RAW, {"spmm_path": 1}, E(SPMV), "k:2028 spmm_path != 1"),
    ("p2_short_l1", SHORT, 1, 2, RAW, {"spmm_path": 2}, E(GATHER2D), "k:1977-1978"),
    # ---- materialized values and the slice walk's chain ---------------------------------------------------------------------------------
    ("sw_values", SHORT, 1, 2, SQ_INNER, {}, E(SLICE_WALK, 1), "k:1991-1994, k:1606-1616"),
    ("sw_values_log", SHORT, 1, 2, LOG_INNER, {}, E(SLICE_WALK, 1), "k:1993"),
    ("sw_lazy", SHORT, 1, 2, SQ_INNER, {"materialize": 0}, E(SLICE_WALK, 4), "k:1994 chain from 0, k:1675: the scale staged beside the vector"),
    ("sw_lazy_no_room", SHORT, 1, 2, SQ_INNER, {"values_room": False}, E(SLICE_WALK, 4), "k:1613-1615, k:1994"),
    ("sw_outer_chain", SHORT, 1, 2, SQ_OUTER, {}, E(SLICE_WALK, 0), "k:1611: no inner-indexed link, nothing kept"),
    ("sw_chain_refused", SHORT, 1, 2, SQ_BOTH, {"materialize": 0}, E(SPMV2D, 0), "k:1675-1678: an inner scale behind the first link, k:2001, k:2011"),
    ("sw_chain_values", SHORT, 1, 2, SQ_BOTH, {}, E(SLICE_WALK, 1), "k:1993-1994"),
    # ---- odd leading dimensions: that commit's error or fall-through ----------------------------------------------------------------------
    ("odd_narrow", SMALL, 1, 1, RAW, {}, E(SPMV, even=1), "k:1986 fails"),
    ("odd_p3", SMALL, 100, 101, RAW, {"spmm_path": 3, **AVAIL}, E(GATHER2D, even=1, cand=0), "t:1581 no tiles, k:1977, k:1720 fails"),
    ("odd_p2_f32", SMALL, 100, 101, RAW, {"spmm_path": 2, "panel_precision": 1}, E(GATHER2D_F32, even=0), "k:1905-1938: no test"),
    ("odd_p1", SMALL, 100, 101, RAW, {"spmm_path": 1}, E(GATHER, even=0), "k:2080"),
    # ---- nothing to do -----------------------------------------------------------------------------------------------------------------------
    ("l0", SMALL, 0, 0, RAW, {}, E(GATHER, cand=0), "k:1985 l > 0, k:2080"),
    ("l0_p2", SMALL, 0, 0, RAW, {"spmm_path": 2}, E(GATHER), "k:1978 l > 0"),
    ("no_outer_l1", (0, 1000, 0), 1, 2, RAW, {}, E(GATHER), "k:1985 n_outer > 0"),
    ("no_outer_p3", (0, 1000, 0), 100, 100, RAW, {"spmm_path": 3, **AVAIL}, E(GATHER, cand=0), "t:1581, k:1978"),
    ("no_inner_l1", (10, 0, 0), 1, 2, RAW, {}, E(SPMV), "k:1985: n_inner is not asked"),
    ("no_inner_p2", (10, 0, 0), 100, 100, RAW, {"spmm_path": 2}, E(GATHER), "k:1978 n_inner > 0"),
    ("no_nnz_p3", (1000, 1000, 0), 100, 100, RAW, {"spmm_path": 3, **AVAIL}, E(GATHER2D, cand=0), "t:1581 nnz > 0, k:1977"),
    # ---- the inner-side table at its 4 GB bound (nothing is allocated: a number in the query) -------------------------------------------
    ("tabi_last", (1000, 33553394, 10 ** 6), 100, 100, LOG_INNER, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 2, 2)), "d:1083-1084: (192 + 16 x 33553906) x 8 < 0xFFFF0000"),
    ("tabi_beyond", (1000, 33553395, 10 ** 6), 100, 100, LOG_INNER, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 0, 2)), "d:1084-1085: the stream, still folded"),
    ("tabo_beyond", (1000, 33553395, 10 ** 6), 100, 100, LOG_OUTER, {"spmm_path": 3, **AVAIL}, E(TILES, tform(1, 0, 1, 1)), "d:1084: the bound is the inner table's"),
]

# ---- the tile form: maps x tile_dense x tile_ku x tile_wtab x tile_fold ----------------------------------------------------------------------
# t:1138-1157 tile_map_separable: "O" separable and the outer side owns the nonlinear links (or there are none), "I" the inner side, "N" not
TILE_MAPS = {"raw": (RAW, "O"), "sq_outer": (SQ_OUTER, "O"), "sq_inner": (SQ_INNER, "I"), "log_outer": (LOG_OUTER, "O"), "log_inner": (LOG_INNER, "I"),
             "sq_both": (SQ_BOTH, "N"), "binom_dev": (DEV, "N"), "binom_pearson": (PEARSON, "N")}
# (class, tile_dense, tile_ku, tile_wtab, tile_fold) -> form. Fixed positions (t:1169): unit mode with unit positions under a separable
# map, nothing else matters. Dense records (d:1055-1085): no unit mode; folded when separable and tile_fold; the table when folded and
# tile_wtab, by place ("O") or by inner position ("I").
TILE_FORMS = {
    ("O", 0, 0, 0, 0): 0, ("O", 0, 0, 0, 1): 0, ("O", 0, 0, 1, 0): 0, ("O", 0, 0, 1, 1): 0, ("O", 0, 1, 0, 0): 2, ("O", 0, 1, 0, 1): 2, ("O", 0, 1, 1, 0): 2, ("O", 0, 1, 1, 1): 2,
    ("I", 0, 0, 0, 0): 0, ("I", 0, 0, 0, 1): 0, ("I", 0, 0, 1, 0): 0, ("I", 0, 0, 1, 1): 0, ("I", 0, 1, 0, 0): 2, ("I", 0, 1, 0, 1): 2, ("I", 0, 1, 1, 0): 2, ("I", 0, 1, 1, 1): 2,
    ("N", 0, 0, 0, 0): 0, ("N", 0, 0, 0, 1): 0, ("N", 0, 0, 1, 0): 0, ("N", 0, 0, 1, 1): 0, ("N", 0, 1, 0, 0): 0, ("N", 0, 1, 0, 1): 0, ("N", 0, 1, 1, 0): 0, ("N", 0, 1, 1, 1): 0,
    ("O", 1, 0, 0, 0): 1, ("O", 1, 0, 0, 1): 17, ("O", 1, 0, 1, 0): 1, ("O", 1, 0, 1, 1): 21, ("O", 1, 1, 0, 0): 1, ("O", 1, 1, 0, 1): 17, ("O", 1, 1, 1, 0): 1, ("O", 1, 1, 1, 1): 21,
    ("I", 1, 0, 0, 0): 1, ("I", 1, 0, 0, 1): 33, ("I", 1, 0, 1, 0): 1, ("I", 1, 0, 1, 1): 41, ("I", 1, 1, 0, 0): 1, ("I", 1, 1, 0, 1): 33, ("I", 1, 1, 1, 0): 1, ("I", 1, 1, 1, 1): 41,
    ("N", 1, 0, 0, 0): 1, ("N", 1, 0, 0, 1): 1, ("N", 1, 0, 1, 0): 1, ("N", 1, 0, 1, 1): 1, ("N", 1, 1, 0, 0): 1, ("N", 1, 1, 0, 1): 1, ("N", 1, 1, 1, 0): 1, ("N", 1, 1, 1, 1): 1,
}


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def _route(sa, sizes, l, ldx, links, opts):
    got = sa.host_spmm_route(sizes[0], sizes[1], sizes[2], l, ldx, links, **opts)
    return dict(zip(("family", "form", "chunks", "width", "even", "cand"), got))


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_route_table(sa, row):
    name, sizes, l, ldx, links, opts, want, src = row
    got = _route(sa, sizes, l, ldx, links, opts)
    assert {k: got[k] for k in want} == want, (name, src, got)


def test_the_table_covers_what_it_should():
    assert len({r[0] for r in ROWS}) == len(ROWS)
    assert {r[5].get("spmm_path", 0) for r in ROWS} == {0, 1, 2, 3}
    assert {1, 2, 3, 15, 16, 100, 104, 106, 200, 500} <= {r[2] for r in ROWS}
    assert {r[6]["family"] for r in ROWS} == {TILES, GATHER2D, GATHER2D_F32, SLICE_WALK, SPMV2D, SPMV_LDS, SPMV, GATHER}
    assert len(TILE_FORMS) == 3 * 16 and tform(1, 0, 1, 1) == 21 and tform(1, 0, 2, 2) == 41 and tform(1, 0, 0, 1) == 17 and tform(1, 0, 0, 2) == 33


@pytest.mark.parametrize("name", sorted(TILE_MAPS))
def test_tile_form_table(sa, name):
    links, cls = TILE_MAPS[name]
    for (c, dense, ku, wtab, fold), form in TILE_FORMS.items():
        if c != cls:
            continue
        opts = dict(spmm_path=3, tile_dense=dense, tile_ku=ku, tile_wtab=wtab, tile_fold=fold, tiles_available=True)
        got = _route(sa, SMALL, 100, 100, links, opts)
        assert (got["family"], got["form"], got["chunks"]) == (TILES, form, 1), (name, opts, got)


def test_the_chunk_rule_has_a_sliver_only_from_4591_columns_on(sa):
    """the rule as launch_spmm_f64 had it (k:1962-1968), walked over every width a solver could ask for"""
    slivers = []
    for l in range(16, 6000):
        n = (l + 103) // 104
        lc = (((l + n - 1) // n) + 1) & ~1
        last = l - (n - 1) * lc
        assert 0 < last <= lc <= 104
        if last < 16:
            slivers.append(l)
    assert slivers[0] == 4591
    got = sa.host_spmm_route(1000, 1000, 10 ** 5, 4591, 4592, (), tiles_available=True, spmm_path=3)
    assert got[2] == 45 | SLIVER


def test_unknown_option_and_too_many_links_are_refused(sa):
    with pytest.raises(sa.ScanrsError):
        sa.host_spmm_route(10, 10, 10, 1, 2, (), no_such_option=1)
    with pytest.raises(sa.ScanrsError):
        sa.host_spmm_route(10, 10, 10, 1, 2, ((SCALE, OUTER),) * 9)
