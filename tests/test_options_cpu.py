"""The tables of options and counters (scan-rs_amd/csrc/options.cpp) through the host-only entries scanrs_host_option_info,
scanrs_host_option_parse and scanrs_host_counter_name: the frozen key sets, every default, and what each key accepts, refuses and
stores. Every expectation is written out here — the keys and ranges from the chains of scanrs_mat_set_option, scanrs_set_global_option
and scanrs_mat_get_counter of the commit before the tables (182d0e2, capi.cpp), the defaults from the initialisers of `Storage` in
that commit's common.hpp (and GlobalOptions of common_err.hpp) — never taken from the library under test."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAN, INF = float("nan"), float("inf")

# ---- what the setters accept: key -> (lo, hi), written out ------------------------------------------------------------------------
INTEGERS = {"tile_k": (2, 4), "tile_ku": (0, 1), "tile_t": (8, 96), "tile_b": (2, 24), "side_build": (0, 2), "spmm_order": (0, 2), "col_moments": (0, 2),
            "merge_fused": (0, 1), "subset_scatter": (0, 1), "sseq_grid_cap": (1, 16384), "d2h_threads": (1, 256), "hot_segment": (0, 4294967295)}
KILOBYTES = {"ov_tile_kb": (0, 4194304), "l2_tile_kb": (64, 4194304)}
FLAGS = ("dense_side_no_lds", "tile_split", "tile_build_one_pass", "tile_weights_wide", "tile_dense", "tile_wtab", "tile_fold", "tile_one_walk",
         "tile_emit_staged", "tile_builder", "tile_auto", "tile_overlap", "materialize", "slice_walk", "spmv_lds", "overlap", "device_factor",
         "tile_spare_cus", "tile_poison_slack", "spmv_row_table", "gemm_direct")
REALS = {"tile_split_x": (0.05, 16.0, True), "tile_split_min": (0.0, 16.0, False), "tile_max_overflow": (0.0, 1.0, True), "reuse_cmax": (0.0, INF, True)}  # (lo, hi, lo is open)
TRUNCATED = {"tile_big_list_cap": (0.0, 4e9), "tile_build_waves": (0.0, 32.0)}
HANDLE_KEYS = sorted(list(INTEGERS) + list(KILOBYTES) + list(FLAGS) + list(REALS) + list(TRUNCATED) + ["tile_s", "tile_sort_slots", "sync_timeout_s"])
UNSETTABLE = ("spmm_path", "panel_precision", "blocked_min_nnz")
GLOBAL_KEYS = sorted(["h5_threads", "eig_threads", "knn_exhaustive", "knn_filter_min_points", "knn_ratio", "knn_block_rows", "knn_stats",
                      "device_cache_fraction", "sync_timeout_s"])
COUNTERS = sorted(
    ["bk_host_retries", "bk_q", "bk_b", "bk_coef_valid", "bk_flagged_older", "bk_limit_branch", "bk_limit_bits", "bk_direct_columns", "bk_last_direct",
     "bk_full_direct", "bk_early_projections", "bk_cmax_dense_bits", "spmm_route", "spmm_form", "spmm_chunks", "transpose_route", "partition_rounds",
     "partition_allreduces", "de_pairs_passes", "de_pairs_literal", "de_shard_tests", "de_shard_allreduces", "subset_masked_passes",
     "subset_scatter_passes", "subset_allreduces", "knn_blocks", "knn_allreduces", "knn_blocks_filtered", "reshard_upload_us", "reshard_count_us",
     "reshard_split_us", "reshard_exchange_us", "reshard_transpose_us", "regather_plan_us", "regather_pull_us", "regather_finish_us", "export_plan_us",
     "export_pull_us", "export_encode_us", "t_layout_us", "t_side_wait_us", "t_start_panel_us", "t_delivery_us", "t_alloc_us", "alloc_calls",
     "tile_positions", "tile_served_nonzeros", "tile_overflow_nonzeros"])
# the defaults, in each key's own unit
HANDLE_DEFAULTS = {
    "tile_k": 2, "tile_s": 32, "tile_ku": 1, "tile_t": 48, "tile_b": 4, "side_build": 1, "tile_split": 1, "tile_split_x": 1.8, "tile_split_min": 0.5,
    "tile_build_one_pass": 1, "tile_weights_wide": 1, "tile_dense": 1, "tile_sort_slots": 2, "tile_emit_staged": 1, "tile_wtab": 1, "tile_fold": 1,
    "tile_big_list_cap": 0, "tile_one_walk": 1, "tile_builder": 1, "tile_build_waves": 0, "ov_tile_kb": 0, "tile_max_overflow": 0.35, "tile_auto": 1,
    "tile_overlap": 1, "subset_scatter": 1, "sseq_grid_cap": 16384, "merge_fused": 1, "l2_tile_kb": 3584, "spmm_order": 1, "hot_segment": 512,
    "slice_walk": 1, "spmv_lds": 1, "dense_side_no_lds": 0, "overlap": 1, "col_moments": 1, "device_factor": 1, "d2h_threads": 4, "tile_poison_slack": 0,
    "tile_spare_cus": 1, "spmv_row_table": 1, "gemm_direct": 1, "reuse_cmax": 1e5, "materialize": 1, "sync_timeout_s": 120,
    "spmm_path": 0, "panel_precision": 0, "blocked_min_nnz": 1 << 22}
GLOBAL_DEFAULTS = {"h5_threads": 8, "eig_threads": 4, "knn_exhaustive": 0, "knn_filter_min_points": 32768, "knn_ratio": 4, "knn_block_rows": 262144,
                   "knn_stats": 0, "device_cache_fraction": 0.5, "sync_timeout_s": 120}
ROUTE_OPTIONS = ("spmm_path", "panel_precision", "tile_auto", "tile_k", "tile_s", "tile_t", "tile_b", "tile_ku", "tile_dense", "tile_builder",
                 "blocked_min_nnz", "slice_walk", "spmv_lds", "spmv_row_table", "spmm_order", "materialize", "tile_wtab", "tile_fold")
REFUSED = None


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def check(sa, key, value, want, scope=0):
    if want is REFUSED:
        with pytest.raises(sa.ScanrsError) as e:
            sa.host_option_parse(key, value, scope)
        assert e.value.code == 6, (key, value)  # SCANRS_ERR_ARGUMENT
    else:
        assert sa.host_option_parse(key, value, scope) == want, (key, value)


def test_the_key_sets_are_frozen(sa):
    rows = sa.option_info(0)
    assert len(HANDLE_KEYS) == 44 and len(GLOBAL_KEYS) == 9 and len(COUNTERS) == 48
    assert sorted(o["name"] for o in rows if o["settable"]) == HANDLE_KEYS
    assert sorted(o["name"] for o in rows if not o["settable"]) == sorted(UNSETTABLE)
    assert len({o["name"] for o in rows}) == len(rows) == 47
    assert sorted(o["name"] for o in sa.option_info(1)) == GLOBAL_KEYS and all(o["settable"] for o in sa.option_info(1))
    assert sorted(sa.counter_names()) == COUNTERS and len(sa.counter_names()) == 48
    with pytest.raises(sa.ScanrsError):
        sa.option_info(2)


def test_every_default_is_the_one_the_handle_had(sa):
    assert {o["name"]: o["default"] for o in sa.option_info(0)} == HANDLE_DEFAULTS
    assert {o["name"]: o["default"] for o in sa.option_info(1)} == GLOBAL_DEFAULTS


def test_the_reported_bounds_are_the_ones_the_parser_holds(sa):
    info = {o["name"]: o for o in sa.option_info(0)}
    for key, (lo, hi) in {**INTEGERS, **KILOBYTES, **TRUNCATED, "tile_s": (28, 32)}.items():
        assert (info[key]["lo"], info[key]["hi"], info[key]["open_lo"]) == (lo, hi, False), key
    for key, (lo, hi, open_lo) in REALS.items():
        assert (info[key]["lo"], info[key]["hi"], info[key]["open_lo"]) == (lo, hi, open_lo), key
    assert (info["sync_timeout_s"]["lo"], info["sync_timeout_s"]["hi"], info["sync_timeout_s"]["open_lo"]) == (0.0, INF, True)


@pytest.mark.parametrize("key", sorted(INTEGERS) + sorted(KILOBYTES))
def test_integer_keys_take_whole_numbers_in_their_closed_range(sa, key):
    lo, hi = {**INTEGERS, **KILOBYTES}[key]
    unit = 1024 if key in KILOBYTES else 1
    for bad in (NAN, INF, -INF, lo - 1, lo + 0.5, hi + 1, hi - 0.5):
        check(sa, key, bad, REFUSED)
    for good in (lo, hi, (lo + hi) // 2):
        check(sa, key, float(good), good * unit)


def test_tile_s_is_28_or_32(sa):
    for bad in (NAN, INF, -INF, 27, 28.5, 29, 30, 31, 33):
        check(sa, "tile_s", bad, REFUSED)
    check(sa, "tile_s", 28, 28)
    check(sa, "tile_s", 32, 32)


@pytest.mark.parametrize("key", FLAGS)
def test_flags_take_any_finite_value(sa, key):
    for bad in (NAN, INF, -INF):
        check(sa, key, bad, REFUSED)
    for value, want in ((-1, 1), (0, 0), (0.5, 1), (1, 1), (2, 1), (1e300, 1)):
        check(sa, key, value, want)


def test_tile_sort_slots_is_three_way(sa):
    for bad in (NAN, INF, -INF):
        check(sa, "tile_sort_slots", bad, REFUSED)
    for value, want in ((0, 0), (1, 1), (2, 2), (3, 1), (-1, 1), (0.5, 1)):
        check(sa, "tile_sort_slots", value, want)


@pytest.mark.parametrize("key", sorted(REALS))
def test_real_keys_are_stored_as_given(sa, key):
    lo, hi, open_lo = REALS[key]
    for bad in (NAN, INF, -INF, lo - 1):
        check(sa, key, bad, REFUSED)
    check(sa, key, lo, REFUSED if open_lo else lo)  # an open bound is refused exactly at the bound
    check(sa, key, lo + 0.5, lo + 0.5)
    check(sa, key, math.nextafter(lo, INF), math.nextafter(lo, INF))
    if hi < INF:
        check(sa, key, hi, hi)
        check(sa, key, hi + 1, REFUSED)
        check(sa, key, math.nextafter(hi, INF), REFUSED)
    else:
        check(sa, key, 1e300, 1e300)


def test_truncated_keys_need_not_be_whole(sa):
    for key, (lo, hi) in TRUNCATED.items():
        for bad in (NAN, INF, -INF, lo - 1, -0.5, hi + 1, hi + 0.5):
            check(sa, key, bad, REFUSED)
        for value, want in ((lo, lo), (lo + 0.5, 0), (hi, hi), (hi - 0.5, hi - 1)):
            check(sa, key, value, want)
    check(sa, "tile_big_list_cap", 2.5, 2)
    check(sa, "tile_build_waves", 7.9, 7)


def test_sync_timeout_is_positive_and_finite_under_both_setters(sa):
    for scope in (0, 1):
        for bad in (NAN, INF, -INF, -1, 0, -0.0):
            check(sa, "sync_timeout_s", bad, REFUSED, scope)
        for good in (0.5, 1, 120, 1e300, 5e-324):
            check(sa, "sync_timeout_s", good, good, scope)


def test_global_options_clamp_and_refuse_what_is_not_finite(sa):
    for key, lo in (("h5_threads", 1), ("eig_threads", 1), ("knn_block_rows", 1), ("knn_filter_min_points", 0), ("knn_ratio", 2)):
        for bad in (NAN, INF, -INF):
            check(sa, key, bad, REFUSED, 1)
        for value, want in ((lo - 1, lo), (-1e300, lo), (lo, lo), (lo + 0.5, lo), (lo + 5, lo + 5), (1000.9, 1000)):
            check(sa, key, value, want, 1)
    check(sa, "knn_ratio", 1, 2, 1)
    check(sa, "h5_threads", 0, 1, 1)
    for key in ("knn_exhaustive", "knn_stats"):
        for value, want in ((0, 0), (1, 1), (-1, 1), (0.5, 1), (7, 1)):
            check(sa, key, value, want, 1)
    for bad in (NAN, INF, -INF, 1.5, -0.1, math.nextafter(1.0, INF)):
        check(sa, "device_cache_fraction", bad, REFUSED, 1)
    for good in (0.0, 0.5, 1.0):
        check(sa, "device_cache_fraction", good, good, 1)


def test_keys_outside_the_tables_are_refused(sa):
    for key in ("no_such", "", "tile_k ", "TILE_K", "ov_tile_bytes") + UNSETTABLE:
        check(sa, key, 1.0, REFUSED)
    for key in ("no_such", "tile_k", "spmm_path"):  # a handle's key is no global one
        check(sa, key, 1.0, REFUSED, 1)
    check(sa, "h5_threads", 1.0, REFUSED, 0)
    with pytest.raises(sa.ScanrsError):
        sa.host_option_parse("tile_k", 2.0, scope=2)
    with pytest.raises(sa.ScanrsError):
        sa.set_global_option("no_such", 1.0)
    for key, bad in (("h5_threads", NAN), ("knn_ratio", INF), ("device_cache_fraction", 1.5), ("sync_timeout_s", 0.0)):
        with pytest.raises(sa.ScanrsError):
            sa.set_global_option(key, bad)


def test_the_route_array_is_decoded_through_the_same_parser(sa):
    assert sa.SPMM_ROUTE_OPTIONS == ROUTE_OPTIONS
    assert [o["name"] for o in sorted((o for o in sa.option_info() if o["route_position"]), key=lambda o: o["route_position"])] == list(ROUTE_OPTIONS)
    assert [o["route_position"] for o in sa.option_info(1)] == [0] * 9
    base = sa.host_spmm_route(1000, 1000, 10 ** 5, 32, 32)
    assert base == sa.host_spmm_route(1000, 1000, 10 ** 5, 32, 32, **{k: HANDLE_DEFAULTS[k] for k in ROUTE_OPTIONS})
    for bad in (dict(tile_k=NAN), dict(tile_s=31), dict(spmm_path=4), dict(spmm_path=-1), dict(panel_precision=2), dict(tile_t=INF),
                dict(blocked_min_nnz=-1), dict(blocked_min_nnz=2.0 ** 63), dict(blocked_min_nnz=0.5), dict(tile_auto=NAN), dict(spmm_order=3)):
        with pytest.raises(sa.ScanrsError) as e:
            sa.host_spmm_route(1000, 1000, 10 ** 5, 32, 32, **bad)
        assert e.value.code == 6, bad
    # the largest whole number below 2^63 is taken, and it keeps every matrix on the plain gather
    assert sa.host_spmm_route(1000, 1000, 1 << 40, 32, 32, blocked_min_nnz=2.0 ** 63 - 1024)[0] == sa.SPMM_GATHER
    assert sa.host_spmm_route(1000, 1000, 1 << 40, 32, 32)[0] == sa.SPMM_GATHER2D
