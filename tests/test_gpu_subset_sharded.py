"""sum_rows / sum_cols / sum_rows_dual / mean_rows / mean_var_rows over sharded and multi-GPU matrices against the
same calls on one unsharded handle, the correctly rounded restatement tests/subset_ref.py and - for the f64 sums that cross the
shards - the Python-integer restatement of the fixed-point form, tests/subset_sharded_ref.py. Fixture: tests/subset_sharded_case.py
(checked on the CPU by tests/test_subset_sharded_cpu.py). All shards share device 0.

Two forms: a MultiMat (the library cuts the matrix and drives the shards), and handles bound with set_shard to the explicit cuts of
the fixture, one thread per rank, with a host hook that sums the ranks' buffers. Three orientations: genes x cells stored CSC,
cells x genes stored CSR, and the transposed view of the latter; the cells are the sharded dimension in all of them."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import subset_ref as ref  # noqa: E402
import subset_sharded_case as sc  # noqa: E402
import subset_sharded_ref as fx  # noqa: E402
from shard_ring import Ring, run_ranks  # noqa: E402

SHARDS = (1, 2, 3, 5)
FORMS = ("multi", "hook")
ORIENTATIONS = ("csc", "csr", "csr_t")  # the view: genes x cells, cells x genes, genes x cells
MAPS = ("raw", "scale", "log")
SUM_TOL = dict(rtol=1e-12, atol=1e-13)  # the tolerances of tests/test_gpu_subset.py for the same quantities
VAR_TOL = dict(rtol=1e-10, atol=1e-12)


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def close(a, b, rtol, atol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        ok = both_nan | (np.abs(a - b) <= np.abs(b) * rtol + atol)
    assert np.all(ok), float(np.nanmax(np.abs(a - b)))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), int(np.sum(a.view(np.uint64) != b.view(np.uint64)))


# ---- the three forms behind one set of calls ------------------------------------------------------------------------------------------
def _genes_by_cells_views(sa, triplet, n_local, orientation):
    """(the genes x cells view the maps are composed on, a function that gives the view of the orientation)"""
    ip, ix, vv = triplet
    if orientation == "csc":
        g = sa.AdaptiveMat.from_csmat(sc.GENES, n_local, sa.CSC, ip, ix, vv)
        return g, g, (lambda g: g)
    base = sa.AdaptiveMat.from_csmat(n_local, sc.GENES, sa.CSR, ip, ix, vv)  # (the CSC arrays of genes x cells ARE the CSR arrays of its transpose)
    g = base.t()
    return base, g, ((lambda g: g) if orientation == "csr_t" else (lambda g: g.t()))


def _apply_map(sa, g, which, lo, hi):
    """`which` on a genes x cells view that holds cells [lo, hi)."""
    if which == "scale":
        fg, fc = sc.factors()
        g.compose_scale_axis(0, fg).compose_scale_axis(1, fc[lo:hi])
    elif which == "log":
        sa.log_normalize_with_size_factor(g, sc.UMI_COUNT_SUM, sa.FN_LOG2_1P, sc.size_factors()[lo:hi])


class Single:
    """One unsharded handle. sharded_calls: through the *_sharded entry points."""

    world = 0

    def __init__(self, sa, csc, orientation, which, sharded_calls=False):
        self.base, g, view = _genes_by_cells_views(sa, sc.shard_csc(csc, 0, sc.CELLS), sc.CELLS, orientation)
        _apply_map(sa, g, which, 0, sc.CELLS)
        self.h, self.sfx = view(g), "_sharded" if sharded_calls else ""

    def call(self, name, *args, **kw):
        return getattr(self.h, name + self.sfx)(*args, **kw)

    def steps(self):
        return [self.h.counter("subset_allreduces")]

    def option(self, key, value):
        self.h.set_option(key, value)

    def close(self):
        pass


class Hooked:
    """Handles bound with set_shard to the fixture's cut, one thread per rank."""

    def __init__(self, sa, csc, orientation, which, world, fc=None):
        self.sa, self.world, self.ring = sa, world, Ring(world)
        bounds = sc.RANGES[world]
        self.bases, self.hs = [], []
        for r, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            base, g, view = _genes_by_cells_views(sa, sc.shard_csc(csc, lo, hi), hi - lo, orientation)
            base.set_shard(r, world, lo, sc.CELLS, self.ring.hook(r))
            if orientation != "csc":
                g = base.t()  # (a view taken after the binding)
            if fc is not None:
                g.compose_scale_axis(0, sc.factors()[0]).compose_scale_axis(1, fc[lo:hi])
            else:
                _apply_map(sa, g, which, lo, hi)
            self.bases.append(base)
            self.hs.append(view(g))

    def on_all(self, fn):
        out, err = run_ranks(self.world, lambda r: fn(self.hs[r]))
        for e in err:
            if e is not None:
                raise e
        return out

    def call(self, name, *args, **kw):
        out = self.on_all(lambda h: getattr(h, name + "_sharded")(*args, **kw))
        for o in out[1:]:  # complete and identical on every rank
            for a, b in zip(_parts(out[0]), _parts(o)):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        return out[0]

    def steps(self):
        return [h.counter("subset_allreduces") for h in self.hs]

    def option(self, key, value):
        for h in self.hs:
            h.set_option(key, value)

    def close(self):
        pass


class Multi:
    """A MultiMat with all shards on device 0."""

    def __init__(self, sa, csc, orientation, which, world):
        ip, ix, vv = sc.shard_csc(csc, 0, sc.CELLS)
        self.world, self.transposed = world, orientation == "csr_t"
        if orientation == "csc":
            self.mm = sa.MultiMat(sc.GENES, sc.CELLS, sa.CSC, ip, ix, vv, world, devices=[0] * world)
            if which == "scale":
                self.mm.compose_scale_axis(0, sc.factors()[0]).compose_scale_axis(1, sc.factors()[1])
            elif which == "log":
                self.mm.log_normalize(sc.UMI_COUNT_SUM, sa.FN_LOG2_1P, sc.size_factors())
        else:
            assert which != "log"  # (log_normalize wants the cells as the stored matrix's columns)
            self.mm = sa.MultiMat(sc.CELLS, sc.GENES, sa.CSR, ip, ix, vv, world, devices=[0] * world)
            if which == "scale":
                self.mm.compose_scale_axis(1, sc.factors()[0]).compose_scale_axis(0, sc.factors()[1])

    def call(self, name, *args, **kw):
        return getattr(self.mm, name)(*args, transposed=self.transposed, **kw)

    def steps(self):
        return [self.mm.counter("subset_allreduces", i) for i in range(self.world)]

    def option(self, key, value):
        self.mm.set_option(key, value)

    def close(self):
        self.mm.close()


def _make(sa, csc, form, orientation, which, world):
    return Multi(sa, csc, orientation, which, world) if form == "multi" else Hooked(sa, csc, orientation, which, world)


# ---- what every form must give ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    m = sc.matrix()
    return {"m": m, "csc": m.tocsc(), "cells": sc.cell_lists(), "genes": sc.gene_lists()}


def _lists_of(case, orientation):
    return case["genes"] if orientation == "csr" else case["cells"]


def _run(x, lists, with_u64):
    """Every call on every list: name -> result. The u64 calls come first and once more at the end: before the f64 calls have built
    the copy of the other orientation (the scatter route) and after (the masked walk)."""
    out = {}

    def u64(tag):
        for n, c in lists.items():
            out[f"sum_rows_u64{tag}/{n}"] = x.call("sum_rows", c, np.uint64)
            out[f"sum_cols_u64{tag}/{n}"] = x.call("sum_cols", c, np.uint64)
        for a, b in sc.dual_pairs(lists):
            out[f"dual_u64{tag}/{a}+{b}"] = x.call("sum_rows_dual", lists[a], lists[b], np.uint64)

    if with_u64:
        u64("")
    for n, c in lists.items():
        out[f"sum_rows/{n}"] = x.call("sum_rows", c)
        out[f"sum_cols/{n}"] = x.call("sum_cols", c)
        out[f"mean_rows/{n}"] = x.call("mean_rows", c)
        out[f"mean_var_rows/{n}"] = x.call("mean_var_rows", c)
    for a, b in sc.dual_pairs(lists):
        out[f"dual/{a}+{b}"] = x.call("sum_rows_dual", lists[a], lists[b])
    if with_u64:
        u64("_again")
    return out


def _parts(v):
    return v if isinstance(v, tuple) else (v,)


def _restate(dense, lists, view, which):
    """name -> what tests/subset_ref.py gives (correctly rounded sums) and, under "fx/...", what the Python-integer restatement of the
    fixed-point form gives for the results that cross the shards (not for the log map: numpy does not reproduce its terms to the bit)."""
    want = {}
    for n, c in lists.items():
        if which == "raw":
            di = dense.astype(np.uint64)
            want[f"sum_rows_u64/{n}"], want[f"sum_cols_u64/{n}"] = ref.sum_rows(di, c), ref.sum_cols(di, c)
        want[f"sum_rows/{n}"], want[f"sum_cols/{n}"] = ref.sum_rows(dense, c), ref.sum_cols(dense, c)
        want[f"mean_var_rows/{n}"] = ref.mean_var_rows(dense, c)
        want[f"mean_rows/{n}"] = want[f"mean_var_rows/{n}"][0]  # (the same sum and division)
        if which == "log":
            continue
        if view == "cg":
            want[f"fx/sum_cols/{n}"] = fx.sum_cols(dense, c)
        else:
            want[f"fx/sum_rows/{n}"] = fx.sum_rows(dense, c)
            want[f"fx/mean_var_rows/{n}"] = fx.mean_var_rows(dense, c) + (fx.mean_var_rows(dense, c, fused=True)[1],)
    for a, b in sc.dual_pairs(lists):
        want[f"dual/{a}+{b}"] = ref.sum_rows_dual(dense, lists[a], lists[b])
        if which != "log" and view == "gc":
            want[f"fx/dual/{a}+{b}"] = fx.sum_rows_dual(dense, lists[a], lists[b])
    return want


@pytest.fixture(scope="module")
def expected(sa, case):
    """(orientation, map) -> (results of ONE unsharded handle through the plain calls, the restatements), made once and left alone."""
    made = {}

    def get(orientation, which):
        key = ("cg" if orientation == "csr" else "gc", which)
        if key not in made:
            d = sc.mapped_dense(case["m"], which)
            d = np.ascontiguousarray(d.T) if key[0] == "cg" else d
            lists = _lists_of(case, orientation)
            single = _run(Single(sa, case["csc"], "csr" if key[0] == "cg" else "csc", which), lists, which == "raw")
            made[key] = (single, _restate(d, lists, key[0], which))
        return made[key]

    return get


_first_seen = {}  # (view, map, call) -> the first result any form and shard count gave: every other one must hold the same bits


def _crosses(orientation, name):
    """Does this result sum over all ranks (else: it runs along the sharded dimension and is owned by one rank)?"""
    return name.startswith("sum_cols") if orientation == "csr" else not name.startswith("sum_cols")


def _check_all(case, expected, x, orientation, which, label):
    lists = _lists_of(case, orientation)
    single, want = expected(orientation, which)
    got = _run(x, lists, which == "raw")
    view = "cg" if orientation == "csr" else "gc"
    for name, value in got.items():
        call = name.partition("/")[0]
        for k, (g, s) in enumerate(zip(_parts(value), _parts(single[name]))):
            assert g.shape == s.shape and g.dtype == s.dtype, name
            same_bits(g, _first_seen.setdefault((view, which, name, k), g))  # 3a: the same bits whatever the cut, the form and the route
            tol = VAR_TOL if call == "mean_var_rows" and k == 1 else SUM_TOL
            if "u64" in call or not _crosses(orientation, call):
                same_bits(g, s)  # 2 and 3b: integers, and results owned by one rank: the unsharded call's bits
            else:
                close(g, s, **tol)  # 3d, against the unsharded handle
            w = want.get(name.replace("_again", ""))
            if w is None:
                continue
            if "u64" in call:
                assert np.array_equal(g, _parts(w)[k]), name  # 2, against the restatement
            else:
                close(g, _parts(w)[k], **tol)  # 3d, against the correctly rounded sums
        if "fx/" + name in want:  # 3c: the Python-integer restatement, bit for bit
            w = want["fx/" + name]
            if call == "mean_var_rows":
                same_bits(value[0], w[0])
                # (the host line var / len - mean * mean, as written or contracted into one fused multiply-add)
                assert np.array_equal(value[1], w[1], equal_nan=True) or np.array_equal(value[1], w[2], equal_nan=True), name
            else:
                for g, e in zip(_parts(value), _parts(w)):
                    same_bits(g, e)
    for n, c in lists.items():
        if "fx/sum_rows/" + n in want:  # mean_rows: the restated sum, divided
            with np.errstate(invalid="ignore"):
                same_bits(got[f"mean_rows/{n}"], want["fx/sum_rows/" + n] / np.float64(len(c)))
    print(f"{label}: {len(got)} calls checked")


# ---- 1-3. every call, every cut, both forms, three orientations, three maps ---------------------------------------------------------
# (scanrs_multi_log_normalize wants the cells as the columns of the STORED matrix: the hook form alone covers the log map on the CSR forms)
EVERY = [(n, f, o, w) for n in SHARDS for f in FORMS for o in ORIENTATIONS for w in MAPS if not (f == "multi" and w == "log" and o != "csc")]


@pytest.mark.parametrize("n_shards, form, orientation, which", EVERY, ids=lambda v: str(v))
def test_every_call_over_the_shards(sa, case, expected, n_shards, form, orientation, which):
    x = _make(sa, case["csc"], form, orientation, which, n_shards)
    try:
        _check_all(case, expected, x, orientation, which, f"{form} x{n_shards} {orientation} {which}")
        if form == "hook":
            assert x.ring.dtypes == {1}  # 4: the transport is the u64 all-reduce only
    finally:
        x.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_the_routes_give_the_same_bits(sa, case, expected, orientation, form):
    """"subset_scatter" 0: the integer sums build the missing copy instead of scattering from the other one."""
    for which in ("raw", "scale"):
        x = _make(sa, case["csc"], form, orientation, which, 3)
        x.option("subset_scatter", 0)
        try:
            _check_all(case, expected, x, orientation, which, f"{form} x3 {orientation} {which} subset_scatter=0")
        finally:
            x.close()


# ---- 4. further behaviour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_exchange_steps(sa, case, orientation, form):
    """The documented counts: 1 for results along the sharded dimension and for u64 sums that cross the shards, 2 for f64 sums that
    cross them, 0 for an output without entries; the same on every rank."""
    lists = _lists_of(case, orientation)
    c, none = lists["third"], lists["empty"]
    x = _make(sa, case["csc"], form, orientation, "raw", 3)
    rows_cross = orientation != "csr"

    def steps(name, *args):
        if form == "hook":
            x.ring.calls = 0
        x.call(name, *args)
        s = x.steps()
        assert len(set(s)) == 1
        if form == "hook":
            assert x.ring.calls == s[0]
        return s[0]

    try:
        assert steps("sum_rows", c, np.uint64) == 1 and steps("sum_cols", c, np.uint64) == 1
        assert steps("sum_rows_dual", c, lists["half"], np.uint64) == 1
        assert steps("sum_rows", c) == (2 if rows_cross else 1) and steps("mean_rows", c) == (2 if rows_cross else 1)
        assert steps("mean_var_rows", c) == (2 if rows_cross else 1) and steps("sum_rows_dual", c, lists["half"]) == (2 if rows_cross else 1)
        assert steps("sum_cols", c) == (1 if rows_cross else 2)
        assert steps("sum_rows", none) == (2 if rows_cross else 1)  # (the output has entries: zeros)
        assert steps("sum_cols", none) == 0 and steps("sum_cols", none, np.uint64) == 0
    finally:
        x.close()


@pytest.mark.parametrize("n_shards", SHARDS)
def test_a_scale_factor_that_is_not_finite(sa, case, n_shards):
    """An infinite factor on one listed cell: NaN in exactly the genes that hold a count there, on every rank and at every shard
    count (the unsharded call propagates the infinity instead); every other result keeps its bits."""
    lists = case["cells"]
    fg, fc = sc.factors()
    j = int(lists["third"][1001])
    fc = fc.copy()
    fc[j] = np.inf
    counts = case["m"].toarray().astype(np.float64)
    with np.errstate(invalid="ignore"):
        dense = np.where(counts != 0.0, fc[None, :] * (fg[:, None] * counts), 0.0)
    hit = np.flatnonzero(case["m"][:, j].toarray().reshape(-1) != 0)
    assert 0 < hit.size < sc.GENES
    x = Hooked(sa, case["csc"], "csc", "scale", n_shards, fc=fc)
    for n in ("third", "all", "inside"):
        got = x.call("sum_rows", lists[n])
        want = fx.sum_rows(dense, lists[n])
        assert np.array_equal(np.flatnonzero(np.isnan(got)), hit if j in lists[n] else []), n
        assert np.array_equal(got, want, equal_nan=True), n
    mean, var = x.call("mean_var_rows", lists["third"])
    assert np.array_equal(np.flatnonzero(np.isnan(mean)), hit) and np.array_equal(np.flatnonzero(np.isnan(var)), hit)
    same_bits(np.nan_to_num(mean), np.nan_to_num(fx.mean_var_rows(dense, lists["third"])[0]))
    s1, s2 = x.call("sum_rows_dual", lists["inside"], lists["third"])  # the flag of list 2 does not touch list 1
    assert not np.isnan(s1).any() and np.array_equal(np.flatnonzero(np.isnan(s2)), hit)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_empty_lists(sa, case, orientation, form):
    x = _make(sa, case["csc"], form, orientation, "raw", 3)
    n_rows = sc.CELLS if orientation == "csr" else sc.GENES
    try:
        for dt in (np.uint64, np.uint32, np.float64):
            r = x.call("sum_rows", [], dt)
            assert r.shape == (n_rows,) and r.dtype == dt and not r.any()
            assert x.call("sum_cols", [], dt).shape == (0,)
            s1, s2 = x.call("sum_rows_dual", [], [], dt)
            assert s1.shape == (n_rows,) and not s1.any() and not s2.any()
        assert np.isnan(x.call("mean_rows", [])).all()  # 0.0 / 0.0, as unsharded
        mean, var = x.call("mean_var_rows", [])
        assert mean.shape == (n_rows,) and np.isnan(mean).all() and np.isnan(var).all()
    finally:
        x.close()


def _dual_raw(sa, fn, handle_args, c1, c2, snoop, o1, o2):
    s = snoop._struct()
    return fn(*handle_args, sa._p(c1), ctypes.c_uint64(c1.shape[0]), sa._p(c2), ctypes.c_uint64(c2.shape[0]), ctypes.byref(s), sa._p(o1), sa._p(o2))


@pytest.mark.parametrize("dt", [np.uint64, np.float64], ids=["u64", "f64"])
def test_a_cancelled_snoop_leaves_the_outputs_untouched(sa, case, dt):
    c1, c2 = case["cells"]["third"].astype(np.uint64), case["cells"]["half"].astype(np.uint64)
    suffix = "f64" if dt == np.float64 else "u64"
    # every rank of the hook form, the flag set before the call
    x = Hooked(sa, case["csc"], "csc", "raw", 3)
    snoop = sa.AtomicSnoop()
    snoop.cancel()
    fn = getattr(sa._lib, f"scanrs_mat_sum_rows_dual_{suffix}_sharded")

    def rank_call(h):
        o1, o2 = np.full(sc.GENES, 7, dtype=dt), np.full(sc.GENES, 9, dtype=dt)
        rc = _dual_raw(sa, fn, (h._h,), c1, c2, snoop, o1, o2)
        return rc, o1, o2

    for rc, o1, o2 in x.on_all(rank_call):
        assert rc == 3 and np.all(o1 == 7) and np.all(o2 == 9)
    ok = x.call("sum_rows_dual", c1, c2, dt, snoop=sa.AtomicSnoop())  # the handles stay usable
    # a MultiMat, cancelled by its own progress report on the way
    y = Multi(sa, case["csc"], "csc", "raw", 3)
    try:
        for stop_at in (0.0, 0.1):
            sn = sa.AtomicSnoop()
            seen = []

            def on_progress(_ctx, frac, sn=sn, seen=seen, stop_at=stop_at):
                seen.append(frac)
                if frac >= stop_at:
                    sn.cancel()

            sn._cb = sa._PROGRESS_FN(on_progress)
            o1, o2 = np.full(sc.GENES, 7, dtype=dt), np.full(sc.GENES, 9, dtype=dt)
            rc = _dual_raw(sa, getattr(sa._lib, f"scanrs_multi_sum_rows_dual_{suffix}"), (y.mm._h, ctypes.c_int(0)), c1, c2, sn, o1, o2)
            assert rc == 3 and np.all(o1 == 7) and np.all(o2 == 9), (stop_at, seen)
        sn = sa.AtomicSnoop()
        again = y.call("sum_rows_dual", c1, c2, dt, snoop=sn)
        assert sn.history[0] == 0.0 and sn.history[-1] == 1.0 and sn.history == sorted(sn.history)  # only shard 0 reports
        for a, b in zip(again, ok):
            same_bits(a, b)
    finally:
        y.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_refusals_leave_the_handles_usable(sa, case, orientation, form):
    """The plain calls' words; a list is checked against the GLOBAL extent of the sharded dimension."""
    lists = _lists_of(case, orientation)
    extent = sc.GENES if orientation == "csr" else sc.CELLS
    dense = (case["m"].T if orientation == "csr" else case["m"]).toarray().astype(np.uint64)
    x = _make(sa, case["csc"], form, orientation, "raw", 3)
    good = lists["third"]

    def refused(name, args, word):
        with pytest.raises(sa.ScanrsError) as ei:
            x.call(name, *args)
        assert ei.value.code == 6 and word in str(ei.value) and not isinstance(ei.value, sa.CancellationError), str(ei.value)
        assert np.array_equal(x.call("sum_rows", good, np.uint64), ref.sum_rows(dense, good))

    try:
        for name in ("sum_rows", "sum_cols", "mean_rows", "mean_var_rows"):
            refused(name, ([5, 4, 9],), "cols must be strictly ascending")
            refused(name, ([4, 4, 9],), "cols must be strictly ascending")
            refused(name, ([4, extent],), f"the matrix has {extent} columns")
        refused("sum_rows_dual", (good, [9, 3], np.uint64), "cols2")
        refused("sum_rows_dual", ([3, 3], good), "cols1")
        # an index beyond every rank's own extent and inside the global one is served
        assert np.array_equal(x.call("sum_cols", [extent - 1], np.uint64), ref.sum_cols(dense, [extent - 1]))
    finally:
        x.close()
    y = _make(sa, case["csc"], form, orientation, "scale", 3)
    try:
        for name, args in (("sum_rows", (good, np.uint64)), ("sum_cols", (good, np.uint32)), ("sum_rows_dual", (good, good, np.uint64))):
            with pytest.raises(sa.ScanrsError) as ei:
                y.call(name, *args)
            assert ei.value.code == 6 and "raw" in str(ei.value)
        assert y.call("sum_rows", good).shape == (dense.shape[0],)
    finally:
        y.close()


def test_the_plain_entry_points_still_refuse_a_sharded_handle(sa, case):
    x = Hooked(sa, case["csc"], "csc", "raw", 2)
    good = case["cells"]["inside"] - sc.RANGES[2][1]
    for h in x.hs:
        for fn in (lambda: h.sum_rows(good, np.uint64), lambda: h.sum_cols(good), lambda: h.sum_rows_dual(good, good), lambda: h.mean_rows(good),
                   lambda: h.mean_var_rows(good)):
            with pytest.raises(sa.ScanrsError) as ei:
                fn()
            assert ei.value.code == 6 and "sharded" in str(ei.value)


@pytest.mark.parametrize("which", MAPS)
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_an_unsharded_handle_through_the_sharded_calls(sa, case, expected, orientation, which):
    """The plain calls: the same kernels, the same bits, no exchange."""
    single, _ = expected(orientation, which)
    x = Single(sa, case["csc"], orientation, which, sharded_calls=True)
    got = _run(x, _lists_of(case, orientation), which == "raw")
    for name, value in got.items():
        for g, s in zip(_parts(value), _parts(single[name])):
            same_bits(g, s)
    assert x.steps() == [0]
