"""The projection plan of svd_bk through `host_bk_plan` (scanrs_host_bk_plan; scan-rs_amd/csrc/bk_plan.hpp, the source solver.cpp
decides by), on the CPU: a table of literal cases read from the code of the commit before the rule was gathered into that header
(0: nothing flagged, 1: the flagged columns fit, 2: bound raised to the largest flagged, 3: raised to `need`, 4: a wide pass at
the bound as given), the cases of the f64 model (tests/bk_reuse_ref.py), a seeded sweep against the Python twin `plan_rule`, which
keeps the cost comparison behind last_direct that the header reduces to n_iter >= 2, and the refusals of the entry point."""
import numpy as np
import pytest

import bk_reuse_ref as R

INF = np.inf


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def ones(b, n_iter):
    return np.ones(b * n_iter)


def with_values(b, n_iter, values, lo=0):
    """colmax of all ones, except `values` from index `lo` on"""
    c = np.ones(b * n_iter)
    c[lo:lo + len(values)] = values
    return c


R104 = tuple(range(104, 208))
SIX = [5e9, 4e9, 3e9, 2e9, 3e5, 2e5]
AT_THE_BOUND = ones(16, 3)
AT_THE_BOUND[[5, 20]] = 1e5, 3e6  # the first one equals the bound: `!(x < limit)` flags it

# (id, colmax, b, n_iter, reuse_cmax, coef_valid, expected fields)
TABLE = [
    ("ones_4x3", ones(4, 3), 4, 3, 1e5, True,
     dict(reuse=True, limit_branch=0, flagged_older=0, limit=1e5, direct=(8, 9, 10, 11), last_direct=True, full_direct=False, cmax_dense=1.0, n_early=1)),
    ("ones_4x1", ones(4, 1), 4, 1, 1e5, True,
     dict(reuse=True, limit_branch=0, flagged_older=0, limit=1e5, direct=(), last_direct=False, full_direct=False, cmax_dense=1.0, n_early=0)),
    ("all_flagged_4x1", ones(4, 1), 4, 1, 1e-300, True,
     dict(limit_branch=0, flagged_older=0, limit=1e-300, direct=(0, 1, 2, 3), last_direct=False, full_direct=True, cmax_dense=0.0)),
    ("odd_block_7x2", ones(7, 2), 7, 2, 1e5, True,
     dict(reuse=False, full_direct=True, direct=(), limit=1e5, last_direct=False, limit_branch=0, flagged_older=0, cmax_dense=0.0, n_early=0)),
    ("coef_invalid_4x2", ones(4, 2), 4, 2, 1e5, False,
     dict(direct=tuple(range(8)), full_direct=True, last_direct=False, limit_branch=0, flagged_older=0, limit=1e5, cmax_dense=0.0)),
    ("room0_raised_top", with_values(104, 2, [2e5], 3), 104, 2, 1e5, True,
     dict(limit_branch=2, flagged_older=1, limit=float(np.nextafter(2e5, INF)), direct=R104, last_direct=True, full_direct=False, cmax_dense=2e5)),
    ("room0_two_decades", with_values(104, 2, [1e7], 3), 104, 2, 1e5, True,
     dict(limit_branch=4, flagged_older=1, limit=1e5, direct=(3,) + R104, last_direct=True, full_direct=False, cmax_dense=1.0)),
    ("room0_below_two_decades", with_values(104, 2, [float(np.nextafter(1e7, 0.0))], 3), 104, 2, 1e5, True,
     dict(limit_branch=2, flagged_older=1, limit=1e7, direct=R104, cmax_dense=float(np.nextafter(1e7, 0.0)))),
    ("raised_need", with_values(100, 2, SIX), 100, 2, 1e5, True,
     dict(limit_branch=3, flagged_older=6, limit=float(np.nextafter(3e5, INF)), direct=(0, 1, 2, 3) + tuple(range(100, 200)), cmax_dense=3e5, last_direct=True)),
    ("tie_at_need", with_values(100, 2, [5e9, 4e9, 3e9, 3e5, 3e5, 2e5]), 100, 2, 1e5, True,
     dict(limit_branch=4, flagged_older=6, limit=1e5, direct=(0, 1, 2, 3, 4, 5) + tuple(range(100, 200)), cmax_dense=1.0)),
    ("need_beyond_two_decades", with_values(100, 2, [5e9, 4e9, 3e9, 2e9, 1e7, 2e5]), 100, 2, 1e5, True,
     dict(limit_branch=4, flagged_older=6, limit=1e5, direct=(0, 1, 2, 3, 4, 5) + tuple(range(100, 200)), cmax_dense=1.0)),
    ("equal_to_the_bound_is_flagged", AT_THE_BOUND, 16, 3, 1e5, True,
     dict(limit_branch=1, flagged_older=2, limit=1e5, direct=(5, 20) + tuple(range(32, 48)), n_early=1, last_direct=True, full_direct=False, cmax_dense=1.0)),
]
N_DIRECT = {"room0_two_decades": 105, "raised_need": 104, "tie_at_need": 106, "need_beyond_two_decades": 106, "equal_to_the_bound_is_flagged": 18}


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_literal_table(sa, row):
    name, colmax, b, n_iter, cmax, valid, want = row
    got = sa.host_bk_plan(colmax, b, n_iter, cmax, valid)
    assert {k: got[k] for k in want} == want, got
    assert len(got["direct"]) == N_DIRECT.get(name, len(want["direct"]))


def test_defaults_are_the_librarys(sa):
    assert sa.host_bk_plan(ones(4, 3), 4, 3) == sa.host_bk_plan(ones(4, 3), 4, 3, 1e5, True)


@pytest.mark.parametrize("name,transposed", R.VIEWS)
def test_model_cases(sa, name, transposed):
    p = R.prepared(name, transposed)
    for cm in R.settings(p):
        r = p.model(cm)
        got = sa.host_bk_plan(r.colmax, r.b, p.case.n_iter, cm)
        want = dict(reuse=r.reuse, flagged_older=r.flagged_older, limit_branch=r.branch, limit=r.limit, direct=tuple(r.direct),
                    last_direct=r.last_direct, full_direct=r.full_direct, n_early=r.early_projections, cmax_dense=r.cmax_dense)
        assert got == want, (cm, got, want)
        assert np.float64(got["limit"]).tobytes() == np.float64(r.limit).tobytes()


def test_seeded_sweep_against_the_twin(sa):
    rng = np.random.default_rng(20261020)
    widths = (2, 4, 16, 52, 100, 104, 106, 128, 130)
    n_draws, seen = 20000, set()
    for draw in range(n_draws):
        b, n_iter = int(rng.choice(widths)), int(rng.integers(1, 5))
        q = b * n_iter
        cmax = float(10.0 ** rng.uniform(0.0, 8.0))
        colmax = 10.0 ** rng.uniform(-1.0, 12.0, size=q)
        if rng.random() < 0.1:  # ties: among the columns, at the bound and at the end of the two decades
            n_tie = int(rng.integers(1, q + 1))
            colmax[rng.integers(0, q, size=n_tie)] = colmax[rng.integers(0, q, size=n_tie)]
            colmax[rng.integers(0, q, size=2)] = cmax
            colmax[rng.integers(0, q, size=2)] = 100.0 * cmax
        valid = rng.random() >= 0.1
        got, want = sa.host_bk_plan(colmax, b, n_iter, cmax, valid), R.plan_rule(colmax, b, n_iter, cmax, valid)
        assert got == want, (draw, b, n_iter, cmax, valid, got, want)
        assert np.float64(got["limit"]).tobytes() == np.float64(want["limit"]).tobytes()
        if got["reuse"] and valid:
            assert got["last_direct"] == (n_iter >= 2), (draw, b, n_iter)
        seen.add(got["limit_branch"])
    # the draws reach every branch but 2, which wants EVERY flagged column within two decades of the bound while more of them are
    # flagged than the pass has room for: over thirteen decades that takes b = 104; the table and the model cases hold it
    assert {0, 1, 3, 4} <= seen


def test_refusals(sa):
    good = ones(4, 2)
    bad_calls = [
        (good[:0], 0, 2, 1e5),          # b == 0
        (good[:0], 4, 0, 1e5),          # n_iter == 0
        (good[:7], 4, 2, 1e5),          # a colmax of another length
        (np.ones(9), 4, 2, 1e5),
        (with_values(4, 2, [np.nan]), 4, 2, 1e5),
        (with_values(4, 2, [np.inf]), 4, 2, 1e5),
        (with_values(4, 2, [-1.0]), 4, 2, 1e5),
        (good, 4, 2, 0.0),
        (good, 4, 2, -1e5),
        (good, 4, 2, np.nan),
    ]
    for colmax, b, n_iter, cmax in bad_calls:
        with pytest.raises(sa.ScanrsError) as e:
            sa.host_bk_plan(colmax, b, n_iter, cmax)
        assert e.value.code == 6, (b, n_iter, cmax, str(e.value))  # SCANRS_ERR_ARGUMENT
    assert sa.host_bk_plan(good, 4, 2, np.inf)["direct"] == (4, 5, 6, 7)  # an infinite bound flags nothing and is no error
