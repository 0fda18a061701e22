"""The moments of compute_sseq_params against exact sums, without a device: tests/sseq_moments_ref.py restates the library's 128-bit
fixed-point accumulation in Python integers and holds it to exact rational sums of the same f64 terms, on the cases of
tests/sseq_moments_cases.py. tests/test_gpu_sseq_moments.py asks the same of the kernels.

The contract: per gene |mean - exact| <= 1e-12 mean (and the same of S1), |var - exact| <= 1e-10 S2 / m, use_genes equal wherever the
exact var >= 1e-9 S2 / m; gene_moment_phi, zeta_hat, delta and gene_phi within those bounds carried through their formulas
(sseq_moments_ref.downstream_bounds holds the derivation). No bound here was measured on a result: the derived ones hold for the
f64 evaluation from exact moments with a margin of five orders (worst error / bound over all cases: gene_moment_phi 4.6e-06, zeta_hat
7.7e-06, delta 2.2e-06, gene_phi 1.3e-06).

The rule the library had (one quantum for all genes, from the bound m max_count max(1 / sf), and in sseq_de_pairs one quantum from the
cell count) violates the contract on, worst error / bound over the case's variants:

  case                     mean      var       use_genes   downstream
  one_huge_count           2.8e-04   1.0e+10   1 differs   zeta_hat 7.7, delta 7.3, gene_phi 44
  umi_spread_1e12          1.4e-04   6.6       equal       within     (median_small; 5.4 and 6.9 in the other two umi variants)
  huge_count_and_spread    1.1e-04   1.2       equal       within
  pairs_total_2^40         2.3e-04   2.2       equal       -

(one_huge_count: Σ (x/sf)² of the gene with a count of 1 beside 4e9 rounds to 0 under the quantum 2^-44, its variance comes out as
-mean² and the gene leaves use_genes.) raw_like, umi_spread_1e3, umi_spread_1e6 and pairs_total_2^34 stay inside the contract under
that rule at these shapes: their quanta keep 40 bits and more of the smallest term. Under the present rule (fixed128.hpp) every case is
inside, with mean <= 2.6e-04 and var <= 1.7e-05 of the bound: what is left is f64 rounding behind the exact integer sum."""
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_moments_cases as mc  # noqa: E402
import sseq_moments_ref as mr  # noqa: E402
import sseq_ref as ref  # noqa: E402

VARIANTS = mc.variant_ids()
IDS = [f"{a}-{b}" for a, b in VARIANTS]
# where the superseded rule leaves the contract (the table above) and where it does not
SINGLE_BREAKS = {("one_huge_count", "natural"), ("one_huge_count", "cells"), ("umi_spread_1e12", "median_small"),
                 ("umi_spread_1e12", "median_large"), ("umi_spread_1e12", "cells+median_large"), ("huge_count_and_spread", "huge_in_large")}
# the inputs that keep the single pass under the present rule: everything ordinary
SINGLE_ROUTE = {"benign", "raw_like", "umi_spread_1e3", "umi_spread_1e6", "single_nonzero_genes", "constant_gene", "zero_factor", "wave_edges"}

exact = mr.exact_variant
_worst = mr.worst_ratios


def test_the_reference_agrees_with_the_f64_restatement_on_benign():
    for v in mc.case("benign")["variants"]:
        mom, par, _ = exact("benign", v["name"])
        exp = ref.compute_sseq_params(mc.case("benign")["mat"], 0.995, v["cell_indices"], v["umi_counts"])
        np.testing.assert_array_equal(exp["use_genes"], par["use"])
        for f, mine in (("gene_means", mom["mean"]), ("gene_variances", mom["var"]), ("gene_moment_phi", par["gene_moment_phi"]),
                        ("gene_phi", par["gene_phi"])):
            mine = np.array([float(x) for x in mine])
            np.testing.assert_allclose(exp[f], mine, rtol=1e-12, atol=0, err_msg=f)
        np.testing.assert_allclose([exp["zeta_hat"], exp["delta"]], [float(par["zeta_hat"]), float(par["delta"])], rtol=1e-12)


@pytest.mark.parametrize("name,vname", VARIANTS, ids=IDS)
def test_the_case_set_conditions_hold(name, vname):
    mom, par, bounds = exact(name, vname)
    posed = mr.use_posed(mom)
    left_out = 1.0 - sum(posed) / len(posed)
    assert left_out <= mc.USE_LEFT_OUT_CAP
    if name == "constant_gene":
        assert not posed[0] and mom["var"][0] == 0 and all(posed[1:])  # the constant gene, and nothing else
        assert not bounds["compare_shrink"]
    else:
        assert left_out == 0.0
        assert bounds["compare_shrink"], "b = Σ (phi - zeta_hat)² has come within 1e-6 of zero relative to Σ phi²"
    if name == "zero_factor":
        assert sum(mom["bad"]) >= 3  # the cell with factor 0 holds nonzeros of several genes
    else:
        assert not any(mom["bad"])


@pytest.mark.parametrize("name,vname", VARIANTS, ids=IDS)
def test_the_library_rule_meets_the_contract(name, vname):
    v = mc.variant(name, vname)
    mom, par, bounds = exact(name, vname)
    got = mr.emulate(mc.case(name)["mat"], v["cell_indices"], v["umi_counts"], "library")
    worst, mism = _worst(mom, par, bounds, got)
    print(name, vname, got["route"], worst)
    assert max(worst.values()) <= 1.0, worst
    assert mism == []
    # ordinary inputs keep the single pass, and the adversarial ones that the single quantum fails do leave it
    if name in SINGLE_ROUTE:
        assert got["route"] == "single"
    if (name, vname) in SINGLE_BREAKS:
        assert got["route"] == "per_gene"


@pytest.mark.parametrize("name,vname", VARIANTS, ids=IDS)
def test_the_superseded_rule_breaks_it_on_the_adversarial_cases(name, vname):
    """the grid is adversarial: one quantum for all genes leaves the contract exactly where the docstring's table says"""
    v = mc.variant(name, vname)
    mom, par, bounds = exact(name, vname)
    got = mr.emulate(mc.case(name)["mat"], v["cell_indices"], v["umi_counts"], "single")
    worst, mism = _worst(mom, par, bounds, got)
    print(name, vname, worst, mism)
    broken = max(worst.values()) > 1.0 or mism != []
    assert broken == ((name, vname) in SINGLE_BREAKS), worst
    if name == "one_huge_count":
        assert mism == [1] and got["gene_variances"][1] < 0.0 and worst["var"] > 1e9  # Σ (x/sf)² rounded to 0


@pytest.mark.parametrize("name,vname", VARIANTS, ids=IDS)
def test_the_host_formulas_meet_the_downstream_bounds_from_exact_moments(name, vname):
    import scanrs_amd as sa

    mom, par, bounds = exact(name, vname)
    mean = np.array([float(x) for x in mom["mean"]])
    var = np.array([float(x) for x in mom["var"]])
    sum_sf = 0.0
    for s in mom["sf"].tolist():  # the host's fold
        if s != 0.0:
            sum_sf += 1.0 / s
    got = sa.sseq.sseq_params_from_moments(mean, var, sum_sf, float(mom["m"]), float(mom["genes"]), 0.995)
    worst = mr.downstream_ratios(par, bounds, got)
    print(name, vname, worst)
    assert max(worst.values()) <= 1.0, worst
    assert mr.use_mismatches(mom, par, got.use_genes) == []


@pytest.mark.parametrize("name", list(mc.PAIRS_CASES))
def test_the_pairs_form_pins_its_boundary(name):
    """terms x / u_c <= 1 under fixed_scale(cells): inside the contract up to a cell total of 2^34, outside at 2^40, where the library
    sends the pairs that hold the cell to the literal route (compute_sseq_params over the union, a quantum per gene)"""
    c = mc.case(name)
    for pair in c["pairs"]:
        mom = mr.pairs_exact(c["mat"], c["labels"], pair)
        par = mr.exact_params(mom)
        holds_huge_cell = 0 in pair
        for rule in ("single", "library"):
            got = mr.pairs_emulate(c["mat"], c["labels"], pair, rule)
            r = mr.contract_ratios(mom, got["mean"], got["var"])
            worst = max(max(r["mean"]), max(r["var"]))
            mism = mr.use_mismatches(mom, par, got["var"] > 0)
            print(name, pair, rule, got["route"], max(r["mean"]), max(r["var"]), mism)
            if rule == "single" and name == "pairs_total_2^40" and holds_huge_cell:
                assert worst > 1.0 and r["var"][0] > 1.0  # the gene with its only count in the huge cell
            else:
                assert worst <= 1.0 and mism == []
        assert got["route"] == ("literal" if name == "pairs_total_2^40" and holds_huge_cell else "batched")
    assert all(mr.use_posed(mom))
