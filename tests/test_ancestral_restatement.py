"""tests/ancestral_ref.py -- the numpy restatement of Ancestral_Sequences_One_Node that the device call is held to -- against the
REAL reference's own `--ancestral` output (tests/golden/ancestral_*.txt.gz, recipe: tests/golden/make_ancestral.py).  CPU-only.

The reference prints with %10g: 6 significant digits, at most 5e-6 relative from rounding; 0.1e-6 on top covers the restatement's
own arithmetic (every term is non-negative, nothing cancels: ~1e-13)."""
import numpy as np
import pytest

import ancestral_ref as ar
import orc

SHAPES = {"synth_nt_300x40": (300, 40, 4), "synth_aa_90x24": (90, 24, 20)}
PRINT_TOL = 5.1e-6


@pytest.fixture(scope="module")
def restated(golden):
    cache = {}

    def get(name):
        if name not in cache:
            ot = orc.tree_from_golden(golden(name))
            ot.lk(None, both_sides=True)
            cache[name] = (ot, ar.node_posteriors(ot)[0])
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_printed_row_is_the_restatements(name, restated):
    n, sites, ns = SHAPES[name]
    ot, post = restated(name)
    assert (ot.n, ot.P, ot.m.ns) == (n, sites, ns)
    ref, seen = ar.load_reference_file(name, n, sites, ns)
    assert len(seen) == (n - 2) * sites and not np.isnan(ref).any()   # every internal node x every site
    err = np.abs(post - ref)
    worst = float(np.max(err / np.maximum(np.abs(ref), 1e-300)))
    print(name, "worst relative difference to the printed value:", worst)
    assert np.all(err <= PRINT_TOL * np.abs(ref)), worst


@pytest.mark.parametrize("name", ["nucleic_gtr_g4", "nucleic_gtr_g4_inv", "nucleic_zero_w", "proteic_lg_g4", "synth_nt_300x40", "synth_aa_90x24"])
def test_weighted_patterns_sum_to_one(name, golden, restated):
    """Looser than rounding on purpose: the eigen system, not the arithmetic, limits how close the sums come (proteic_lg_g4:
    4e-10); the reference itself allows 0.01."""
    if name in SHAPES:
        ot, post = restated(name)
    else:
        ot = orc.tree_from_golden(golden(name))
        ot.lk(None, both_sides=True)
        post = ar.node_posteriors(ot)[0]
    w = ot.wght > 0
    assert w.any()
    sums = post.sum(axis=2)
    print(name, "worst |sum - 1|:", float(np.max(np.abs(sums[:, w] - 1.0))))
    assert np.all(np.abs(sums[:, w] - 1.0) <= 1e-6)
    assert not np.any(post[:, ~w])
