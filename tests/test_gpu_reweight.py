"""
Every variant of the reweighting kernels against the oracle, count for count (no tolerances: integer work), on the cases
of tests/reweight_cases.py -- pairs exactly at the threshold and one identity below it, in every layout and row placement
that the early exits, the T ranges and the tile edges can get wrong.  tests/test_reweight_cases_host.py shows on the CPU
that the cases hold such pairs.  Needs a real MI355X: run with -m gpu.

  kernel                       cases
  k_reweight_reg<32>           sweep L 1, 2, 32, 33 .. 128 (Lw 8, 16, 24, 32), tile (L 40), conv L 25 .. 65, thr L 40, state123
  k_reweight_reg<64>           sweep L 129, 256 (Lw 40, 64), conv L 130 (bits 64, 32), state123 L 136
  k_reweight_reg<96>           sweep L 257, 384 (Lw 72, 96)
  k_reweight_reg<128>          sweep L 385, 512 (Lw 104, 128), tile (L 400), thr L 385, trange L 512
  k_reweight_reg<192>          sweep L 513, 640, 768 (Lw 136, 160, 192), trange L 768
  k_reweight<false>            sweep L 769 (last chunk 8 dwords), 1024 (full), trange L 800, conv L 800 (bits 64, 32)
  k_reweight<true>             conv128, conv192, conv160 at L 25 (one chunk), 65, 130, 800 (several, short last chunk)
each in plain and in gap mode where the kernel has both.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reweight_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
Q = 21
RUN = [n for n in rc.NAMES if not rc.PARAMS[n].get("reject")]
REFUSED = [n for n in rc.NAMES if rc.PARAMS[n].get("reject")]
# a context holds a model and needs two sites and the states of its alphabet
IN_CONTEXT = [n for n in RUN if rc.PARAMS[n].get("top", 20) < 32 and rc.PARAMS[n]["L"] >= 2]


@pytest.fixture(scope="module")
def plm():
    from evcouplings_amd import plm as _plm
    assert _plm.device_count() >= 1, "no gfx950 device: the HIP path has no fallback"
    return _plm


@pytest.fixture(scope="module")
def want(oracle64):
    """the oracle's counts of a case, computed once"""
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = rc.oracle_counts(oracle64, case)
            cache[case.name].flags.writeable = False
        return cache[case.name]
    return get


def _same(case, got, ref, what="plm.reweight"):
    bad = np.flatnonzero(got != ref)
    if bad.size:
        planted = {s: (centre, layout, k) for centre, s, layout, k in case.planted}
        lines = ["%s, case %s (N %d, L %d, theta %r, flags %d, T %d): %d of %d counts differ"
                 % (what, case.name, case.N, case.L, case.theta, case.flags, case.T, bad.size, case.N)]
        for s in bad[:12]:
            note = "  satellite of %d, %s, identity thr%+d" % planted[s] if s in planted else ""
            lines.append("  row %5d: got %5d, want %5d%s" % (s, got[s], ref[s], note))
        print("\n".join(lines))
    np.testing.assert_array_equal(got, ref, err_msg="%s, case %s" % (what, case.name))


@pytest.mark.parametrize("name", RUN)
def test_counts_equal_the_oracles(plm, want, name):
    c = rc.build(name)
    _same(c, plm.reweight(c.msa, c.theta, ignore_gaps=c.gaps, conventions=c.conv), want(c))


@pytest.mark.parametrize("name", IN_CONTEXT)
def test_a_context_counts_and_weighs_the_same(plm, want, name):
    """the path a fit takes: dims of the real q, the counts left on the device, w = 1 / count in float32"""
    c = rc.build(name)
    with plm.PlmContext(c.msa, q=Q, theta_id=c.theta, ignore_gaps=c.gaps, conventions=c.conv) as ctx:
        w, counts, n_eff = ctx.reweight()
    _same(c, counts, want(c), "PlmContext.reweight")
    assert w.dtype == np.float32
    np.testing.assert_array_equal(w, np.float32(1) / want(c).astype(np.float32))


@pytest.mark.parametrize("name,conv", [("trange-L768-plain", 0), ("trange-L512-gap", 0), ("trange-L800-plain", 0),
                                       ("trange-L800-gap", 0), ("trange-L800-gap", 128)])
def test_counts_follow_a_permutation_of_the_rows(plm, name, conv):
    """k_reweight_reg, k_reweight<false> and k_reweight<true> at N = 3000: a permutation moves every pair to other waves,
    tiles and T ranges, the counts move with the rows"""
    c = rc.build(name)
    counts = plm.reweight(c.msa, c.theta, ignore_gaps=c.gaps, conventions=conv)
    perm = np.random.default_rng(3000).permutation(c.N)
    got = plm.reweight(c.msa[perm], c.theta, ignore_gaps=c.gaps, conventions=conv)
    bad = np.flatnonzero(got != counts[perm])
    if bad.size:
        print("case %s, conventions %d: %d counts differ after the permutation; rows (before -> after: count before, after) %s"
              % (name, conv, bad.size, [(int(perm[s]), int(s), int(counts[perm[s]]), int(got[s])) for s in bad[:12]]))
    np.testing.assert_array_equal(got, counts[perm])


@pytest.mark.parametrize("name", REFUSED)
def test_an_alignment_with_a_fill_value_is_refused(plm, name):
    """124..126 are bytes the kernels fill with (include/plm_hip.h, PLM_REWEIGHT_MAX_STATE): the parent of this test
    counted a satellite one site beyond the limit into its centre's cluster where the row after it held 126, or where it
    held 124 against the centre's gap"""
    from evcouplings_amd._lib import PlmError
    c = rc.build(name)
    with pytest.raises(PlmError) as err:
        plm.reweight(c.msa, c.theta, ignore_gaps=c.gaps)
    assert err.value.code == -1 and "outside 0..123" in str(err.value), str(err.value)


@pytest.mark.parametrize("state", [124, 125, 126])
def test_each_fill_value_is_refused_and_named(plm, oracle64, state):
    from evcouplings_amd._lib import PlmError
    c = rc.build("state123-L8-plain")
    msa = c.msa.copy()
    msa[77, 3] = state
    for gaps in (False, True):
        with pytest.raises(PlmError) as err:
            plm.reweight(msa, c.theta, ignore_gaps=gaps)
        assert err.value.code == -1 and "msa[%d] = %d outside 0..123" % (77 * c.L + 3, state) in str(err.value)
    msa[77, 3] = 123
    np.testing.assert_array_equal(plm.reweight(msa, c.theta), oracle64.reweight(msa, c.theta))
