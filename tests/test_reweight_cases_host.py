"""
The cases of tests/reweight_cases.py can catch something: checked on the CPU, against oracle64 and against the per-pair
rule restated in numpy.  tests/test_gpu_reweight.py runs the same cases through the kernels.

Conditions every case has to meet (a case that cannot is changed, the condition stays):
  * at least 8 ordered pairs at exactly thr identities and 8 at thr - 1, by the rule of the case's convention, overall
    and for every layout the case plants;
  * for L >= 64 the largest identity between two background rows is below T by at least L / 4 (the early exit fires);
  * at least 5 % of the rows have a count above 1 and the counts are not all equal;
  * state range: the oracle's count of a satellite one site beyond the limit does not include the centre;
  * tail star: count of the centre = 1 + #(satellites at or inside the limit), without the oracle.
Where a condition cannot hold for any alignment of the case's shape it is not asked, for these reasons only:
  * N <= 2 has fewer than 8 ordered pairs and no 5 % of rows; N = 2 holds its one pair at thr (L = 40) or thr - 1 (L = 400);
  * theta = 0 (T = 0): no pair has -1 identities and every count is N;
  * T < L / 4 (theta = 0, T = 1): no identity is below T - L / 4 < 0.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reweight_cases as rc  # noqa: E402


@pytest.fixture(scope="module")
def counts_of(oracle64):
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = rc.oracle_counts(oracle64, case)
        return cache[case.name]
    return get


def test_every_kernel_path_has_a_case():
    """LW of k_reweight_reg by row length in dwords (rounded up to 8), Lw % 16 both ways, the chunked kernel with a short
    and a full last chunk, PLM_CONV_G_UNGAPPED_LENGTH over one chunk and several"""
    def lw(L):
        return (L + 31) // 32 * 8
    sweep = [rc.PARAMS[n]["L"] for n in rc.NAMES if n.startswith("sweep-") and n.endswith("-plain")]
    for lo, hi in ((1, 32), (33, 64), (65, 96), (97, 128), (129, 192)):
        inst = [L for L in sweep if lo <= lw(L) <= hi]
        assert {lw(L) % 16 for L in inst} == {0, 8}, (lo, hi, inst)
        if hi < 192:
            assert min(lw(L) for L in inst) == lo + 7 and max(lw(L) for L in inst) == hi
    assert any(lw(L) > 192 and lw(L) % 16 == 8 for L in sweep) and any(lw(L) > 192 and lw(L) % 16 == 0 for L in sweep)
    ung = [rc.PARAMS[n]["L"] for n in rc.NAMES if n.startswith("conv128-")]
    assert min(map(lw, ung)) <= 16 and max(map(lw, ung)) > 32
    assert all(lw(rc.PARAMS[n]["L"]) % 16 == 8 or rc.PARAMS[n]["L"] == 64 for n in rc.NAMES if n.startswith("state"))


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_is_built_as_described(name):
    c = rc.build(name)
    again = rc._build(name)
    np.testing.assert_array_equal(c.msa, again.msa)                      # deterministic from the name
    assert c.msa.shape == (c.N, c.L) and c.msa.dtype == np.int8
    assert c.msa.min() >= 0 and c.msa.max() <= c.top
    assert (c.msa.max() > 123) == c.reject
    rows = [s for _, s, _, _ in c.planted]
    assert len(set(rows)) == len(rows)
    for centre, sat, layout, k in c.planted:
        ident, thr = c.pair_stats(c.msa[centre], c.msa[sat])
        assert ident[0] - thr[0] == k, (name, centre, sat, layout, k, ident, thr)
        back, thr2 = c.pair_stats(c.msa[sat], c.msa[centre])             # the rule is symmetric
        assert back[0] == ident[0] and thr2[0] == thr[0]
    if c.N > 2:
        where = {tag for tag, _, _ in rc._classes(c, np.random.default_rng(0))}
        assert {"wave", "ends"} <= where and ("tile" in where) == (c.N > 200) and ("edge" in where) == (c.N > 256)
        sat_of = {}
        for centre, sat, _, _ in c.planted:
            sat_of.setdefault(centre, []).append(sat)
        assert any(64 <= s < 128 for s in sat_of.get(70, []))                                 # one wave
        assert c.N <= 200 or any(128 <= s < 256 for s in sat_of.get(10, []))                  # two waves of a tile
        assert c.N <= 256 or 256 in sat_of.get(255, []) or 255 in sat_of.get(256, [])                                       # rows 255 | 256
        assert c.N - 1 in sat_of.get(0, []) or 0 in sat_of.get(c.N - 1, [])                                                   # rows 0 and N - 1
    if c.gaps and c.N > 2:
        assert (c.msa == 0).all(axis=1).any()                                                 # the all-gap row
        if c.limit >= 3 and c.L >= 8 and c.T > 1:
            centres = sorted({centre for centre, _, _, _ in c.planted})
            a = c.msa[centres]
            assert ((a[:, :-1] == 0) & (a[:, 1:] == 1) & (np.arange(c.L - 1) % 4 != 3)[None, :]).any(axis=1).all()
            sats = c.msa[[s for _, s, _, _ in c.planted]]
            cen = c.msa[[centre for centre, _, _, _ in c.planted]]
            assert ((sats == 0) & (cen == 0)).any() and ((sats == 0) & (cen != 0)).any() and ((sats != 0) & (cen == 0)).any()
            nb = ((c.msa != 0)[None, :, :] & (c.msa[centres] != 0)[:, None, :]).sum(axis=2)
            assert (nb[:, ~(c.msa == 0).all(axis=1)] == 0).any()        # n_both = 0 with a row that has residues
    if c.conv & rc.CONV_UNGAPPED:
        nb = {int(((c.msa[a] != 0) & (c.msa[b] != 0)).sum()) for a, b, _, _ in c.planted}
        assert len(nb) >= 4, nb                                          # n_both differs between the planted pairs


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_can_catch_a_wrong_count(name, counts_of, oracle64):
    c = rc.build(name)
    counts = counts_of(c)
    assert counts.shape == (c.N,) and counts.min() >= 1 and counts.max() <= c.N

    # ---- pairs at the threshold and one below it, overall and per layout
    if c.N > 2:
        for layouts in [rc.LAYOUTS] + [(lay,) for lay in c.layouts]:
            at = 2 * sum(1 for _, _, lay, k in c.planted if k == 0 and lay in layouts)
            below = 2 * sum(1 for _, _, lay, k in c.planted if k == -1 and lay in layouts)
            assert at >= 8, (name, layouts, at)
            assert below >= 8 or c.T == 0, (name, layouts, below)
    elif c.N == 2:
        assert [k for _, _, _, k in c.planted] == [0 if c.L == 40 else -1]
        assert counts.tolist() == ([2, 2] if c.L == 40 else [1, 1])

    # ---- unrelated rows are far below the threshold: the early exit is taken
    if c.L >= 64 and 4 * c.T >= c.L and c.N > 2:
        bg = c.msa[c.background_rows[:400]]
        top = 0
        for lo in range(0, bg.shape[0], 50):
            ident = (bg[lo:lo + 50, None, :] == bg[None, :, :]).sum(axis=2)
            ident[np.arange(ident.shape[0]), lo + np.arange(ident.shape[0])] = 0
            top = max(top, int(ident.max()))
        assert top <= c.T - c.L / 4, (name, top, c.T)

    # ---- the counts say something
    if c.N > 2 and c.T > 0:
        assert (counts > 1).mean() >= 0.05, (name, (counts > 1).mean())
        assert counts.min() != counts.max()
    if c.T <= 0:
        assert (counts == c.N).all()

    # ---- the numpy rule is the oracle's: every centre's count, and the satellites next to the kernels' fill values
    for centre in sorted({centre for centre, _, _, _ in c.planted}):
        assert counts[centre] == c.neighbours(centre).size, (name, centre)
    if c.family == "state":
        assert len(c.beyond) >= (16 if c.gaps else 8)
    for centre, sat in c.beyond:
        nb = c.neighbours(sat)
        assert centre not in nb and counts[sat] == nb.size, (name, centre, sat)
        ident, thr = c.pair_stats(c.msa[centre], c.msa[sat])
        assert ident[0] == thr[0] - 1
        if centre == 5:
            assert c.top in c.msa[sat + 1, :32]
        else:
            assert ((c.msa[centre] == 0) & (c.msa[sat] == c.top - 2)).sum() == 1

    # ---- the tail star in closed form (unrelated rows far away, no gaps in the star)
    if c.tail_star and c.L >= 64 and 2 * c.T >= c.L:
        centre, sats = c.tail_star
        assert len(sats) == 6 or c.limit == 0
        assert not (c.msa[[centre] + [s for s, _ in sats]] == 0).any() or c.top > 20
        want = 1 + sum(1 for _, k in sats if k >= 0)
        if c.gaps and c.conv & rc.CONV_UNGAPPED:
            want += 1                    # the all-gap row: n_both = 0 needs ceil(-1e-9) = 0 identities
        assert counts[centre] == want, (name, counts[centre], want)

    # ---- bit 32: the float32 threshold is another one here
    if c.conv & rc.CONV_F32:
        assert rc.threshold(c.L, c.theta, 32) != rc.threshold(c.L, c.theta, 0)
        oracle64.set_conventions(32)
        try:
            assert oracle64.threshold(c.L, c.theta) == rc.threshold(c.L, c.theta, 32)
        finally:
            oracle64.set_conventions(0)
        assert oracle64.threshold(c.L, c.theta) == rc.threshold(c.L, c.theta, 0)
        if not c.conv & rc.CONV_UNGAPPED:             # (under bit 128 the threshold is per pair and in float64)
            other = oracle64.reweight(c.msa, c.theta)
            assert (other != counts).any()


def test_num_cluster_members_refuses_the_fill_values_before_the_library_is_called(monkeypatch):
    from evcouplings_amd import alignment_accel, plm
    calls = []
    monkeypatch.setattr(plm, "reweight", lambda msa, theta: calls.append(msa.max()) or np.ones(msa.shape[0], np.int32))
    for state in (124, 125, 126, 127, 200, -1):
        with pytest.raises(ValueError, match="outside 0..123"):
            alignment_accel.num_cluster_members(np.array([[0, 1], [state, 2]]), 0.8)
    assert calls == []
    assert alignment_accel.num_cluster_members(np.array([[0, 123], [123, 2]]), 0.8).tolist() == [1.0, 1.0]
    assert calls == [123]
    assert alignment_accel._int8_states(np.array([[0, 127]]), "matrix").dtype == np.int8      # other callers: 0..127


def test_the_library_refuses_the_fill_values_before_the_device_is_looked_at():
    from evcouplings_amd import _lib, plm
    for name in [n for n in rc.NAMES if rc.PARAMS[n].get("reject")][:2]:
        c = rc.build(name)
        with pytest.raises(_lib.PlmError) as err:
            plm.reweight(c.msa, c.theta, ignore_gaps=c.gaps)
        assert err.value.code == -1 and "outside 0..123" in str(err.value), str(err.value)
    for state in (124, 125, 126, 127):
        with pytest.raises(_lib.PlmError) as err:
            plm.reweight(np.array([[1, 2, 3], [4, state, 6]], np.int8), 0.8)
        assert err.value.code == -1 and "msa[4] = %d outside 0..123" % state in str(err.value), str(err.value)
    with pytest.raises(_lib.PlmError) as err:
        plm.reweight(np.zeros((3, 0), np.int8), 0.8)
    assert err.value.code == -1 and "n_sites > 0" in str(err.value)
