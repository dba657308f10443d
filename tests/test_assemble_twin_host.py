"""
CPU: tests/assemble_twin.py against the f64 oracle, and the power of the bound tests/test_gpu_assemble.py applies.

For every case of assemble_twin.cases() and every regulariser setting, with the strengths rounded to float32 first:

  oracle   oracle(lambda) - oracle(0) is the regulariser alone (the oracle's data part is a deterministic f64 sum).  Its
           value must equal reg_value within (N L + parameters + pairs) 2^-53 of |f(lambda)| + |f(0)| -- one rounding per
           term the oracle adds, -log P terms included, whose OpenMP reduction has no fixed order -- and every gradient
           entry must equal c x, the EXACT float64 product of the twin's float32 coefficient and x, within 4 2^-53 of
           |g(lambda)| + |g(0)| + |c x| (the oracle adds 2 lambda x and the group term to the data sum: two roundings each
           side at most).  With lambda_g > 0 the twin's deliberate float32 steps add 4 2^-24 relative: of the group part
           for the value, of |c x| for an entry (n2 half an ulp, delta^2 + n2 half, sqrtf one, the division one, the sum
           2 lambda_j + gcoef one).  reg_gradient itself is float32(c x), bit for bit: the one rounding the oracle lacks.
  power    with the oracle's gradient as the size of g, |p_A - p_B| exceeds 8 times the GPU test's bound in at least 90 %
           of the live coupling entries (those of blocks that are not exactly zero) of every case and every pair of
           settings the GPU test differences: an error of an eighth of the term would fail there.
  mutants  three wrong twins -- lambda for 2 lambda, the group value counted by every state block (qm times), delta left
           out on the tiny-norm blocks -- each break the oracle comparison: the first in more than half of the live
           coupling entries of every setting with lambda_j > 0, the third in more than half of the entries of the blocks
           it changes (the tiny ones) of every setting with lambda_g > 0, the second in the value (it has no entries) of
           every such setting; the first and third also miss the GPU test's bound there when the oracle stands in for g.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_twin as at  # noqa: E402

F32, F64 = np.float32, np.float64
CASES = at.cases()
U53, U24 = 2.0 ** -53, 2.0 ** -24
_cache = {}


def _oracle_runs(oracle64, case):
    """the case, its weights and the oracle at every setting, computed once and shared (never modified)"""
    if case[0] in _cache:
        return _cache[case[0]]
    _, L, q, gap = case
    msa = at.case_alignment(case)
    x, kind = at.case_x(case)
    w = (1.0 / (oracle64.reweight_gaps if gap else oracle64.reweight)(msa, 0.8)).astype(F32)
    ev = oracle64.eval_gaps if gap else oracle64.eval
    runs = []
    try:
        for (lh, lj, lg) in at.SETTINGS:
            oracle64.set_lambda_group(float(F32(lg)))
            f, nll, g = ev(msa, w.astype(F64), q, float(F32(lh)), float(F32(lj)), x.astype(F64))
            g.setflags(write=False)
            runs.append((f, nll, g))
    finally:
        oracle64.set_lambda_group(0.0)
    for a in (msa, x, kind, w):
        a.setflags(write=False)
    _cache[case[0]] = (msa, x, kind, w, runs)
    return _cache[case[0]]


def _compare(case, x, runs, k, mutant=None):
    """-> (value error, value tolerance, per-entry error, per-entry tolerance, p) of setting k against the zero setting"""
    _, L, q, gap = case
    qm = q - 1 if gap else q
    lh, lj, lg = at.SETTINGS[k]
    (f, _, g), (f0, _, g0) = runs[k], runs[0]
    parts = at.reg_parts(x, L, qm, lh, lj, lg, mutant)
    verr = abs((f - f0) - sum(parts))
    vtol = (at.N_SEQS * L + at.value_terms(L, qm)) * U53 * (abs(f) + abs(f0)) + (4 * U24 * parts[2] if lg > 0 else 0.0)
    c = at.reg_coefficients(x, L, qm, lh, lj, lg, mutant).astype(F64)
    cx = c * x.astype(F64)                                    # exact: 24 x 24 bits
    err = np.abs((g - g0) - cx)
    tol = 4 * U53 * (np.abs(g) + np.abs(g0) + np.abs(cx)) + (4 * U24 * np.abs(cx) if lg > 0 else 0.0)
    return verr, vtol, err, tol, cx


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_twin_is_the_oracles_regulariser(oracle64, case):
    _, L, q, gap = case
    qm = q - 1 if gap else q
    msa, x, kind, w, runs = _oracle_runs(oracle64, case)
    assert len(set(np.unique(w).tolist())) > 1, "the cluster weights of the case are all equal"
    assert at.reg_value(x, L, qm, *at.SETTINGS[0]) == 0.0 and not at.reg_gradient(x, L, qm, *at.SETTINGS[0]).any()
    for k in range(1, len(at.SETTINGS)):
        verr, vtol, err, tol, cx = _compare(case, x, runs, k)
        print("%s %r: value error %.3g (tolerance %.3g), worst entry error / tolerance %.3g" % (
            case[0], at.SETTINGS[k], verr, vtol, float((err / np.maximum(tol, 1e-300)).max())))
        assert verr <= vtol
        assert (err <= tol).all()
        p = at.reg_gradient(x, L, qm, *at.SETTINGS[k])
        np.testing.assert_array_equal(p.view(np.uint32), cx.astype(F32).view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_gpu_bound_has_power_on_nine_live_entries_in_ten(oracle64, case):
    _, L, q, gap = case
    qm = q - 1 if gap else q
    msa, x, kind, w, runs = _oracle_runs(oracle64, case)
    live = at.live_coupling_entries(L, qm, kind)
    assert live.any() and (kind == 2).any()
    if at.n_pairs(L) >= 10:
        assert (kind == 0).sum() == at.n_pairs(L) // 3 and (kind == 1).sum() >= 1
        n2, _ = at.block_norms(x, L, qm)
        assert (n2[kind == 0] == 0).all() and (np.sqrt(n2[kind == 1]) < 1.01e-3).all() and (np.sqrt(n2[kind == 1]) > 0.99e-5).all()
    assert (np.abs(at.couplings_of(x, L, qm)) == at.BIG).sum() >= 1
    for (a, b) in at.PAIRS:
        pA = at.reg_gradient(x, L, qm, *at.SETTINGS[a]).astype(F64)
        pB = at.reg_gradient(x, L, qm, *at.SETTINGS[b]).astype(F64)
        bound = at.gradient_bound(runs[a][2], runs[b][2], pA, pB, at.SETTINGS[a], at.SETTINGS[b])
        strong = (np.abs(pA - pB) > 8.0 * bound)[L * qm:][live]
        print("%s settings %d - %d: %.4f of %d live coupling entries above 8 x bound" % (
            case[0], a, b, float(strong.mean()), strong.size))
        assert strong.mean() >= 0.9
        assert not (pA - pB)[L * qm:][~live].any()           # all-zero blocks: p = 0, counted nowhere


def _simulated_gpu_miss(x, L, qm, runs, k, mutant):
    """the GPU test's check with the oracle standing in for the kernels: g = float32(data + p) with the RIGHT p, the twin
    under test the mutant's -> mask of the entries that miss the bound"""
    s, s0 = at.SETTINGS[k], at.SETTINGS[0]
    data = runs[0][2]
    gA = (data + at.reg_gradient(x, L, qm, *s).astype(F64)).astype(F32).astype(F64)
    gB = data.astype(F32).astype(F64)
    pA = at.reg_gradient(x, L, qm, *s, mutant=mutant).astype(F64)
    pB = at.reg_gradient(x, L, qm, *s0, mutant=mutant).astype(F64)
    return np.abs((gA - gB) - (pA - pB)) > at.gradient_bound(gA, gB, pA, pB, s, s0)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_three_wrong_twins_break_the_comparison(oracle64, case):
    _, L, q, gap = case
    qm = q - 1 if gap else q
    msa, x, kind, w, runs = _oracle_runs(oracle64, case)
    live = at.live_coupling_entries(L, qm, kind)
    tiny = np.repeat(kind == 1, qm * qm)
    for k in range(1, len(at.SETTINGS)):
        lh, lj, lg = at.SETTINGS[k]
        if lj > 0:
            _, _, err, tol, _ = _compare(case, x, runs, k, "lambda_not_doubled")
            broken = (err > tol)[L * qm:][live]
            miss = _simulated_gpu_miss(x, L, qm, runs, k, "lambda_not_doubled")[L * qm:][live]
            print("%s %r lambda for 2 lambda: %.3f of the live entries break, %.3f miss the GPU bound" % (
                case[0], at.SETTINGS[k], broken.mean(), miss.mean()))
            assert broken.mean() > 0.5 and miss.mean() > 0.5
            assert (err > tol)[:L * qm].mean() > 0.5                      # the fields carry the same factor
        if lg > 0:
            verr, vtol, _, _, _ = _compare(case, x, runs, k, "group_counted_qm_times")
            print("%s %r group value counted qm times: value error %.3g against %.3g" % (case[0], at.SETTINGS[k], verr, vtol))
            assert verr > vtol
            if tiny.any():
                _, _, err, tol, _ = _compare(case, x, runs, k, "delta_omitted")
                broken = (err > tol)[L * qm:][tiny]
                miss = _simulated_gpu_miss(x, L, qm, runs, k, "delta_omitted")[L * qm:][tiny]
                print("%s %r delta omitted: %.3f of the tiny blocks' entries break, %.3f miss the GPU bound" % (
                    case[0], at.SETTINGS[k], broken.mean(), miss.mean()))
                assert broken.mean() > 0.5 and miss.mean() > 0.5
                assert not (err > tol)[L * qm:][~tiny].any()              # nothing else moves
    if at.n_pairs(L) >= 10:
        assert tiny.any()
