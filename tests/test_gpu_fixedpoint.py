"""
GPU: every digit plane of the fixed-point GEMM operands against tests/fixedpoint_twin.py, without tolerances
(DESIGN_NEXT_ROWS.md 9.17).  For the inputs of the shared case list every float step of the chain is exact or a single
rounding, so the expected output is an integer computation; the CPU suite (tests/test_fixedpoint_twin_host.py) checks the
preconditions of every case and ties the twin to the f64 oracle.

  forward   plm.potentials with PLM_FWD_ACCURATE=1 (k_expand_x + k_fwd_x: five int8 digit planes) on the general, plane-
            isolating, digit-extreme and scale-edge models, and with PLM_FWD_ACCURATE=0 (k_expand + k_fwd: hi + lo f16
            planes on the sparse matrix cores) on the 22-bit models: assert_array_equal on float32
  backward  PlmContext.marginals (k_onehot_rt -> k_bwd / k_bwd_w -> k_assemble mode 1) and the pair gradient at zero
            couplings and saturated fields (k_hpass -> k_bwd -> k_assemble mode 0): the float32 the twin derives from the
            exact integer sums, bit for bit, and the integer itself recovered as rint(out / scale) wherever |V| < 2^22;
            three / four planes x both backward kernels x PLM_KSPLIT x plain / accurate softmax x gap mode x L
  headroom  130 816 equal sequences in ONE K range (int32 partials up to 2 143 289 344), and 131 328, where pick_ksplit
            must form two ranges whatever PLM_KSPLIT says
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixedpoint_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FWD = tw.forward_cases()
_expected = {}


@pytest.fixture(scope="module")
def plm():
    from evcouplings_amd import plm as _plm
    assert _plm.device_count() >= 1, "no gfx950 device: the HIP path has no fallback"
    return _plm


def forward_expected(case):
    """the case and its twin result, computed once and shared (never modified)"""
    if case[0] not in _expected:
        seqs, jij = tw.forward_case(case)
        want = tw.potentials_exact(seqs, case[4], jij)
        for a in (seqs, jij, want):
            a.setflags(write=False)
        _expected[case[0]] = (seqs, jij, want)
    return _expected[case[0]]


def _report(name, got, want):
    bad = got != want
    print("%s: %d of %d values differ, max |diff| %.3g (max |want| %.3g)" % (
        name, int(bad.sum()), bad.size, float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(want).max())))


@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_accurate_potentials_are_the_twins_bits(plm, monkeypatch, case):
    """k_expand_x + k_fwd_x: float32(float64(S 2^-(jexp + 23) + C)) with S the integer sum of the 39-bit differences"""
    name, kind, L, N, q, _ = case
    seqs, jij, want = forward_expected(case)
    monkeypatch.setenv("PLM_FWD_ACCURATE", "1")
    hi = np.random.default_rng(L).normal(size=(L, q)).astype(F32)       # the fields take no part in the potentials
    got = plm.potentials(seqs, q, hi, jij)
    _report(name, got, want)
    assert got.shape == (N, L, q) and got.dtype == F32
    np.testing.assert_array_equal(got, want)


PLAIN = [c for c in FWD if c[1] == "plain"]


@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_plain_potentials_are_the_twins_bits_on_22_bit_models(plm, monkeypatch, case):
    """k_expand + k_fwd<FWD_POTENTIALS>: differences of at most 22 bits split exactly into hi + lo f16 planes, sums
    below 2^24 units: the f32 accumulation of the sparse matrix cores and the power-of-two unscale lose nothing."""
    name, kind, L, N, q, _ = case
    seqs, jij, want = forward_expected(case)
    monkeypatch.setenv("PLM_FWD_ACCURATE", "0")
    got = plm.potentials(seqs, q, np.zeros((L, q), F32), jij)
    _report(name, got, want)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ backward operands
def _env(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _backward_twin(family, L, gap, q, N, planes):
    key = ("bwd", family, L, gap, q, N, planes)
    if key not in _expected:
        msa, w, astar = tw.backward_case(family, L, gap, N=N, q=q)
        R = tw.residual_ints(w, planes)
        Vm = tw.pair_sums(msa, tw.marginal_site_ints(msa, q, R), q)
        Vr = tw.pair_sums(msa, tw.residual_site_ints(msa, q, R, astar, gap), q)
        _expected[key] = (msa, w, astar, tw.marginals_expected(Vm, w, planes, gap) + (tw.pair_blocks(Vm),),
                          tw.gradient_expected(Vr, w, planes, gap))
    return _expected[key]


def _check_marginals(plm, family, L, gap, q, N, planes, tag):
    msa, w, astar, (want, scale, Vb), _ = _backward_twin(family, L, gap, q, N, planes)
    with plm.PlmContext(msa, q=q, ignore_gaps=gap) as ctx:
        ctx.set_weights(w)
        _, fij = ctx.marginals()
    bad = fij != want
    print("marginals %s: %d of %d differ" % (tag, int(bad.sum()), bad.size))
    np.testing.assert_array_equal(fij, want, err_msg=tag)
    if not gap:                         # (gap mode divides by the block total afterwards: the bits above are the check)
        small = np.abs(Vb) < 2 ** 22
        assert small.any()
        np.testing.assert_array_equal(tw.recover_ints(fij, scale)[small], Vb[small], err_msg=tag)


def _check_gradient(plm, family, L, gap, q, N, planes, tag):
    msa, w, astar, _, (want, Vs, gscale, Vmag) = _backward_twin(family, L, gap, q, N, planes)
    qm = q - 1 if gap else q
    h = tw.saturated_fields(L, q, astar)
    x = np.concatenate([(h[:, 1:] if gap else h).ravel(), np.zeros(L * (L - 1) // 2 * qm * qm, F32)]).astype(F32)
    with plm.PlmContext(msa, q=q, ignore_gaps=gap, lambda_h=0.01, lambda_j=3.0) as ctx:
        ctx.set_weights(w)
        ctx.set_x(x)
        ctx.eval()
        g = ctx.get_g()[L * qm:].reshape(want.shape)
    bad = g != want
    print("gradient %s: %d of %d differ" % (tag, int(bad.sum()), bad.size))
    np.testing.assert_array_equal(g, want, err_msg=tag)
    small = Vmag < 2 ** 21                             # two float32 roundings (sum, product): a quarter unit below 2^21
    assert small.any() and np.abs(Vs).max() > 0
    np.testing.assert_array_equal(tw.recover_ints(g, gscale)[small], Vs[small], err_msg=tag)


CROSS = [(planes, kern, ks) for planes in (3, 4) for kern in (0, 1) for ks in (None, 3)]


@pytest.mark.parametrize("gap", [False, True], ids=["nogap", "gap"])
@pytest.mark.parametrize("L", tw.BWD_L)
@pytest.mark.parametrize("family", ["a", "b"])
def test_marginals_are_the_exact_integer_sums(plm, monkeypatch, family, L, gap):
    q = tw.BWD_Q
    N = tw.BWD_B_N[L] if family == "b" else None
    for planes, kern, ks in CROSS:
        _env(monkeypatch, PLM_BWD_PLANES=planes, PLM_BWD_KERNEL=kern, PLM_KSPLIT=ks)
        _check_marginals(plm, family, L, gap, q, N, planes, "planes=%d kernel=%d ksplit=%s" % (planes, kern, ks))


@pytest.mark.parametrize("gap", [False, True], ids=["nogap", "gap"])
@pytest.mark.parametrize("L", tw.BWD_L)
@pytest.mark.parametrize("family", ["a", "b"])
def test_gradient_at_saturated_fields_is_the_exact_integer_sum(plm, monkeypatch, family, L, gap):
    q = tw.BWD_Q
    N = tw.BWD_B_N[L] if family == "b" else None
    for planes, kern, ks in CROSS:
        for acc in (0, 1):
            _env(monkeypatch, PLM_BWD_PLANES=planes, PLM_BWD_KERNEL=kern, PLM_KSPLIT=ks, PLM_FWD_ACCURATE=acc)
            _check_gradient(plm, family, L, gap, q, N, planes,
                            "planes=%d kernel=%d ksplit=%s accurate=%d" % (planes, kern, ks, acc))


@pytest.mark.parametrize("q", tw.OTHER_Q)
def test_other_alphabets_run_the_same_digits(plm, monkeypatch, q):
    """k_bwd<Q, FM, FN> and k_hpass<Q> of the other instantiated alphabets and one padded alphabet (7 runs as 20)"""
    for planes in (3, 4):
        for gap in (False, True):
            _env(monkeypatch, PLM_BWD_PLANES=planes, PLM_BWD_KERNEL=None, PLM_KSPLIT=None, PLM_FWD_ACCURATE=None)
            _check_marginals(plm, "a", 17, gap, q, q, planes, "q=%d planes=%d gap=%d" % (q, planes, gap))
            _check_gradient(plm, "a", 17, gap, q, q, planes, "q=%d planes=%d gap=%d" % (q, planes, gap))


@pytest.mark.parametrize("N,ksplit,planes", [(tw.HEADROOM_N[0], 1, 4), (tw.HEADROOM_N[0], 1, 3), (tw.HEADROOM_N[0], 3, 4),
                                             (tw.HEADROOM_N[1], 1, 4)])
def test_int32_headroom_at_the_largest_k_range(plm, monkeypatch, N, ksplit, planes):
    """All sequences equal (column j holds state j mod q), all weights 1: R = QMAX, whose four digits are
    (-128, 75, 111, 127).  N = 130 816 = 1022 K steps is the largest range of one split: plane 0 accumulates
    (-128)(-128) N = 2 143 289 344 < 2^31, plane 3 -128 * 127 N.  At N = 131 328 one range would overflow plane 0;
    PLM_KSPLIT=1 must be raised to 2 by pick_ksplit (neither plm_ctx_solver_stats nor PLM_DEBUG reports the split: the
    exact result is the evidence).  PLM_KSPLIT=3 at 130 816 is the one case of this file in which a K split above 1 is in
    force (below 1024 sequences pick_ksplit admits none)."""
    L, q = tw.HEADROOM_L, tw.HEADROOM_Q
    row = (np.arange(L) % q).astype(np.int8)
    msa = np.broadcast_to(row, (N, L)).copy()
    w = np.ones(N, dtype=F32)
    R = int(tw.residual_ints(w[:8], planes)[0])
    V1 = tw.pair_sums(msa[:1], tw.marginal_site_ints(msa[:1], q, np.array([R])), q)       # one sequence: 0 / R per cell
    scale = tw.marginal_scale(w, planes, False)
    want = (scale * tw.combine(tw.pair_blocks(V1) * N, unit=N)).astype(F32)
    _env(monkeypatch, PLM_BWD_PLANES=planes, PLM_BWD_KERNEL=None, PLM_KSPLIT=ksplit)
    with plm.PlmContext(msa, q=q) as ctx:
        ctx.set_weights(w)
        fi, fij = ctx.marginals()
    print("headroom N=%d ksplit=%d planes=%d: %d of %d differ, occupied cells hold %r" % (
        N, ksplit, planes, int((fij != want).sum()), fij.size, np.unique(fij[want != 0]).tolist()))
    np.testing.assert_array_equal(fij, want)
    assert np.count_nonzero(want) == L * (L - 1) // 2 and abs(float(want.max()) - 1.0) < 2e-7
