"""
GPU: gradient assembly and the regulariser terms entry by entry, against tests/assemble_twin.py -- the last stage of an
evaluation (k_pair_norms, k_assemble_v / k_assemble, k_assemble_h, k_slab_reduce, k_pack_g with the gradient halo, the
reg_part partials, k_finish_fx).  tests/test_assemble_twin_host.py ties the twin to the f64 oracle on the CPU and shows
that the bound used here fails a term that is wrong by an eighth.  Everything goes through PlmContext (set_weights, set_x,
eval, get_g; plm_ctx_get_g itself where the raw q-state vector of gap mode is needed); N = 130 sequences, weights 1 /
oracle64.reweight, the cases, settings and x of assemble_twin.cases().

  a  differencing   the data part of an evaluation does not depend on the regulariser strengths, so for two contexts A, B
                    at the same x and weights and EVERY entry |(g_A - g_B) - (p_A - p_B)| <= ulp32(g_A) / 2 + ulp32(g_B) / 2
                    (each g is one fused rounding of data + p), the left side in float64.  Where a context has
                    lambda_g > 0, 4 ulp32(p) more: n2 is summed in another order before its rounding, then sqrtf and the
                    division.  evcouplings_amd/csrc/Makefile builds with -O3 and WITHOUT -ffast-math (sqrtf and the
                    division are correctly rounded, nothing is reassociated); with other flags the allowance would have
                    to be derived again.  First the precondition: two contexts with the same strengths return the same
                    bits.  For q = 21 at L = 33 crossed with PLM_BWD_KERNEL, PLM_BWD_PLANES and PLM_FWD_ACCURATE.
  b  value          fx - nll == reg_value within terms 2^-53 reg + 2^-52 |fx| (+ 4 2^-24 of the group part); zero
                    strengths: fx == nll exactly
  c  structure      the entries of the raw canonical gradient no parameter owns are 0.0; set_x / get_x returns x's bits
  d  replicated     dist.LoopbackShards (k_slab_reduce -> float slabs -> k_assemble) returns the bits of the single-GPU
                    path (int32 partials -> g_combine4 in k_assemble_v), fields included; fx to 1e-12 (the shards' -log P
                    partials are added in another order)
  e  sharded state  dist.ThreadedShards: a and b on every rank's gathered gradient and the all-reduced fx, nll (remote
                    fragments, k_pack_g, the gradient halo, the rectangles behind the triangle); with the exact forward
                    GEMM and max|J| planted in every pair of site blocks, the coupling gradient has the single-GPU bits
  f  reduced        after optimize() of a variable-projection context the field part of the gradient is exactly zero
                    (k_assemble_h mode 2) and the structural zeros hold

Measured on an MI355X: the 154 tests of this file take 4 s together (3.3 s and 4.2 s in two runs of the file alone; the
slowest, the four ranks at L = 100, 1.2 s), inside a GPU suite of 684 s that took about 680 s without it.  In those runs the
shards of d and e returned the single-GPU bits in every entry, fields included, and no bit-equality had to be relaxed.
The vacuity guards of c and f ask that more than half of the live entries are non-zero: at q = 32 some 1.5 % of the data
sums of the all-zero blocks round to an exact zero.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_twin as at  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
CASES = at.cases()
U53, U24 = 2.0 ** -53, 2.0 ** -24
_inputs, _runs = {}, {}


@pytest.fixture(scope="module")
def plm():
    from evcouplings_amd import plm as _plm
    assert _plm.device_count() >= 1, "no gfx950 device: the HIP path has no fallback"
    return _plm


def _env(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _case_inputs(oracle64, case, planted=False):
    """alignment, x (model layout), block kinds and weights of a case: computed once, shared, read-only"""
    key = (case[0], planted)
    if key not in _inputs:
        _, L, q, gap = case
        msa = at.case_alignment(case)
        x, kind = at.model_x(L, q - 1 if gap else q, at.case_seed(case), plant_max_in_block_pairs=planted)
        w = (1.0 / (oracle64.reweight_gaps if gap else oracle64.reweight)(msa, 0.8)).astype(F32)
        for a in (msa, x, kind, w):
            a.setflags(write=False)
        _inputs[key] = (msa, x, kind, w)
    return _inputs[key]


def _raw_gradient(plm, ctx):
    """plm_ctx_get_g as it is: the q-state canonical vector (get_g strips the gap state)"""
    from evcouplings_amd._lib import check
    g = np.full(plm.n_params(ctx.L, ctx.q), np.nan, F32)
    check(ctx.lib.plm_ctx_get_g(ctx._h, g.ctypes.data_as(C.c_void_p)))
    return g


def _evaluate(plm, case, inputs, setting, collective=None, **kw):
    """one context, one evaluation -> (fx, nll, raw gradient, x read back)"""
    _, L, q, gap = case
    msa, x, kind, w = inputs
    with plm.PlmContext(msa, q=q, ignore_gaps=gap, lambda_h=setting[0], lambda_j=setting[1], lambda_group=setting[2],
                        **kw) as ctx:
        if collective is not None:
            ctx.set_collective(collective)
        ctx.set_weights(w)
        ctx.set_x(x)
        xb = ctx.get_x()
        fx, nll = ctx.eval()
        return fx, nll, _raw_gradient(plm, ctx), xb


def _case_runs(plm, oracle64, case, tag=""):
    """every setting of a case evaluated once (the first and fourth twice: the precondition), shared by the tests"""
    key = (case[0], tag)
    if key not in _runs:
        inputs = _case_inputs(oracle64, case)
        runs = [_evaluate(plm, case, inputs, s) for s in at.SETTINGS]
        again = {k: _evaluate(plm, case, inputs, at.SETTINGS[k]) for k in (0, 3)}
        _runs[key] = (runs, again)
    return _runs[key]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _check_differencing(case, x, runs, tag):
    """test a on the raw gradients of one context per setting"""
    _, L, q, gap = case
    qm = q - 1 if gap else q
    for (a, b) in at.PAIRS:
        sA, sB = at.SETTINGS[a], at.SETTINGS[b]
        gA, gB = runs[a][2].astype(F64), runs[b][2].astype(F64)
        pA, pB = (at.reg_gradient(x, L, qm, *s).astype(F64) for s in (sA, sB))
        if gap:
            pA, pB = at.embed_gaps(pA, L, q), at.embed_gaps(pB, L, q)
        assert np.isfinite(gA).all() and np.isfinite(gB).all()
        err = np.abs((gA - gB) - (pA - pB))
        bound = at.gradient_bound(gA, gB, pA, pB, sA, sB)
        over = err > bound
        print("%s%s settings %d - %d: %d of %d entries over the bound, worst error / bound %.3f, max |g| %.3g, max |p_A - p_B| %.3g"
              % (case[0], tag, a, b, int(over.sum()), over.size, float((err / bound).max()), float(np.abs(gA).max()),
                 float(np.abs(pA - pB).max())))
        assert not over.any(), "%s%s settings %d - %d: first entry %d" % (case[0], tag, a, b, int(np.flatnonzero(over)[0]))


def _check_values(case, x, runs, tag):
    """test b"""
    _, L, q, gap = case
    qm = q - 1 if gap else q
    for k, s in enumerate(at.SETTINGS):
        fx, nll = runs[k][0], runs[k][1]
        if k == 0:
            assert fx == nll, (fx, nll)
            continue
        parts = at.reg_parts(x, L, qm, *s)
        reg = sum(parts)
        tol = at.value_terms(L, qm) * U53 * reg + 2.0 ** -52 * abs(fx) + (4 * U24 * parts[2] if s[2] > 0 else 0.0)
        print("%s%s %r: fx - nll = %.17g, twin %.17g, error %.3g, tolerance %.3g" % (case[0], tag, s, fx - nll, reg,
                                                                                 abs((fx - nll) - reg), tol))
        assert abs((fx - nll) - reg) <= tol


# ------------------------------------------------------------------------------------------------ a, b, c: one GPU
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_same_strengths_give_the_same_bits(plm, oracle64, case):
    runs, again = _case_runs(plm, oracle64, case)
    for k, (fx, nll, g, _) in again.items():
        assert fx == runs[k][0] and nll == runs[k][1] and _same_bits(g, runs[k][2])
    for k in range(1, len(at.SETTINGS)):
        assert runs[k][1] == runs[0][1], "nll depends on the strengths"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_regulariser_gradient_by_differencing(plm, oracle64, case):
    runs, _ = _case_runs(plm, oracle64, case)
    _check_differencing(case, _case_inputs(oracle64, case)[1], runs, "")


CROSS = [(kern, planes, acc) for kern in (0, 1) for planes in (3, 4) for acc in (0, 1)]
CROSS_CASES = [c for c in CASES if c[1] == 33 and c[2] == 21]


@pytest.mark.parametrize("kern,planes,acc", CROSS)
@pytest.mark.parametrize("case", CROSS_CASES, ids=[c[0] for c in CROSS_CASES])
def test_regulariser_gradient_under_every_backward_kernel(plm, oracle64, monkeypatch, case, kern, planes, acc):
    _env(monkeypatch, PLM_BWD_KERNEL=kern, PLM_BWD_PLANES=planes, PLM_FWD_ACCURATE=acc)      # read when a context is made
    tag = " kernel=%d planes=%d accurate=%d" % (kern, planes, acc)
    runs, again = _case_runs(plm, oracle64, case, tag)
    for k, (fx, nll, g, _) in again.items():
        assert fx == runs[k][0] and nll == runs[k][1] and _same_bits(g, runs[k][2])
    x = _case_inputs(oracle64, case)[1]
    _check_differencing(case, x, runs, tag)
    _check_values(case, x, runs, tag)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_regulariser_value(plm, oracle64, case):
    runs, _ = _case_runs(plm, oracle64, case)
    _check_values(case, _case_inputs(oracle64, case)[1], runs, "")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_structural_zeros_and_the_round_trip_of_x(plm, oracle64, case):
    _, L, q, gap = case
    runs, _ = _case_runs(plm, oracle64, case)
    x = _case_inputs(oracle64, case)[1]
    dead = at.raw_structural_zeros(L, q, gap)
    assert dead.sum() == plm.n_params(L, q) - x.size
    for k, (_, _, g, xb) in enumerate(runs):
        assert g.shape == dead.shape and not np.isnan(g).any()
        assert (g[dead] == 0.0).all(), "setting %d: %d structural entries are not zero" % (k, int((g[dead] != 0).sum()))
        assert xb.dtype == F32 and _same_bits(xb, x)
    live = runs[1][2][~dead]
    assert (live != 0).mean() > 0.5                 # ... and the live ones are there


# ------------------------------------------------------------------------------------------------ d: replicated shards
def _loopback(plm, msa, w, q, setting, n_shards):
    """dist.LoopbackShards with the group strength: its own constructor takes none"""
    from evcouplings_amd.dist import LoopbackShards

    class Shards(LoopbackShards):
        def __init__(self):
            self.hip = C.CDLL("libamdhip64.so")
            self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            self.n_shards = n_shards
            self.ctx = [plm.PlmContext(msa, q=q, lambda_h=setting[0], lambda_j=setting[1], lambda_group=setting[2],
                                       n_shards=n_shards, shard=r) for r in range(n_shards)]
            for c in self.ctx:
                c.set_weights(w)
            self.slabs = {}

    return Shards()


SHARD_CASES = {40: ("shards-L40", 40, 21, False), 100: ("shards-L100", 100, 21, False)}


@pytest.mark.parametrize("lg", [0.0, 7.5])
@pytest.mark.parametrize("L,n_shards", [(40, 2), (40, 3), (40, 4), (100, 3)])
def test_replicated_shards_return_the_single_gpu_bits(plm, oracle64, L, n_shards, lg):
    """k_slab_reduce's g_combine and k_assemble against g_combine4 and k_assemble_v: the same integer sums, one rounding
    each, the same fused multiply-add.  L = 40 has three site blocks: with 4 shards one shard owns nothing."""
    case = SHARD_CASES[L]
    inputs = _case_inputs(oracle64, case)
    msa, x, kind, w = inputs
    setting = (0.01, 1.7, lg)
    fx1, nll1, g1, _ = _evaluate(plm, case, inputs, setting)
    shards = _loopback(plm, msa, w, 21, setting, n_shards)
    try:
        fx, nll, g = shards.evaluate(x)
    finally:
        for c in shards.ctx:
            c.close()
    diff = g.view(np.uint32) != g1.view(np.uint32)
    print("L=%d shards=%d lambda_g=%g: %d of %d gradient entries differ (%d of them fields), fx %.17g against %.17g" % (
        L, n_shards, lg, int(diff.sum()), diff.size, int(diff[:L * 21].sum()), fx, fx1))
    np.testing.assert_array_equal(g, g1)
    assert fx == pytest.approx(fx1, rel=1e-12, abs=0) and nll == pytest.approx(nll1, rel=1e-12, abs=0)


# ------------------------------------------------------------------------------------------------ e: sharded state
def _sharded_runs(plm, case, inputs, settings, n_shards):
    """every rank in its own thread: one context per setting, in the same order on every rank -> [rank][setting]"""
    from evcouplings_amd.dist import ThreadedShards

    def work(r, coll):
        return [_evaluate(plm, case, inputs, s, collective=coll, n_shards=n_shards, shard=r, sharded_state=True)
                for s in settings]

    return ThreadedShards(n_shards).run(work)


@pytest.mark.parametrize("L,n_shards", [(40, 2), (40, 3), (40, 4), (100, 4)])
def test_sharded_state_regulariser_on_every_rank(plm, oracle64, L, n_shards):
    case = SHARD_CASES[L]
    inputs = _case_inputs(oracle64, case)
    x = inputs[1]
    outs = _sharded_runs(plm, case, inputs, list(at.SETTINGS) + [at.SETTINGS[3]], n_shards)
    for r, runs in enumerate(outs):
        tag = " rank %d of %d" % (r, n_shards)
        assert runs[5][0] == runs[3][0] and runs[5][1] == runs[3][1] and _same_bits(runs[5][2], runs[3][2]), tag
        assert _same_bits(runs[0][3], x), tag
        for k in range(1, len(at.SETTINGS)):
            assert runs[k][1] == runs[0][1], "nll depends on the strengths" + tag
        _check_differencing(case, x, runs, tag)
        _check_values(case, x, runs, tag)
        for k in range(len(runs)):
            assert runs[k][0] == outs[0][k][0] and _same_bits(runs[k][2], outs[0][k][2]), "ranks disagree" + tag


@pytest.mark.parametrize("L,n_shards", [(40, 2), (40, 3), (40, 4), (100, 4)])
def test_sharded_state_coupling_gradient_has_the_single_gpu_bits(plm, oracle64, monkeypatch, L, n_shards):
    """PLM_FWD_ACCURATE=1: the forward GEMM is exact integer work given the scale exponent, which every rank takes from the
    max|J| of its own block pairs and halo (k_maxabs2) -- the x of this test plants the global maximum in every pair of
    site blocks.  The residuals, their integer sums and the one rounding per fragment (g_combine4 at home, k_pack_g for the
    halo) are then the single-GPU ones."""
    _env(monkeypatch, PLM_FWD_ACCURATE=1, PLM_BWD_KERNEL=None, PLM_BWD_PLANES=None)
    case = SHARD_CASES[L]
    inputs = _case_inputs(oracle64, case, planted=True)
    x = inputs[1]
    nblk = (L + 15) // 16
    iu, ju = at.pair_sites(L)
    top = np.abs(at.couplings_of(x, L, 21)).reshape(iu.size, -1).max(axis=1) == at.BIG
    assert len(set(zip((iu[top] // 16).tolist(), (ju[top] // 16).tolist()))) == nblk * (nblk + 1) // 2
    setting = at.SETTINGS[3]
    fx1, nll1, g1, _ = _evaluate(plm, case, inputs, setting)
    outs = _sharded_runs(plm, case, inputs, [setting], n_shards)
    for r, runs in enumerate(outs):
        fx, nll, g, _ = runs[0]
        diff = g.view(np.uint32) != g1.view(np.uint32)
        print("L=%d rank %d of %d: %d of %d entries differ (%d of them fields)" % (L, r, n_shards, int(diff.sum()), diff.size,
                                                                                int(diff[:L * 21].sum())))
        np.testing.assert_array_equal(g[L * 21:], g1[L * 21:])
        assert fx == pytest.approx(fx1, rel=1e-12, abs=0)


# ------------------------------------------------------------------------------------------------ f: reduced objective
REDUCED = [c for c in CASES if (c[1], c[2]) in ((17, 21), (33, 7), (16, 32), (2, 5))]


@pytest.mark.parametrize("lg", [0.0, 7.5])
@pytest.mark.parametrize("case", REDUCED, ids=[c[0] for c in REDUCED])
def test_reduced_objective_has_no_field_gradient(plm, oracle64, case, lg):
    _, L, q, gap = case
    msa, x, kind, w = _case_inputs(oracle64, case)
    with plm.PlmContext(msa, q=q, ignore_gaps=gap, lambda_h=0.01, lambda_j=1.7, lambda_group=lg, max_iter=2) as ctx:
        ctx.set_weights(w)
        ctx.marginals(pairs=False)
        ctx.set_x(x)
        res = ctx.optimize()
        g = _raw_gradient(plm, ctx)
    assert res["n_evals"] >= 1 and not np.isnan(g).any()
    assert not g[:L * q].any(), "%d field entries of the reduced gradient are not zero" % int((g[:L * q] != 0).sum())
    dead = at.raw_structural_zeros(L, q, gap)
    assert (g[dead] == 0.0).all()
    assert (g[L * q:][~dead[L * q:]] != 0).mean() > 0.5
