"""The Gibbs sampler on the MI355X (plm_sample / plm.sample) against its numpy twin (tests/sampler_twin.py) and against
exactly enumerated distributions.  The chi-square thresholds are scipy's at a false-alarm level of 1e-6 (family-wise
where a test makes several); with the fixed seeds below the tests are deterministic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_twin as tw  # noqa: E402
from evcouplings_amd import _lib, model_io, plm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _random_model(rng, L, q, h_scale=1.0, j_scale=0.15):
    h = _f32(rng.normal(scale=h_scale, size=(L, q)))
    J = _f32(rng.normal(scale=j_scale, size=(L * (L - 1) // 2, q, q)))
    return h, J


def _explained(name, gpu, twin, margin, maxbu, L, q, cap=0.01):
    """The condition of the draw-for-draw tests.  gpu, twin: [S][C][L] states after each of S steps (sweeps, or the
    start rule); margin, maxbu: the twin's diagnostics per (step, chain, site).  A chain may differ only if at its first
    differing (step, site) the twin's u lies within delta = 2^-24 (L + 4q)(1 + max|beta U|) of a step of the twin's
    normalised CDF, and at most `cap` of the chains may differ at all."""
    S, Cn, _ = twin.shape
    differs = (gpu != twin).any(axis=2)                   # [S][C]
    bad = np.nonzero(differs.any(axis=0))[0]
    unexplained = []
    for c in bad:
        s = int(np.argmax(differs[:, c]))
        i = int(np.argmax(gpu[s, c] != twin[s, c]))
        delta = 2.0 ** -24 * (L + 4 * q) * (1.0 + maxbu[s, c, i])
        if not margin[s, c, i] <= delta:
            unexplained.append((int(c), s, i, float(margin[s, c, i]), float(delta)))
    print("%s: %d of %d chains differ from the twin, %d unexplained" % (name, len(bad), Cn, len(unexplained)))
    assert not unexplained, unexplained[:5]
    assert len(bad) <= cap * Cn, (len(bad), Cn)


def _twin_sweeps(h, W, x0, seed, n, beta=1.0):
    Cn, L = x0.shape
    x = x0.astype(np.int64).copy()
    out = np.zeros((n, Cn, L), np.int64)
    margin, maxbu = np.ones((n, Cn, L)), np.zeros((n, Cn, L))
    for s in range(n):
        tw.sweep(x, h, W, seed, s, beta, margin=margin[s], maxbu=maxbu[s])
        out[s] = x
    return out, margin, maxbu


@pytest.mark.parametrize("L,q,Cn", [(32, 21, 4096), (300, 21, 512), (45, 32, 2048), (17, 2, 4096), (64, 5, 2048)])
def test_draw_for_draw_against_the_twin(L, q, Cn):
    rng = np.random.default_rng(1000 + L)
    h, J = _random_model(rng, L, q)
    x0 = rng.integers(0, q, size=(Cn, L))
    seed = 12345 + L
    gpu, _ = plm.sample(h, J, q, Cn, burn_in=1, n_snapshots=2, thin=1, seed=seed, start=x0, energies=False)
    twin, margin, maxbu = _twin_sweeps(h, tw.dense(J, L, q), x0, seed, 2)
    _explained("L=%d q=%d C=%d" % (L, q, Cn), gpu.astype(np.int64), twin, margin, maxbu, L, q)


def test_draw_for_draw_on_a_fitted_model():
    m = model_io.read_model_file(os.path.join(ROOT, "golden", "hip_fit_L24.model"))
    L, q, Cn = m["L"], m["q"], 4096
    h, J = _f32(m["hi"]), _f32(m["jij"])
    x0 = np.random.default_rng(5).integers(0, q, size=(Cn, L))
    gpu, _ = plm.sample(h, J, q, Cn, burn_in=1, n_snapshots=2, thin=1, seed=99, start=x0, energies=False)
    twin, margin, maxbu = _twin_sweeps(h, tw.dense(J, L, q), x0, 99, 2)
    _explained("hip_fit_L24", gpu.astype(np.int64), twin, margin, maxbu, L, q)


def test_field_only_model_of_one_site():
    rng = np.random.default_rng(8)
    q, Cn = 7, 1000
    h = _f32(rng.normal(size=(1, q)))
    J = np.zeros((0, q, q), np.float32)
    gpu, en = plm.sample(h, J, q, Cn, burn_in=2, seed=3)
    x = np.zeros((Cn, 1), np.int64)
    margin, maxbu = np.ones((1, Cn, 1)), np.zeros((1, Cn, 1))
    tw.sweep(x, h, tw.dense(J, 1, q), 3, 1, margin=margin[0], maxbu=maxbu[0])   # the last sweep decides alone
    _explained("L=1", gpu.astype(np.int64), x[None], margin, maxbu, 1, q)
    hx = h[0, gpu[0, :, 0]]
    assert np.array_equal(en[0], np.stack([hx, np.zeros(Cn), hx], axis=1))


def test_independent_of_chain_count_run_and_start_rule():
    rng = np.random.default_rng(21)
    L, q = 40, 21
    h, J = _random_model(rng, L, q)
    x0 = rng.integers(0, q, size=(4096, L))
    small, _ = plm.sample(h, J, q, 1024, burn_in=3, seed=7, start=x0[:1024], energies=False)
    large, _ = plm.sample(h, J, q, 4096, burn_in=3, seed=7, start=x0, energies=False)
    again, _ = plm.sample(h, J, q, 4096, burn_in=3, seed=7, start=x0, energies=False)
    assert np.array_equal(small[0], large[0, :1024])
    assert np.array_equal(large, again)
    other, _ = plm.sample(h, J, q, 4096, burn_in=3, seed=8, start=x0, energies=False)
    assert (other[0] != large[0]).any(axis=1).mean() > 0.9
    # start == NULL, burn_in == 0: the start rule; and it does not depend on the chain count either
    s_small, _ = plm.sample(h, J, q, 1000, burn_in=0, seed=7, energies=False)
    s_large, _ = plm.sample(h, J, q, 4096, burn_in=0, seed=7, energies=False)
    assert np.array_equal(s_small[0], s_large[0, :1000])
    margin, maxbu = np.ones((1, 4096, L)), np.zeros((1, 4096, L))
    twin = tw.start_states(h, 4096, 7, margin=margin[0], maxbu=maxbu[0])
    _explained("start rule", s_large.astype(np.int64), twin[None], margin, maxbu, L, q)


# ---- exact distribution, small model ------------------------------------------------------------------------------

SL, SQ, SC = 4, 3, 1 << 18


def _small_model():
    rng = np.random.default_rng(2)
    h = _f32(rng.normal(scale=0.5, size=(SL, SQ)))
    J = _f32(rng.normal(scale=0.5, size=(SL * (SL - 1) // 2, SQ, SQ)))
    return h, J, tw.dense(J, SL, SQ)


def _check_counts(name, samples, p):
    counts = np.bincount(tw.state_index(samples.astype(np.int64), SQ), minlength=SQ ** SL)
    assert counts[p == 0].sum() == 0, "%s: states of probability zero were drawn" % name
    chi, dof = tw.chi2_counts(counts, p, len(samples))
    bound = stats.chi2.isf(1e-6, dof)
    print("%s: chi2 = %.1f on %d degrees of freedom (bound %.1f)" % (name, chi, dof, bound))
    assert chi < bound, (chi, dof, bound)


def test_small_model_exact_distribution():
    h, J, W = _small_model()
    p = tw.boltzmann(h, W)
    assert SC * p.min() >= 5                               # 20.9 for this model
    rng = np.random.default_rng(3)
    st = tw.all_states(SL, SQ)
    x0 = st[rng.choice(len(p), size=SC, p=p)]
    out, _ = plm.sample(h, J, SQ, SC, burn_in=20, seed=777, start=x0, energies=False)
    _check_counts("from exact samples, 20 sweeps", out[0], p)
    worst = int(np.argmin(p))
    B = tw.sweeps_to_mix(np.eye(len(p))[worst], tw.transition_matrix(h, W), p)
    out, _ = plm.sample(h, J, SQ, SC, burn_in=B, seed=778, start=np.tile(st[worst], (SC, 1)), energies=False)
    _check_counts("from the least likely state, %d sweeps" % B, out[0], p)


def test_small_model_masks_and_temperature():
    h, J, W = _small_model()
    st = tw.all_states(SL, SQ)
    K = len(st)
    # allowed states: chains start from the start rule, burn_in from its exact distance to the target
    allowed = np.array([1, 0, 1], np.uint8)
    p = tw.conditioned(tw.boltzmann(h, W), SL, SQ, allowed=allowed)
    B = tw.sweeps_to_mix(tw.start_distribution(h, 1.0, allowed), tw.transition_matrix(h, W, allowed=allowed), p)
    out, _ = plm.sample(h, J, SQ, SC, burn_in=max(B, 4), seed=31, allowed=allowed, energies=False)
    assert not (out == 1).any()                            # 2^20 sites, each drawn max(B, 4) times
    _check_counts("allowed = {0, 2}, %d sweeps" % max(B, 4), out[0], p)
    # fixed sites: site 1 holds state 2 and site 3 state 0; start from the least likely state that agrees
    fixed = np.array([0, 1, 0, 1], np.uint8)
    p = tw.conditioned(tw.boltzmann(h, W), SL, SQ, fixed={1: 2, 3: 0})
    worst = int(np.argmin(np.where(p > 0, p, np.inf)))
    B = tw.sweeps_to_mix(np.eye(K)[worst], tw.transition_matrix(h, W, fixed=fixed), p)
    out, _ = plm.sample(h, J, SQ, SC, burn_in=B, seed=32, start=np.tile(st[worst], (SC, 1)), fixed=fixed, energies=False)
    assert (out[0, :, 1] == 2).all() and (out[0, :, 3] == 0).all()
    _check_counts("fixed sites 1 and 3, %d sweeps" % B, out[0], p)
    # a fixed site may hold a state that is not allowed
    both, _ = plm.sample(h, J, SQ, 4096, burn_in=3, seed=33, start=np.tile(st[worst], (4096, 1)), fixed=fixed,
                         allowed=np.array([1, 1, 0], np.uint8), energies=False)
    assert (both[0, :, 1] == 2).all() and not (both[0][:, [0, 2]] == 2).any()
    # beta = 2
    p = tw.boltzmann(h, W, beta=2.0)
    worst = int(np.argmin(p))
    B = tw.sweeps_to_mix(np.eye(K)[worst], tw.transition_matrix(h, W, beta=2.0), p)
    out, _ = plm.sample(h, J, SQ, SC, burn_in=B, beta=2.0, seed=34, start=np.tile(st[worst], (SC, 1)), energies=False)
    _check_counts("beta = 2, %d sweeps" % B, out[0], p)


# ---- exact distribution, full size --------------------------------------------------------------------------------

FL, FQ, FC = 300, 21, 65536


def test_full_size_fields_only():
    rng = np.random.default_rng(41)
    h = _f32(rng.normal(size=(FL, FQ)))
    J = np.zeros((FL * (FL - 1) // 2, FQ, FQ), np.float32)
    x0 = rng.integers(0, FQ, size=(FC, FL))
    out, _ = plm.sample(h, J, FQ, FC, burn_in=1, seed=5, start=x0, energies=False)
    p = np.exp(h - h.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    worst = 0.0
    for i in range(FL):
        chi, dof = tw.chi2_counts(np.bincount(out[0, :, i], minlength=FQ), p[i], FC)
        bound = stats.chi2.isf(1e-6 / FL, dof)
        worst = max(worst, chi / bound)
        assert chi < bound, (i, chi, dof, bound)
    print("fields only: largest chi2 / bound over %d sites = %.3f" % (FL, worst))


def test_full_size_triples():
    """Couplings only inside the 100 triples (i, i+100, i+200): the model factorises, every triple is enumerated."""
    rng = np.random.default_rng(42)
    L, q, Cn = FL, FQ, FC
    h = _f32(rng.normal(scale=0.5, size=(L, q)))
    J = np.zeros((L * (L - 1) // 2, q, q), np.float32)

    def pair(i, j):
        return i * (2 * L - i - 1) // 2 + (j - i - 1)

    st = tw.all_states(3, q)
    x0 = np.zeros((Cn, L), np.int64)
    marginals = {}
    for t in range(100):
        sites = (t, t + 100, t + 200)
        blocks = {}
        for u, v in ((0, 1), (0, 2), (1, 2)):
            blocks[(u, v)] = _f32(rng.normal(scale=0.3, size=(q, q)))
            J[pair(sites[u], sites[v])] = blocks[(u, v)]
        E = h[sites[0], st[:, 0]] + h[sites[1], st[:, 1]] + h[sites[2], st[:, 2]]
        for (u, v), blk in blocks.items():
            E = E + blk[st[:, u], st[:, v]]
        p = np.exp(E - E.max())
        p /= p.sum()
        x0[:, sites] = st[rng.choice(len(p), size=Cn, p=p)]
        p3 = p.reshape(q, q, q)
        marginals[(sites[0], sites[1])] = p3.sum(axis=2)
        marginals[(sites[0], sites[2])] = p3.sum(axis=1)
        marginals[(sites[1], sites[2])] = p3.sum(axis=0)
    out, _ = plm.sample(h, J, q, Cn, burn_in=5, seed=6, start=x0, energies=False)
    x = out[0].astype(np.int64)
    assert (x != x0).any(axis=1).mean() > 0.99
    worst = 0.0
    for (i, j), pm in marginals.items():
        chi, dof = tw.chi2_counts(np.bincount(x[:, i] * q + x[:, j], minlength=q * q), pm, Cn)
        bound = stats.chi2.isf(1e-6 / len(marginals), dof)
        worst = max(worst, chi / bound)
        assert chi < bound, (i, j, chi, dof, bound)
    print("triples: largest chi2 / bound over %d pair tables = %.3f" % (len(marginals), worst))


# ---- energies, snapshots, errors ----------------------------------------------------------------------------------

def test_energies_and_snapshots():
    rng = np.random.default_rng(51)
    L, q, Cn = 24, 21, 300
    h, J = _random_model(rng, L, q)
    out, en = plm.sample(h, J, q, Cn, burn_in=2, n_snapshots=3, thin=2, seed=11)
    assert out.shape == (3, Cn, L) and en.shape == (3, Cn, 3)
    for k in range(3):
        assert np.array_equal(en[k], plm.hamiltonians(out[k], q, h, J))
        fresh, en_f = plm.sample(h, J, q, Cn, burn_in=2 + 2 * k, seed=11)
        assert np.array_equal(fresh[0], out[k]) and np.array_equal(en_f[0], en[k])
    assert (out[0] != out[1]).any()


def test_both_forms_of_the_sweep_agree_bit_for_bit(monkeypatch):
    """PLM_SAMPLE_FORM=direct selects the kernel with one lane per state (the one long models run on)."""
    rng = np.random.default_rng(71)
    for L, q, Cn in ((50, 21, 1500), (33, 32, 700), (20, 2, 900), (70, 6, 1100)):
        h, J = _random_model(rng, L, q)
        allowed = ((np.arange(q) != 1) | (q == 2)).astype(np.uint8)        # two states: nothing to forbid
        fixed = (np.arange(L) % 7 == 3).astype(np.uint8)
        x0 = rng.integers(0, q, size=(Cn, L))
        if q > 2:
            x0[:, ~fixed.astype(bool)] = np.where(x0 == 1, 0, x0)[:, ~fixed.astype(bool)]
        runs = {}
        for form in ("tiled", "direct"):
            monkeypatch.setenv("PLM_SAMPLE_FORM", form)
            runs[form] = (plm.sample(h, J, q, Cn, burn_in=3, seed=5, beta=1.3, energies=False)[0],
                          plm.sample(h, J, q, Cn, burn_in=2, n_snapshots=2, thin=1, seed=6, start=x0, fixed=fixed,
                                     allowed=allowed, energies=False)[0])
        assert np.array_equal(runs["tiled"][0], runs["direct"][0])
        assert np.array_equal(runs["tiled"][1], runs["direct"][1])
        assert (runs["tiled"][1][1] != x0).any(axis=1).mean() > 0.9


def test_long_model_runs_on_the_direct_form():
    """L = 2600: the chain states of the tiled form no longer fit the LDS.  Couplings only inside the pairs
    (i, i + 1300), chains start from exact samples of every pair, 3 sweeps, every pair table against its distribution."""
    rng = np.random.default_rng(72)
    L, q, Cn, half = 2600, 9, 4096, 1300
    h = _f32(rng.normal(scale=0.5, size=(L, q)))
    J = np.zeros((L * (L - 1) // 2, q, q), np.float32)
    i = np.arange(half)
    blocks = _f32(rng.normal(scale=0.5, size=(half, q, q)))
    J[i * (2 * L - i - 1) // 2 + half - 1] = blocks
    p = np.exp(h[:half, :, None] + h[half:, None, :] + blocks).reshape(half, q * q)
    p /= p.sum(axis=1, keepdims=True)
    cum = np.cumsum(p, axis=1)
    cell = (rng.random((Cn, half, 1)) > cum[None]).sum(axis=2).clip(0, q * q - 1)
    x0 = np.concatenate([cell // q, cell % q], axis=1)
    out, _ = plm.sample(h, J, q, Cn, burn_in=3, seed=9, start=x0, energies=False)
    x = out[0].astype(np.int64)
    assert (x != x0).any(axis=1).all()
    worst = 0.0
    for k in range(half):
        chi, dof = tw.chi2_counts(np.bincount(x[:, k] * q + x[:, k + half], minlength=q * q), p[k], Cn)
        bound = stats.chi2.isf(1e-6 / half, dof)
        worst = max(worst, chi / bound)
        assert chi < bound, (k, chi, dof, bound)
    print("long model: largest chi2 / bound over %d pair tables = %.3f" % (half, worst))


def _raw(L, q, x, opts, samples, energies=None):
    return _lib.load().plm_sample(L, q, plm._ptr(x), C.byref(opts), 0, None, plm._ptr(samples), plm._ptr(energies))


def test_error_codes():
    rng = np.random.default_rng(61)
    L, q, Cn = 6, 4, 8
    h, J = _random_model(rng, L, q)
    for kwargs in (dict(beta=0.0), dict(beta=float("nan")), dict(beta=float("inf")), dict(allowed=np.zeros(q, np.uint8)),
                   dict(start=np.full((Cn, L), 3), allowed=np.array([1, 1, 1, 0], np.uint8)),
                   dict(start=np.full((Cn, L), q))):
        with pytest.raises(_lib.PlmError) as err:
            plm.sample(h, J, q, Cn, **kwargs)
        assert err.value.code == -1, kwargs
    with pytest.raises(_lib.PlmError) as err:
        plm.sample(np.zeros((3, 33)), np.zeros((3, 33, 33)), 33, Cn)
    assert err.value.code == -4
    # a model no device holds: L = 10 000, q = 32 is a 410 GB table.  The sizes are checked before any array is read
    dummy, samples = np.zeros(16, np.float32), np.zeros(16, np.int8)
    opts = _lib.PlmSampleOpts(1, 1, 1, 1, 1.0, 0, None, None, None)
    assert _raw(10000, 32, dummy, opts, samples) == -2
    assert b"GB" in _lib.load().plm_last_error()
    out, en = plm.sample(h, J, q, Cn, burn_in=2)
    assert out.shape == (1, Cn, L) and np.array_equal(en[0], plm.hamiltonians(out[0], q, h, J))
