"""The autoregressive Potts model on the GPU (plm_ar_logprob / plm_ar_sample / plm_ar_eval / plm_ar_fit, DESIGN_NEXT_ROWS.md
section 9.19) against the float64 twin tests/ar_twin.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import optimize, stats
from scipy.special import logsumexp

import ar_twin as tw
import sampler_twin as st
from evcouplings_amd import alignment_io, ar_model, plm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (L, q, n): the first five are the working shapes; the rest are the edges -- counts that are no multiple of 4 or 64,
# fewer sequences than a wave, q at both ends, one site (no pair, an empty J)
SHAPES = [(24, 21, 4096), (300, 21, 512), (45, 32, 2048), (17, 2, 4096), (64, 5, 1000),
          (33, 21, 1023), (70, 5, 333), (17, 32, 1021), (3, 2, 1), (2, 3, 5), (1, 7, 1000)]
SEED = 11
EPS = 2.0 ** -50


@functools.lru_cache(maxsize=None)
def _model(L, q):
    return tw.random_model(L, q)


@functools.lru_cache(maxsize=None)
def _sequences(L, q, n):
    return np.random.default_rng(100 + L).integers(0, q, (n, L)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _twin_pass(L, q, n):
    h, J = _model(L, q)
    return tw.sample(h, J, n, seed=SEED)


# ---- sampler, draw for draw -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,n", SHAPES)
def test_sampler_draw_for_draw(L, q, n):
    h, J = _model(L, q)
    gpu = plm.ar_sample(h, J, q, n, seed=SEED)
    assert gpu.shape == (n, L) and gpu.min() >= 0 and gpu.max() < q
    x, margin, maxbu = _twin_pass(L, q, n)
    tw.explained("ar_sample %s" % ((L, q, n),), gpu, x, margin, maxbu, L, q)


def test_sampler_beta_and_mask():
    L, q, n = 24, 21, 4096
    h, J = _model(L, q)
    allowed = np.ones(q, bool)
    allowed[0] = False
    gpu = plm.ar_sample(h, J, q, n, seed=SEED, beta=0.5, allowed=allowed)
    assert gpu.min() >= 1
    x, margin, maxbu = tw.sample(h, J, n, seed=SEED, beta=0.5, allowed=allowed)
    tw.explained("ar_sample beta 0.5, no state 0", gpu, x, margin, maxbu, L, q)


@pytest.mark.parametrize("L,q", [(24, 21), (45, 32), (70, 5)])
def test_sampler_chain_identity(L, q):
    """chain c is the same chain whatever n_samples and however a run is cut by first_chain"""
    h, J = _model(L, q)
    big = plm.ar_sample(h, J, q, 4096, seed=SEED)
    small = plm.ar_sample(h, J, q, 1000, seed=SEED)
    assert np.array_equal(big[:1000], small)
    a = plm.ar_sample(h, J, q, 600, seed=SEED)
    b = plm.ar_sample(h, J, q, 400, seed=SEED, first_chain=600)
    assert np.array_equal(np.concatenate([a, b]), small)
    assert not np.array_equal(plm.ar_sample(h, J, q, 1000, seed=SEED + 1), small)


@pytest.mark.parametrize("L,q,n", [(24, 21, 4096), (300, 21, 512), (17, 32, 1021), (17, 2, 4096), (3, 2, 1), (1, 7, 1000)])
def test_sampler_forms_agree_bit_for_bit(L, q, n, monkeypatch):
    h, J = _model(L, q)
    monkeypatch.setenv("PLM_AR_FORM", "tiled")
    tiled = plm.ar_sample(h, J, q, n, seed=SEED)
    monkeypatch.setenv("PLM_AR_FORM", "direct")
    direct = plm.ar_sample(h, J, q, n, seed=SEED)
    assert np.array_equal(tiled, direct)
    monkeypatch.setenv("PLM_AR_FORM", "neither")
    with pytest.raises(plm._lib.PlmError):
        plm.ar_sample(h, J, q, n, seed=SEED)


def test_sampler_distribution():
    L, q, n = 5, 4, 200000
    h, J = _model(L, q)
    x = plm.ar_sample(h, J, q, n, seed=3)
    counts = np.bincount(st.state_index(x, q), minlength=q ** L)
    chi2, dof = st.chi2_counts(counts, tw.enumerate_p(h, J), n)
    bound = stats.chi2.isf(1e-6, dof)
    print("chi2 = %.1f with %d degrees of freedom, bound %.1f" % (chi2, dof, bound))
    assert chi2 < bound


# ---- log P -------------------------------------------------------------------------------------------------------------

def _logp_bound(x, h, J):
    """|log P_gpu - log P_twin| per sequence.  A logit is a float64 sum of at most L terms of size <= max|logit|: error
    <= L 2^-53 max|logit| in either implementation.  A site term adds the max (exact), q exp and q adds (q 2^-53 each,
    relative to a sum in [1, q], whose log has derivative <= 1), one log and two subtractions: a few 2^-53 (1 + |logit|).
    So a site term differs by at most ~2 (L + q + 4) 2^-53 (1 + max|logit|) <= 2^-50 (q + L)(1 + max|logit|) / 2 between
    the two, libm's exp and log (<= 1 ulp here, 2 ulp allowed for) included, and log P sums L of them with L more
    roundings of size 2^-53 |log P| <= 2^-53 L (1 + max|logit|) log q each: 2^-50 L (q + L)(1 + max|logit|) in all."""
    L, q = h.shape
    return EPS * L * (q + L) * (1.0 + np.abs(tw.logits(x, h, J)).max(axis=(1, 2)))


@pytest.mark.parametrize("L,q,n", SHAPES)
def test_logprob_against_twin(L, q, n):
    h, J = _model(L, q)
    x = _sequences(L, q, n)
    lp, site = plm.ar_logprob(x, q, h, J, site_terms=True)
    ref = tw.site_logp(x, h, J)
    bound = _logp_bound(x, h, J)
    err = np.abs(lp - ref.sum(axis=1))
    print("log P %s: max |err| / bound = %.3g (bound %.3g)" % ((L, q, n), (err / bound).max(), bound.max()))
    assert (err <= bound).all()
    assert (np.abs(site - ref) <= bound[:, None]).all()
    # the site terms sum to log P, in site order
    t = np.zeros(n)
    for i in range(L):
        t += site[:, i]
    assert np.array_equal(t, lp)
    # the result depends on (sequence, model) only
    k = max(1, n // 3)
    assert np.array_equal(plm.ar_logprob(x[:k], q, h, J), lp[:k])
    assert np.array_equal(plm.ar_logprob(x[::-1], q, h, J), lp[::-1])


def test_logprob_normalised():
    L, q = 5, 3
    h, J = _model(L, q)
    xs = st.all_states(L, q).astype(np.int8)
    lp = plm.ar_logprob(xs, q, h, J)
    bound = _logp_bound(xs, h, J).max()
    print("logsumexp over all %d sequences: %.3g (bound %.3g)" % (len(xs), logsumexp(lp), bound))
    assert abs(logsumexp(lp)) <= bound


# ---- evaluation ----------------------------------------------------------------------------------------------------------

# every shape without and with a regulariser; a weight vector with zeros once per shape that has sequences to spare
EVAL_CASES = [s + (lam, False) for s in SHAPES for lam in ((0.0, 0.0), (0.01, 0.02))] + \
             [s + ((0.01, 0.02), True) for s in SHAPES if s[2] >= 5]


@pytest.mark.parametrize("L,q,n,lam,zeros", EVAL_CASES)
def test_eval_against_twin(L, q, n, lam, zeros):
    h, J = _model(L, q)
    x = _sequences(L, q, n)
    w = np.random.default_rng(200 + L).uniform(0.2, 1.0, n).astype(np.float32)
    if zeros:
        w[::3] = 0.0
    F, nll, gh, gJ = plm.ar_evaluate(x, w, q, lam[0], lam[1], h, J)
    F2, nll2, gh2, gJ2 = plm.ar_evaluate(x, w, q, lam[0], lam[1], h, J)
    assert F == F2 and nll == nll2 and gh.tobytes() == gh2.tobytes() and gJ.tobytes() == gJ2.tobytes()
    rF, rnll, rgh, rgJ = tw.objective(x, w, h, J, lam[0], lam[1])
    xinf = max(np.abs(h).max(), np.abs(J).max() if J.size else 0.0)
    # nll is a weighted mean of log P: the bound of log P carries over (the weights are exact, their n products and
    # sums add 2 n 2^-53 relative, far inside).  The regulariser is a float64 sum of P squares that neither side takes
    # in one chain: the library in 65 536 strided chains of P / 65 536 terms and two trees of depth 8, numpy in blocks
    # of 128 and a tree; the relative error of either is at most (longest chain + tree depth) 2^-53
    reg = lam[0] * float((h.astype(np.float64) ** 2).sum()) + lam[1] * float((J.astype(np.float64) ** 2).sum())
    fb = _logp_bound(x, h, J).max() + EPS * abs(rnll) + 2.0 ** -53 * ((h.size + J.size) / 65536.0 + 256.0) * reg
    print("eval %s lambda %s: |dF| = %.3g, |dnll| = %.3g (bound %.3g)" % ((L, q, n), lam, abs(F - rF), abs(nll - rnll), fb))
    assert abs(nll - rnll) <= fb and abs(F - rF) <= fb
    # An entry is -(1/N_eff) sum_s w_s (delta - p) + 2 lambda x.  Each of the n terms is at most w_s in size and carries
    # the relative error of p -- the error of the logit differences, L 2^-53 max|logit| <~ 2^-52 L (1 + |x|_inf) L / L,
    # plus exp and the division -- and the sum adds n roundings; with N_eff >= 0.2 n that is 2^-50 n (1 + |x|_inf) with
    # room.  The regulariser term 2 lambda x is one product and one add: 2^-52 |2 lambda x| + 2^-53 |entry|.
    gb = EPS * n * (1.0 + xinf) + 2.0 ** -52 * 2.0 * max(lam) * xinf + 2.0 ** -53 * (1.0 + 2.0 * max(lam) * xinf)
    eh, eJ = np.abs(gh - rgh).max(), (np.abs(gJ - rgJ).max() if J.size else 0.0)
    print("      max |dg_h| = %.3g, max |dg_J| = %.3g (bound %.3g)" % (eh, eJ, gb))
    assert eh <= gb and eJ <= gb


# ---- fit -------------------------------------------------------------------------------------------------------------------

FITS = [(6, 4, 200), (12, 21, 300), (24, 5, 1000)]
LAM, FIT_EPS = 0.01, 1e-4


@functools.lru_cache(maxsize=None)
def _fit_data(L, q, n):
    h, J = tw.random_model(L, q, sd_j=0.4)
    x = plm.ar_sample(h, J, q, n, seed=5)
    w = np.random.default_rng(300 + L).uniform(0.2, 1.0, n).astype(np.float32)
    return x, w


@functools.lru_cache(maxsize=None)
def _fit(L, q, n):
    x, w = _fit_data(L, q, n)
    trace = []
    res = plm.ar_fit(x, w, q, LAM, LAM, max_iter=2000, epsilon=FIT_EPS, callback=lambda *a: trace.append(a) and False)
    return res, trace


def _cond(g_h, g_J, h, J):
    gn = np.sqrt((g_h ** 2).sum() + (g_J ** 2).sum())
    xn = np.sqrt((h.astype(np.float64) ** 2).sum() + (J.astype(np.float64) ** 2).sum())
    return gn, xn


@pytest.mark.parametrize("L,q,n", FITS)
def test_fit_converges_to_the_optimum(L, q, n):
    x, w = _fit_data(L, q, n)
    res, trace = _fit(L, q, n)
    print("fit %s: %s after %d iterations, %d evaluations, F = %.9f" % ((L, q, n), res["status"], res["iterations"],
                                                                         res["evaluations"], res["fx"]))
    assert res["status"] == "converged"
    assert res["hi"].dtype == np.float32 and len(trace) == res["iterations"]
    # the twin's float64 gradient at the returned float32 point satisfies the stop rule
    F, nll, gh, gJ = tw.objective(x, w, res["hi"], res["jij"], LAM, LAM)
    gn, xn = _cond(gh, gJ, res["hi"], res["jij"])
    print("      twin: |g| = %.6e, eps max(1, |x|) = %.6e; library: |g| = %.6e, |x| = %.6f" % (gn, FIT_EPS * max(1.0, xn),
                                                                                               res["gnorm"], res["xnorm"]))
    assert gn <= FIT_EPS * max(1.0, xn) * (1.0 + 1e-6)
    fb = _logp_bound(x, res["hi"], res["jij"]).max() + EPS * abs(F)      # as in test_eval_against_twin
    assert abs(res["fx"] - F) <= fb and abs(res["nll"] - nll) <= fb
    F0 = tw.objective(x, w, np.zeros((L, q)), np.zeros((L * (L - 1) // 2, q, q)), LAM, LAM, gradient=False)[0]
    assert res["fx"] <= F0
    # distance to the optimum of an independent optimiser on the twin's objective: F is 2 min(lambda)-strongly convex,
    # so (g(a) - g(b)).(a - b) >= 2 lambda |a - b|^2 and |a - b| <= |g(a) - g(b)| / (2 lambda) <= (|g_a| + |g_b|) / (2 lambda)

    def fg(p):
        f, _, a, b = tw.objective(x, w, *tw.unpack(p, L, q), LAM, LAM)
        return f, tw.pack(a, b)

    ref = optimize.minimize(fg, np.zeros(tw.n_params(L, q)), jac=True, method="L-BFGS-B",
                            options={"gtol": 1e-12, "ftol": 0.0, "maxiter": 20000, "maxfun": 40000, "maxcor": 10})
    g_ref = np.linalg.norm(fg(ref.x)[1])
    dist = np.linalg.norm(tw.pack(res["hi"], res["jij"]) - ref.x)
    print("      |x_fit - x_ref| = %.6e <= (|g_fit| + |g_ref|) / (2 lambda) = %.6e  (|g_ref| = %.3e)"
          % (dist, (gn + g_ref) / (2 * LAM), g_ref))
    assert dist <= (gn + g_ref) / (2 * LAM)


def test_fit_statuses_and_restart():
    L, q, n = FITS[0]
    x, w = _fit_data(L, q, n)
    res, _ = _fit(L, q, n)
    trace = []
    r3 = plm.ar_fit(x, w, q, LAM, LAM, max_iter=3, epsilon=FIT_EPS, callback=lambda *a: trace.append(a[0]) and False)
    assert r3["status"] == "maxiter" and r3["iterations"] == 3 and trace == [1, 2, 3]
    r2 = plm.ar_fit(x, w, q, LAM, LAM, max_iter=2, epsilon=FIT_EPS)
    stop = plm.ar_fit(x, w, q, LAM, LAM, max_iter=2000, epsilon=FIT_EPS, callback=lambda it, *a: it == 2)
    assert stop["status"] == "interrupted" and stop["iterations"] == 2
    assert np.array_equal(stop["hi"], r2["hi"]) and np.array_equal(stop["jij"], r2["jij"])
    again = plm.ar_fit(x, w, q, LAM, LAM, max_iter=2000, epsilon=FIT_EPS, start=(res["hi"], res["jij"]))
    assert again["status"] == "converged" and again["iterations"] <= 1
    twice = plm.ar_fit(x, w, q, LAM, LAM, max_iter=2000, epsilon=FIT_EPS)
    assert twice["hi"].tobytes() == res["hi"].tobytes() and twice["jij"].tobytes() == res["jij"].tobytes()
    assert twice["fx"] == res["fx"] and twice["iterations"] == res["iterations"]


def test_closed_loop():
    """A model fitted to samples of a planted model is closer to it (in KL, estimated on an independent draw) than the
    independent-site model fitted to the same samples."""
    L, q, n = 8, 4, 100000
    h, J = tw.random_model(L, q, sd_j=0.4)
    train = plm.ar_sample(h, J, q, n, seed=1)
    test = plm.ar_sample(h, J, q, n, seed=2)
    res = plm.ar_fit(train, np.ones(n, np.float32), q, 1e-4, 1e-4, max_iter=2000, epsilon=1e-4)
    planted = plm.ar_logprob(test, q, h, J).mean()
    fitted = plm.ar_logprob(test, q, res["hi"], res["jij"]).mean()
    fi = ar_model.weighted_frequencies(train, np.ones(n), q)
    indep = plm.ar_logprob(test, q, np.log(fi), np.zeros_like(J)).mean()
    print("mean log P on the held-out draw: planted %.6f, fitted %.6f (gap %.3e), independent sites %.6f (gap %.3e); %s "
          "after %d iterations" % (planted, fitted, planted - fitted, indep, planted - indep, res["status"], res["iterations"]))
    assert planted - fitted < planted - indep


# ---- command line ----------------------------------------------------------------------------------------------------------

def test_command_line_fit_sample_score(tmp_path):
    run = lambda *a: subprocess.run([sys.executable, "-m", "evcouplings_amd.ar_model"] + [str(v) for v in a], cwd=ROOT,
                                    capture_output=True, text=True, timeout=300)
    model, a2m, csv = tmp_path / "m.npz", tmp_path / "s.a2m", tmp_path / "s.csv"
    r = run("fit", os.path.join(ROOT, "tests", "golden", "hip_fit_L24.a2m"), "-o", model, "--max-iter", 30)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("sample", model, "-n", 64, "-o", a2m, "--no-gaps", "--seed", 4)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("score", model, "--sequences", a2m, "-o", csv)
    assert r.returncode == 0, r.stderr[-2000:]
    m = ar_model.load(str(model))
    assert m.L == 24 and m.q == 21 and sorted(m.order.tolist()) == list(range(24))
    enc = alignment_io.encode_alignment(str(a2m), alphabet=m.alphabet)
    assert enc.msa.shape == (65, 24) and (enc.msa[1:] > 0).all()
    lines = open(csv).read().split()
    assert lines[0] == "id,log_p" and len(lines) == 66
    scored = np.array([float(ln.split(",")[1]) for ln in lines[1:]])
    direct = plm.ar_logprob(np.ascontiguousarray(enc.msa[:, m.order]), m.q, m.hi, m.jij)
    assert np.array_equal(scored, direct)
    assert np.array_equal(enc.msa[1:], ar_model.sample_sequences(m, 64, seed=4, exclude=m.alphabet[0]))
