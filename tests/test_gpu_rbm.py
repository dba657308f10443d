"""The restricted Boltzmann machine on the GPU (plm_rbm_score / plm_rbm_sample / plm_rbm_fit, DESIGN_NEXT_ROWS.md section
9.22) against the float64 twin tests/rbm_twin.py.  The shapes, seeds and options are those of tests/rbm_cases.py, whose
conditions (the float32 mode of the twin, no near tie in the fits compared byte for byte, the twin's own histogram and
the twin's learning) test_rbm_host.py checks on the CPU.

Observed on one MI355X: the score within 0.02 of its bound and the inputs bit for bit; 1 chain of 1000 at (70, 32, 65)
differs from the twin (a near tie), none elsewhere; chi-square 232 on 230 degrees of freedom (bound 347); the fits'
statistics within 7e-15, parameters bit for bit, trace within 3e-14; the whole file in 3 s."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

import rbm_cases as cases
import rbm_twin as tw
import sampler_twin as st
from evcouplings_amd import alignment_io, plm, rbm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


# ---- 1. the score -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M", cases.SHAPES)
def test_score_and_inputs_against_the_twin(L, q, M):
    """L + M float64 adds and the softplus terms: |error| <= (L + M + 8) 2^-52 A, A the sum of |terms| of the row"""
    g, c, W = cases.model(L, q, M)
    rng = np.random.default_rng(100 + L)
    seqs = rng.integers(0, q, (max(cases.ROWS), L)).astype(np.int8)
    want, A = tw.score(seqs, g, c, W, with_scale=True)
    want_I = tw.inputs(seqs, c, W)
    for n in cases.ROWS:
        got, I = plm.rbm_score(seqs[:n], q, g, c, W, inputs=True)
        bound = (L + M + 8) * EPS * A[:n]
        err, err_I = np.abs(got - want[:n]), np.abs(I - want_I[:n]).max(axis=1)
        print("L=%d q=%d M=%d n=%d: max error / bound = %.3g (score), %.3g (inputs)"
              % (L, q, M, n, (err / bound).max(), (err_I / bound).max()))
        assert (err <= bound).all() and (err_I <= bound).all()
        if n == max(cases.ROWS):
            whole, whole_I = got, I
    # a row alone gives the bytes it gives inside a larger call, wherever it stands
    for r in (0, 3, 256, 999):
        alone, alone_I = plm.rbm_score(seqs[r:r + 1], q, g, c, W, inputs=True)
        assert alone[0].tobytes() == whole[r].tobytes() and alone_I[0].tobytes() == whole_I[r].tobytes()
    shifted = plm.rbm_score(seqs[5:262], q, g, c, W)
    assert shifted.tobytes() == whole[5:262].tobytes()


# ---- 2. sampling, draw for draw ---------------------------------------------------------------------------------------

def _every_step(g, c, W, q, C, steps, seed, **kw):
    return plm.rbm_sample(g, c, W, q, C, burn_in=1, n_snapshots=steps, thin=1, seed=seed, hidden=True, **kw)


@pytest.mark.parametrize("L,q,M,C,variant,seed,steps", cases.DRAW_CASES)
def test_sampling_draw_for_draw_against_the_twin(L, q, M, C, variant, seed, steps):
    g, c, W = cases.model(L, q, M)
    kw = cases.draw_options(L, q, C, variant, seed)
    states, hidden = _every_step(g, c, W, q, C, steps, seed, **kw)
    tw_states, tw_hidden, rec = tw.run(g, c, W, C, steps, seed=seed, **kw)
    tw.explained("L=%d q=%d M=%d C=%d %s" % (L, q, M, C, variant), states.astype(np.int64), hidden.astype(np.int64),
                 tw_states, tw_hidden, rec, q)
    assert set(np.unique(hidden)) <= {0, 1}
    if "fixed" in kw:
        f = kw["fixed"]
        assert (states[:, :, f] == kw["start"][None][:, :, f]).all()
        assert (states[:, :, ~f] != kw["start"][None][:, :, ~f]).any()
    if "allowed" in kw:
        assert kw["allowed"][states.astype(np.int64)].all()


def test_start_rule_against_the_twin():
    """a run without steps returns the start states; its hidden units are zeros"""
    L, q, M = 13, 21, 7
    g, c, W = cases.model(L, q, M)
    allowed = np.ones(q, bool)
    allowed[0] = False
    for kw in ({}, {"allowed": allowed}):
        x, h = plm.rbm_sample(g, c, W, q, 1000, burn_in=0, seed=21, hidden=True, **kw)
        want, margin, maxu = tw.start_states(g, 1000, 21, kw.get("allowed"), diagnostics=True)
        assert not h.any()
        # one draw per site with no sum before it: the visible delta without hidden units
        differs = x[0] != want
        bad = np.nonzero(differs.any(axis=1))[0]
        for ch in bad:
            i = int(np.argmax(differs[ch]))
            assert margin[ch, i] <= tw.delta_visible(0, q, maxu[ch, i]), (ch, i)
        assert len(bad) <= 10


# ---- 3. chain independence --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M", [(13, 21, 7), (70, 32, 65)])
def test_chain_independence(L, q, M, monkeypatch):
    g, c, W = cases.model(L, q, M)
    kw = dict(burn_in=2, n_snapshots=3, thin=2, seed=91, hidden=True)
    big, big_h = plm.rbm_sample(g, c, W, q, 300, **kw)
    small, small_h = plm.rbm_sample(g, c, W, q, 5, **kw)
    assert small.tobytes() == big[:, :5].tobytes() and small_h.tobytes() == big_h[:, :5].tobytes()
    tail, tail_h = plm.rbm_sample(g, c, W, q, 43, first_chain=257, **kw)
    assert tail.tobytes() == big[:, 257:].tobytes() and tail_h.tobytes() == big_h[:, 257:].tobytes()
    # cut by first_step: the first two snapshots, then the third from the second's states
    a, a_h = plm.rbm_sample(g, c, W, q, 300, burn_in=2, n_snapshots=2, thin=2, seed=91, hidden=True)
    b, b_h = plm.rbm_sample(g, c, W, q, 300, burn_in=2, n_snapshots=1, seed=91, hidden=True, start=a[-1], first_step=4)
    assert a.tobytes() == big[:2].tobytes() and b[0].tobytes() == big[2].tobytes() and b_h[0].tobytes() == big_h[2].tobytes()
    # every launch plan gives the same chains
    for waves in ("1", "2", "4", "8"):
        monkeypatch.setenv("PLM_RBM_WAVES", waves)
        again, again_h = plm.rbm_sample(g, c, W, q, 300, **kw)
        assert again.tobytes() == big.tobytes() and again_h.tobytes() == big_h.tobytes(), waves
    monkeypatch.setenv("PLM_RBM_WAVES", "3")
    with pytest.raises(plm._lib.PlmError) as e:
        plm.rbm_sample(g, c, W, q, 300, **kw)
    assert e.value.code == -1


# ---- 4. the distribution after a few steps ----------------------------------------------------------------------------

def test_distribution_after_a_few_steps():
    """The histogram of 20 000 chains after CHI_STEPS steps from the start rule against the exact mu0 T^B, at the
    false-alarm level 1e-6 of test_gpu_sampler.py."""
    L, q, M = cases.CHI_SHAPE
    g, c, W = cases.model(L, q, M)
    x = plm.rbm_sample(g, c, W, q, cases.CHI_CHAINS, burn_in=cases.CHI_STEPS, seed=cases.CHI_SEED)[0]
    mu = st.start_distribution(g.astype(np.float64)) @ np.linalg.matrix_power(tw.transition_matrix(g, c, W), cases.CHI_STEPS)
    counts = np.bincount(st.state_index(x, q), minlength=q ** L)
    chi, dof = st.chi2_counts(counts, mu, cases.CHI_CHAINS)
    bound = stats.chi2.isf(1e-6, dof)
    print("chi2 = %.1f on %d degrees of freedom (bound %.1f)" % (chi, dof, bound))
    assert chi < bound


# ---- 5, 6. the fit against the twin -----------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M,N,C,E,k,seed", cases.FIT_CASES)
def test_fit_against_the_twin(L, q, M, N, C, E, k, seed):
    msa, w, (g, c, W) = cases.fit_data(L, q, M, N, seed)
    want = tw.fit(msa, w, q, g, c, W, C, E, steps_per_epoch=k, seed=seed, **cases.FIT_OPTS)
    assert want["worst"] > 1.0, "the twin has a near tie: this seed cannot be compared byte for byte"
    got = plm.rbm_fit(msa, w, q, g, c, W, C, E, steps_per_epoch=k, seed=seed, **cases.FIT_OPTS)
    assert got["status"] == "maxiter" and got["epochs_done"] == E
    assert np.array_equal(got["chains"], want["chains"])
    d_err = max(np.abs(a - b).max() for a, b in zip(got["data"], want["data"]))
    m_err = max(np.abs(a - b).max() for a, b in zip(got["model"], want["model"]))
    x_got = tw.pack(got["g"], got["c"], got["W"])
    x_err = np.abs(x_got.astype(np.float64) - want["x"].astype(np.float64)).max()
    x_tol = 4 * E * 2.0 ** -24 * max(1.0, np.abs(want["x"]).max())
    t_err = np.abs(got["trace"] - want["trace"]).max()
    print("L=%d q=%d M=%d N=%d C=%d E=%d: |data| %.2e, |model| %.2e, |x| %.2e (tolerance %.2e), |trace| %.2e"
          % (L, q, M, N, C, E, d_err, m_err, x_err, x_tol, t_err))
    assert d_err <= 1e-12 and m_err <= 1e-12
    assert x_err <= x_tol
    assert got["trace"].shape == (E, 5) and t_err <= 1e-10
    for part in got["data"] + got["model"]:
        assert (part >= 0.0).all() and (part <= 1.0 + 1e-12).all()


@pytest.mark.parametrize("L,q,M,N,C,E,k,seed", cases.FIT_STAT_CASES)
def test_fit_statistics_of_many_chains(L, q, M, N, C, E, k, seed):
    """One epoch with many chains: the model statistics are those of the chains the call returns."""
    msa, w, (g, c, W) = cases.fit_data(L, q, M, N, seed)
    got = plm.rbm_fit(msa, w, q, g, c, W, C, 1, steps_per_epoch=k, seed=seed, **cases.FIT_OPTS)
    data = tw.statistics(msa.astype(np.int64), w.astype(np.float64), c, W, q, float(w.astype(np.float64).sum()))
    model = tw.statistics(got["chains"].astype(np.int64), np.ones(C), c, W, q, float(C))
    d_err = max(np.abs(a - b).max() for a, b in zip(got["data"], data))
    m_err = max(np.abs(a - b).max() for a, b in zip(got["model"], model))
    print("L=%d q=%d M=%d N=%d C=%d: |data| %.2e, |model| %.2e" % (L, q, M, N, C, d_err, m_err))
    assert d_err <= 1e-12 and m_err <= 1e-12
    # the chains themselves: k steps from the start rule, as plm_rbm_sample makes them
    assert np.array_equal(got["chains"], plm.rbm_sample(g, c, W, q, C, burn_in=k, seed=seed)[0])


# ---- 7. the fit, bytes ------------------------------------------------------------------------------------------------

def _bytes(r):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in
                    (r["g"], r["c"], r["W"]) + tuple(r["data"]) + tuple(r["model"]) + (r["chains"], r["trace"]))


@pytest.mark.parametrize("L,q,M,N,C", [(13, 21, 7, 257, 257), (70, 32, 65, 1000, 1000)])
def test_fit_is_reproducible_resumes_and_stops(L, q, M, N, C):
    msa, w, (g, c, W) = cases.fit_data(L, q, M, N, 55)
    kw = dict(steps_per_epoch=2, seed=56, lr_decay_after=2, **cases.FIT_OPTS)
    whole = plm.rbm_fit(msa, w, q, g, c, W, C, 4, **kw)
    assert _bytes(whole) == _bytes(plm.rbm_fit(msa, w, q, g, c, W, C, 4, **kw))
    a = plm.rbm_fit(msa, w, q, g, c, W, C, 2, **kw)
    b = plm.rbm_fit(msa, w, q, a["g"], a["c"], a["W"], C, 2, start=a["chains"], first_epoch=2, **kw)
    for key in ("g", "c", "W", "chains"):
        assert whole[key].tobytes() == b[key].tobytes(), key
    assert whole["trace"].tobytes() == np.concatenate([a["trace"], b["trace"]]).tobytes()
    assert _bytes(dict(whole, trace=b["trace"])) == _bytes(b)
    assert whole["trace"][3, 3] == cases.FIT_OPTS["lr"] * 2 / 4
    seen = []
    stopped = plm.rbm_fit(msa, w, q, g, c, W, C, 4, callback=lambda e, *row: seen.append((e, row)) or e == 1, **kw)
    one = plm.rbm_fit(msa, w, q, g, c, W, C, 1, **kw)
    assert stopped["status"] == "interrupted" and stopped["epochs_done"] == 1 and [e for e, _ in seen] == [0, 1]
    assert all(stopped[key].tobytes() == one[key].tobytes() for key in ("g", "c", "W"))
    assert stopped["trace"].shape == (2, 5) and np.array_equal(stopped["trace"][1], np.array(seen[1][1]))
    assert stopped["trace"].tobytes() == whole["trace"][:2].tobytes()


# ---- 8. the fit learns ------------------------------------------------------------------------------------------------

def test_fit_learns_the_planted_model():
    """The exact mean log-likelihood of data planted by an RBM, by enumeration: above its value at the start, which is
    the independent-site model."""
    L, q, M = cases.LEARN["shape"]
    data, _ = cases.planted_data()
    w = np.ones(len(data), np.float32)
    g0, c0, W0 = rbm.start_point(data, w, q, M)
    r = plm.rbm_fit(data, w, q, g0, c0, W0, cases.LEARN["C"], cases.LEARN["epochs"], steps_per_epoch=cases.LEARN["steps"],
                    lr=cases.LEARN["lr"], seed=cases.LEARN["seed"])
    ll0 = tw.mean_log_likelihood(data, w, g0, c0, W0)
    ll1 = tw.mean_log_likelihood(data, w, r["g"], r["c"], r["W"])
    print("mean log-likelihood: %.4f at the start, %.4f after %d epochs" % (ll0, ll1, r["epochs_done"]))
    assert r["status"] == "maxiter" and ll1 > ll0
    # the last column of the trace is the mean score, log P + log Z
    from types import SimpleNamespace
    assert abs(r["trace"][0, 4] - rbm.log_partition_exact(SimpleNamespace(g=g0, c=c0, W=W0)) - ll0) < 1e-9


# ---- 9. the Python layer ----------------------------------------------------------------------------------------------

def _namespace(L, q, M):
    from types import SimpleNamespace
    g, c, W = cases.model(L, q, M)
    return SimpleNamespace(g=g, c=c, W=W, L=L, q=q, M=M, alphabet=alignment_io.ALPHABET_PROTEIN[:q])


def test_single_mutant_matrix_and_features():
    L, q, M = 13, 21, 7
    m = _namespace(L, q, M)
    target = np.random.default_rng(8).integers(0, q, L).astype(np.int8)
    smm = rbm.single_mutant_matrix(m, target)
    assert smm.shape == (L, q) and (smm[np.arange(L), target] == 0.0).all()
    base = rbm.scores(m, target[None])[0]
    for i, a in ((0, 0), (5, 20), (12, 7)):
        row = target.copy()
        row[i] = a
        assert smm[i, a] == rbm.scores(m, row[None])[0] - base
    feats = rbm.hidden_inputs(m, target[None])
    assert feats.shape == (1, M) and np.abs(feats - tw.inputs(target[None], m.c, m.W)).max() < 1e-12
    x = rbm.sample_sequences(m, 64, burn_in=5, seed=3, exclude=m.alphabet[0], fix={2: 4, 7: 0})
    assert x.shape == (64, L) and (x[:, 2] == 4).all() and (x[:, 7] == 0).all() and (np.delete(x, 7, axis=1) > 0).all()


def test_command_line_fit_sample_score(tmp_path):
    run = lambda *a: subprocess.run([sys.executable, "-m", "evcouplings_amd.rbm"] + [str(v) for v in a], cwd=ROOT,
                                    capture_output=True, text=True, timeout=300)
    L, q = 12, 21
    alphabet = alignment_io.ALPHABET_PROTEIN[:q]
    rows = np.random.default_rng(6).integers(1, q, (50, L))
    src = tmp_path / "in.a2m"
    with open(src, "w") as f:
        for s, row in enumerate(rows):
            f.write(">seq%d/1-%d\n%s\n" % (s, L, "".join(alphabet[k] for k in row)))
    model, a2m, csv, npy = tmp_path / "m.npz", tmp_path / "s.a2m", tmp_path / "s.csv", tmp_path / "f.npy"
    r = run("fit", src, "-o", model, "--hidden", 5, "--epochs", 10, "--chains", 100)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("sample", model, "-n", 32, "-o", a2m, "--no-gaps", "--seed", 4, "--burn-in", 10)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("score", model, "--sequences", a2m, "-o", csv, "--features", npy)
    assert r.returncode == 0, r.stderr[-2000:]
    m = rbm.load(str(model))
    assert (m.L, m.q, m.M) == (L, q, 5)
    enc = alignment_io.encode_alignment(str(a2m), alphabet=m.alphabet)
    assert enc.msa.shape == (33, L) and (enc.msa[1:] > 0).all()
    lines = open(csv).read().split()
    assert lines[0] == "id,score" and len(lines) == 34
    got = np.array([float(line.split(",")[1]) for line in lines[1:]])
    assert np.array_equal(got, rbm.scores(m, enc.msa))
    feats = np.load(npy)
    assert feats.shape == (33, 5) and np.array_equal(feats, rbm.hidden_inputs(m, enc.msa))
