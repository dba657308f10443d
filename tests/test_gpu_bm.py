"""The Boltzmann-machine refinement on the MI355X (plm_bm_fit / plm.bm_fit, DESIGN_NEXT_ROWS.md section 9.7): every epoch
against the sampler and against numpy's counts (one epoch, no step, continuation: by induction all of them, bit for
bit), the purpose of the feature on an exactly enumerated model and on the golden fitted model, the stopping rules, the
error codes and the command line."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm_twin as bt  # noqa: E402
import sampler_plan_cases as cases  # noqa: E402
from evcouplings_amd import _lib, model_io, plm  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = os.path.join(HERE, "golden", "hip_fit_L24.model")
GOLDEN_NPZ = os.path.join(HERE, "golden", "hip_fit_L24.npz")
SHAPES = [(24, 21, 4096), (300, 21, 512), (45, 32, 2048), (17, 2, 4096), (64, 5, 1000)]
# the edges of k_bm_transpose / k_bm_count: chain counts that are no multiple of 4 (padding chains in the last word),
# fewer than 4 chains, 1251 chain words over five slices of 251 (the last holds 247), q > 22 (8 sites per workgroup),
# and one site (no pair, fij and J empty)
SHAPES += [(70, 5, 333), (33, 21, 1023), (17, 32, 1021), (6, 4, 5001), (3, 2, 1), (2, 3, 5), (1, 7, 1000)]


def _case(L, q, Cn):
    """Model, targets and start states of a shape; (24, 21, .) is the golden fitted model with its own frequencies."""
    rng = np.random.default_rng(3000 + L)
    if (L, q) == (24, 21):
        d = np.load(GOLDEN_NPZ)
        h, J, fi, fij = d["hi"], d["jij"], d["fi"], d["fij"]
    else:
        h = rng.normal(scale=1.0, size=(L, q)).astype(np.float32)
        J = rng.normal(scale=0.15, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
        fi = rng.dirichlet(np.ones(q), size=L).astype(np.float32)
        fij = (fi[:, None, :, None] * fi[None, :, None, :])[np.triu_indices(L, 1)].astype(np.float32)
    x0 = rng.integers(0, q, size=(Cn, L)).astype(np.int8)
    return h, J, fi, fij, x0


def _same(a, b, keys=("hi", "jij", "pi", "pij", "chains", "trace")):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("L,q,Cn", SHAPES)
def test_one_epoch_is_the_sampler_the_counts_and_the_step(L, q, Cn):
    h, J, fi, fij, x0 = _case(L, q, Cn)
    k, lr, lam_h, lam_j, seed = 2, 0.5, 0.01, 0.02, 77 + L
    res = plm.bm_fit(fi, fij, q, h, J, Cn, 1, sweeps_per_epoch=k, lr=lr, lambda_h=lam_h, lambda_j=lam_j, seed=seed,
                     start=x0)
    assert res["epochs_done"] == 1 and res["status"] == "maxiter" and res["trace"].shape == (1, 4)
    ref, _ = plm.sample(h, J, q, Cn, burn_in=k, seed=seed, start=x0, energies=False)
    assert np.array_equal(res["chains"], ref[0])
    ni, nij = bt.counts(res["chains"], q)
    assert np.array_equal(np.rint(res["pi"].astype(np.float64) * Cn).astype(np.int64), ni)
    assert np.array_equal(np.rint(res["pij"].astype(np.float64) * Cn).astype(np.int64), nij)
    for p, n in ((res["pi"], ni), (res["pij"], nij)):
        exact = n.astype(np.float64) / Cn
        assert (np.abs(p.astype(np.float64) - exact) <= np.spacing(exact.astype(np.float32))).all()
    bound = 2.0 ** -22 * max(1.0, float(np.abs(h).max()), float(np.abs(J).max(initial=0.0)))      # J is empty at L = 1
    for got, x, f, p, lam in ((res["hi"], h, fi, res["pi"], lam_h), (res["jij"], J, fij, res["pij"], lam_j)):
        x, f, p = (a.astype(np.float64) for a in (x, f, p))
        want = x + lr * ((f - p) - 2.0 * np.float64(np.float32(lam)) * x)
        err = float(np.abs(got.astype(np.float64) - want).max(initial=0.0))
        print("L=%d q=%d: max |x_out - step 6| = %.3g (bound %.3g)" % (L, q, err, bound))
        assert err <= bound
    row = bt.trace_row(fi, fij, res["pi"], res["pij"], lr)
    assert res["trace"][0, 0] == row[0] and res["trace"][0, 1] == row[1] and res["trace"][0, 3] == lr
    assert abs(res["trace"][0, 2] - row[2]) <= 1e-12 * max(row[2], 1.0)


@pytest.mark.parametrize("L,q,Cn", SHAPES)
def test_without_a_step_the_chains_persist_and_the_sweeps_are_numbered_on(L, q, Cn):
    h, J, fi, fij, x0 = _case(L, q, Cn)
    k, seed = 2, 5 + L
    res = plm.bm_fit(fi, fij, q, h, J, Cn, 3, sweeps_per_epoch=k, lr=0.0, lambda_h=0.01, lambda_j=0.02, seed=seed, start=x0)
    assert res["epochs_done"] == 3
    assert res["hi"].tobytes() == h.tobytes() and res["jij"].tobytes() == J.tobytes()
    ref, _ = plm.sample(h, J, q, Cn, burn_in=3 * k, seed=seed, start=x0, energies=False)
    assert np.array_equal(res["chains"], ref[0])


@pytest.mark.parametrize("L,q,Cn", SHAPES)
def test_continuation_and_repetition_are_bitwise(L, q, Cn):
    h, J, fi, fij, x0 = _case(L, q, Cn)
    kw = dict(sweeps_per_epoch=2, lr=0.5, lr_decay_after=1, lambda_h=0.01, lambda_j=0.02, seed=19 + L)
    whole = plm.bm_fit(fi, fij, q, h, J, Cn, 4, start=x0, **kw)
    again = plm.bm_fit(fi, fij, q, h, J, Cn, 4, start=x0, **kw)
    _same(whole, again)
    first = plm.bm_fit(fi, fij, q, h, J, Cn, 2, start=x0, **kw)
    second = plm.bm_fit(fi, fij, q, first["hi"], first["jij"], Cn, 2, start=first["chains"], first_epoch=2, **kw)
    _same(whole, second, keys=("hi", "jij", "pi", "pij", "chains"))
    assert whole["trace"].shape == (4, 4)
    assert whole["trace"][:2].tobytes() == first["trace"].tobytes()
    assert whole["trace"][2:].tobytes() == second["trace"].tobytes()
    assert whole["trace"][:, 3].tolist() == [float(np.float32(0.5 / (g + 1))) for g in range(4)]
    assert not np.array_equal(whole["hi"], first["hi"])


@pytest.mark.parametrize("L,q,Cn", [(6, 4, 5001), (33, 21, 1023)])
def test_every_chain_in_one_bin(L, q, Cn):
    """h_i(a_i) = 40 for one state per site, J = 0: every draw gives a_i (the other states weigh e^-40 against a u of
    at least 2^-25), so all C increments of a histogram land on one LDS bin, and at (6, 4, 5001) the five chain slices
    add to one global bin.  The targets are multiples of 2^-8 (fi) and 2^-16 (fij): every (f - p)^2 is a multiple of
    2^-32 and their sum stays below 2^18, exact in float64 in any order, so the whole trace row is the twin's.
    (At (33, 21, 1023) chain 722 meets, at site 32 of sweep 0, the one random word in 2^24 whose u rounds to 1 in
    float32: the draw that used to fall through to the last state, tests/test_gpu_sampler_plans.py.)"""
    rng = np.random.default_rng(4000 + L)
    a = rng.integers(0, q, size=L)
    h = np.zeros((L, q), np.float32)
    h[np.arange(L), a] = 40.0
    J = np.zeros((L * (L - 1) // 2, q, q), np.float32)
    fi = (np.rint(rng.dirichlet(np.ones(q), size=L) * 256) / 256).astype(np.float32)
    fij = (fi[:, None, :, None] * fi[None, :, None, :])[np.triu_indices(L, 1)].astype(np.float32)
    x0 = rng.integers(0, q, size=(Cn, L)).astype(np.int8)
    res = plm.bm_fit(fi, fij, q, h, J, Cn, 2, sweeps_per_epoch=1, lr=0.0, seed=9, start=x0)
    assert res["epochs_done"] == 2 and res["trace"].shape == (2, 4)
    assert np.array_equal(res["chains"], np.tile(a.astype(np.int8), (Cn, 1)))
    pi = np.zeros((L, q), np.float32)
    pi[np.arange(L), a] = 1.0
    iu, ju = np.triu_indices(L, 1)
    pij = np.zeros((len(iu), q, q), np.float32)
    pij[np.arange(len(iu)), a[iu], a[ju]] = 1.0
    assert res["pi"].tobytes() == pi.tobytes() and res["pij"].tobytes() == pij.tobytes()
    assert res["hi"].tobytes() == h.tobytes() and res["jij"].tobytes() == J.tobytes()
    row = bt.trace_row(fi, fij, pi, pij, 0.0)
    assert res["trace"][0].tolist() == row and res["trace"][1].tolist() == row, (res["trace"], row)
    # the same from the start rule
    res = plm.bm_fit(fi, fij, q, h, J, Cn, 1, sweeps_per_epoch=1, lr=0.0, seed=9)
    assert np.array_equal(res["chains"], np.tile(a.astype(np.int8), (Cn, 1)))
    assert res["pi"].tobytes() == pi.tobytes() and res["pij"].tobytes() == pij.tobytes()


def test_forced_tiles_give_the_chains_of_tile_64():
    """plm_bm_fit plans its sweeps where plm_sample does: under PLM_SAMPLE_TILE both run k_gibbs<6, 128> and <6, 256>,
    and the chains are those of the tile the planner picks for 300 chains."""
    L, q, Cn = 24, 21, 300
    h, J, fi, fij, x0 = _case(L, q, Cn)
    kw = dict(sweeps_per_epoch=2, lr=0.5, lambda_h=0.01, lambda_j=0.02, seed=41, start=x0)
    with cases.forced():
        assert plm.sample_plan(L, q, Cn)["tile"] == 64
        base = plm.bm_fit(fi, fij, q, h, J, Cn, 2, **kw)
        ref, _ = plm.sample(h, J, q, Cn, burn_in=2, seed=41, start=x0, energies=False)
    for tile in (128, 256):
        with cases.forced(tile=tile):
            p = plm.sample_plan(L, q, Cn)
            assert (p["direct"], p["tile"], p["n_workgroups"]) == (False, tile, -(-Cn // tile))
            one = plm.bm_fit(fi, fij, q, h, J, Cn, 1, **kw)
            smp, _ = plm.sample(h, J, q, Cn, burn_in=2, seed=41, start=x0, energies=False)
            two = plm.bm_fit(fi, fij, q, h, J, Cn, 2, **kw)
        assert np.array_equal(one["chains"], smp[0]) and np.array_equal(smp[0], ref[0])
        _same(two, base)


def test_start_rule_is_the_samplers():
    h, J, fi, fij, _ = _case(24, 21, 4096)
    res = plm.bm_fit(fi, fij, 21, h, J, 4096, 1, sweeps_per_epoch=3, lr=0.1, seed=31)
    ref, _ = plm.sample(h, J, 21, 4096, burn_in=3, seed=31, energies=False)
    assert np.array_equal(res["chains"], ref[0])


def test_exact_enumeration_the_refined_model_has_the_target_marginals():
    """L = 5, q = 4: the exact marginals of the fitted model, by enumeration, miss the targets by at most 0.1 x the error
    of the independent-site start point (0.0976).  The numpy twin reaches 0.00297 under this schedule."""
    case = bt.enumerable_case()
    err0 = bt.max_pair_error(case["h0"], case["J0"], case["fij"], 4)
    s = bt.ENUM_SCHEDULE
    res = plm.bm_fit(case["fi"], case["fij"], 4, case["h0"], case["J0"], s["n_chains"], s["n_epochs"],
                     sweeps_per_epoch=s["sweeps_per_epoch"], lr=s["lr"], lr_decay_after=s["lr_decay_after"],
                     lambda_h=s["lambda_h"], lambda_j=s["lambda_j"], seed=s["seed"])
    err = bt.max_pair_error(res["hi"], res["jij"], case["fij"], 4)
    print("exact max pair-marginal error: start point %.5f, refined %.5f" % (err0, err))
    assert res["epochs_done"] == 300 and res["status"] == "maxiter"
    assert err <= 0.1 * err0, (err, err0)


def test_golden_model_samples_reproduce_the_frequencies_after_refinement():
    """hip_fit_L24: fresh chains of the refined model against fresh chains of the pseudo-likelihood model.  The numpy twin
    gives rms(fij) 0.00134 against 0.00428 and max |fi| 0.0138 against 0.147."""
    d = np.load(GOLDEN_NPZ)
    h, J, fi, fij = d["hi"], d["jij"], d["fi"], d["fij"]
    q, Cn, n_eff = 21, 4096, float(d["n_eff"])
    start, _ = plm.sample(h, J, q, Cn, burn_in=100, seed=7, energies=False)
    res = plm.bm_fit(fi, fij, q, h, J, Cn, 120, sweeps_per_epoch=2, lr=0.5, lr_decay_after=60, lambda_h=0.01 / n_eff,
                     lambda_j=float(d["lambda_j"]) / n_eff, seed=8, start=start[0])
    assert res["epochs_done"] == 120

    def errors(hh, jj):
        x, _ = plm.sample(hh, jj, q, Cn, burn_in=100, seed=9, energies=False)
        pi, pij = bt.frequencies(x[0], q)
        return float(np.abs(fi - pi).max()), float(np.sqrt(((fij - pij).astype(np.float64) ** 2).mean()))

    max0, rms0 = errors(h, J)
    max1, rms1 = errors(res["hi"], res["jij"])
    print("fresh chains: max |fi - pi| %.5f -> %.5f, rms(fij - pij) %.6f -> %.6f" % (max0, max1, rms0, rms1))
    assert rms1 <= 0.5 * rms0, (rms1, rms0)
    assert max1 <= 0.3 * max0, (max1, max0)


def test_stopping_and_status():
    h, J, fi, fij, x0 = _case(24, 21, 4096)
    kw = dict(sweeps_per_epoch=2, lr=0.5, seed=3, start=x0)
    res = plm.bm_fit(fi, fij, 21, h, J, 4096, 5, tol=1.5, **kw)
    assert res["epochs_done"] == 0 and res["status"] == "converged" and res["trace"].shape == (1, 4)
    assert res["hi"].tobytes() == h.tobytes() and res["jij"].tobytes() == J.tobytes()
    seen = []
    res = plm.bm_fit(fi, fij, 21, h, J, 4096, 5, callback=lambda g, *row: seen.append((g,) + row) or g == 2, **kw)
    assert res["epochs_done"] == 2 and res["status"] == "interrupted" and [s[0] for s in seen] == [0, 1, 2]
    assert np.array_equal(np.array([s[1:] for s in seen]), res["trace"]) and res["trace"].shape == (3, 4)
    full = plm.bm_fit(fi, fij, 21, h, J, 4096, 2, **kw)
    assert full["hi"].tobytes() == res["hi"].tobytes() and full["jij"].tobytes() == res["jij"].tobytes()
    res = plm.bm_fit(fi, fij, 21, h, J, 4096, 3, first_epoch=4, callback=lambda g, *row: seen.append(g) or False, **kw)
    assert seen[-3:] == [4, 5, 6] and res["status"] == "maxiter"


def _raw(L, q, fi, fij, x, opts, res=None):
    res = res if res is not None else _lib.PlmBmResult()
    return _lib.load().plm_bm_fit(L, q, plm._ptr(fi), plm._ptr(fij), plm._ptr(x), C.byref(opts) if opts is not None else None,
                                  0, None, _lib.BM_EPOCH_CB(), None, C.byref(res))


def test_error_codes():
    lib = _lib.load()
    rng = np.random.default_rng(61)
    L, q, Cn = 6, 4, 8
    fi = np.full((L, q), 0.25, np.float32)
    fij = np.full((15, q, q), 1 / 16, np.float32)
    x = rng.normal(size=L * q + 15 * q * q).astype(np.float32)

    def opts(**kw):
        v = dict(n_chains=Cn, n_epochs=2, sweeps_per_epoch=1, first_epoch=0, lr=0.5, lr_decay_after=0, lambda_h=0.0,
                 lambda_j=0.0, tol=0.0, seed=1, start=None)
        v.update(kw)
        return _lib.PlmBmOpts(*[v[f] for f, _ in _lib.PlmBmOpts._fields_])

    assert _raw(L, q, fi, fij, x, opts()) == 0
    for kw, word in ((dict(lr=-1.0), b"lr"), (dict(lr=float("nan")), b"lr"), (dict(lambda_h=-1.0), b"lambda_h"),
                     (dict(lambda_j=float("inf")), b"lambda_j"), (dict(tol=-0.5), b"tol"), (dict(n_chains=0), b"n_chains"),
                     (dict(n_epochs=0), b"n_epochs"), (dict(sweeps_per_epoch=0), b"sweeps_per_epoch"),
                     (dict(first_epoch=-1), b"first_epoch")):
        assert _raw(L, q, fi, fij, x, opts(**kw)) == -1, kw
        assert word in lib.plm_last_error(), (kw, lib.plm_last_error())
    bad = np.full((Cn, L), q, np.int8)
    assert _raw(L, q, fi, fij, x, opts(start=plm._ptr(bad))) == -1 and b"start" in lib.plm_last_error()
    assert _raw(L, q, fi, fij, x, None) == -1 and b"options" in lib.plm_last_error()
    assert _raw(L, q, None, fij, x, opts()) == -1 and b"fi" in lib.plm_last_error()
    assert _raw(L, q, fi, None, x, opts()) == -1 and b"fij" in lib.plm_last_error()
    assert _raw(L, q, fi, fij, None, opts()) == -1 and b"x_start" in lib.plm_last_error()
    assert lib.plm_bm_fit(L, q, plm._ptr(fi), plm._ptr(fij), plm._ptr(x), C.byref(opts()), 0, None, _lib.BM_EPOCH_CB(),
                          None, None) == -1 and b"result" in lib.plm_last_error()
    assert _raw(0, q, fi, fij, x, opts()) == -1 and b"n_sites" in lib.plm_last_error()
    for qq in (1, 33):
        assert _raw(L, qq, fi, fij, x, opts()) == -4 and b"states" in lib.plm_last_error()
    # a model no device holds (L = 10 000, q = 32 is a 410 GB table): decided before any array is read
    dummy = np.zeros(16, np.float32)
    assert _raw(10000, 32, dummy, dummy, dummy, opts()) == -2 and b"GB" in lib.plm_last_error()
    with pytest.raises(_lib.PlmError) as err:
        plm.bm_fit(fi, fij, q, x[:L * q].reshape(L, q), x[L * q:], Cn, 2, start=bad)
    assert err.value.code == -1


def test_command_line(tmp_path, capsys):
    from evcouplings_amd import bm_refine
    out = str(tmp_path / "refined.model")
    assert bm_refine.main([GOLDEN_MODEL, "-o", out, "--epochs", "5", "--chains", "2048", "--sweeps", "2", "--lr", "0.4",
                           "--decay-after", "3", "--seed", "21"]) == 0
    printed = capsys.readouterr().out
    assert "epoch    0:" in printed and "epoch    4:" in printed
    m, r = model_io.read_model_file(GOLDEN_MODEL), model_io.read_model_file(out)
    a, b = open(GOLDEN_MODEL, "rb").read(), open(out, "rb").read()
    L, q = m["L"], m["q"]
    head = 40 + q + 4 * (m["n_valid"] + m["n_invalid"]) + 5 * L + 4 * L * q          # the header .. f_i
    pairs = 4 * L * (L - 1) // 2 * q * q
    assert len(a) == len(b) and a[:head] == b[:head]
    assert a[head + 4 * L * q:head + 4 * L * q + pairs] == b[head + 4 * L * q:head + 4 * L * q + pairs]      # f_ij
    res = plm.bm_fit(m["fi"], m["fij"], q, m["hi"], m["jij"], 2048, 5, sweeps_per_epoch=2, lr=0.4, lr_decay_after=3,
                     lambda_h=m["lambda_h"] / m["n_eff"], lambda_j=m["lambda_j"] / m["n_eff"], seed=21)
    assert r["hi"].tobytes() == res["hi"].tobytes() and r["jij"].tobytes() == res["jij"].tobytes()
    assert not np.array_equal(r["hi"], m["hi"])
