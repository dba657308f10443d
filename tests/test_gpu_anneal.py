"""Simulated annealing and greedy ascent on the MI355X (plm_anneal / plm.anneal, DESIGN_NEXT_ROWS.md section 9.13): every
launch plan against the sampler itself (an annealing step is a sweep of plm_sample, bit for bit), the greedy phase
against the numpy twin (tests/anneal_twin.py) bit for bit, annealing plus greedy against the twin draw for draw, chunk
geometry, masks, ties, the tracked gain against float64 energies, independence of the chain count and of how the
schedule is cut into launches, an enumerable model, a fitted model, and the error codes."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anneal_twin as an  # noqa: E402
import sampler_plan_cases as cases  # noqa: E402
import test_anneal_host as host  # noqa: E402
from test_gpu_sampler import _explained, _random_model  # noqa: E402
from evcouplings_amd import _lib, alignment_io, model_accel, plm, sample  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
CAP = 0.01                                # of the chains may differ from the twin at all
FIELDS = ("states", "gain", "best", "best_gain", "best_at", "last_move", "converged")
EVERY = FIELDS + ("energies", "best_energies")
L37 = cases.WIDTH_L
C_MAX = max(cases.TILES) + 37


def _same(a, b, what, fields=EVERY, rows=slice(None)):
    for k in fields:
        assert np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows]), (what, k)
    assert (a["steps_done"], a["status"]) == (b["steps_done"], b["status"]), what


def _ran(L, q, Cn, **want):
    p = plm.sample_plan(L, q, Cn)
    assert {k: p[k] for k in want} == want, (L, q, Cn, p)
    return p


def _tiled(tile, q, Cn):
    _ran(L37, q, Cn, direct=False, tile=tile, jc=cases.WIDTH_JC[tile][q], nv=(q + 3) // 4, n_workgroups=2)


def _width_model(q, j_scale=0.15):
    """The model, the uniform random starts and the seed of alphabet q at L = 37, for the largest chain count: a smaller
    tile takes the first chains (a chain does not depend on the others)."""
    rng = np.random.default_rng(9100 + q)
    h, J = _random_model(rng, L37, q, j_scale=j_scale)
    return h, J, rng.integers(0, q, size=(C_MAX, L37)).astype(np.int8), 4242 + q


# ---- 1. every plan draws as the sampler does -----------------------------------------------------------------------

@pytest.mark.parametrize("tile", cases.TILES)
def test_every_plan_draws_as_the_sampler(tile):
    """k_anneal<1 .. 8, tile> and k_anneal_direct<2 .. 32>: L = 37, two workgroups with 37 live lanes in the second.  No
    twin and no cap: a constant schedule is plm.sample at that beta, a varying one the chain of its one-step calls."""
    Cn = tile + 37
    for q in cases.WIDTH_QS:
        name = "tile %d q=%d" % (tile, q)
        h, J, x0, seed = _width_model(q)
        x0 = x0[:Cn]
        b = 0.7
        with cases.forced(tile=tile):
            _tiled(tile, q, Cn)
            const = plm.anneal(h, J, q, Cn, betas=[b, b, b], max_greedy=0, seed=seed, start=x0)
            sampled = plm.sample(h, J, q, Cn, burn_in=3, beta=b, seed=seed, start=x0)
            vary = plm.anneal(h, J, q, Cn, betas=[0.5, 1.0, 2.0], max_greedy=0, seed=seed, start=x0)
            x, gain = x0, np.zeros(Cn)
            for k, bk in enumerate((0.5, 1.0, 2.0)):
                one = plm.anneal(h, J, q, Cn, betas=[bk], max_greedy=0, seed=seed, start=x, first_sweep=k)
                x, gain = one["states"], gain + one["gain"]
            full = plm.anneal(h, J, q, Cn, betas=[0.5, 1.0, 2.0], max_greedy=8, seed=seed)
        assert np.array_equal(const["states"], sampled[0][0]), name
        assert np.array_equal(const["energies"], sampled[1][0]), name
        assert const["steps_done"] == 3 and const["status"] == "converged"
        assert not const["last_move"].any() and not const["converged"].any()         # no greedy phase ran
        assert np.array_equal(vary["states"], x), name
        assert np.abs(vary["gain"] - gain).max() <= 1e-9 * max(1.0, np.abs(gain).max()), name    # another order of sums
        with cases.forced(form="direct"):
            assert Cn % _ran(L37, q, Cn, direct=True)["tile"] != 0                   # a partial last workgroup
            direct = plm.anneal(h, J, q, Cn, betas=[0.5, 1.0, 2.0], max_greedy=8, seed=seed)
            direct_given = plm.anneal(h, J, q, Cn, betas=[0.5, 1.0, 2.0], max_greedy=0, seed=seed, start=x0)
        _same(full, direct, name + ": tiled against direct, start rule")
        _same(vary, direct_given, name + ": tiled against direct, given start")
        assert full["converged"].any() and (full["best_at"] > 0).any()


# ---- 2. the greedy phase against the twin, bit for bit ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _greedy_twin(q, G):
    h, J, x0, _ = _width_model(q, j_scale=0.5)
    return an.anneal(h, J, q, C_MAX, betas=np.zeros(0, np.float32), max_greedy=G, start=x0)


@pytest.mark.parametrize("form", cases.TILES + ("direct",))
def test_greedy_phase_equals_the_twin(form):
    """No expf is involved: states, gain, last_move and converged equal the twin's.  With 64 sweeps every chain converges,
    at different sweeps, so the early exit of a workgroup and the per-chain flags are exercised; with 3 some have not."""
    tile = 256 if form == "direct" else form
    Cn = tile + 37
    last = []
    for q in cases.WIDTH_QS:
        h, J, x0, _ = _width_model(q, j_scale=0.5)
        for G in (64, 3):
            twin = _greedy_twin(q, G)
            with (cases.forced(form="direct") if form == "direct" else cases.forced(tile=tile)):
                if form == "direct":
                    _ran(L37, q, Cn, direct=True)
                else:
                    _tiled(tile, q, Cn)
                gpu = plm.anneal(h, J, q, Cn, n_steps=0, max_greedy=G, start=x0[:Cn])
            for k in ("states", "gain", "last_move", "converged", "best", "best_gain"):
                assert np.array_equal(gpu[k], twin[k][:Cn]), (form, q, G, k)
            assert np.array_equal(gpu["best_at"], np.where(gpu["gain"] > 0, 1, 0))
            if G == 64:
                assert gpu["converged"].all()
                assert len(set(gpu["last_move"].tolist())) > 1                       # chains stop at different sweeps
                last.append((int(gpu["last_move"].min()), int(gpu["last_move"].max())))
            else:
                assert not gpu["converged"].all() and gpu["last_move"].max() == 3
    print("%s: (first, last) sweep with a last move per q: %s" % (form, last))


# ---- 3. annealing plus greedy against the twin --------------------------------------------------------------------

@pytest.mark.parametrize("tile", cases.TILES)
def test_every_plan_follows_the_twin(tile):
    """Three steps from the start rule, then greedy sweeps.  The states after every step (from calls with the prefixes of
    the schedule) follow the twin under the condition of the draw-for-draw tests; where they agree before the greedy
    phase, everything after agrees exactly."""
    Cn = tile + 37
    betas = np.array([0.4, 1.3, 0.8], np.float32)
    K = len(betas)
    differ = chains = 0
    for q in cases.WIDTH_QS:
        name = "tile %d q=%d" % (tile, q)
        h, J, _, seed = _width_model(q)
        twin = an.anneal(h, J, q, Cn, betas=betas, max_greedy=16, seed=seed, trace=True)
        with cases.forced(tile=tile):
            _tiled(tile, q, Cn)
            start = plm.sample(h, J, q, Cn, burn_in=0, seed=seed, energies=False)[0][0]
            prefix = [plm.anneal(h, J, q, Cn, betas=betas[:k], max_greedy=0, seed=seed) for k in range(1, K + 1)]
            full = plm.anneal(h, J, q, Cn, betas=betas, max_greedy=16, seed=seed)
        gpu = np.stack([start] + [r["states"] for r in prefix]).astype(np.int64)
        steps = twin["steps"]
        _explained(name, gpu, steps["states"], steps["margin"], steps["maxarg"], L37, q, cap=1.0)
        agree = (gpu == steps["states"]).all(axis=(0, 2))
        differ += int((~agree).sum())
        chains += Cn
        _same(full, twin, name, fields=FIELDS, rows=agree)
        assert np.abs(full["energies"][agree] - twin["energies"][agree]).max() < 1e-3
    print("tile %d: %d of %d chains differ from the twin" % (tile, differ, chains))
    assert differ <= CAP * chains, (differ, chains)


# ---- 4. chunk geometry --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", sorted(cases.CHUNK_QS))
def test_chunk_geometry(q):
    """Tile 64, every chunk length the planner accepts, at lengths below, at and above it: each run equals the direct form
    bit for bit.  One site has no couplings: greedy takes the first maximal field."""
    Cn = cases.CHUNK_C
    for L in cases.CHUNK_LS:
        h, J = _random_model(np.random.default_rng(8300 + 100 * q + L), L, q, j_scale=0.4)
        kw = dict(betas=[0.6, 1.7], max_greedy=8, seed=91 + L)
        with cases.forced(form="direct"):
            _ran(L, q, Cn, direct=True)
            direct = plm.anneal(h, J, q, Cn, **kw)
        if L == 1:
            assert (direct["states"][:, 0] == int(np.argmax(h[0]))).all() and direct["converged"].all()
            assert np.array_equal(direct["energies"][:, 0], h[0][direct["states"][:, 0]])
            assert not direct["energies"][:, 1].any()
        for jc in cases.CHUNK_QS[q]:
            with cases.forced(tile=64, jc=jc):
                _ran(L, q, Cn, direct=False, tile=64, jc=jc, n_workgroups=2)
                tiled = plm.anneal(h, J, q, Cn, **kw)
            _same(tiled, direct, "q=%d L=%d jc=%d" % (q, L, jc))


# ---- 5. masks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q", [(37, 21), (49, 3)])
def test_masks_and_local_optimality(L, q):
    rng = np.random.default_rng(500 + L)
    Cn = 256 + 37
    h, J = _random_model(rng, L, q, j_scale=0.3)
    fixed = np.zeros(L, bool)
    fixed[[0, 5, L - 1]] = True
    allowed = np.ones(q, bool)
    allowed[[0, q - 1]] = False
    x0 = rng.choice(np.nonzero(allowed)[0], size=(Cn, L)).astype(np.int8)
    x0[:, fixed] = 0                                          # a state that is not allowed, at fixed sites only
    r = plm.anneal(h, J, q, Cn, betas=[0.5, 1.0, 2.0], max_greedy=64, seed=3, start=x0, fixed=fixed, allowed=allowed)
    for k in ("states", "best"):
        assert np.array_equal(r[k][:, fixed], x0[:, fixed]), k
        assert allowed[r[k][:, ~fixed]].all(), k
    assert r["converged"].all()
    # no allowed state at a free site is better than the current one, up to the float32 rounding of one sum
    U = h[None].astype(np.float64) + plm.potentials(r["states"], q, h, J).astype(np.float64)      # [C, L, q]
    cur = np.take_along_axis(U, r["states"].astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    Jmax = np.zeros((L, L))
    iu, ju = np.triu_indices(L, 1)
    Jmax[iu, ju] = Jmax[ju, iu] = np.abs(J).max(axis=(1, 2))
    slack = (L - 1) * 2.0 ** -24 * (np.abs(h).max(axis=1) + Jmax.sum(axis=1))                     # [L]
    excess = (U[:, ~fixed][:, :, allowed] - cur[:, ~fixed][:, :, None]).max()
    print("L=%d q=%d: largest U[a] - U[x] at a converged chain %.3g (slack %.3g)" % (L, q, excess, slack.min()))
    assert (U[:, ~fixed][:, :, allowed] - cur[:, ~fixed][:, :, None] <= slack[~fixed][None, :, None]).all()
    # the start rule under a mask, with fixed sites: they keep what the rule drew
    s = plm.anneal(h, J, q, Cn, betas=[1.0], max_greedy=4, seed=3, fixed=fixed, allowed=allowed)
    drawn = plm.sample(h, J, q, Cn, burn_in=0, seed=3, allowed=allowed, energies=False)[0][0]
    assert np.array_equal(s["states"][:, fixed], drawn[:, fixed]) and allowed[s["states"]].all()


# ---- 6. ties ------------------------------------------------------------------------------------------------------

def test_ties_never_move():
    L, q, Cn = 11, 5, 70
    x0 = np.random.default_rng(2).integers(0, q, size=(Cn, L)).astype(np.int8)
    for form in ({"tile": 64}, {"form": "direct"}):
        with cases.forced(**form):
            flat = plm.greedy_ascent(np.zeros((L, q)), np.zeros((L * (L - 1) // 2, q, q)), q, x0, max_sweeps=5)
            assert np.array_equal(flat["states"], x0) and not flat["last_move"].any() and flat["converged"].all()
            assert not flat["gain"].any() and not flat["best_at"].any() and np.array_equal(flat["best"], x0)
            # integer-valued fields with two equal maxima at the states 1 and 3 (no couplings: every sum is exact)
            h = np.tile(np.array([0.0, 2.0, 1.0, 2.0, -1.0]), (L, 1))
            tie = plm.greedy_ascent(h, np.zeros((L * (L - 1) // 2, q, q)), q, x0, max_sweeps=5)
            want = np.where(x0 == 3, 3, 1)                    # the lower state when it improves, no move on equality
            assert np.array_equal(tie["states"], want)
            assert np.array_equal(tie["gain"], (h[0][want] - h[0][x0]).sum(axis=1))
            assert np.array_equal(tie["last_move"], ((x0 != 1) & (x0 != 3)).any(axis=1).astype(np.int32))
            assert tie["converged"].all()
            # the same with the tie between couplings: J_01(a, b) = 1 for a in {1, 3}, site 0 only is free
            J = np.zeros((L * (L - 1) // 2, q, q))
            J[0, 1, :] = J[0, 3, :] = 1.0
            hold = np.ones(L, bool)
            hold[0] = False
            tj = plm.greedy_ascent(np.zeros((L, q)), J, q, x0, max_sweeps=5, fixed=hold)
            assert np.array_equal(tj["states"][:, 0], want[:, 0]) and np.array_equal(tj["states"][:, 1:], x0[:, 1:])


# ---- 7. the tracked gain ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,K,j_scale", [(37, 21, 16, 0.15), (49, 3, 8, 0.5)])
def test_tracked_gain_against_float64(L, q, K, j_scale):
    """gain against H(final) - H(start) of plm.hamiltonians.  Every site update adds the difference of two float32 sums of
    L terms (the field and L - 1 couplings), each off by at most (L - 1) 2^-24 times the sum of its |terms|; a sweep
    updates every site once, so after K n annealing and at most G greedy sweeps the worst case is
    2 (K n + G)(L - 1) 2^-24 sum_i (max |h_i| + sum_{j != i} max |J_ij|)."""
    Cn, n, G = 1024 + 37, 1, 32
    rng = np.random.default_rng(300 + L)
    h, J = _random_model(rng, L, q, j_scale=j_scale)
    x0 = rng.integers(0, q, size=(Cn, L)).astype(np.int8)
    r = plm.anneal(h, J, q, Cn, n_steps=K, sweeps_per_step=n, max_greedy=G, seed=L, start=x0)
    H0 = plm.hamiltonians(x0, q, h, J)[:, 0]
    terms = np.abs(h).max(axis=1).sum() + 2.0 * np.abs(J).max(axis=(1, 2)).sum()
    bound = 2 * (K * n + G) * (L - 1) * 2.0 ** -24 * terms
    err = np.abs(r["gain"] - (r["energies"][:, 0] - H0)).max()
    err_best = np.abs(r["best_gain"] - (r["best_energies"][:, 0] - H0)).max()
    print("L=%d q=%d K=%d: max |gain - dH| = %.3g, at the best checkpoint %.3g (bound %.3g)" % (L, q, K, err, err_best, bound))
    assert err <= bound and err_best <= bound, (err, err_best, bound)
    assert np.array_equal(r["energies"], plm.hamiltonians(r["states"], q, h, J))
    assert np.array_equal(r["best_energies"], plm.hamiltonians(r["best"], q, h, J))
    assert (r["best_gain"] >= r["gain"]).all() and (r["best_gain"] >= 0).all()


# ---- 8. independence ----------------------------------------------------------------------------------------------

def test_independent_of_launches_and_chain_count_and_cancellation():
    L, q, K = 23, 21, 7
    h, J = _random_model(np.random.default_rng(41), L, q, j_scale=0.3)
    kw = dict(n_steps=K, sweeps_per_step=2, max_greedy=12, seed=17)
    whole = plm.anneal(h, J, q, 300, steps_per_launch=K, **kw)
    for spl in (1, 3, 0):
        _same(plm.anneal(h, J, q, 300, steps_per_launch=spl, **kw), whole, "steps_per_launch=%d" % spl)
    # the greedy phase is cut too (steps_per_launch x sweeps_per_step sweeps per launch): from random starts it is long
    x0 = np.random.default_rng(42).integers(0, q, size=(300, L)).astype(np.int8)
    climb = plm.anneal(h, J, q, 300, n_steps=0, max_greedy=40, start=x0)
    assert climb["last_move"].max() > 3 and climb["converged"].all()
    for spl in (1, 3):
        _same(plm.anneal(h, J, q, 300, n_steps=0, max_greedy=40, start=x0, steps_per_launch=spl), climb, "greedy, %d" % spl)
    small = plm.anneal(h, J, q, 64 + 37, **kw)
    for k in EVERY:
        assert np.array_equal(small[k], whole[k][:101]), k
    other = plm.anneal(h, J, q, 300, **dict(kw, seed=18))
    assert (other["states"] != whole["states"]).any(axis=1).mean() > 0.9
    # a callback is called between launches while work remains, and cancels
    seen = []
    done = plm.anneal(h, J, q, 300, steps_per_launch=3, callback=lambda d, t: seen.append((d, t)), **kw)
    assert seen == [(3, K), (6, K), (7, K)]
    _same(done, whole, "with a callback")
    stopped = plm.anneal(h, J, q, 300, steps_per_launch=3, callback=lambda d, t: d >= 6, **kw)
    assert stopped["status"] == "interrupted" and stopped["steps_done"] == 6
    assert not stopped["last_move"].any() and not stopped["converged"].any()
    six = plm.anneal(h, J, q, 300, betas=plm.annealing_schedule(K)[:6], sweeps_per_step=2, max_greedy=0, seed=17)
    for k in EVERY:                                            # the prefix schedule's state, but for the status
        assert np.array_equal(stopped[k], six[k]), k
    # a continuation from the states reached: the remaining step and the greedy phase
    rest = plm.anneal(h, J, q, 300, betas=plm.annealing_schedule(K)[6:], sweeps_per_step=2, max_greedy=12, seed=17,
                      start=stopped["states"], first_sweep=12)
    assert np.array_equal(rest["states"], whole["states"])

    class Boom(Exception):
        pass

    def raising(d, t):
        raise Boom()

    with pytest.raises(Boom):
        plm.anneal(h, J, q, 300, steps_per_launch=3, callback=raising, **kw)


# ---- 9. the enumerable model --------------------------------------------------------------------------------------

def test_finds_the_enumerated_optimum():
    """The three assertions of tests/test_anneal_host.py on the twin, here on the GPU."""
    for seed, (top_is_opt, annealed, greedy, sweeps) in zip(host.ENUM_SEEDS, host.optimisation_fractions(plm.anneal)):
        print("seed %d: annealed %.3f, greedy only %.3f, last greedy move in sweep %d" % (seed, annealed, greedy, sweeps))
        assert top_is_opt
        assert annealed >= host.ANNEALED_AT_LEAST
        assert greedy <= host.GREEDY_AT_MOST


# ---- 10. a fitted model -------------------------------------------------------------------------------------------

def test_fitted_model():
    model = sample.model_from_file(os.path.join(ROOT, "golden", "hip_fit_L24.model"))
    _, seqs = alignment_io.read_fasta_records(os.path.join(ROOT, "golden", "hip_fit_L24.a2m"))
    rows = [s.decode("ascii") for s in seqs]
    L, q = model.L, model.q
    optima, en, mutations, last_move, res = model_accel.local_optima(model, rows, info=True)
    code = {a: k for k, a in enumerate(model.alphabet)}
    x0 = np.array([[code[a] for a in r] for r in rows], np.int8)
    H0 = model_accel.hamiltonians(x0, model.J_ij, model.h_i)[:, 0]
    jij = model_accel._pairs_from_dense(model.J_ij)
    terms = np.abs(model.h_i).max(axis=1).sum() + 2.0 * np.abs(jij).max(axis=(1, 2)).sum()
    bound = 2 * 100 * (L - 1) * 2.0 ** -24 * terms
    assert res["converged"].all() and (res["gain"] >= 0).all()
    assert (en[:, 0] >= H0 - bound).all()
    assert np.array_equal(mutations, (res["states"] != x0).sum(axis=1)) and np.array_equal(last_move, res["last_move"])
    assert optima.shape == (len(rows), L) and ((mutations == 0) == (last_move == 0)).all()
    fixed = [int(model.index_list[3]), int(model.index_list[17])]
    gap = model.alphabet[0]
    best, ben, chains, info = model_accel.optimize_sequences(model, 512, n_steps=40, seed=5, exclude=gap, fixed=fixed,
                                                             top=20, info=True)
    assert 1 <= len(best) <= 20 and len(set("".join(r) for r in best)) == len(best)
    assert (np.diff(ben[:, 0]) <= 0).all() and chains.sum() <= 512 and (chains >= 1).all()
    assert not (best == gap).any()
    assert (best[:, 3] == model.target_seq[3]).all() and (best[:, 17] == model.target_seq[17]).all()
    assert ben[0, 0] == info["best_energies"][:, 0].max()
    print("hip_fit_L24: best designed H = %.3f (no gaps, two fixed positions), best natural H = %.3f, best local optimum "
          "of a natural sequence %.3f" % (ben[0, 0], H0.max(), en[:, 0].max()))


# ---- 11. error codes ----------------------------------------------------------------------------------------------

def test_error_codes():
    rng = np.random.default_rng(61)
    L, q, Cn = 6, 4, 8
    h, J = _random_model(rng, L, q)
    for kwargs in (dict(betas=[0.0]), dict(betas=[float("nan")]), dict(betas=[float("inf")]), dict(betas=[1.0, -2.0]),
                   dict(allowed=np.zeros(q, np.uint8)), dict(n_steps=0, max_greedy=0), dict(sweeps_per_step=0),
                   dict(start=np.full((Cn, L), 3), allowed=np.array([1, 1, 1, 0], np.uint8)),
                   dict(start=np.full((Cn, L), q)), dict(first_sweep=2 ** 32 - 2)):
        with pytest.raises(_lib.PlmError) as err:
            plm.anneal(h, J, q, Cn, **kwargs)
        assert err.value.code == -1, kwargs
    with pytest.raises(_lib.PlmError) as err:
        plm.anneal(np.zeros((3, 33)), np.zeros((3, 33, 33)), 33, Cn)
    assert err.value.code == -4
    # a state that is not allowed is accepted at a fixed site
    ok = plm.anneal(h, J, q, Cn, n_steps=2, start=np.full((Cn, L), 3), allowed=np.array([1, 1, 1, 0], np.uint8),
                    fixed=np.ones(L, np.uint8))
    assert (ok["states"] == 3).all() and not ok["gain"].any() and ok["converged"].all()
    # a model no device holds: L = 10 000, q = 32 is a 410 GB table.  The sizes are checked before any array is read
    dummy = np.zeros(16, np.float32)
    betas = np.ones(1, np.float32)
    opts = _lib.PlmAnnealOpts(1, 1, 1, 1, 0, 0, plm._ptr(betas), 0, None, None, None)
    res = _lib.PlmAnnealResult()
    lib = _lib.load()
    assert lib.plm_anneal(10000, 32, plm._ptr(dummy), C.byref(opts), 0, None, _lib.ANNEAL_CB(), None, C.byref(res)) == -2
    assert b"GB" in lib.plm_last_error()
    # every output pointer may be NULL
    opts = _lib.PlmAnnealOpts(Cn, 1, 1, 1, 0, 0, plm._ptr(betas), 0, None, None, None)
    x = np.concatenate([np.asarray(h, np.float32).ravel(), np.asarray(J, np.float32).ravel()])
    assert lib.plm_anneal(L, q, plm._ptr(x), C.byref(opts), 0, None, _lib.ANNEAL_CB(), None, C.byref(res)) == 0
    assert res.steps_done == 1 and res.status == _lib.STATUS_CONVERGED
