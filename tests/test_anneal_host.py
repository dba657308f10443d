"""Simulated annealing and greedy ascent (plm_anneal, DESIGN_NEXT_ROWS.md section 9.13) without a GPU: the binding, the
validation that comes before the device check, the schedule, and the numpy twin (tests/anneal_twin.py) on an enumerable
model, where the optimum is known, and against its own prefix runs for the checkpoints."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_twin as at  # noqa: E402
import anneal_twin as an  # noqa: E402
import sampler_twin as tw  # noqa: E402
from evcouplings_amd import _lib, plm  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
EINVAL, EDEVICE, EUNSUPPORTED = -1, -3, -4

# the enumerable model of the optimisation tests (also tests/test_gpu_anneal.py): 3^9 = 19 683 states
ENUM_MODEL = (9, 3, 1.5, 7)
ENUM_C, ENUM_G, ENUM_SEEDS = 512, 16, (1, 2, 3)
ENUM_BETAS = np.geomspace(0.1, 4, 48).astype(np.float32)
ANNEALED_AT_LEAST, GREEDY_AT_MOST = 0.5, 0.25


def enumerated_optimum(h, J, q):
    """(the state of largest H, that H, the gap to the second largest) by enumeration in float64."""
    L = h.shape[0]
    st = tw.all_states(L, q)
    H = tw.hamiltonians(st, np.asarray(h, np.float64), tw.dense(np.asarray(J, np.float64), L, q))[:, 0]
    order = np.argsort(-H, kind="stable")
    return st[order[0]], float(H[order[0]]), float(H[order[0]] - H[order[1]])


def optimisation_fractions(anneal, greedy_only=None):
    """For every seed of ENUM_SEEDS: (the best chain is the optimum, the fraction of chains that end in the optimum after
    annealing and greedy sweeps, the same fraction with greedy sweeps alone from the start rule, the last greedy sweep
    with a move after annealing).  anneal: plm.anneal or its twin."""
    L, q = ENUM_MODEL[:2]
    h, J = at.enumerable_model(*ENUM_MODEL)
    x_opt, H_opt, _ = enumerated_optimum(h, J, q)
    rows = []
    for seed in ENUM_SEEDS:
        full = anneal(h, J, q, ENUM_C, betas=ENUM_BETAS, sweeps_per_step=1, max_greedy=ENUM_G, seed=seed)
        only = anneal(h, J, q, ENUM_C, betas=np.zeros(0, np.float32), max_greedy=ENUM_G, seed=seed)
        top = int(np.argmax(full["best_energies"][:, 0]))
        rows.append((bool(np.array_equal(full["best"][top], x_opt)) and abs(full["best_energies"][top, 0] - H_opt) < 1e-4,
                     float((full["states"] == x_opt).all(axis=1).mean()), float((only["states"] == x_opt).all(axis=1).mean()),
                     int(full["last_move"].max())))
    return rows


# ---- binding and validation --------------------------------------------------------------------------------------

def test_binding_is_declared_and_matches_the_header_layout():
    assert "plm_anneal" in {name for name, _, _ in _lib.SYMBOLS}
    assert hasattr(_lib.load(), "plm_anneal")
    o, r = _lib.PlmAnnealOpts, _lib.PlmAnnealResult
    assert (o.n_chains.offset, o.n_steps.offset, o.sweeps_per_step.offset, o.max_greedy.offset, o.first_sweep.offset,
            o.steps_per_launch.offset, o.betas.offset, o.seed.offset, o.start.offset, o.fixed.offset, o.allowed.offset,
            C.sizeof(o)) == (0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64)
    assert (r.states.offset, r.gain.offset, r.best.offset, r.best_gain.offset, r.best_at.offset, r.last_move.offset,
            r.converged.offset, r.energies.offset, r.best_energies.offset, r.steps_done.offset, r.status.offset,
            C.sizeof(r)) == (0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80)
    text = open(os.path.join(os.path.dirname(ROOT), "include", "plm_hip.h")).read()
    assert "typedef int (*plm_anneal_cb)(" in text and "} plm_anneal_opts;" in text and "} plm_anneal_result;" in text


def _model(L=4, q=3):
    rng = np.random.default_rng(1)
    return rng.normal(size=(L, q)).astype(np.float32), rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)


def test_validation_comes_before_the_device():
    """Every PLM_EINVAL / PLM_EUNSUPPORTED of the scalars, the schedule and the mask, with or without a GPU."""
    lib = _lib.load()
    h, J = _model()
    x = np.concatenate([h.ravel(), J.ravel()])
    xp = x.ctypes.data_as(C.c_void_p)
    betas = np.array([0.5, 2.0, 1.0], np.float32)                           # any order: reheating is allowed

    def call(L=4, q=3, opts=True, res=True, betas=betas, allowed=None, **kw):
        b = None if betas is None else np.asarray(betas, np.float32)
        al = None if allowed is None else np.asarray(allowed, np.uint8)
        f = dict(n_chains=8, n_steps=0 if b is None else len(b), sweeps_per_step=1, max_greedy=4, first_sweep=0,
                 steps_per_launch=0, betas=plm._ptr(b), seed=0, start=None, fixed=None, allowed=plm._ptr(al))
        f.update(kw)
        o, r = _lib.PlmAnnealOpts(**f), _lib.PlmAnnealResult()
        return lib.plm_anneal(L, q, xp, C.byref(o) if opts else None, 0, None, _lib.ANNEAL_CB(), None,
                              C.byref(r) if res else None)

    assert call(opts=False) == EINVAL and call(res=False) == EINVAL
    assert call(L=0) == EINVAL and call(n_chains=0) == EINVAL
    assert call(n_steps=-1) == EINVAL and call(sweeps_per_step=0) == EINVAL
    assert call(max_greedy=-1) == EINVAL and call(steps_per_launch=-1) == EINVAL
    assert call(betas=None, max_greedy=0) == EINVAL                         # K == 0 with G == 0
    assert call(betas=None, n_steps=3) == EINVAL                            # NULL with K > 0
    assert call(n_steps=0) == EINVAL                                        # given with K == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(betas=[0.5, bad, 1.0]) == EINVAL, bad
    # first_sweep + K n: 2^32 - 1 and 2^32 are refused, 2^32 - 2 passes the check
    assert call(first_sweep=2 ** 32 - 4) == EINVAL                          # + 3 = 2^32 - 1
    assert call(first_sweep=0, sweeps_per_step=2 ** 31 - 1) == EINVAL       # 3 (2^31 - 1) > 2^32
    assert call(allowed=[0, 0, 0]) == EINVAL                                # no allowed state
    assert call(q=1) == EUNSUPPORTED and call(q=33) == EUNSUPPORTED
    if lib.plm_device_count() <= 0:                                         # a valid call: no CPU path
        assert call() == EDEVICE
        assert call(betas=None) == EDEVICE                                  # K == 0: greedy ascent alone
        assert call(first_sweep=2 ** 32 - 5) == EDEVICE
    # what the wrappers refuse themselves
    with pytest.raises(ValueError):
        plm.anneal(h, J[:-1], 3, 8)
    with pytest.raises(ValueError):
        plm.anneal(h, J, 3, 8, start=np.zeros((7, 4), np.int8))
    with pytest.raises(ValueError):
        plm.anneal(h, J, 3, 8, fixed=np.zeros(3))
    with pytest.raises(ValueError):
        plm.anneal(h, J, 3, 8, allowed=np.ones(4))
    with pytest.raises(ValueError):
        plm.greedy_ascent(h, J, 3, np.zeros(4, np.int8))
    with pytest.raises(_lib.PlmError) as err:
        plm.anneal(h, J, 3, 8, n_steps=0, max_greedy=0)
    assert err.value.code == EINVAL


def test_annealing_schedule():
    geo = plm.annealing_schedule(5, 0.25, 4.0)
    assert geo.dtype == np.float32 and np.array_equal(geo, np.array([0.25, 0.5, 1, 2, 4], np.float32))
    lin = plm.annealing_schedule(5, 1.0, 3.0, kind="linear")
    assert np.array_equal(lin, np.array([1, 1.5, 2, 2.5, 3], np.float32))
    assert np.array_equal(plm.annealing_schedule(1), np.array([4.0], np.float32))
    assert plm.annealing_schedule(0).shape == (0,) and plm.annealing_schedule(0).dtype == np.float32
    # the rounding: every value in float64, one rounding to float32
    K = 48
    b = plm.annealing_schedule(K)
    want = np.array([0.1 * (4.0 / 0.1) ** (k / (K - 1)) for k in range(K)], np.float64)
    assert b.dtype == np.float32 and np.array_equal(b, want.astype(np.float32))
    assert b[0] == np.float32(0.1) and abs(float(b[-1]) - 4.0) <= 2.0 ** -22 and (np.diff(b) > 0).all()
    assert np.abs(b.astype(np.float64) - np.geomspace(0.1, 4.0, K)).max() <= 2.0 ** -22
    for bad in (dict(n_steps=-1), dict(n_steps=3, beta_min=0.0), dict(n_steps=3, beta_min=2.0, beta_max=1.0),
                dict(n_steps=3, beta_max=float("inf")), dict(n_steps=3, kind="other")):
        with pytest.raises(ValueError):
            plm.annealing_schedule(**bad)


# ---- the twin ----------------------------------------------------------------------------------------------------

def test_the_twin_finds_the_enumerated_optimum():
    """ais_twin.enumerable_model(9, 3, 1.5, 7): H_max = 23.203, the next state 0.987 below.  A float64-U prototype of the
    same rules gave 0.60 of 512 chains in the optimum after 48 steps and 16 greedy sweeps, 0.15 - 0.18 with greedy
    sweeps alone, every greedy phase after annealing over within 2 sweeps.  The committed float32 twin gives
    0.605 / 0.600 / 0.602 annealed and 0.145 / 0.184 / 0.172 greedy-only for the seeds 1, 2, 3 (last greedy move after
    annealing in sweep 1, 1, 2): the prototype's figures, so the thresholds 0.5 and 0.25 stand; each is more than 4
    binomial standard deviations (0.022 at p = 0.6, 0.017 at p = 0.18, C = 512) from what is measured at two of the seeds
    and 3.9 from the 0.184 of seed 2.  (Counted over `best` instead of the final states, 0.742 / 0.717 / 0.719.)"""
    h, J = at.enumerable_model(*ENUM_MODEL)
    _, H_opt, gap = enumerated_optimum(h, J, ENUM_MODEL[1])
    assert abs(H_opt - 23.203) < 1e-3 and abs(gap - 0.987) < 1e-3
    for seed, (top_is_opt, annealed, greedy, sweeps) in zip(ENUM_SEEDS, optimisation_fractions(an.anneal)):
        print("seed %d: annealed %.3f, greedy only %.3f, last greedy move in sweep %d" % (seed, annealed, greedy, sweeps))
        assert top_is_opt
        assert annealed >= ANNEALED_AT_LEAST
        assert greedy <= GREEDY_AT_MOST


def test_checkpoints_against_prefix_runs():
    """best_gain is the maximum of the gain over the checkpoints 0 .. K + 1 and best_at its first index: the gain after
    K' steps comes from the twin's own runs of the prefixes betas[:K'] without greedy sweeps."""
    L, q, Cn, G, seed = 7, 4, 96, 5, 17
    h, J = at.enumerable_model(L, q, 0.8, 23)
    betas = np.array([0.3, 2.5, 0.2, 1.0, 3.0, 0.4], np.float32)            # reheats: the best is often not the last
    K = len(betas)
    prefix = [an.anneal(h, J, q, Cn, betas=betas[:k], max_greedy=0, seed=seed) for k in range(K + 1)]
    full = an.anneal(h, J, q, Cn, betas=betas, max_greedy=G, seed=seed)
    gains = np.stack([p["gain"] for p in prefix] + [full["gain"]])          # [K + 2][C]
    states = np.stack([p["states"] for p in prefix] + [full["states"]])
    assert np.array_equal(gains[0], np.zeros(Cn))
    assert np.array_equal(full["best_gain"], gains.max(axis=0))
    first = gains.argmax(axis=0)                                            # argmax returns the first maximum
    assert np.array_equal(full["best_at"], first)
    assert np.array_equal(full["best"], states[first, np.arange(Cn)])
    assert len(set(first.tolist())) > 3                                     # several different checkpoints are hit
    # every prefix is itself consistent, and the tracked gain is H(final) - H(start) up to the float32 sums
    for k, p in enumerate(prefix):
        assert np.array_equal(p["best_gain"], gains[:k + 1].max(axis=0))
        assert np.array_equal(p["best_at"], gains[:k + 1].argmax(axis=0))
    dH = full["energies"][:, 0] - prefix[0]["energies"][:, 0]
    assert np.abs(full["gain"] - dH).max() < 1e-4
    assert np.abs(full["best_gain"] - (full["best_energies"][:, 0] - prefix[0]["energies"][:, 0])).max() < 1e-4


def test_the_twin_greedy_rule_on_ties():
    """Two equal maxima: the lower state is taken when it improves, no move on equality; masks are respected."""
    U = np.array([[1, 3, 3, 0], [3, 1, 3, 0], [0, 3, 1, 3], [2, 2, 2, 2]], np.float32)
    ok = np.ones(4, bool)
    a, moved = an.greedy_update(U, np.array([0, 2, 3, 3]), ok)
    assert a.tolist() == [1, 2, 3, 3] and moved.tolist() == [True, False, False, False]
    a, moved = an.greedy_update(U, np.array([0, 1, 2, 3]), np.array([1, 0, 1, 1], bool))
    assert a.tolist() == [2, 0, 3, 3] and moved.tolist() == [True, True, True, False]
