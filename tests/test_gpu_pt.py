"""Parallel tempering on the MI355X (plm_pt / plm.parallel_tempering, DESIGN_NEXT_ROWS.md section 9.9): one rung against
the sweep of plm_ais bit for bit; every launch plan against the numpy twin (tests/pt_twin.py) draw for draw and decision
for decision, and the direct form bit for bit; the chunk geometry; the bookkeeping of the exchanges where every one is
accepted; independence of the ladder count and of the plan, continuation and cancellation; stationary rungs of enumerable
models; a fitted model against annealed importance sampling."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_twin as at  # noqa: E402
import pt_twin as pt  # noqa: E402
import sampler_plan_cases as cases  # noqa: E402
from test_gpu_sampler import _random_model  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
CAP = 0.01                                # of the ladders may leave the twin at all
DECISION = 1e-12                          # |u - exp(Delta)| below which an exchange decision may differ
FIELDS = ("samples", "e_j", "energies", "accepts", "attempts")
PLAN_LADDERS = {64: 34, 128: 55, 256: 98}  # x 3 rungs: a ladder across the end of the first workgroup, a partial second


def _same(a, b, what):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), (what, k, np.argwhere(a[k] != b[k])[:5])
    for k, (x, y) in enumerate(zip(a["walkers"], b["walkers"])):
        assert np.array_equal(x, y), (what, "walkers[%d]" % k, np.argwhere(x != y)[:5])
    assert a["rounds_done"] == b["rounds_done"] and a["status"] == b["status"]


def _ran(L, q, Cn, **want):
    p = plm.sample_plan(L, q, Cn)
    assert {k: p[k] for k in want} == want, (L, q, Cn, p)
    return p


def _slots(rungs, R):
    """slot_of_rung [C, R] from the walkers' rungs."""
    ros = np.asarray(rungs).reshape(-1, R)
    assert (np.sort(ros, axis=1) == np.arange(R)[None, :]).all()
    return np.argsort(ros, axis=1)


def _check_rung_order(res, R):
    """The last snapshot of an all_rungs call holds the final walkers gathered through the final maps."""
    x, rungs, e = res["walkers"]
    Cn = len(rungs) // R
    w = (np.arange(Cn)[:, None] * R + _slots(rungs, R)).ravel()
    assert np.array_equal(res["samples"][-1].reshape(Cn * R, -1), x[w])
    assert np.array_equal(res["e_j"][-1].ravel(), e[w])


@pytest.mark.parametrize("L,q,Cn,b", [(37, 21, 101, 0.8), (17, 32, 61, 1.3)])
def test_one_rung_is_the_ais_sweep(L, q, Cn, b):
    """R = 1, one round of two sweeps: the states and the tracked energy of plm_ais with the schedule (0, b)."""
    h, J = _random_model(np.random.default_rng(9100 + L), L, q)
    ais = plm.log_partition(h, J, q, n_chains=Cn, betas=[0.0, b], sweeps_per_temp=2, seed=L)
    one = plm.parallel_tempering(h, J, q, Cn, [b], burn_in=1, sweeps_per_round=2, seed=L)
    assert np.array_equal(one["samples"][0], ais["states"]) and np.array_equal(one["e_j"][0], ais["e_j"])
    assert np.array_equal(one["walkers"][0], ais["states"]) and np.array_equal(one["walkers"][2], ais["e_j"])
    assert not one["walkers"][1].any() and one["accepts"].size == 0 and one["rounds_done"] == 1


def _left_out(name, gpu, twin, L, q, R):
    """gpu: per round (the start first) the walkers triple of the prefix call; twin: the trace of pt.pt.  Returns alive
    [rounds + 1, C]: whether ladder l still follows the twin after round s.  A ladder may leave only by a draw inside the
    margin of section 9.6 or by an exchange decision with |u - exp(Delta)| <= DECISION; every other difference fails."""
    S = len(gpu)
    Cn = twin["rungs"].shape[1]
    alive = np.ones((S, Cn), bool)
    unexplained = []
    for s in range(S):
        if s:
            alive[s] = alive[s - 1]
        gx = gpu[s][0].astype(np.int64).reshape(Cn, R, L)
        tx = twin["walkers"][s].reshape(Cn, R, L)
        gsor, tsor = _slots(gpu[s][1], R), np.argsort(twin["rungs"][s], axis=1)
        for l in np.nonzero(alive[s])[0]:
            bad_x = (gx[l] != tx[l]).any(axis=1)
            if bad_x.any():
                alive[s, l] = False
                for k in np.nonzero(bad_x)[0]:
                    w, i = l * R + k, int(np.argmax(gx[l, k] != tx[l, k]))
                    delta = 2.0 ** -24 * (L + 4 * q) * (1.0 + twin["maxarg"][s, w, i])
                    if not twin["margin"][s, w, i] <= delta:
                        unexplained.append(("draw", int(l), s, int(k), i, float(twin["margin"][s, w, i]), float(delta)))
            elif (gsor[l] != tsor[l]).any():
                alive[s, l] = False
                for r in range((s - 1) % 2, R - 1, 2):                  # round s - 1 of the call: parity of g = s - 1
                    if (gsor[l, r:r + 2] != tsor[l, r:r + 2]).any() and not twin["decision"][s - 1, l, r] <= DECISION:
                        unexplained.append(("decision", int(l), s, r, float(twin["decision"][s - 1, l, r])))
    print("%s: %d of %d ladders leave the twin, %d unexplained" % (name, int((~alive[-1]).sum()), Cn, len(unexplained)))
    assert not unexplained, unexplained[:5]
    return alive


@pytest.mark.parametrize("tile", cases.TILES)
def test_every_plan_follows_the_twin(tile):
    """k_pt<1 .. 8, tile> and k_pt_direct<2 .. 32>: L = 37, three rungs, four rounds of one sweep; the walkers after every
    round come from calls that run a prefix of the rounds."""
    L, R, rounds = cases.WIDTH_L, 3, 4
    betas = np.array([0.0, 0.6, 1.3], np.float32)
    Cn = PLAN_LADDERS[tile]
    assert Cn * R > tile and tile % R != 0 and (Cn * R) % tile != 0
    left = ladders = 0
    for q in cases.WIDTH_QS:
        name = "tile %d q=%d" % (tile, q)
        h, J = _random_model(np.random.default_rng(7300 + q + tile), L, q)
        seed = 6161 + q
        kw = dict(sweeps_per_round=1, seed=seed, all_rungs=True)
        twin = pt.pt(h, J, q, Cn, betas, rounds, seed=seed, trace=True)
        with cases.forced(tile=tile):
            _ran(L, q, Cn * R, direct=False, tile=tile, jc=cases.WIDTH_JC[tile][q], nv=(q + 3) // 4, n_workgroups=2)
            tiled = [plm.parallel_tempering(h, J, q, Cn, betas, burn_in=k, **kw) for k in range(rounds + 1)]
            series = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=0, n_snapshots=rounds + 1, thin=1, **kw)
        with cases.forced(form="direct"):
            assert (Cn * R) % _ran(L, q, Cn * R, direct=True)["tile"] != 0          # a partial last workgroup
            direct = [plm.parallel_tempering(h, J, q, Cn, betas, burn_in=k, **kw) for k in range(rounds + 1)]
        for k in range(rounds + 1):
            _same(tiled[k], direct[k], "%s, %d rounds: tiled against direct" % (name, k))
            assert tiled[k]["rounds_done"] == k and tiled[k]["status"] == "converged"
            _check_rung_order(tiled[k], R)
            assert np.array_equal(series["samples"][k], tiled[k]["samples"][0]), (name, k)
            assert np.array_equal(series["e_j"][k], tiled[k]["e_j"][0]), (name, k)
        _same(dict(series, samples=0, e_j=0, energies=0), dict(tiled[-1], samples=0, e_j=0, energies=0), name)
        alive = _left_out(name, [r["walkers"] for r in tiled], twin["trace"], L, q, R)
        left += int((~alive[-1]).sum())
        ladders += Cn
        accepted = np.zeros((Cn, R - 1), np.int64)                     # of the GPU, read off its maps round by round
        for k in range(rounds + 1):
            ok = np.repeat(alive[k], R)
            assert np.array_equal(tiled[k]["walkers"][2][ok], twin["trace"]["e_j"][k][ok]), (name, k, "e_j")
            assert np.array_equal(tiled[k]["walkers"][1].reshape(Cn, R)[alive[k]], twin["trace"]["rungs"][k][alive[k]])
            if k:
                before, after = _slots(tiled[k - 1]["walkers"][1], R), _slots(tiled[k]["walkers"][1], R)
                moved = before[:, :-1] != after[:, :-1]
                moved[:, 1 - (k - 1) % 2::2] = False                     # only the pairs of this round's parity start there
                accepted += moved
                assert np.array_equal(moved[alive[k]], twin["trace"]["accepted"][k - 1][alive[k]]), (name, k, "accepts")
                assert np.array_equal(tiled[k]["accepts"], accepted.sum(axis=0)), (name, k)
                assert np.array_equal(tiled[k]["attempts"], Cn * np.array([(k + 1) // 2, k // 2])), (name, k)
        if alive[-1].all():
            assert np.array_equal(tiled[-1]["accepts"], twin["accepts"]), name
    print("tile %d: %d of %d ladders left out" % (tile, left, ladders))
    assert left <= CAP * ladders, (left, ladders)


@pytest.mark.parametrize("q", sorted(cases.CHUNK_QS))
def test_chunk_geometry(q):
    """Tile 64, every chunk length the planner accepts, at lengths below, at and above it: each run equals the direct form
    bit for bit.  One site has no couplings: every E is 0, so every Delta is 0 and every exchange is accepted."""
    Cn, R, rounds = 51, 2, 3
    betas = [0.4, 1.1]
    for L in cases.CHUNK_LS:
        h, J = _random_model(np.random.default_rng(8300 + 100 * q + L), L, q)
        kw = dict(burn_in=rounds, seed=177 + L, all_rungs=True)
        with cases.forced(form="direct"):
            _ran(L, q, Cn * R, direct=True)
            direct = plm.parallel_tempering(h, J, q, Cn, betas, **kw)
        _check_rung_order(direct, R)
        if L == 1:
            assert not direct["e_j"].any() and not direct["walkers"][2].any()
            assert np.array_equal(direct["accepts"], direct["attempts"]) and direct["attempts"][0] == 2 * Cn
        else:
            assert direct["e_j"].std() > 0 and 0 < direct["accepts"][0] <= direct["attempts"][0]
        for jc in cases.CHUNK_QS[q]:
            with cases.forced(tile=64, jc=jc):
                _ran(L, q, Cn * R, direct=False, tile=64, jc=jc, n_workgroups=2)
                tiled = plm.parallel_tempering(h, J, q, Cn, betas, **kw)
            _same(tiled, direct, "q=%d L=%d jc=%d" % (q, L, jc))


@pytest.mark.parametrize("R", [2, 3, 4, 5])
def test_exchange_bookkeeping_where_every_exchange_is_accepted(R):
    """All temperatures equal: Delta = 0 and every attempt is accepted, so the counts are known, the rung order after
    every round is that of the odd-even transposition network, and, since states never move, walker w is the one-rung
    chain with chain index w."""
    L, q, Cn, rounds = 9, 21, 33, 7
    h, J = _random_model(np.random.default_rng(5200 + R), L, q)
    kw = dict(seed=40 + R, all_rungs=True)
    order = list(range(R))
    for k in range(1, rounds + 1):
        r = plm.parallel_tempering(h, J, q, Cn, [0.7] * R, burn_in=k, **kw)
        g = k - 1
        for j in range(g % 2, R - 1, 2):
            order[j], order[j + 1] = order[j + 1], order[j]
        assert (_slots(r["walkers"][1], R) == np.array(order)[None, :]).all(), (R, k)
        want = Cn * np.array([(k + 1 - (j % 2)) // 2 for j in range(R - 1)])
        assert np.array_equal(r["accepts"], want) and np.array_equal(r["attempts"], want), (R, k, r["accepts"], want)
        _check_rung_order(r, R)
    alone = plm.parallel_tempering(h, J, q, Cn * R, [0.7], burn_in=rounds, **kw)
    assert np.array_equal(alone["walkers"][0], r["walkers"][0]) and np.array_equal(alone["walkers"][2], r["walkers"][2])
    assert np.array_equal(alone["samples"][0, :, 0], r["walkers"][0])


def test_independence_and_continuation_and_cancellation():
    L, q, R, Cn = 24, 21, 4, 300
    h, J = _random_model(np.random.default_rng(43), L, q)
    betas = plm.tempering_ladder(R, 1.2)
    kw = dict(sweeps_per_round=2, seed=19, all_rungs=True)
    whole = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=4, n_snapshots=3, thin=1, **kw)
    assert whole["rounds_done"] == 6 and whole["status"] == "converged"
    assert np.array_equal(whole["attempts"], Cn * np.array([3, 3, 3]))
    assert (whole["accepts"] > 0).all() and (whole["accepts"] < whole["attempts"]).all()
    # the plan does not matter
    for plan in (dict(tile=64), dict(tile=128), dict(tile=256), dict(form="direct")):
        with cases.forced(**plan):
            _ran(L, q, Cn * R, direct="form" in plan, **({"tile": plan["tile"]} if "tile" in plan else {}))
            _same(plm.parallel_tempering(h, J, q, Cn, betas, burn_in=4, n_snapshots=3, thin=1, **kw), whole, str(plan))
    # nor the number of ladders
    small = plm.parallel_tempering(h, J, q, 101, betas, burn_in=4, n_snapshots=3, thin=1, **kw)
    for k in ("samples", "e_j", "energies"):
        assert np.array_equal(small[k], whole[k][:, :101]), k
    for x, y in zip(small["walkers"], whole["walkers"]):
        assert np.array_equal(x, y[:101 * R])
    other = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=4, n_snapshots=3, thin=1, sweeps_per_round=2, seed=20,
                                   all_rungs=True)
    assert (other["e_j"] != whole["e_j"]).mean() > 0.9
    # 3 + 3 rounds through the walkers and first_round, on another plan than the first half
    a = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=3, **kw)
    with cases.forced(tile=64):
        b = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=1, n_snapshots=3, thin=1, start=a["walkers"], first_round=3,
                                   **kw)
    for k in ("samples", "e_j", "energies"):
        assert np.array_equal(b[k], whole[k]), k
    for x, y in zip(b["walkers"], whole["walkers"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["accepts"] + b["accepts"], whole["accepts"])
    assert np.array_equal(a["attempts"], Cn * np.array([2, 1, 2])) and np.array_equal(b["attempts"], Cn * np.array([1, 2, 1]))
    # without the energies they are measured anew from the states: the same to rounding, and the states stand
    m = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=0, start=a["walkers"][:2], first_round=3, **kw)
    assert np.array_equal(m["walkers"][0], a["walkers"][0]) and np.array_equal(m["walkers"][1], a["walkers"][1])
    assert np.abs(m["walkers"][2] - a["walkers"][2]).max() < 1e-3
    assert np.allclose(m["walkers"][2], plm.hamiltonians(a["walkers"][0], q, h, J)[:, 1], rtol=0, atol=1e-3)
    # a callback is called between rounds, and cancels
    seen = []
    done = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=4, n_snapshots=3, thin=1,
                                  callback=lambda d, t: seen.append((d, t)), **kw)
    assert seen == [(k, 6) for k in range(1, 6)]
    _same(done, whole, "with a callback")
    stop = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=4, n_snapshots=3, thin=1, callback=lambda d, t: d >= 2, **kw)
    two = plm.parallel_tempering(h, J, q, Cn, betas, burn_in=2, **kw)
    assert stop["status"] == "interrupted" and stop["rounds_done"] == 2 and not stop["samples"].any()
    for x, y in zip(stop["walkers"], two["walkers"]):
        assert np.array_equal(x, y)
    assert np.array_equal(stop["accepts"], two["accepts"]) and np.array_equal(stop["attempts"], two["attempts"])
    with pytest.raises(ZeroDivisionError):
        plm.parallel_tempering(h, J, q, Cn, betas, burn_in=4, callback=lambda d, t: 1 // 0, **kw)


@pytest.mark.parametrize("L,q,j_scale,model_seed", at.ENUMERABLE)
def test_stationary_rungs_against_enumeration(L, q, j_scale, model_seed):
    """The models, starts and bound of tests/test_pt_host.py: every walker starts from an exact draw of its rung, so after
    12 rounds the C rows of every rung are C independent exact draws."""
    h, J = at.enumerable_model(L, q, j_scale, model_seed)
    betas, Cn = pt.STATIONARY_BETAS, pt.STATIONARY_C
    p = pt.rung_distributions(h, J, q, betas)
    x0 = pt.stationary_start(h, J, q, betas, Cn, 100 + L)
    res = plm.log_partition_tempered(h, J, q, Cn, betas, burn_in=pt.STATIONARY_ROUNDS, seed=3, start=(x0,))
    ratios = [chi / stats.chi2.isf(1e-6 / len(betas), dof) for chi, dof in pt.rung_chi2(res["samples"][0], p, q)]
    print("L=%d q=%d: chi2 / bound per rung %s, acceptance %s" % (L, q, np.round(ratios, 3), np.round(res["acceptance"], 3)))
    assert max(ratios) < 1.0, ratios
    exact = at.exact_log_z(h, J, q, beta=float(betas[-1]))
    b = np.asarray(betas, np.float64)
    plain = at.log_z0(h) + sum(np.log(np.exp((b[r + 1] - b[r]) * res["e_j"][:, :, r]).mean()) for r in range(len(b) - 1))
    print("log Z %.5f, exact %.5f, se %.5f, sum of se_r %.5f" % (res["log_z"], exact, res["log_z_se"], res["se_rungs"].sum()))
    assert abs(res["log_z"] - exact) <= 5 * res["se_rungs"].sum()
    assert abs(res["log_z"] - plain) <= 1e-9


def test_a_fitted_model():
    """tests/golden/hip_fit_L24.npz: eight rungs, linear to 1.  Every pair of rungs exchanges, but not always; log Z agrees
    with annealed importance sampling at K = 128 within four joint standard errors."""
    d = np.load(os.path.join(ROOT, "golden", "hip_fit_L24.npz"))
    h, J = d["hi"], d["jij"]
    L, q = h.shape
    r = plm.log_partition_tempered(h, J, q, 512, plm.tempering_ladder(8), burn_in=20, n_snapshots=4, thin=5, seed=1)
    a = plm.log_partition(h, J, q, n_chains=1024, n_temps=128, seed=1)
    print("hip_fit_L24: tempered log Z %.4f +- %.4f, AIS K=128 %.4f +- %.4f, acceptance %s" % (
        r["log_z"], r["log_z_se"], a["log_z"], a["log_z_se"], np.round(r["acceptance"], 3)))
    assert r["samples"].shape == (4, 512, 8, L) and r["rounds_done"] == 35
    assert ((r["acceptance"] > 0) & (r["acceptance"] < 1)).all()
    assert abs(r["log_z"] - a["log_z"]) <= 4 * np.hypot(r["log_z_se"], a["log_z_se"])
    assert np.isfinite(r["energies"][:, :, -1]).all()
