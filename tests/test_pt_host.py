"""Parallel tempering (plm_pt, DESIGN_NEXT_ROWS.md section 9.9) without a GPU: the binding and the validation that comes
before the device check, the wrappers (model_accel, the command line) with plm.parallel_tempering replaced by the numpy
twin (tests/pt_twin.py), and the twin itself on enumerable models: from exact draws of every rung the process is
stationary, so every rung stays an exact sample, which a wrong exchange rule breaks."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_twin as at  # noqa: E402
import pt_twin as pt  # noqa: E402
import sampler_twin as tw  # noqa: E402
from evcouplings_amd import _lib, model_accel, model_io, plm  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = os.path.join(ROOT, "golden", "hip_fit_L24.model")
EINVAL, EDEVICE, EUNSUPPORTED = -1, -3, -4


# ---- binding and validation --------------------------------------------------------------------------------------

def test_binding_is_declared_and_matches_the_header_layout():
    assert "plm_pt" in {name for name, _, _ in _lib.SYMBOLS}
    assert hasattr(_lib.load(), "plm_pt")
    o, r = _lib.PlmPtOpts, _lib.PlmPtResult
    assert (o.n_ladders.offset, o.n_rungs.offset, o.burn_in.offset, o.n_snapshots.offset, o.thin.offset,
            o.sweeps_per_round.offset, o.first_round.offset, o.all_rungs.offset, o.betas.offset, o.seed.offset,
            o.start.offset, o.start_rungs.offset, o.start_e.offset, C.sizeof(o)) == (0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48,
                                                                                     56, 64, 72)
    assert (r.samples.offset, r.e_j.offset, r.accepts.offset, r.attempts.offset, r.walkers.offset, r.rungs.offset,
            r.walker_e.offset, r.rounds_done.offset, r.status.offset, C.sizeof(r)) == (0, 8, 16, 24, 32, 40, 48, 56, 60, 64)
    text = open(os.path.join(os.path.dirname(ROOT), "include", "plm_hip.h")).read()
    assert "typedef int (*plm_pt_cb)(" in text and "} plm_pt_opts;" in text and "} plm_pt_result;" in text


def _model(L=4, q=3):
    rng = np.random.default_rng(1)
    return rng.normal(size=(L, q)).astype(np.float32), rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)


def _code(betas=(0.0, 0.5, 1.0), n_ladders=8, L=4, q=3, **kw):
    h, J = _model(L, q)
    with pytest.raises(_lib.PlmError) as err:
        plm.parallel_tempering(h, J, q, n_ladders, betas, **kw)
    return err.value.code


def test_validation_comes_before_the_device():
    """Every PLM_EINVAL / PLM_EUNSUPPORTED of the scalars, the ladder and the start pointers, with or without a GPU."""
    assert _code(n_ladders=0) == EINVAL
    assert _code(n_snapshots=0) == EINVAL
    assert _code(sweeps_per_round=0) == EINVAL
    assert _code(burn_in=-1) == EINVAL
    assert _code(first_round=-1) == EINVAL
    assert _code(thin=0) == EINVAL
    assert _code(betas=[0.0, 0.5, 0.4]) == EINVAL                           # decreases
    assert _code(betas=[-0.5, 0.0, 1.0]) == EINVAL                          # negative
    assert _code(betas=[0.0, float("nan"), 1.0]) == EINVAL
    assert _code(betas=[float("nan")]) == EINVAL
    assert _code(betas=[0.0, 0.5, float("inf")]) == EINVAL
    # (first_round + rounds + 1) n: 2^32 - 1 and 2^32 are refused
    assert _code(burn_in=65534, sweeps_per_round=65537) == EINVAL           # 65535 x 65537 = 2^32 - 1
    assert _code(burn_in=65534, first_round=1, sweeps_per_round=65536) == EINVAL          # 2^32
    assert _code(burn_in=65530, n_snapshots=3, thin=2, first_round=1, sweeps_per_round=65536) == EINVAL      # 2^32
    assert _code(burn_in=0, n_snapshots=3, thin=2 ** 30, first_round=2 ** 31 - 1, sweeps_per_round=1) == EINVAL
    assert _code(burn_in=2 ** 31 - 1, sweeps_per_round=2) == EINVAL
    assert _code(q=33, L=2) == EUNSUPPORTED
    lib = _lib.load()
    h, J = _model()
    x = np.concatenate([h.ravel(), J.ravel()])
    xp = x.ctypes.data_as(C.c_void_p)
    betas = np.array([0.0, 1.0], np.float32)
    bp = betas.ctypes.data_as(C.c_void_p)
    states, rungs, e = np.zeros((16, 4), np.int8), np.tile(np.arange(2, dtype=np.int32), 8), np.zeros(16)
    sp, rp, ep = (a.ctypes.data_as(C.c_void_p) for a in (states, rungs, e))

    def call(L=4, q=3, opts=True, res=True, **kw):
        f = dict(n_ladders=8, n_rungs=2, burn_in=1, n_snapshots=1, thin=1, sweeps_per_round=1, first_round=0, all_rungs=0,
                 betas=bp, seed=0, start=None, start_rungs=None, start_e=None)
        f.update(kw)
        o, r = _lib.PlmPtOpts(**f), _lib.PlmPtResult()
        return lib.plm_pt(L, q, xp, C.byref(o) if opts else None, 0, None, _lib.PT_CB(), None, C.byref(r) if res else None)

    assert call(opts=False) == EINVAL and call(res=False) == EINVAL
    assert call(L=0) == EINVAL and call(n_rungs=0) == EINVAL
    assert call(q=1) == EUNSUPPORTED
    assert call(betas=None) == EINVAL
    assert call(start_rungs=rp) == EINVAL                                   # rungs without states
    assert call(start_e=ep) == EINVAL                                       # energies without both
    assert call(start=sp, start_e=ep) == EINVAL                             # energies without rungs
    assert call(start_rungs=rp, start_e=ep) == EINVAL                       # energies without states
    assert call(n_ladders=2 ** 29, L=4) == EINVAL                           # C R L = 2^32
    # what the wrapper refuses itself
    with pytest.raises(ValueError):
        plm.parallel_tempering(h, J[:-1], 3, 8, betas)
    with pytest.raises(ValueError):
        plm.parallel_tempering(h, J, 3, 8, [])
    with pytest.raises(ValueError):
        plm.parallel_tempering(h, J, 3, 8, betas, start=(states[:-1],))
    with pytest.raises(ValueError):
        plm.parallel_tempering(h, J, 3, 8, betas, start=(states, rungs[:-1]))
    with pytest.raises(ValueError):
        plm.parallel_tempering(h, J, 3, 8, betas, start=(states, None, e))
    with pytest.raises(ValueError):
        plm.log_partition_tempered(h, J, 3, 8, [0.5, 1.0])


def test_a_valid_call_fails_loudly_without_a_gpu():
    lib = _lib.load()
    if lib.plm_device_count() <= 0:                        # no CPU path
        h, J = _model()
        with pytest.raises(_lib.PlmError) as err:
            plm.parallel_tempering(h, J, 3, 8, [0.0, 1.0], burn_in=2)
        assert err.value.code == EDEVICE


def test_tempering_ladder():
    lin = plm.tempering_ladder(5)
    assert lin.dtype == np.float32 and np.array_equal(lin, np.array([0, 0.25, 0.5, 0.75, 1], np.float32))
    geo = plm.tempering_ladder(5, beta_max=2.0, kind="geometric")
    assert np.array_equal(geo, np.array([0, 0.25, 0.5, 1, 2], np.float32))
    assert np.array_equal(plm.tempering_ladder(1, 0.7), np.array([0.7], np.float32))
    assert np.array_equal(plm.tempering_ladder(2, 1.5, "geometric"), np.array([0, 1.5], np.float32))
    for bad in (dict(n_rungs=0), dict(n_rungs=3, beta_max=-1.0), dict(n_rungs=3, beta_max=float("nan")),
                dict(n_rungs=3, kind="other")):
        with pytest.raises(ValueError):
            plm.tempering_ladder(**bad)


# ---- the twin ------------------------------------------------------------------------------------------------------

def test_one_rung_is_the_ais_sweep_and_the_uniform_is_the_samplers():
    """R = 1: no exchange, and the sweeps are those of the AIS twin at the same beta.  The float32 uniform equals the
    float64 one wherever that is a float32, and stays below 1."""
    h, J = at.enumerable_model(*at.ENUMERABLE[0])
    one = pt.pt(h, J, 4, 40, [0.6], 1, sweeps_per_round=2, seed=5)
    ais = at.ais(h, J, 4, 40, betas=[0.0, 0.6], sweeps_per_temp=2, seed=5)
    assert np.array_equal(one["state"].x, ais["states"]) and np.array_equal(one["state"].E, ais["e_j"])
    assert one["accepts"].size == 0
    chains = np.arange(5000)
    u32 = pt.uniform_f32(9, chains, 1, 3, 2)
    u64 = ((tw.philox4x32_10(chains, 1, 3, 2, 9, 0)[0] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    assert (u32 < 1.0).all() and np.abs(u32 - u64).max() <= 2.0 ** -25
    assert np.array_equal(u32[u64 < 0.5], u64[u64 < 0.5])


def test_equal_temperatures_accept_every_exchange_and_the_maps_stay_inverse():
    h, J = at.enumerable_model(*at.ENUMERABLE[0])
    R, Cn, rounds = 5, 7, 6
    r = pt.pt(h, J, 4, Cn, [0.7] * R, rounds, seed=2, trace=True)
    assert np.array_equal(r["accepts"], r["attempts"]) and np.array_equal(r["attempts"], Cn * np.array([3, 3, 3, 3]))
    order = list(range(R))                                              # slot at every rung: odd-even transposition
    for g in range(rounds):
        for k in range(g % 2, R - 1, 2):
            order[k], order[k + 1] = order[k + 1], order[k]
        sor = np.argsort(r["trace"]["rungs"][g + 1], axis=1)
        assert (sor == np.array(order)[None, :]).all()
    # the states do not know of the exchanges: every walker is the one-rung chain with its chain index
    alone = pt.pt(h, J, 4, Cn * R, [0.7], rounds, seed=2)
    assert np.array_equal(alone["state"].x, r["state"].x) and np.array_equal(alone["state"].E, r["state"].E)


def test_twin_continuation_and_independence_of_the_ladder_count():
    h, J = at.enumerable_model(*at.ENUMERABLE[1])
    betas = (0.0, 0.6, 1.3)
    whole = pt.parallel_tempering(h, J, 7, 12, betas, burn_in=5, n_snapshots=2, thin=1, seed=4, all_rungs=True)
    a = pt.parallel_tempering(h, J, 7, 12, betas, burn_in=3, seed=4, all_rungs=True)
    b = pt.parallel_tempering(h, J, 7, 12, betas, burn_in=2, n_snapshots=2, seed=4, all_rungs=True, start=a["walkers"],
                              first_round=3)
    for k in ("samples", "e_j", "energies"):
        assert np.array_equal(whole[k], b[k]), k
    assert np.array_equal(whole["accepts"], a["accepts"] + b["accepts"])
    assert np.array_equal(whole["attempts"], a["attempts"] + b["attempts"])
    for x, y in zip(whole["walkers"], b["walkers"]):
        assert np.array_equal(x, y)
    few = pt.parallel_tempering(h, J, 7, 5, betas, burn_in=5, n_snapshots=2, thin=1, seed=4, all_rungs=True)
    assert np.array_equal(few["samples"], whole["samples"][:, :5]) and np.array_equal(few["e_j"], whole["e_j"][:, :5])
    top = pt.parallel_tempering(h, J, 7, 5, betas, burn_in=5, n_snapshots=2, thin=1, seed=4)
    assert np.array_equal(top["samples"], few["samples"][:, :, -1]) and top["e_j"].shape == (2, 5)
    # the tracked energy is the coupling energy of the rows
    assert np.allclose(whole["e_j"], whole["energies"][..., 1], rtol=0, atol=1e-5)


def _flipped_rule(delta, u):
    """pt.exchange_rule with the sign of delta wrong."""
    delta = -delta
    with np.errstate(over="ignore"):
        return (delta >= 0.0) | (u < np.exp(delta))


@pytest.mark.parametrize("L,q,j_scale,model_seed", at.ENUMERABLE)
def test_stationary_rungs_against_enumeration(L, q, j_scale, model_seed, monkeypatch):
    """Every walker starts from an exact draw of the distribution of its rung, so the process is stationary from round 0
    and the C rows of rung r after 12 rounds are C independent exact draws of p_{beta_r}: chi-square of every rung at a
    family-wise 1e-6.  With the sign of Delta flipped in the exchange rule the same test fails, so it sees a wrong exchange.
    log Z from those starts (K = 1): within 5 sum_r se_r of the exact value, the worst case over the correlation of rungs."""
    h, J = at.enumerable_model(L, q, j_scale, model_seed)
    betas, Cn = pt.STATIONARY_BETAS, pt.STATIONARY_C
    p = pt.rung_distributions(h, J, q, betas)
    x0 = pt.stationary_start(h, J, q, betas, Cn, 100 + L)
    worst = {}
    for rule in (pt.exchange_rule, _flipped_rule):
        r = pt.pt(h, J, q, Cn, betas, pt.STATIONARY_ROUNDS, seed=3, start=(x0,), rule=rule)
        rows, _ = r["state"].in_rung_order()
        ratios = [chi / stats.chi2.isf(1e-6 / len(betas), dof) for chi, dof in pt.rung_chi2(rows, p, q)]
        print("L=%d q=%d %s: chi2 / bound per rung %s, acceptance %s" % (
            L, q, rule.__name__, np.round(ratios, 3), np.round(r["accepts"] / r["attempts"], 3)))
        worst[rule] = max(ratios)
    assert worst[pt.exchange_rule] < 1.0
    assert worst[_flipped_rule] > 1.0
    monkeypatch.setattr(plm, "parallel_tempering", pt.parallel_tempering)
    res = plm.log_partition_tempered(h, J, q, Cn, betas, burn_in=0, seed=3, start=(x0,))
    exact = at.exact_log_z(h, J, q, beta=float(betas[-1]))
    print("log Z %.5f, exact %.5f, se %.5f, sum of se_r %.5f" % (res["log_z"], exact, res["log_z_se"], res["se_rungs"].sum()))
    assert abs(res["log_z"] - exact) <= 5 * res["se_rungs"].sum()
    assert res["log_z0"] == at.log_z0(h) and abs(res["log_z_se"] - np.sqrt((res["se_rungs"] ** 2).sum())) < 1e-15
    assert 0 < res["log_z_se"] <= res["se_rungs"].sum() < 0.1


def test_log_z_formula_on_known_energies():
    """Two ladders, two snapshots, three rungs: the formula by hand."""
    e = np.array([[[1.0, 2.0, 9.0], [3.0, -1.0, 9.0]], [[0.5, 0.0, 9.0], [2.5, 1.0, 9.0]]])       # [K, C, R]
    betas = np.array([0.0, 0.5, 2.0], np.float32)
    lz, se, ser = plm.tempered_log_z(e, betas, 1.25)
    w0, w1 = np.exp(0.5 * e[:, :, 0]), np.exp(1.5 * e[:, :, 1])
    assert abs(lz - (1.25 + np.log(w0.mean()) + np.log(w1.mean()))) < 1e-12
    s0 = w0.mean(axis=0).std(ddof=1) / (np.sqrt(2) * w0.mean())
    s1 = w1.mean(axis=0).std(ddof=1) / (np.sqrt(2) * w1.mean())
    assert np.allclose(ser, [s0, s1], rtol=1e-12) and abs(se - np.hypot(s0, s1)) < 1e-12
    one = plm.tempered_log_z(e[:, :1], betas, 0.0)
    assert one[1] == 0.0 and not one[2].any()                             # one ladder has no spread
    lz1, se1, ser1 = plm.tempered_log_z(e[:, :, :1], betas[:1], 3.0)         # one rung: log Z_0 itself
    assert (lz1, se1, ser1.size) == (3.0, 0.0, 0)


# ---- wrappers ------------------------------------------------------------------------------------------------------

def _twin_hamiltonians(seqs, q, hi, jij, device=0):
    h = np.asarray(hi, np.float64)
    return tw.hamiltonians(np.asarray(seqs).astype(np.int64), h, tw.dense(np.asarray(jij, np.float64), h.shape[0], q))


def _toy_model():
    h, J = at.enumerable_model(4, 3, 0.5, 2)
    return SimpleNamespace(J_ij=tw.dense(J, 4, 3), h_i=h, alphabet=np.array(list("-AC")), target_seq=np.array(list("CA-C")),
                           index_list=np.array([10, 11, 13, 14]), L=4, q=3), h, J


def test_model_accel_sample_tempered(monkeypatch):
    calls = []

    def fake(hi, jij, q, n_ladders, betas, **kw):
        calls.append((np.asarray(betas).copy(), kw))
        return pt.parallel_tempering(hi, jij, q, n_ladders, betas, **kw)

    monkeypatch.setattr(plm, "parallel_tempering", fake)
    m, h, J = _toy_model()
    seqs, en, info = model_accel.sample_tempered(m, 6, n_rungs=3, burn_in=4, n_snapshots=2, thin=2, seed=8, energies=True,
                                                 info=True)
    ref = pt.parallel_tempering(h, J, 3, 6, plm.tempering_ladder(3), burn_in=4, n_snapshots=2, thin=2, seed=8)
    assert np.array_equal(calls[0][0], np.array([0, 0.5, 1], np.float32)) and calls[0][1]["start"] is None
    assert seqs.shape == (12, 4) and set(np.unique(seqs)) <= set("-AC")
    assert np.array_equal(seqs, m.alphabet[ref["samples"].reshape(-1, 4)])
    assert np.array_equal(en, ref["energies"].reshape(-1, 3)) and np.array_equal(info["accepts"], ref["accepts"])
    states = model_accel.sample_tempered(m, 6, betas=[0.0, 0.5, 1.0], burn_in=4, n_snapshots=2, thin=2, seed=8,
                                         as_letters=False)
    assert states.dtype == np.int8 and np.array_equal(states, ref["samples"].reshape(-1, 4))
    # starts: the target for every walker, letters, states
    model_accel.sample_tempered(m, 2, n_rungs=2, burn_in=1, start="target")
    x0 = calls[-1][1]["start"]
    assert len(x0) == 1 and np.array_equal(x0[0], np.tile(np.array([2, 1, 0, 2], np.int8), (4, 1)))
    model_accel.sample_tempered(m, 1, n_rungs=2, burn_in=1, start=[list("AC-A"), list("--CC")])
    assert np.array_equal(calls[-1][1]["start"][0], np.array([[1, 2, 0, 1], [0, 0, 2, 2]], np.int8))
    with pytest.raises(ValueError):
        model_accel.sample_tempered(m, 1, n_rungs=2, start=[list("AXCA"), list("--CC")])
    with pytest.raises(ValueError):
        model_accel.sample_tempered(m, 1, n_rungs=2, start="query")


def test_command_line(monkeypatch, tmp_path, capsys):
    from evcouplings_amd import sample as cli
    pt_calls, gibbs_calls = [], []

    def fake_pt(hi, jij, q, n_ladders, betas, **kw):
        pt_calls.append((int(n_ladders), np.asarray(betas).copy(), kw))
        return pt.parallel_tempering(hi, jij, q, n_ladders, betas, **kw)

    def fake_sample(hi, jij, q, n_chains, **kw):
        gibbs_calls.append(kw)
        return tw.sample(hi, jij, q, n_chains, **kw)

    monkeypatch.setattr(plm, "parallel_tempering", fake_pt)
    monkeypatch.setattr(plm, "sample", fake_sample)
    m = model_io.read_model_file(GOLDEN_MODEL)
    out, csv = str(tmp_path / "s.a2m"), str(tmp_path / "e.csv")
    argv = [GOLDEN_MODEL, "-n", "3", "-o", out, "--burn-in", "2", "--snapshots", "2", "--thin", "1", "--seed", "6"]
    assert cli.main(argv + ["--tempering", "3", "--beta-max", "1.5", "--energies", csv]) == 0
    assert len(pt_calls) == 1 and not gibbs_calls
    n, betas, kw = pt_calls[0]
    assert n == 3 and np.array_equal(betas, np.array([0, 0.75, 1.5], np.float32))
    assert (kw["burn_in"], kw["n_snapshots"], kw["thin"], kw["seed"], kw["start"]) == (2, 2, 1, 6, None)
    ref = pt.parallel_tempering(m["hi"], m["jij"], m["q"], 3, betas, burn_in=2, n_snapshots=2, thin=1, seed=6)
    records = open(out).read().split(">")[1:]
    assert len(records) == 7 and records[0].split("\n")[1] == "".join(m["target_seq"])
    letters = np.array(list(m["alphabet"]))
    assert [r.split("\n")[1] for r in records[1:]] == ["".join(letters[row]) for row in ref["samples"].reshape(-1, m["L"])]
    rows = open(csv).read().splitlines()
    assert rows[0] == "id,H,H_J,H_h" and len(rows) == 7
    vals = np.array([[float(v) for v in r.split(",")[1:]] for r in rows[1:]])
    assert np.allclose(vals, ref["energies"].reshape(-1, 3), atol=1e-5)
    err = capsys.readouterr().err
    assert "acceptance between neighbouring temperatures: " + " ".join("%.3f" % v for v in ref["acceptance"]) in err
    # the top of the ladder defaults to 1; without the flag the command samples as before
    assert cli.main(argv + ["--tempering", "2"]) == 0
    assert np.array_equal(pt_calls[-1][1], np.array([0, 1], np.float32))
    assert cli.main(argv) == 0
    assert len(pt_calls) == 2 and len(gibbs_calls) == 1 and gibbs_calls[0]["burn_in"] == 2
    for bad in (["--beta-max", "2"], ["--tempering", "3", "--no-gaps"], ["--tempering", "3", "--fix", "5"],
                ["--tempering", "3", "--beta", "0.5"], ["--tempering", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(argv + bad)
