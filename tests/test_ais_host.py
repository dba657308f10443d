"""Annealed importance sampling for log Z (plm_ais, DESIGN_NEXT_ROWS.md section 9.8) without a GPU: the numpy twin
(tests/ais_twin.py) against exact enumeration and in its exact special cases, the binding and the validation that comes
before the device check, and the wrappers (model_accel, the command line) with plm.log_partition replaced by the twin."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_twin as at  # noqa: E402
import sampler_twin as tw  # noqa: E402
from evcouplings_amd import _lib, model_accel, model_io, plm  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = os.path.join(ROOT, "golden", "hip_fit_L24.model")
EINVAL, EUNSUPPORTED = -1, -4


@pytest.mark.parametrize("L,q,j_scale,model_seed", at.ENUMERABLE)
def test_twin_against_enumeration(L, q, j_scale, model_seed):
    """Linear schedule, K = 16, n = 1, C = 4096: the estimate lies within three of its own standard errors of the exact
    log Z, for three seeds."""
    h, J = at.enumerable_model(L, q, j_scale, model_seed)
    exact = at.exact_log_z(h, J, q)
    for seed in at.ENUMERABLE_SEEDS:
        r = at.ais(h, J, q, at.ENUMERABLE_C, at.ENUMERABLE_K, seed=seed)
        z = (r["log_z"] - exact) / r["log_z_se"]
        print("L=%d q=%d seed %d: log Z %.5f, exact %.5f, se %.5f, z %.2f, ess %.0f" % (L, q, seed, r["log_z"], exact,
                                                                                         r["log_z_se"], z, r["ess"]))
        assert abs(r["log_z"] - exact) <= 3 * r["log_z_se"], (seed, r["log_z"], exact, r["log_z_se"])
        assert 0 < r["log_z_se"] < 0.02 and 0.5 * at.ENUMERABLE_C < r["ess"] <= at.ENUMERABLE_C


def test_more_temperatures_narrow_the_weights():
    h, J = at.enumerable_model(*at.ENUMERABLE[0])
    se = [at.ais(h, J, 4, 1024, K, seed=5)["log_z_se"] for K in (1, 8, 64)]
    assert se[0] > 2 * se[1] > 4 * se[2], se


def test_one_step_is_plain_importance_sampling():
    """K = 1: x ~ the independent model of the fields, log w = beta_1 H_J(x); a schedule that ends at beta_K gives log Z
    of the couplings scaled by beta_K."""
    L, q, j_scale, ms = at.ENUMERABLE[1]
    h, J = at.enumerable_model(L, q, j_scale, ms)
    Cn = 2000
    for b1 in (1.0, 0.25):
        r = at.ais(h, J, q, Cn, betas=[0.0, b1], seed=9)
        x0 = tw.start_states(h.astype(np.float64), Cn, 9)
        hj = tw.hamiltonians(x0, h.astype(np.float64), tw.dense(J.astype(np.float64), L, q))[:, 1]
        assert np.allclose(r["log_w"], np.float64(np.float32(b1)) * hj, rtol=0, atol=1e-5)
        plain = at.log_z0(h) + np.log(np.mean(np.exp(np.float32(b1) * hj)))
        assert abs(r["log_z"] - plain) < 1e-6
        assert abs(r["log_z"] - at.exact_log_z(h, J, q, beta=b1)) <= 4 * r["log_z_se"]
    # the tracked energy of the final states is their coupling energy
    hj_end = tw.hamiltonians(r["states"].astype(np.int64), h.astype(np.float64), tw.dense(J.astype(np.float64), L, q))[:, 1]
    assert np.allclose(r["e_j"], hj_end, rtol=0, atol=1e-5)


def test_without_couplings_the_estimate_is_exact():
    rng = np.random.default_rng(3)
    L, q, Cn = 6, 5, 300
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = np.zeros((L * (L - 1) // 2, q, q), np.float32)
    r = at.ais(h, J, q, Cn, 4, sweeps_per_temp=2, seed=1)
    assert not r["log_w"].any() and not r["e_j"].any()
    assert r["log_z"] == r["log_z0"] == at.log_z0(h) and r["ess"] == Cn and r["log_z_se"] == 0.0
    exact = at.exact_log_z(h, J, q)
    assert abs(r["log_z"] - exact) < 1e-12 * abs(exact)


def test_twin_does_not_depend_on_the_chain_count_and_prefixes_are_schedules():
    h, J = at.enumerable_model(*at.ENUMERABLE[0])
    betas = np.array([0.0, 0.4, 0.7, 1.3], np.float32)
    full = at.ais(h, J, 4, 64, betas=betas, seed=2, trace=True)
    part = at.ais(h, J, 4, 16, betas=betas[:3], seed=2)
    assert np.array_equal(part["log_w"], full["steps"]["log_w"][2][:16])
    assert np.array_equal(part["e_j"], full["steps"]["e_j"][2][:16])
    assert np.array_equal(part["states"], full["steps"]["states"][2][:16])


# ---- binding and validation --------------------------------------------------------------------------------------

def test_binding_is_declared_and_matches_the_header_layout():
    assert "plm_ais" in {name for name, _, _ in _lib.SYMBOLS}
    assert hasattr(_lib.load(), "plm_ais")
    o, r = _lib.PlmAisOpts, _lib.PlmAisResult
    assert (o.n_chains.offset, o.n_temps.offset, o.sweeps_per_temp.offset, o.steps_per_launch.offset, o.betas.offset,
            o.seed.offset, C.sizeof(o)) == (0, 4, 8, 12, 16, 24, 32)
    assert (r.log_z.offset, r.log_z0.offset, r.log_z_se.offset, r.ess.offset, r.log_w.offset, r.e_j.offset,
            r.states.offset, r.steps_done.offset, r.status.offset, C.sizeof(r)) == (0, 8, 16, 24, 32, 40, 48, 56, 60, 64)


def _model(L=4, q=3):
    rng = np.random.default_rng(1)
    return rng.normal(size=(L, q)).astype(np.float32), rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)


def _code(**kw):
    h, J = _model(kw.pop("L", 4), kw.pop("q", 3))
    with pytest.raises(_lib.PlmError) as err:
        plm.log_partition(h, J, h.shape[1], **kw)
    return err.value.code


def test_validation_comes_before_the_device():
    """Every PLM_EINVAL / PLM_EUNSUPPORTED of the scalars and the schedule, on a machine with or without a GPU."""
    assert _code(n_chains=0) == EINVAL
    assert _code(n_temps=0) == EINVAL
    assert _code(sweeps_per_temp=0) == EINVAL
    assert _code(steps_per_launch=-1) == EINVAL
    assert _code(n_temps=65536, sweeps_per_temp=65536) == EINVAL            # K n = 2^32
    assert _code(n_temps=65537, sweeps_per_temp=65535) == EINVAL            # K n = 2^32 - 1
    assert _code(betas=[0.0, 0.5, 0.4]) == EINVAL                           # decreases
    assert _code(betas=[0.1, 0.5, 1.0]) == EINVAL                           # starts above 0
    assert _code(betas=[0.0, float("nan"), 1.0]) == EINVAL
    assert _code(betas=[float("nan"), 0.5, 1.0]) == EINVAL
    assert _code(betas=[0.0, 0.5, float("inf")]) == EINVAL
    assert _code(betas=[-0.5, 0.0, 1.0]) == EINVAL
    assert _code(q=33, L=2) == EUNSUPPORTED
    lib = _lib.load()
    h, J = _model()
    x = np.concatenate([h.ravel(), J.ravel()])
    opts, res = _lib.PlmAisOpts(8, 2, 1, 0, None, 0), _lib.PlmAisResult()
    xp = x.ctypes.data_as(C.c_void_p)
    assert lib.plm_ais(4, 3, xp, None, 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL
    assert lib.plm_ais(4, 3, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None, None) == EINVAL
    assert lib.plm_ais(0, 3, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL
    assert lib.plm_ais(4, 1, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EUNSUPPORTED
    with pytest.raises(ValueError):
        plm.log_partition(h, J[:-1], 3)
    with pytest.raises(ValueError):
        plm.log_partition(h, J, 3, betas=[0.0])


def test_a_valid_call_fails_loudly_without_a_gpu():
    lib = _lib.load()
    if lib.plm_device_count() <= 0:                        # no CPU path
        h, J = _model()
        with pytest.raises(_lib.PlmError) as err:
            plm.log_partition(h, J, 3, n_chains=8, n_temps=2)
        assert err.value.code == -3


# ---- wrappers ------------------------------------------------------------------------------------------------------

def _twin_hamiltonians(seqs, q, hi, jij, device=0):
    h = np.asarray(hi, np.float64)
    return tw.hamiltonians(np.asarray(seqs).astype(np.int64), h, tw.dense(np.asarray(jij, np.float64), h.shape[0], q))


def _toy_model():
    h, J = at.enumerable_model(4, 3, 0.5, 2)
    return SimpleNamespace(J_ij=tw.dense(J, 4, 3), h_i=h, alphabet=np.array(list("-AC")), target_seq=np.array(list("CA-C")),
                           index_list=np.array([10, 11, 13, 14]), L=4, q=3), h, J


def test_model_accel_log_partition_and_log_probabilities(monkeypatch):
    monkeypatch.setattr(plm, "log_partition", at.log_partition)
    monkeypatch.setattr(plm, "hamiltonians", _twin_hamiltonians)
    m, h, J = _toy_model()
    res = model_accel.log_partition(m, n_chains=512, n_temps=8, seed=3)
    exact = at.exact_log_z(h, J, 3)
    assert abs(res["log_z"] - exact) <= 4 * res["log_z_se"]
    assert res["sequences"].shape == (512, 4) and set(np.unique(res["sequences"])) <= set("-AC")
    assert np.array_equal(m.alphabet[res["states"]], res["sequences"])
    assert np.isfinite(res["entropy"]) and res["entropy"] < 4 * np.log(3)
    # log P over all states sums to one with the exact log Z, from letters, strings and states alike
    st = tw.all_states(4, 3)
    lp = model_accel.log_probabilities(m, st, exact)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-12
    assert np.array_equal(model_accel.log_probabilities(m, m.alphabet[st], exact), lp)
    assert np.array_equal(model_accel.log_probabilities(m, ["".join(r) for r in m.alphabet[st[:7]]], exact), lp[:7])
    H = _twin_hamiltonians(st, 3, h, J)[:, 0]
    assert np.array_equal(lp, H - exact)
    with pytest.raises(ValueError):
        model_accel.log_probabilities(m, ["CAXC"], exact)
    with pytest.raises(ValueError):
        model_accel.log_probabilities(m, ["CAC"], exact)
    with pytest.raises(ValueError):
        model_accel.log_probabilities(m, np.array([[0, 1, 2, 3]]), exact)


def test_command_line(monkeypatch, tmp_path, capsys):
    from evcouplings_amd import logz as cli
    calls = []

    def fake(hi, jij, q, **kw):
        calls.append(kw)
        return at.log_partition(hi, jij, q, **kw)

    monkeypatch.setattr(plm, "log_partition", fake)
    monkeypatch.setattr(plm, "hamiltonians", _twin_hamiltonians)
    m = model_io.read_model_file(GOLDEN_MODEL)
    L, target = m["L"], m["target_seq"]
    other = m["alphabet"][1] * L
    a2m, out = str(tmp_path / "s.a2m"), str(tmp_path / "p.csv")
    with open(a2m, "w") as f:
        f.write(">target/1-%d some words\n%s\n" % (L, target))
        f.write(">inserts\n%sxy%s\n..%s\n" % (target[:5], target[5:11], target[11:]))      # the same match columns
        f.write(">other\n%s\n" % other)
    rc = cli.main([GOLDEN_MODEL, "-n", "16", "-k", "2", "--sweeps", "1", "--seed", "4", "--sequences", a2m, "-o", out])
    assert rc == 0
    assert calls == [dict(n_chains=16, n_temps=2, sweeps_per_temp=1, seed=4)]
    ref = at.log_partition(m["hi"], m["jij"], m["q"], n_chains=16, n_temps=2, seed=4)
    text = capsys.readouterr().out
    assert "log Z = %.6f +- %.6f" % (ref["log_z"], ref["log_z_se"]) in text and "ESS = %.1f of 16" % ref["ess"] in text
    rows = open(out).read().splitlines()
    assert rows[0] == "id,H,logP" and [r.split(",")[0] for r in rows[1:]] == ["target/1-%d" % L, "inserts", "other"]
    vals = np.array([[float(v) for v in r.split(",")[1:]] for r in rows[1:]])
    code = {a: k for k, a in enumerate(m["alphabet"])}
    x = np.array([[code[c] for c in s] for s in (target, target, other)])
    H = _twin_hamiltonians(x, m["q"], m["hi"], m["jij"])[:, 0]
    assert np.allclose(vals[:, 0], H, atol=1e-5) and np.allclose(vals[:, 1], H - ref["log_z"], atol=1e-5)
    # without sequences nothing is written; a record of another length is an error; the two options go together
    assert cli.main([GOLDEN_MODEL, "-n", "8", "-k", "1"]) == 0
    with open(a2m, "w") as f:
        f.write(">short\n%s\n" % target[:-1])
    with pytest.raises(ValueError):
        cli.main([GOLDEN_MODEL, "-n", "8", "-k", "1", "--sequences", a2m, "-o", out])
    with pytest.raises(SystemExit):
        cli.main([GOLDEN_MODEL, "--sequences", a2m])
