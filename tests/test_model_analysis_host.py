"""
CPU side of the CouplingsModel analysis drop-ins (model_accel.install(analysis=True)): the float64 numpy twins of
tests/model_twins.py are checked against the reference's numbers (tests/golden/model_analysis_L24.npz), then stand in
for plm.model_pair_scores / double_mutant_matrix / independent_fields (no GPU here) while the REFERENCE's own classes
and its mean_field protocol run on top of the drop-ins.  The tests that drive the reference skip where it is absent.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_twins as tw  # noqa: E402
import refstubs  # noqa: E402

from evcouplings_amd import model_io  # noqa: E402

ALPHABET = "-ACDEFGHIKLMNPQRSTVWY"
needs_reference = pytest.mark.skipif(not refstubs.reference_available(), reason="reference tree not present")


@pytest.fixture(scope="module")
def golden(golden_dir):
    m = model_io.read_model_file(os.path.join(golden_dir, "hip_fit_L24.model"))
    z = np.load(os.path.join(golden_dir, "model_analysis_L24.npz"))
    return m, z, os.path.join(golden_dir, "hip_fit_L24.model")


@pytest.fixture()
def twins(monkeypatch):
    """plm's three analysis calls on the numpy twins; returns the call log"""
    from evcouplings_amd import plm
    calls = []

    def pair_scores(J_ij, f_ij, f_i, device=0):
        calls.append("pair_scores")
        return tw.pair_scores(J_ij, f_ij, f_i)

    def double_mutants(J_ij, smm, target, device=0):
        calls.append("double_mutants")
        return tw.double_mutants(J_ij, smm, target)

    def independent_fields(f_i, lambda_h, n_eff, device=0):
        calls.append("independent_fields")
        return tw.independent_fields(f_i, float(lambda_h), float(n_eff))

    # install() also puts the Hamiltonians (which single_mut_mat uses) on plm: the C oracle stands in for them
    from oracle.oracle import Oracle
    o = Oracle("f64")

    def canon(hi, jij):
        return np.concatenate([np.asarray(hi, np.float64).ravel(), np.asarray(jij, np.float64).ravel()])

    monkeypatch.setattr(plm, "hamiltonians", lambda seqs, q, hi, jij, device=0: o.hamiltonians(seqs, q, canon(hi, jij)))
    monkeypatch.setattr(plm, "single_mutant_matrix",
                        lambda t, q, hi, jij, device=0: o.single_mutants(np.asarray(t).ravel(), q, canon(hi, jij)))
    monkeypatch.setattr(plm, "model_pair_scores", pair_scores)
    monkeypatch.setattr(plm, "double_mutant_matrix", double_mutants)
    monkeypatch.setattr(plm, "independent_fields", independent_fields)
    return calls


@pytest.fixture()
def ref_model():
    refstubs.install()
    import evcouplings.couplings.model as ref_model
    return ref_model


def test_the_numpy_twins_reproduce_the_reference_numbers(golden):
    m, z, _ = golden
    L = m["L"]
    J, F = tw.dense_from_pairs(m["jij"], L), tw.dense_from_pairs(m["fij"], L)
    assert (m["fij"] == 0).sum() > 100000          # the p > 0 mask of the MI sum is exercised
    fn, mi = tw.pair_scores(J, F, m["fi"])
    np.testing.assert_allclose(fn, z["fn_scores"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(mi, z["mi_scores_raw"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(tw.apc(fn), z["cn_scores"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(tw.apc(mi), z["mi_scores_apc"], rtol=1e-12, atol=1e-13)
    target = np.array([ALPHABET.index(c) for c in m["target_seq"]])
    D = tw.double_mutants(J, z["single_mut_mat"], target)
    p = z["dmm_pairs"]
    np.testing.assert_allclose(D[p[:, 0], p[:, 1]], z["dmm_blocks"], rtol=1e-12, atol=1e-13)
    lam, n_eff = float(z["lambda_h"]), float(z["n_eff"])
    h, iters = tw.independent_fields(m["fi"], lam, n_eff)
    _, g_ref, _ = tw.objective(z["h_indep"], m["fi"].astype(np.float64), lam, n_eff)
    assert (np.abs(h - z["h_indep"]).max(axis=1) <= np.linalg.norm(g_ref, axis=1) / (2 * lam)).all()
    assert np.abs(tw.objective(h, m["fi"].astype(np.float64), lam, n_eff)[1]).max() <= 1e-10 * n_eff
    assert (iters < 100).all()


@needs_reference
def test_couplings_model_on_the_drop_ins_matches_the_reference(golden, twins, ref_model, monkeypatch):
    import pandas as pd
    from evcouplings_amd import model_accel, plm
    _, z, path = golden
    # single_mut_mat through the reference's own loop behind the energy drop-in, so that dmm's input is the reference's
    loop = ref_model._single_mutant_hamiltonians
    monkeypatch.setattr(plm, "single_mutant_matrix",
                        lambda t, q, hi, jij, device=0: loop(t, tw.dense_from_pairs(jij, len(hi)), hi))
    cls = ref_model.CouplingsModel
    slow = cls(path)                  # the reference's own methods, computed before the class is patched
    want, dmm_slow, ind_slow = slow.ecs, slow.dmm(), slow.to_independent_model()
    model_accel.install(ref_model, analysis=True)
    try:
        fast = cls(path)
        got = fast.ecs
        assert twins == ["pair_scores"]
        pd.testing.assert_frame_equal(got.sort_index(), want.sort_index(), rtol=1e-12)
        assert list(got.index[:20]) == list(want.index[:20])
        assert list(got.index) == list(z["ecs_index"])
        for name in ("fn_scores", "cn_scores", "mi_scores_raw", "mi_scores_apc"):
            np.testing.assert_allclose(getattr(fast, name), getattr(slow, name), rtol=1e-12, atol=1e-13, err_msg=name)
        np.testing.assert_allclose(fast.dmm(), dmm_slow, rtol=1e-12, atol=1e-13)
        assert fast.double_mut_mat is fast.double_mut_mat          # cached, as the reference's property
        ind_fast = fast.to_independent_model()
    finally:
        model_accel.uninstall(ref_model)
    lam, n_eff = float(slow.lambda_h), float(slow.N_eff)
    _, g_ref, _ = tw.objective(ind_slow.h_i, slow.f_i.astype(np.float64), lam, n_eff)
    assert (np.abs(ind_fast.h_i - ind_slow.h_i).max(axis=1) <= np.linalg.norm(g_ref, axis=1) / (2 * lam)).all()
    assert not ind_fast.J_ij.any() and ind_fast._ecs is None and fast.J_ij.any()
    assert twins.count("independent_fields") == 1 and twins.count("double_mutants") == 1


@needs_reference
def test_non_numeric_index_list_gives_nan_seqdist(golden, twins, ref_model):
    import pandas as pd
    from evcouplings_amd import model_accel
    _, _, path = golden
    slow = ref_model.CouplingsModel(path)
    slow.index_list = np.array(["A_%d" % k for k in range(slow.L)])
    slow._reset_precomputed()
    want = slow.ecs
    model_accel.install(ref_model, analysis=True)
    try:
        fast = ref_model.CouplingsModel(path)
        fast.index_list = slow.index_list
        fast._reset_precomputed()
        got = fast.ecs
    finally:
        model_accel.uninstall(ref_model)
    assert got["seqdist"].isna().all()
    pd.testing.assert_frame_equal(got.sort_index(), want.sort_index(), rtol=1e-12)


@needs_reference
def test_lambda_h_zero_goes_to_the_original_method(golden, twins, ref_model):
    from evcouplings_amd import model_accel
    _, _, path = golden
    model_accel.install(ref_model, analysis=True)
    try:
        m = ref_model.CouplingsModel(path)
        m.lambda_h = 0.0
        m.f_i = np.full_like(m.f_i, 1.0 / m.f_i.shape[1])    # uniform: the lambda_h = 0 optimum exists (h = 0)
        ind = m.to_independent_model()
    finally:
        model_accel.uninstall(ref_model)
    assert "independent_fields" not in twins
    assert np.abs(ind.h_i).max() < 1e-5


def _oracle_backed_mean_field(monkeypatch):
    """the mean-field fit and DI on the numpy / C oracle (no GPU here), as test_reference_pipeline does"""
    from evcouplings_amd import plm
    from oracle import meanfield_ref
    from oracle.oracle import Oracle
    o = Oracle("f64")

    def fake_mean_field(msa, q, theta_id=0.8, pseudo_count=0.5, **kw):
        w = 1.0 / o.reweight(msa, theta_id)
        fi, fij = o.marginals(msa, w, q)
        out = meanfield_ref.mean_field(fi, fij, pseudo_count, want_di=False)
        return dict(weights=w.astype(np.float32), n_eff=float(w.sum()), fi=fi.astype(np.float32),
                    fij=fij.astype(np.float32), hi=out["hi"], jij=out["jij"].astype(np.float32),
                    jij_full=out["jij_full"])

    monkeypatch.setattr(plm, "mean_field", fake_mean_field)
    monkeypatch.setattr(plm, "direct_information",
                        lambda J, f: meanfield_ref.direct_information(np.asarray(J), np.asarray(f)))


@needs_reference
def test_mean_field_protocol_on_the_drop_ins(golden_dir, twins, ref_model, monkeypatch, tmp_path):
    """the reference's mean_field protocol (MeanFieldCouplingsModel._calculate_ecs reaches the drop-in through super(),
    to_raw_ec_file reads MI / DI / CN) writes the raw EC file the unpatched class writes"""
    import pandas as pd
    import evcouplings.couplings.mean_field as ref_mf
    import evcouplings.couplings.protocol as cp
    from evcouplings_amd import mean_field as our_mf, model_accel
    _oracle_backed_mean_field(monkeypatch)
    kwargs = dict(alignment_file=os.path.join(golden_dir, "hip_fit_L24.a2m"), segments=None, focus_mode=True,
                  focus_sequence="SYN/10-33", theta=0.8, pseudo_count=0.5, alphabet=None, min_sequence_distance=6,
                  ec_score_type="cn", scoring_model="skewnormal", frequencies_file=None)
    names = ["i", "A_i", "j", "A_j", "mi_raw", "mi_apc", "di", "cn"]
    raws = {}
    our_mf.install(ref_mf)
    try:
        for analysis in (False, True):
            if analysis:
                model_accel.install(ref_model, analysis=True)
            try:
                out = cp.run(protocol="mean_field", prefix=str(tmp_path / str(analysis) / "job"), **kwargs)
            finally:
                model_accel.uninstall(ref_model)
            raws[analysis] = pd.read_csv(out["raw_ec_file"], sep=" ", names=names)
            if analysis:
                mf = ref_model.CouplingsModel(out["model_file"])
                model_accel.install(ref_model, analysis=True)
                try:
                    assert type(mf).__name__ == "MeanFieldCouplingsModel"
                    assert "di" in mf.ecs.columns and np.isfinite(mf.ecs["di"]).all()
                finally:
                    model_accel.uninstall(ref_model)
    finally:
        our_mf.uninstall(ref_mf)
    assert "pair_scores" in twins
    slow, fast = raws[False], raws[True]
    assert len(fast) == 276
    pd.testing.assert_frame_equal(fast[["i", "A_i", "j", "A_j"]], slow[["i", "A_i", "j", "A_j"]])
    np.testing.assert_allclose(fast[names[4:]].to_numpy(), slow[names[4:]].to_numpy(), rtol=0, atol=1e-6)


@needs_reference
def test_uninstall_restores_and_install_all_leaves_the_analysis_alone(ref_model):
    from evcouplings_amd import model_accel, protocol as hip_protocol
    cls = ref_model.CouplingsModel
    before = {name: cls.__dict__[name] for name in ("_calculate_ecs", "double_mut_mat", "to_independent_model")}
    hip_protocol.install_all()
    try:
        assert all(cls.__dict__[name] is attr for name, attr in before.items())
    finally:
        hip_protocol.uninstall_all()
    hip_protocol.install_all(analysis=True)
    try:
        assert cls._calculate_ecs is model_accel.calculate_ecs
        assert cls.__dict__["double_mut_mat"] is model_accel.double_mut_mat
        assert cls.to_independent_model is model_accel.to_independent_model
        import evcouplings.couplings.mean_field as ref_mf
        assert "to_independent_model" in ref_mf.MeanFieldCouplingsModel.__dict__     # its own override stays
    finally:
        hip_protocol.uninstall_all()
    assert all(cls.__dict__[name] is attr for name, attr in before.items())
