"""
The drop-in for the mutate stage's `predict_mutation_table` (model_accel.install(mutations=True), DESIGN_NEXT_ROWS.md
section 9.16) behind the REFERENCE's own modules, against the unpatched reference.  `plm.mutant_effects` stands on its
numpy twin here (no GPU); everything else is the real host code and the real reference code.  Skipped where the
reference tree is absent.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutants_twin as mt  # noqa: E402
import refstubs  # noqa: E402

pytestmark = pytest.mark.skipif(not refstubs.reference_available(), reason="reference tree not present")


@pytest.fixture(scope="module")
def ref():
    refstubs.install()
    import evcouplings.mutate.calculations as mc
    import evcouplings.mutate.protocol as mp
    from evcouplings.couplings.model import CouplingsModel
    return dict(mc=mc, mp=mp, CouplingsModel=CouplingsModel)


@pytest.fixture()
def model(ref, golden_dir, monkeypatch):
    from evcouplings_amd import plm
    monkeypatch.setattr(plm, "mutant_effects", mt.mutant_effects)
    return ref["CouplingsModel"](os.path.join(golden_dir, "hip_fit_L24.model"))


def _same(got, want, column):
    assert list(got.columns) == list(want.columns) and got.index.equals(want.index)
    g, w = got[column].to_numpy(float), want[column].to_numpy(float)
    assert np.array_equal(np.isnan(g), np.isnan(w))
    # float32 parameters either way; the numba-less reference loop sums the field part in float32
    np.testing.assert_allclose(g, w, rtol=1e-6, atol=1e-6, equal_nan=True)
    for c in want.columns:
        if c != column:
            assert got[c].equals(want[c])


def _table(m):
    import pandas as pd
    t, ix = m.target_seq, m.index_list
    rows = ["%s%dW" % (t[2], ix[2]), "%s%dK,%s%dD" % (t[10], ix[10], t[21], ix[21]), "wild", "WT", "",
            "%s%dA,%s%dC,%s%d-" % (t[0], ix[0], t[23], ix[23], t[7], ix[7]),
            "%s%dW" % (t[2], ix[0] - 1),                      # position outside the model
            "%s%dX" % (t[2], ix[2]),                          # letter outside the alphabet
            "%s%dW" % ("W" if t[3] != "W" else "A", ix[3]),   # wrong from-letter
            "%s%d%s" % (t[5], ix[5], t[5])]                   # the target's own letter
    return pd.DataFrame({"mutant": rows, "effect": np.arange(len(rows), dtype=float)})


def test_predict_mutation_table_against_the_reference(ref, model):
    from evcouplings_amd import model_accel
    table = _table(model)
    for hamiltonian in ("full", "couplings", "fields"):
        want = ref["mc"].predict_mutation_table(model, table, "prediction_epistatic", hamiltonian=hamiltonian)
        got = model_accel.predict_mutation_table(model, table, "prediction_epistatic", hamiltonian=hamiltonian)
        _same(got, want, "prediction_epistatic")
        assert np.isnan(want["prediction_epistatic"]).sum() == 3
    # the index as the mutant column, another output column
    by_index = table.set_index("mutant")
    _same(model_accel.predict_mutation_table(model, by_index, "dE", mutant_column=None),
          ref["mc"].predict_mutation_table(model, by_index, "dE", mutant_column=None), "dE")
    # the table itself is not written to
    assert list(table.columns) == ["mutant", "effect"]
    # the reference's ValueErrors
    for fn in (ref["mc"].predict_mutation_table, model_accel.predict_mutation_table):
        with pytest.raises(ValueError):
            fn(model, table, hamiltonian="other")
        with pytest.raises(ValueError):
            fn(model, table.assign(mutant=["A1x2B"] * len(table)))


def test_predict_mutation_table_with_segments(ref, model):
    """a model numbered by (segment, position): the `segment` column of the table, and the `segment` argument"""
    import pandas as pd
    from evcouplings_amd import model_accel
    t = model.target_seq
    model.index_list = [("A_1", 10 + k) for k in range(12)] + [("B_1", 100 + k) for k in range(12)]
    table = pd.DataFrame({
        "mutant": ["%s12W" % t[2], "%s20K,%s105D" % (t[10], t[17]), "wild", "%s100A,%s101C" % (t[12], t[13]), "%s12W" % t[2]],
        "segment": ["A_1", "A_1,B_1", "A_1", "B_1,B_1", "B_1"],
    })
    want = ref["mc"].predict_mutation_table(model, table, "prediction_epistatic")
    _same(model_accel.predict_mutation_table(model, table, "prediction_epistatic"), want, "prediction_epistatic")
    assert np.isnan(want["prediction_epistatic"]).tolist() == [False, False, False, False, True]
    plain = table.drop(columns="segment").iloc[[0, 2]]
    want = ref["mc"].predict_mutation_table(model, plain, "prediction_epistatic", segment="A_1")
    _same(model_accel.predict_mutation_table(model, plain, "prediction_epistatic", segment="A_1"), want, "prediction_epistatic")
    assert not np.isnan(want["prediction_epistatic"]).any()
    # a segment column with a null is ignored, as the reference ignores it
    holes = table.assign(segment=["A_1", None, "A_1", "B_1,B_1", "B_1"])
    want = ref["mc"].predict_mutation_table(model, holes, "prediction_epistatic")
    _same(model_accel.predict_mutation_table(model, holes, "prediction_epistatic"), want, "prediction_epistatic")


def test_install_rebinds_both_modules_and_uninstall_restores_them(ref, model):
    from evcouplings_amd import model_accel, protocol as hip_protocol
    import evcouplings.couplings.model as ref_model
    mc, mp = ref["mc"], ref["mp"]
    original = mc.predict_mutation_table
    assert mp.predict_mutation_table is original
    table = _table(model)
    want = original(model, table, "prediction_epistatic")
    model_accel.install()                                      # as before: the table function is left alone
    try:
        assert mc.predict_mutation_table is original and mp.predict_mutation_table is original
    finally:
        model_accel.uninstall()
    for install, uninstall in ((lambda: model_accel.install(mutations=True), model_accel.uninstall),
                               (lambda: hip_protocol.install_all(mutations=True), hip_protocol.uninstall_all)):
        install()
        try:
            assert mc.predict_mutation_table is model_accel.predict_mutation_table
            assert mp.predict_mutation_table is model_accel.predict_mutation_table
            assert ref_model._hamiltonians.__module__ == "evcouplings_amd.model_accel"
            got = mc.predict_mutation_table(model, table, "prediction_epistatic")
            install()                                          # twice: the originals are kept
        finally:
            uninstall()
        assert mc.predict_mutation_table is original and mp.predict_mutation_table is original
        assert ref_model._hamiltonians.__module__ != "evcouplings_amd.model_accel"
        _same(got, want, "prediction_epistatic")


def test_delta_hamiltonians_against_the_reference(model):
    from evcouplings_amd import model_accel
    t, ix = model.target_seq, model.index_list
    subs = [[(ix[2], t[2], "W")], [], [(ix[10], t[10], "K"), (ix[21], t[21], "D"), (ix[0], t[0], "-")], [(ix[2], "?", "W")],
            [(ix[2] + 100, t[2], "W")]]
    got = model_accel.delta_hamiltonians(model, subs)
    for row, s in zip(got, subs):
        try:
            want = model.delta_hamiltonian(s)
        except ValueError:
            assert np.isnan(row).all()
            continue
        np.testing.assert_allclose(row, want, rtol=1e-6, atol=1e-6)
