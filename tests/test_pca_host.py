"""CPU-side checks of the principal components of an alignment: the numpy twin (tests/pca_twin.py) against hand
calculations, trace and variance identities, the argument checks of the library that run before it looks for a device,
and the files and command line of evcouplings_amd.pca on twin outputs."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_twin as twin  # noqa: E402

from evcouplings_amd import _lib, pca, plm  # noqa: E402

HAND = np.array([[0, 1, 2, 0],
                 [0, 1, 2, 1],
                 [1, 1, 0, 2],
                 [2, 0, 2, 0],
                 [0, 1, 2, 0],
                 [1, 2, 1, 1],
                 [2, 2, 2, 2]], dtype=np.int8)
HAND_W = np.array([1.0, 0.5, 0.25, 1.0, 0.0, 0.125, 0.75], dtype=np.float32)


# ---- the twin against hand calculations

@pytest.mark.parametrize("ones,zeros", [(4, 4), (3, 5), (1, 7)])
def test_two_perfectly_correlated_binary_columns(ones, zeros):
    """x_1 = x_2 with p = P(1): both features of a site are +-(x - p), so C = p (1 - p) s s^T with s = (-1, 1, -1, 1):
    one eigenvalue 4 p (1 - p) with eigenvector +-s / 2, every other eigenvalue 0.  (The four magnitudes tie, so the
    sign rule is decided by the last bit here: the vector is compared up to its sign.)"""
    msa = np.array([[1, 1]] * ones + [[0, 0]] * zeros, np.int8)
    p = ones / (ones + zeros)
    r = twin.fit(msa, 2, 2)
    assert abs(r["eigenvalues"][0] - 4 * p * (1 - p)) <= 4e-16
    assert np.abs(r["spectrum"][1:]).max() <= 4e-16
    v = r["components"][0].reshape(-1)
    np.testing.assert_allclose(v * np.sign(v[0]), [0.5, -0.5, 0.5, -0.5], rtol=0, atol=1e-15)
    assert v[int(np.argmax(np.abs(v)))] > 0
    assert abs(r["total_variance"] - 4 * p * (1 - p)) <= 4e-16
    # without state 0 two features are left: C = p (1 - p) [[1, 1], [1, 1]]
    r = twin.fit(msa, 2, 1, skip_state=0)
    assert abs(r["eigenvalues"][0] - 2 * p * (1 - p)) <= 4e-16
    np.testing.assert_allclose(r["components"][0], [[0, np.sqrt(0.5)], [0, np.sqrt(0.5)]], rtol=0, atol=1e-15)


@pytest.mark.parametrize("q", [2, 3, 4])
def test_a_full_product_design_is_block_diagonal(q):
    """Every combination once: the sites are independent, C is block-diagonal with the single-site block
    diag(1/q) - 1/q^2, whose eigenvalues are 1/q (q - 1 times) and 0.  eigh is backward stable: its eigenvalues are
    off by a small multiple of D 2^-52 |C|, and |C| = 1/q <= 1 here; 4 D 2^-52 leaves that multiple room."""
    L = 3
    msa = np.array(list(itertools.product(range(q), repeat=L)), dtype=np.int8)
    r = twin.fit(msa, q, 1)
    C = r["C"]
    for i, j in itertools.permutations(range(L), 2):
        assert np.abs(C[i * q:(i + 1) * q, j * q:(j + 1) * q]).max() <= 1e-16
    want = np.sort(np.array(([1.0 / q] * (q - 1) + [0.0]) * L))[::-1]
    np.testing.assert_allclose(r["spectrum"], want, rtol=0, atol=4 * L * q * 2.0 ** -52)


def test_a_conserved_alignment_has_no_variance():
    msa = np.full((9, 4), 2, np.int8)
    r = twin.fit(msa, 4, 2, weights=np.linspace(0.1, 1, 9).astype(np.float32))
    assert (r["C"] == 0).all() and (r["spectrum"] == 0).all() and r["total_variance"] == 0.0
    assert (twin.project(msa, 4, r["mean"], r["components"]) == 0).all()


@pytest.mark.parametrize("weights", [None, HAND_W])
@pytest.mark.parametrize("skip", [None, 0, 2])
def test_trace_and_score_variance(weights, skip):
    r = twin.fit(HAND, 3, 3, weights, skip)
    assert abs(np.trace(r["C"]) - r["total_variance"]) <= 12 * 2.0 ** -52
    assert abs(r["spectrum"].sum() - r["total_variance"]) <= 12 * 2.0 ** -52
    t = twin.project(HAND, 3, r["mean"], r["components"], skip)
    mean, var = twin.weighted_moments(t, r["wq"])
    assert np.abs(mean).max() <= 12 * 2.0 ** -52
    np.testing.assert_allclose(var, r["eigenvalues"], rtol=0, atol=12 * 2.0 ** -52)
    gram = r["components"].reshape(3, -1) @ r["components"].reshape(3, -1).T
    np.testing.assert_allclose(gram, np.eye(3), rtol=0, atol=12 * 2.0 ** -52)
    if skip is not None:
        assert (r["components"][:, :, skip] == 0).all()


def test_projection_formula_by_hand():
    mean = np.array([[0.25, 0.75], [0.5, 0.5]])
    comp = np.array([[[1.0, 2.0], [3.0, 5.0]]])
    t = twin.project(np.array([[0, 0], [1, 0], [1, 1]], np.int8), 2, mean, comp)
    offset = 0.25 * 1 + 0.75 * 2 + 0.5 * 3 + 0.5 * 5
    np.testing.assert_array_equal(t[:, 0], [1 + 3 - offset, 2 + 3 - offset, 2 + 5 - offset])
    t = twin.project(np.array([[0, 0], [1, 1]], np.int8), 2, mean, comp, skip_state=0)
    np.testing.assert_array_equal(t[:, 0], [0 - (0.75 * 2 + 0.5 * 5), 2 + 5 - (0.75 * 2 + 0.5 * 5)])


def test_sign_rule():
    np.testing.assert_array_equal(twin.sign_rule([0.1, -0.7, 0.7]), [-0.1, 0.7, -0.7])      # the tie: index 1 decides
    np.testing.assert_array_equal(twin.sign_rule([0.1, 0.7, -0.7]), [0.1, 0.7, -0.7])


# ---- the library's argument checks: they run before the device is looked at, so they are the same on every machine

def _einval(call, word):
    with pytest.raises(_lib.PlmError) as err:
        call()
    assert err.value.code == -1 and word in str(err.value), str(err.value)


def test_bad_fit_arguments_are_refused_before_the_device_is_looked_at():
    fit = lambda m, q=3, **kw: plm.pca_fit(m, q, **kw)      # noqa: E731
    _einval(lambda: fit(np.zeros((0, 4), np.int8)), "n_seqs")
    _einval(lambda: fit(np.zeros((3, 0), np.int8)), "n_sites")
    _einval(lambda: fit(HAND, 1), "2..32")
    _einval(lambda: fit(HAND, 33), "2..32")
    _einval(lambda: fit(HAND, 2), "outside 0..1")                        # HAND holds state 2
    _einval(lambda: fit(-HAND), "outside 0..2")
    _einval(lambda: fit(HAND, k=0), "n_components")
    _einval(lambda: fit(HAND, k=13), "n_components")                     # D = 4 * 3 = 12
    _einval(lambda: fit(HAND, k=9, skip_state=0), "n_components")        # D = 4 * 2 = 8
    _einval(lambda: fit(np.zeros((4, 40), np.int8), k=65), "n_components")
    _einval(lambda: fit(HAND, oversample=-1), "oversample")
    _einval(lambda: fit(HAND, skip_state=3), "skip_state")
    _einval(lambda: fit(HAND, skip_state=-2), "skip_state")
    _einval(lambda: fit(HAND, tol=0.0), "tol")
    _einval(lambda: fit(HAND, tol=-1e-3), "tol")
    _einval(lambda: fit(HAND, tol=float("nan")), "tol")
    _einval(lambda: fit(HAND, max_iter=0), "max_iter")
    _einval(lambda: fit(HAND, weights=-HAND_W), "negative")
    _einval(lambda: fit(HAND, weights=np.where(HAND_W > 0.9, np.nan, HAND_W)), "finite")
    _einval(lambda: fit(HAND, weights=np.where(HAND_W > 0.9, np.inf, HAND_W)), "finite")
    _einval(lambda: fit(HAND, weights=np.zeros(len(HAND), np.float32)), "W = 0")
    _einval(lambda: fit(HAND, weights=np.full(len(HAND), 1e-30, np.float32)), "W = 0")
    with pytest.raises(ValueError):
        fit(HAND, weights=HAND_W[:3])


def test_bad_projection_arguments_are_refused_before_the_device_is_looked_at():
    mean = np.full((4, 3), 1 / 3)
    comp = np.zeros((2, 4, 3))
    comp[0, 0, 0] = comp[1, 1, 1] = 1.0
    proj = lambda s, q=3, m=mean, c=comp, **kw: plm.pca_project(s, q, m, c, **kw)      # noqa: E731
    _einval(lambda: proj(np.zeros((0, 4), np.int8)), "n must be")
    _einval(lambda: proj(-HAND), "outside 0..2")
    _einval(lambda: proj(HAND, skip_state=3), "skip_state")
    _einval(lambda: proj(HAND, c=np.zeros((0, 4, 3))), "k = 0")
    _einval(lambda: proj(HAND, c=np.zeros((13, 4, 3))), "k = 13")
    _einval(lambda: proj(HAND, m=np.where(np.arange(12).reshape(4, 3) == 5, np.nan, mean)), "mean[5]")
    bad = comp.copy()
    bad[1, 2, 0] = np.inf
    _einval(lambda: proj(HAND, c=bad), "components[18]")
    _einval(lambda: plm.pca_project(HAND, 33, np.zeros((4, 33)), np.zeros((1, 4, 33))), "2..32")
    with pytest.raises(ValueError):
        proj(HAND, m=mean[:3])
    with pytest.raises(ValueError):
        proj(HAND, c=comp[:, :3])


def test_null_pointers_are_refused():
    lib = _lib.load()
    opts = _lib.PlmPcaOpts(1, 8, 10, -1, 1e-10, 0)
    out = [np.zeros(12), np.zeros(12), np.zeros(1), np.zeros(1)]
    ptr = [plm._ptr(a) for a in out]
    tail = (None, None, None, None, None, 0, None)
    assert lib.plm_pca_fit(None, None, 7, 4, 3, opts, *ptr, *tail) == -1
    assert lib.plm_pca_fit(plm._ptr(HAND), None, 7, 4, 3, None, *ptr, *tail) == -1
    for missing in range(4):
        args = [None if i == missing else p for i, p in enumerate(ptr)]
        assert lib.plm_pca_fit(plm._ptr(HAND), None, 7, 4, 3, opts, *args, *tail) == -1
    arrays = (HAND, np.zeros(12), np.zeros(12), np.zeros(7))
    for missing in range(4):
        a = [None if i == missing else plm._ptr(x) for i, x in enumerate(arrays)]
        assert lib.plm_pca_project(a[0], 7, 4, 3, a[1], a[2], 1, -1, a[3], 0, None) == -1


@pytest.mark.parametrize("value", ["", "g", "g0", "g-4", "g70000", "s0", "s2000000", "r0", "r70000", "x4", "g2,", ",g2", "g2 s8",
                                   "g2;s8", "u", "s12x"])
def test_a_bad_plan_hook_is_refused_before_the_device_is_looked_at(monkeypatch, value):
    monkeypatch.setenv("PLM_PCA_PLAN", value)
    mean, comp = np.full((4, 3), 1 / 3), np.ones((1, 4, 3))
    for call in (lambda: plm.pca_fit(HAND, 3), lambda: plm.pca_project(HAND, 3, mean, comp)):
        with pytest.raises(_lib.PlmError) as err:
            call()
        assert err.value.code == -1 and "PLM_PCA_PLAN" in str(err.value)


def test_no_cpu_fallback_without_a_gpu(monkeypatch):
    if _lib.load().plm_device_count() > 0:
        pytest.skip("GPU present")
    mean, comp = np.full((4, 3), 1 / 3), np.ones((1, 4, 3))
    for plan in (None, "g2,s8,r3"):
        if plan:
            monkeypatch.setenv("PLM_PCA_PLAN", plan)
        for call in (lambda: plm.pca_fit(HAND, 3, weights=HAND_W), lambda: plm.pca_project(HAND, 3, mean, comp)):
            with pytest.raises(_lib.PlmError) as err:
                call()
            assert err.value.code == -3


# ---- evcouplings_amd.pca: what runs without a device

def _twin_model(k=2, skip=None):
    r = twin.fit(HAND, 3, k, HAND_W, skip)
    t = twin.project(HAND, 3, r["mean"], r["components"], skip)
    return {"mean": r["mean"], "components": r["components"], "eigenvalues": r["eigenvalues"],
            "explained": r["eigenvalues"] / r["total_variance"], "total_variance": r["total_variance"],
            "residuals": np.zeros(k), "iterations": 7, "converged": True, "total": r["total"], "scores": t, "q": 3,
            "skip_state": -1 if skip is None else skip}


def test_npz_round_trip(tmp_path):
    model = _twin_model(skip=0)
    path = pca.save(str(tmp_path / "m.npz"), model)
    back = pca.load(path)
    assert set(back) == set(pca.MODEL_KEYS)
    for key in ("mean", "components", "eigenvalues", "explained", "residuals"):
        np.testing.assert_array_equal(back[key], model[key])
    assert (back["total_variance"], back["iterations"], back["converged"], back["total"], back["q"], back["skip_state"]) == \
        (model["total_variance"], 7, True, model["total"], 3, 0)
    assert type(back["total"]) is int and type(back["converged"]) is bool


def test_command_line_arguments():
    a = pca.parse_args(["nat.a2m", "-o", "out.csv"])
    assert (a.natural, a.samples, a.components, a.theta, a.skip_gap, a.output, a.model) == \
        ("nat.a2m", [], 2, 0.8, False, "out.csv", None)
    a = pca.parse_args(["n", "s1", "s2", "-k", "4", "--theta", "0.9", "--skip-gap", "-o", "o.csv", "--model", "m.npz"])
    assert (a.samples, a.components, a.theta, a.skip_gap, a.output, a.model) == (["s1", "s2"], 4, 0.9, True, "o.csv", "m.npz")
    for bad in (["n"], [], ["n", "-o", "o", "-k", "0"], ["n", "-o", "o", "-k", "65"], ["n", "-o", "o", "--theta", "0"]):
        with pytest.raises(SystemExit):
            pca.parse_args(bad)


def test_table_writer_and_histograms_on_twin_outputs(tmp_path):
    model = _twin_model()
    other = twin.project(HAND[::-1][:3], 3, model["mean"], model["components"])
    path = pca.write_table(str(tmp_path / "t.csv"), [("natural", model["scores"]), ("sample", other)])
    lines = open(path).read().splitlines()
    assert lines[0] == "set,index,t_1,t_2" and len(lines) == 1 + 7 + 3
    cells = lines[8].split(",")
    assert cells[:2] == ["sample", "0"] and [float(c) for c in cells[2:]] == list(other[0])      # %.17g round-trips
    mean, var = pca.weighted_moments(model["scores"], HAND_W)
    assert np.abs(mean).max() <= 1e-15 and np.abs(var - model["eigenvalues"]).max() <= 1e-15
    h_nat, h_sam, overlap, e1, e2 = pca.histogram_overlap(model["scores"], other, HAND_W, bins=5)
    assert h_nat.shape == h_sam.shape == (5, 5) and len(e1) == len(e2) == 6
    assert abs(h_nat.sum() - 1) <= 1e-15 and abs(h_sam.sum() - 1) <= 1e-15 and 0.0 <= overlap <= 1.0
    assert pca.histogram_overlap(model["scores"], model["scores"], None, bins=5)[2] == pytest.approx(1.0)
    far = model["scores"] + 100.0
    assert pca.histogram_overlap(model["scores"], far, None, bins=5)[2] == 0.0
    one = pca.histogram_overlap(model["scores"][:, :1], other[:, :1], None, bins=4)
    assert one[0].shape == (4, 1)
