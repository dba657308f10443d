"""CPU-side checks of the Boltzmann-machine refinement's layers (plm_bm_fit, DESIGN_NEXT_ROWS.md section 9.7): the binding
against the header, the argument checks of `plm.bm_fit`, the command line, and the numpy twin (tests/bm_twin.py) on an
exactly enumerated model under the schedule and the condition that the GPU test uses."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm_twin as bt  # noqa: E402
from evcouplings_amd import _lib, model_accel, model_io, plm  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN_MODEL = os.path.join(HERE, "golden", "hip_fit_L24.model")
CTYPES = {"int32_t": C.c_int32, "float": C.c_float, "double": C.c_double, "uint64_t": C.c_uint64}


def _header_struct(name):
    """[(field, ctypes type)] of `typedef struct { ... } name;` in include/plm_hip.h."""
    text = open(os.path.join(ROOT, "include", "plm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, text).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)$", decl)
        assert m, decl
        fields.append((m.group(3), C.c_void_p if m.group(2) else CTYPES[m.group(1)]))
    return fields


@pytest.mark.parametrize("name,cls", [("plm_bm_opts", "PlmBmOpts"), ("plm_bm_result", "PlmBmResult")])
def test_binding_matches_the_header_field_for_field(name, cls):
    declared = _header_struct(name)
    bound = list(getattr(_lib, cls)._fields_)
    assert [f for f, _ in bound] == [f for f, _ in declared]
    assert [t for _, t in bound] == [t for _, t in declared]
    assert "plm_bm_fit" in {n for n, _, _ in _lib.SYMBOLS}
    assert hasattr(_lib.load(), "plm_bm_fit")
    assert _lib.PlmBmOpts.seed.offset == 40 and _lib.PlmBmOpts.start.offset == 48 and C.sizeof(_lib.PlmBmOpts) == 56
    assert _lib.PlmBmResult.epochs_done.offset == 40 and C.sizeof(_lib.PlmBmResult) == 48


def _small():
    rng = np.random.default_rng(2)
    L, q = 4, 3
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    fi = np.full((L, q), 1.0 / q, np.float32)
    fij = np.full((L * (L - 1) // 2, q, q), 1.0 / (q * q), np.float32)
    return L, q, h, J, fi, fij


def test_bm_fit_rejects_bad_arguments_before_the_library(monkeypatch):
    L, q, h, J, fi, fij = _small()

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError):
        plm.bm_fit(fi, fij[:-1], q, h, J, 8, 2)
    with pytest.raises(ValueError):
        plm.bm_fit(fi, fij, q, h, J, 8, 2, start=np.zeros((7, L), np.int8))
    with pytest.raises(ValueError):
        plm.bm_fit(fi, fij, q, h, J, 8, 2, lr=-0.1)
    with pytest.raises(ValueError):
        plm.bm_fit(fi, fij, q, h, J, 8, 0)
    with pytest.raises(ValueError):
        plm.bm_fit(fi, fij, q, h, J[:-1], 8, 2)
    with pytest.raises(ValueError):
        plm.bm_fit(fi[:-1], fij, q, h, J, 8, 2)
    with pytest.raises(ValueError):
        plm.bm_fit(fi, fij, q, h, J, 8, 2, tol=float("nan"))
    with pytest.raises(ValueError):
        plm.bm_fit(fi, fij, q, h, J, 8, 2, sweeps_per_epoch=0)


def test_no_cpu_fallback_without_a_gpu():
    L, q, h, J, fi, fij = _small()
    if _lib.load().plm_device_count() > 0:
        pytest.skip("GPU present: the refusal without a device cannot be seen here")
    with pytest.raises(_lib.PlmError):                       # no CPU path: the entry point raises
        plm.bm_fit(fi, fij, q, h, J, 8, 2)


def test_command_line_parser_and_file(monkeypatch, tmp_path):
    from evcouplings_amd import bm_refine
    a = bm_refine.parser().parse_args(["in.model", "-o", "out.model", "--epochs", "7", "--chains", "99", "--sweeps", "3",
                                       "--lr", "0.25", "--decay-after", "4", "--seed", "11"])
    assert (a.model, a.o, a.epochs, a.chains, a.sweeps, a.lr, a.decay_after, a.seed) == \
        ("in.model", "out.model", 7, 99, 3, 0.25, 4, 11)
    with pytest.raises(SystemExit):
        bm_refine.parser().parse_args(["in.model"])
    # the whole command with the twin in place of the library: only h_i and J_ij of the file change
    seen = {}

    def twin(*args, **kwargs):
        seen.update(kwargs, n_chains=args[5], n_epochs=args[6])
        return bt.bm_fit(*args, **kwargs)

    monkeypatch.setattr(plm, "bm_fit", twin)
    out = str(tmp_path / "refined.model")
    assert bm_refine.main([GOLDEN_MODEL, "-o", out, "--epochs", "2", "--chains", "64", "--sweeps", "1", "--seed", "3"]) == 0
    m, r = model_io.read_model_file(GOLDEN_MODEL), model_io.read_model_file(out)
    assert seen["n_chains"] == 64 and seen["n_epochs"] == 2 and seen["lr_decay_after"] == 1 and seen["seed"] == 3
    assert seen["lambda_h"] == pytest.approx(m["lambda_h"] / m["n_eff"]) and seen["lambda_j"] == pytest.approx(m["lambda_j"] / m["n_eff"])
    a, b = open(GOLDEN_MODEL, "rb").read(), open(out, "rb").read()
    L, q = m["L"], m["q"]
    head = 40 + q + 4 * (m["n_valid"] + m["n_invalid"]) + 5 * L + 4 * L * q          # up to and with f_i
    pairs = 4 * L * (L - 1) // 2 * q * q
    assert len(a) == len(b) and a[:head] == b[:head]
    assert a[head + 4 * L * q:head + 4 * L * q + pairs] == b[head + 4 * L * q:head + 4 * L * q + pairs]      # f_ij
    assert not np.array_equal(m["hi"], r["hi"]) and not np.array_equal(m["jij"], r["jij"])


def test_refine_model_takes_a_couplings_model_or_a_dict(monkeypatch):
    from types import SimpleNamespace
    calls = []
    monkeypatch.setattr(plm, "bm_fit", lambda *a, **k: calls.append((a, k)) or {})
    m = model_io.read_model_file(GOLDEN_MODEL)
    L, q = m["L"], m["q"]
    iu, ju = np.triu_indices(L, 1)
    dense = {}
    for key in ("fij", "jij"):
        d = np.zeros((L, L, q, q), np.float32)
        d[iu, ju] = m[key]
        d[ju, iu] = m[key].transpose(0, 2, 1)
        dense[key] = d
    obj = SimpleNamespace(f_i=m["fi"], h_i=m["hi"], f_ij=dense["fij"], J_ij=dense["jij"], lambda_h=m["lambda_h"],
                          lambda_J=m["lambda_j"], N_eff=m["n_eff"])
    model_accel.refine_model(m, n_chains=16, n_epochs=10)
    model_accel.refine_model(obj, n_chains=16, n_epochs=10)
    (a1, k1), (a2, k2) = calls
    for u, v in zip(a1[:5], a2[:5]):
        assert np.array_equal(u, v)
    assert a1[5:] == a2[5:] == (16, 10) and k1 == k2 and k1["lr_decay_after"] == 5
    assert k1["lambda_h"] == pytest.approx(0.01 / m["n_eff"], rel=1e-6)


def test_twin_counts_and_update():
    rng = np.random.default_rng(4)
    Cn, L, q = 200, 6, 5
    x = rng.integers(0, q, size=(Cn, L))
    ni, nij = bt.counts(x, q)
    assert ni.sum(axis=1).tolist() == [Cn] * L and nij.sum(axis=(1, 2)).tolist() == [Cn] * (L * (L - 1) // 2)
    k = 0
    for i in range(L):
        for j in range(i + 1, L):
            ref = np.zeros((q, q), np.int64)
            np.add.at(ref, (x[:, i], x[:, j]), 1)
            assert np.array_equal(nij[k], ref)
            k += 1
    assert bt.step_size(0.5, 0, 10) == np.float32(0.5) and bt.step_size(0.5, 4, 3) == np.float32(0.5)
    assert bt.step_size(0.5, 4, 4) == np.float32(0.4)
    xs = rng.normal(size=7).astype(np.float32)
    assert bt.update(xs, xs, xs, 0.0, 0.3).tobytes() == xs.tobytes()
    f, p = rng.random(7).astype(np.float32), rng.random(7).astype(np.float32)
    want = xs.astype(np.float64) + 0.25 * ((f.astype(np.float64) - p) - 2 * 0.125 * xs)
    assert np.abs(bt.update(xs, f, p, 0.25, 0.125) - want).max() < 1e-6


def test_twin_converges_on_the_enumerable_model():
    """The schedule and the condition of the GPU test (tests/test_gpu_bm.py): the exact pair marginals of the fitted
    model miss the targets by at most 0.1 x the error of the independent-site start point (0.0976)."""
    case = bt.enumerable_case()
    err0 = bt.max_pair_error(case["h0"], case["J0"], case["fij"], 4)
    assert abs(err0 - 0.0976) < 5e-4, err0
    res = bt.bm_fit(case["fi"], case["fij"], 4, case["h0"], case["J0"], **bt.ENUM_SCHEDULE)
    err = bt.max_pair_error(res["hi"], res["jij"], case["fij"], 4)
    print("start point %.5f, refined %.5f" % (err0, err))
    assert res["status"] == "maxiter" and res["epochs_done"] == 300 and res["trace"].shape == (300, 4)
    assert err <= 0.1 * err0, (err, err0)
