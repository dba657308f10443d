"""CPU-side checks of the Gibbs sampler's layers: the numpy twin that the GPU tests compare against (known answers of
its Philox block; it leaves an exactly enumerated distribution invariant), the binding, and the model-level and
command-line layers with `plm.sample` replaced by the twin."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_twin as tw  # noqa: E402
from evcouplings_amd import _lib, model_accel, model_io, plm  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = os.path.join(ROOT, "golden", "hip_fit_L24.model")


@pytest.mark.parametrize("counter,key,words", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, words):
    out = tw.philox4x32_10(*counter, *key)
    assert " ".join("%08x" % int(w) for w in out) == words


def test_uniform_is_inside_the_open_interval_and_vectorised():
    u = tw.uniform(0x123456789ABCDEF0, np.arange(1000), 3, 7)
    assert u.shape == (1000,) and (u > 0).all() and (u < 1).all() and len(np.unique(u)) > 990
    assert u[5] == tw.uniform(0x123456789ABCDEF0, 5, 3, 7)
    w0 = tw.philox4x32_10(5, 0, 3, 7, 0x9ABCDEF0, 0x12345678)[0]
    assert u[5] == ((int(w0) >> 8) + 0.5) * 2.0 ** -24


def _small_model(scale=1.0):
    rng = np.random.default_rng(2)
    L, q = 4, 3
    h = rng.normal(scale=scale, size=(L, q))
    J = rng.normal(scale=scale, size=(L * (L - 1) // 2, q, q))
    return L, q, h, J, tw.dense(J, L, q)


def test_twin_leaves_the_enumerated_distribution_invariant():
    L, q, h, J, W = _small_model()
    p = tw.boltzmann(h, W)
    P = tw.transition_matrix(h, W)
    assert np.abs(P.sum(axis=1) - 1).max() < 1e-12 and np.abs(p @ P - p).max() < 1e-15
    Cn = 1 << 16
    rng = np.random.default_rng(3)
    st = tw.all_states(L, q)
    x = st[rng.choice(len(p), size=Cn, p=p)]
    for s in range(20):
        tw.sweep(x, h, W, 777, s)
    chi, dof = tw.chi2_counts(np.bincount(tw.state_index(x, q), minlength=len(p)), p, Cn)
    assert chi < stats.chi2.isf(1e-6, dof), (chi, dof)
    # a sampler that drops the couplings to the last site is seen
    W2 = W.copy()
    W2[:, L - 1] = 0
    W2[L - 1, :] = 0
    x = st[rng.choice(len(p), size=Cn, p=p)]
    for s in range(20):
        tw.sweep(x, h, W2, 777, s)
    chi, dof = tw.chi2_counts(np.bincount(tw.state_index(x, q), minlength=len(p)), p, Cn)
    assert chi > 100 * stats.chi2.isf(1e-6, dof)


def test_twin_masks_and_start_rule():
    L, q, h, J, W = _small_model(0.5)
    allowed = np.array([1, 0, 1], np.uint8)
    fixed = np.array([0, 1, 0, 0], np.uint8)
    x = tw.start_states(h, 5000, 9, allowed=allowed)
    assert not (x == 1).any()
    pi = tw.start_distribution(h, 1.0, allowed)
    chi, dof = tw.chi2_counts(np.bincount(tw.state_index(x, q), minlength=q ** L), pi, 5000)
    assert chi < stats.chi2.isf(1e-6, dof)
    x[:, 1] = 1
    tw.sweep(x, h, W, 9, 0, fixed=fixed, allowed=allowed)
    assert (x[:, 1] == 1).all() and not (x[:, [0, 2, 3]] == 1).any()
    # the conditioned target is invariant under the masked transition matrix
    p = tw.conditioned(tw.boltzmann(h, W), L, q, allowed=allowed, fixed={1: 1})
    assert np.abs(p @ tw.transition_matrix(h, W, allowed=allowed, fixed=fixed) - p).max() < 1e-15
    # chain c of a large call is chain c of a small one
    a, _ = tw.sample(h, J, q, 64, burn_in=2, seed=4)
    b, _ = tw.sample(h, J, q, 16, burn_in=2, seed=4)
    assert np.array_equal(a[0, :16], b[0])


def test_binding_is_declared_and_fails_loudly_without_a_gpu():
    assert "plm_sample" in {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    assert hasattr(lib, "plm_sample")
    assert _lib.PlmSampleOpts.start.offset == 32 and _lib.PlmSampleOpts.seed.offset == 24   # the C struct's layout
    L, q, h, J, W = _small_model()
    if lib.plm_device_count() <= 0:                        # no CPU path: every compute entry point raises
        with pytest.raises(_lib.PlmError):
            plm.sample(h, J, q, 8)


def test_sample_rejects_bad_shapes_before_the_library():
    L, q, h, J, W = _small_model()
    with pytest.raises(ValueError):
        plm.sample(h, J[:-1], q, 8)
    with pytest.raises(ValueError):
        plm.sample(h, J, q + 1, 8)
    with pytest.raises(ValueError):
        plm.sample(h, J, q, 0)
    with pytest.raises(ValueError):
        plm.sample(h, J, q, 8, start=np.zeros((7, L), np.int8))
    with pytest.raises(ValueError):
        plm.sample(h, J, q, 8, fixed=np.zeros(L + 1))
    with pytest.raises(ValueError):
        plm.sample(h, J, q, 8, allowed=np.ones(q + 1))
    with pytest.raises(ValueError):
        plm.sample(h, J, q, 8, thin=0)


def _toy_model():
    L, q, h, J, W = _small_model(0.5)
    return SimpleNamespace(J_ij=W, h_i=h, alphabet=np.array(list("-AC")), target_seq=np.array(list("CA-C")),
                           index_list=np.array([10, 11, 13, 14]), L=L, q=q)


def test_sample_sequences_letters_numbering_and_masks(monkeypatch):
    monkeypatch.setattr(plm, "sample", tw.sample)
    m = _toy_model()
    seqs = model_accel.sample_sequences(m, 50, burn_in=3, seed=1)
    assert seqs.shape == (50, 4) and set(np.unique(seqs)) <= set("-AC")
    raw = model_accel.sample_sequences(m, 50, burn_in=3, seed=1, as_letters=False)
    assert raw.dtype == np.int8 and np.array_equal(m.alphabet[raw], seqs)
    twin, _ = tw.sample(m.h_i, model_accel._pairs_from_dense(m.J_ij), 3, 50, burn_in=3, seed=1)
    assert np.array_equal(raw, twin[0])
    # positions in the model's numbering keep the target's residue, even an excluded one
    seqs = model_accel.sample_sequences(m, 200, burn_in=3, seed=1, fixed=[13, 10], exclude="-")
    assert (seqs[:, 2] == "-").all() and (seqs[:, 0] == "C").all() and not (seqs[:, [1, 3]] == "-").any()
    assert len(np.unique(seqs[:, 1])) == 2
    with pytest.raises(ValueError):
        model_accel.sample_sequences(m, 5, fixed=[12])
    with pytest.raises(ValueError):
        model_accel.sample_sequences(m, 5, exclude="X")
    # start = "target", no sweeps: the target itself; snapshots are stacked; energies on request
    seqs = model_accel.sample_sequences(m, 3, burn_in=0, start="target")
    assert ["".join(r) for r in seqs] == ["CA-C"] * 3
    seqs, en = model_accel.sample_sequences(m, 7, burn_in=1, n_snapshots=3, thin=2, energies=True)
    assert seqs.shape == (21, 4) and en.shape == (21, 3) and np.allclose(en[:, 0], en[:, 1] + en[:, 2])


def test_command_line(monkeypatch, tmp_path):
    from evcouplings_amd import sample as cli
    monkeypatch.setattr(plm, "sample", tw.sample)
    m = model_io.read_model_file(GOLDEN_MODEL)
    out, csv = str(tmp_path / "s.a2m"), str(tmp_path / "e.csv")
    first, last = int(m["index_list"][0]), int(m["index_list"][-1])
    fix = [int(m["index_list"][3]), int(m["index_list"][20])]
    rc = cli.main([GOLDEN_MODEL, "-n", "12", "-o", out, "--burn-in", "2", "--snapshots", "2", "--thin", "1", "--seed", "5",
                   "--beta", "1.5", "--no-gaps", "--fix", "%d,%d" % tuple(fix), "--energies", csv, "--id", "GOLD"])
    assert rc == 0
    lines = open(out).read().splitlines()
    assert len(lines) == 2 * (1 + 24)
    assert lines[0] == ">GOLD/%d-%d" % (first, last) and lines[1] == m["target_seq"]
    assert lines[2] == ">sample1/1-%d" % m["L"] and lines[-2] == ">sample24/1-%d" % m["L"]
    gap = m["alphabet"][0]
    for row in lines[3::2]:
        assert len(row) == m["L"] and set(row) <= set(m["alphabet"])
        assert row[3] == m["target_seq"][3] and row[20] == m["target_seq"][20]
        assert all(c != gap for k, c in enumerate(row) if k not in (3, 20))
    rows = open(csv).read().splitlines()
    assert rows[0] == "id,H,H_J,H_h" and len(rows) == 25 and rows[1].startswith("sample1,")
    # the energies are those of the written sequences
    code = {a: k for k, a in enumerate(m["alphabet"])}
    x = np.array([[code[c] for c in row] for row in lines[3::2]])
    en = tw.hamiltonians(x, m["hi"].astype(np.float64), tw.dense(m["jij"], m["L"], m["q"]))
    assert np.allclose(en, np.array([[float(v) for v in r.split(",")[1:]] for r in rows[1:]]), atol=1e-5)
