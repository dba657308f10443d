"""The model level and the command line of sequence optimisation (model_accel.optimize_sequences, model_accel.local_optima,
python -m evcouplings_amd.design; DESIGN_NEXT_ROWS.md section 9.13).  Without a GPU: the argument checks, and the wrappers
with plm.anneal and plm.sample replaced by their numpy twins.  On the GPU: the command line through the library."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anneal_twin as an  # noqa: E402
import sampler_twin as tw  # noqa: E402
from evcouplings_amd import design, model_accel, model_io, plm  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = os.path.join(ROOT, "golden", "hip_fit_L24.model")
GOLDEN_A2M = os.path.join(ROOT, "golden", "hip_fit_L24.a2m")


def _twins(monkeypatch):
    monkeypatch.setattr(plm, "anneal", an.anneal)
    monkeypatch.setattr(plm, "sample", tw.sample)


def _toy_model():
    rng = np.random.default_rng(3)
    L, q = 4, 3
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(scale=0.5, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    return SimpleNamespace(J_ij=tw.dense(J, L, q).astype(np.float32), h_i=h, alphabet=np.array(list("-AC")),
                           target_seq=np.array(list("CA-C")), index_list=np.array([10, 11, 13, 14]), L=L, q=q)


@pytest.mark.parametrize("argv", [
    ["m", "-o", "x"],                                         # no -n
    ["m", "-n", "0", "-o", "x"],
    ["m", "-n", "4"],                                         # no -o
    ["m", "-n", "4", "-o", "x", "--steps", "-1"],
    ["m", "-n", "4", "-o", "x", "--steps", "0", "--greedy", "0"],
    ["m", "-n", "4", "-o", "x", "--sweeps", "0"],
    ["m", "-n", "4", "-o", "x", "--beta-min", "0"],
    ["m", "-n", "4", "-o", "x", "--beta-min", "2", "--beta-max", "1"],
    ["m", "-n", "4", "-o", "x", "--top", "0"],
    ["m", "-n", "4", "-o", "x", "--fix", "3,x"],
    ["m", "-n", "4", "-o", "x", "--start", "elsewhere"],
    ["m", "-o", "x", "--from", "a", "--steps", "5"],
    ["m", "-o", "x", "--from", "a", "--top", "3"],
    ["m", "-o", "x", "--from", "a", "--start", "target"],
])
def test_arguments_that_are_refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        design.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_arguments_that_are_taken():
    a = design.parse_args(["m", "-n", "4", "-o", "x"])
    assert (a.steps, a.sweeps, a.greedy, a.beta_min, a.beta_max, a.fixed, a.start) == (100, 1, 100, 0.1, 4.0, [], "random")
    a = design.parse_args(["m", "-o", "x", "--from", "a.a2m", "--fix", "3, 7", "--no-gaps"])
    assert (a.steps, a.from_a2m, a.fixed, a.no_gaps) == (0, "a.a2m", [3, 7], True)
    assert design.parse_args(["m", "-n", "4", "-o", "x", "--steps", "0"]).steps == 0


def test_optimize_sequences_on_the_twin(monkeypatch):
    _twins(monkeypatch)
    m = _toy_model()
    jij = model_accel._pairs_from_dense(m.J_ij)
    seqs, en, chains, info = model_accel.optimize_sequences(m, 60, n_steps=6, seed=2, info=True)
    # distinct rows, sorted by H descending, the counts those of the chains' best states
    assert len(set("".join(r) for r in seqs)) == len(seqs) and (np.diff(en[:, 0]) <= 0).all() and chains.sum() == 60
    best = m.alphabet[info["best"].astype(np.int64)]
    for row, e, c in zip(seqs, en, chains):
        hit = (best == row).all(axis=1)
        assert hit.sum() == c and np.allclose(info["best_energies"][hit], e)
    st = tw.all_states(4, 3)
    H = tw.hamiltonians(st, m.h_i.astype(np.float64), tw.dense(jij, 4, 3))[:, 0]
    assert "".join(seqs[0]) == "".join(m.alphabet[st[np.argmax(H)]]) and abs(en[0, 0] - H.max()) < 1e-5
    raw = model_accel.optimize_sequences(m, 60, n_steps=6, seed=2, as_letters=False, top=2)
    assert raw[0].dtype == np.int8 and np.array_equal(m.alphabet[raw[0]], seqs[:2]) and len(raw[2]) == 2
    # fixed positions keep the target's residue, even an excluded one; excluded letters appear nowhere else
    seqs, en, chains = model_accel.optimize_sequences(m, 40, n_steps=4, seed=1, fixed=[13, 10], exclude="-")
    assert (seqs[:, 2] == "-").all() and (seqs[:, 0] == "C").all() and not (seqs[:, [1, 3]] == "-").any()
    ok = (st[:, 2] == 0) & (st[:, 0] == 2) & (st[:, 1] != 0) & (st[:, 3] != 0)
    assert abs(en[0, 0] - H[ok].max()) < 1e-5
    # ties in H keep the order of the chains: the same model twice gives the same table
    again = model_accel.optimize_sequences(m, 40, n_steps=4, seed=1, fixed=[13, 10], exclude="-")
    assert np.array_equal(again[0], seqs) and np.array_equal(again[2], chains)
    seqs, _, _ = model_accel.optimize_sequences(m, 5, n_steps=0, max_greedy=0 + 3, start="target")
    assert len(seqs) == 1                                     # one start, a deterministic climb
    with pytest.raises(ValueError):
        model_accel.optimize_sequences(m, 5, fixed=[12])
    with pytest.raises(ValueError):
        model_accel.optimize_sequences(m, 5, exclude="X")
    with pytest.raises(ValueError):
        model_accel.optimize_sequences(m, 5, start="elsewhere")


def test_local_optima_on_the_twin(monkeypatch):
    _twins(monkeypatch)
    m = _toy_model()
    st = tw.all_states(4, 3)
    rows = ["".join(r) for r in m.alphabet[st]]
    optima, en, mutations, last_move = model_accel.local_optima(m, rows)
    H = tw.hamiltonians(st, m.h_i.astype(np.float64), tw.dense(model_accel._pairs_from_dense(m.J_ij), 4, 3))[:, 0]
    assert (en[:, 0] >= H - 1e-5).all() and ((mutations == 0) == (last_move == 0)).all()
    assert np.array_equal(mutations, (optima != m.alphabet[st]).sum(axis=1))
    # an optimum is a fixed point: no single-site change raises H, and climbing from it stays there
    again = model_accel.local_optima(m, optima)
    assert np.array_equal(again[0], optima) and not again[2].any() and not again[3].any()
    assert "".join(m.alphabet[st[np.argmax(H)]]) in {"".join(r) for r in optima}
    held = model_accel.local_optima(m, rows, fixed=[11], as_letters=False)
    assert np.array_equal(held[0][:, 1], st[:, 1])            # the sequence's own residue stays
    with pytest.raises(ValueError):
        model_accel.local_optima(m, ["CA-"])
    with pytest.raises(ValueError):
        model_accel.local_optima(m, ["CAXC"])


def _check_outputs(out, csv, m, n_max):
    lines = open(out).read().splitlines()
    assert lines[0] == ">GOLD/%d-%d" % (int(m["index_list"][0]), int(m["index_list"][-1])) and lines[1] == m["target_seq"]
    seqs = lines[3::2]
    assert 1 <= len(seqs) <= n_max and lines[2] == ">sample1/1-%d" % m["L"]
    rows = open(csv).read().splitlines()
    assert rows[0] == "id,H,H_J,H_h,chains,mutations" and len(rows) == 1 + len(seqs) and rows[1].startswith("sample1,")
    code = {a: k for k, a in enumerate(m["alphabet"])}
    x = np.array([[code[c] for c in row] for row in seqs])
    en = tw.hamiltonians(x, m["hi"].astype(np.float64), tw.dense(m["jij"], m["L"], m["q"]))
    table = np.array([[float(v) for v in r.split(",")[1:]] for r in rows[1:]])
    assert np.allclose(en, table[:, :3], atol=1e-4)
    assert np.array_equal(table[:, 4], [sum(a != b for a, b in zip(row, m["target_seq"])) for row in seqs])
    return seqs, table


def _run_design(tmp_path):
    m = model_io.read_model_file(GOLDEN_MODEL)
    out, csv = str(tmp_path / "d.a2m"), str(tmp_path / "d.csv")
    fix = [int(m["index_list"][3]), int(m["index_list"][20])]
    rc = design.main([GOLDEN_MODEL, "-n", "24", "-o", out, "--steps", "5", "--sweeps", "1", "--greedy", "20", "--seed", "5",
                      "--no-gaps", "--fix", "%d,%d" % tuple(fix), "--top", "6", "--energies", csv, "--id", "GOLD"])
    assert rc == 0
    seqs, table = _check_outputs(out, csv, m, 6)
    assert len(set(seqs)) == len(seqs) and (np.diff(table[:, 0]) <= 0).all() and table[:, 3].sum() <= 24
    gap = m["alphabet"][0]
    for row in seqs:
        assert row[3] == m["target_seq"][3] and row[20] == m["target_seq"][20]
        assert all(c != gap for k, c in enumerate(row) if k not in (3, 20))
    # --from: greedy ascent from the sequences of an alignment, one optimum per record, in the order of the input
    few = str(tmp_path / "few.a2m")
    with open(few, "w") as f:
        f.write("\n".join(open(GOLDEN_A2M).read().splitlines()[:2 * 9]) + "\n")
    rc = design.main([GOLDEN_MODEL, "-o", out, "--from", few, "--greedy", "50", "--energies", csv, "--id", "GOLD"])
    assert rc == 0
    seqs, table = _check_outputs(out, csv, m, 9)
    assert len(seqs) == 9 and (table[:, 3] == 1).all()
    assert seqs[0] != m["target_seq"] or table[0, 4] == 0


def test_command_line_on_the_twin(monkeypatch, tmp_path):
    _twins(monkeypatch)
    _run_design(tmp_path)


@pytest.mark.gpu
def test_command_line_on_the_gpu(tmp_path):
    _run_design(tmp_path)
