"""Mutation tables and combinatorial libraries (plm_mutant_effects, plm_mutant_scan; DESIGN_NEXT_ROWS.md section 9.16)
without a GPU: the binding, the validation that comes before the device check, the numpy twin (tests/mutants_twin.py)
against the reference's fixture, and the model level, the drop-in and the command line with the library calls replaced
by the twin."""
import ctypes as C
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutants_twin as mt  # noqa: E402
from evcouplings_amd import _lib, model_accel, model_io, mutate, plm, sample  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = os.path.join(ROOT, "golden", "hip_fit_L24.model")
GOLDEN_TABLE = os.path.join(ROOT, "golden", "mutation_table_L24.npz")
OK, EINVAL, EDEVICE, EUNSUPPORTED = 0, -1, -3, -4


def golden_model():
    """(file dict, target states) of the fixture model"""
    m = model_io.read_model_file(GOLDEN_MODEL)
    code = {a: k for k, a in enumerate(m["alphabet"])}
    return m, np.array([code[c] for c in m["target_seq"]], np.int8)


def _twins(monkeypatch):
    monkeypatch.setattr(plm, "mutant_effects", mt.mutant_effects)
    monkeypatch.setattr(plm, "mutant_scan", mt.mutant_scan)
    monkeypatch.setattr(plm, "independent_fields", lambda f, lam, n, device=0: (np.log(np.asarray(f, np.float64) + 0.01), None))


# ---- binding and validation --------------------------------------------------------------------------------------

def test_binding_is_declared_and_matches_the_header_layout():
    names = {name for name, _, _ in _lib.SYMBOLS}
    assert {"plm_mutant_effects", "plm_mutant_scan"} <= names
    lib = _lib.load()
    assert hasattr(lib, "plm_mutant_effects") and hasattr(lib, "plm_mutant_scan")
    o, r = _lib.PlmScanOpts, _lib.PlmScanResult
    assert (o.n_scan_sites.offset, o.flags.offset, o.sites.offset, o.letter_offsets.offset, o.letters.offset, o.first.offset,
            o.count.offset, o.edges.offset, o.n_edges.offset, o.use_threshold.offset, o.threshold.offset, o.capacity.offset,
            C.sizeof(o)) == (0, 4, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80)
    assert (r.energies.offset, r.histogram.offset, r.kept_index.offset, r.kept_energies.offset, r.dh_min.offset,
            r.dh_max.offset, r.n_kept.offset, r.n_combinations.offset, C.sizeof(r)) == (0, 8, 16, 24, 32, 40, 48, 56, 64)
    text = open(os.path.join(os.path.dirname(ROOT), "include", "plm_hip.h")).read()
    assert "} plm_scan_opts;" in text and "} plm_scan_result;" in text
    for name, value in (("PLM_MUT_ETOOMANY", _lib.MUT_ETOOMANY), ("PLM_MUT_EPOSITION", _lib.MUT_EPOSITION),
                        ("PLM_MUT_ESTATE", _lib.MUT_ESTATE), ("PLM_MUT_EREPEAT", _lib.MUT_EREPEAT),
                        ("PLM_SCAN_MAX_SITES", _lib.SCAN_MAX_SITES), ("PLM_SCAN_MAX_EDGES", _lib.SCAN_MAX_EDGES)):
        assert "#define %s %d" % (name, value) in text
    assert (mt.ETOOMANY, mt.EPOSITION, mt.ESTATE, mt.EREPEAT) == (_lib.MUT_ETOOMANY, _lib.MUT_EPOSITION, _lib.MUT_ESTATE,
                                                                  _lib.MUT_EREPEAT)
    assert set(plm.MUTANT_STATUS) == {0, 1, 2, 3, 4}


def _model(L=4, q=3):
    rng = np.random.default_rng(1)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    return np.concatenate([h.ravel(), J.ravel()]), np.zeros(L, np.int8)


def test_effects_validation_comes_before_the_device():
    lib = _lib.load()
    x, target = _model()
    off, pos, st = np.array([0, 1, 3], np.int64), np.array([0, 1, 2], np.int32), np.array([1, 2, 0], np.int8)
    out, status = np.zeros((2, 3)), np.zeros(2, np.uint8)
    p = plm._ptr

    def call(L=4, q=3, x=x, target=target, n=2, off=off, n_entries=3, pos=pos, st=st, out=out, status=status):
        return lib.plm_mutant_effects(p(x), L, q, p(target), n, p(off), n_entries, p(pos), p(st), 0, None, p(out), p(status),
                                      None)

    assert call(x=None) == EINVAL and call(target=None) == EINVAL and call(off=None) == EINVAL
    assert call(out=None) == EINVAL and call(status=None) == EINVAL and call(pos=None) == EINVAL and call(st=None) == EINVAL
    assert call(L=1) == EINVAL and call(n=-1) == EINVAL and call(n_entries=-1) == EINVAL
    assert call(q=1) == EUNSUPPORTED and call(q=33) == EUNSUPPORTED
    assert call(target=np.array([0, 3, 0, 0], np.int8)) == EINVAL and call(target=np.array([0, -1, 0, 0], np.int8)) == EINVAL
    assert call(off=np.array([1, 1, 3], np.int64)) == EINVAL                # does not start at 0
    assert call(off=np.array([0, 2, 1], np.int64), n_entries=1) == EINVAL   # decreases
    assert call(off=np.array([0, 1, 2], np.int64)) == EINVAL                # ends before the entries do
    assert call(n_entries=4) == EINVAL
    assert b"offsets" in lib.plm_last_error()
    if lib.plm_device_count() <= 0:                                         # valid calls: no CPU path
        assert call() == EDEVICE
        assert call(n=0, off=np.zeros(1, np.int64), n_entries=0, out=None, status=None) == EDEVICE
        # malformed variants are the kernel's business, not a reason to refuse the call
        assert call(pos=np.array([0, 1, 99], np.int32)) == EDEVICE and call(st=np.array([1, 2, 7], np.int8)) == EDEVICE
    with pytest.raises(ValueError):
        plm.mutant_effects(target, 3, x[:12].reshape(4, 3), x[12:-1], off, pos, st)
    with pytest.raises(ValueError):
        plm.mutant_effects(target[:3], 3, x[:12].reshape(4, 3), x[12:], off, pos, st)
    with pytest.raises(ValueError):
        plm.mutant_effects(target, 3, x[:12].reshape(4, 3), x[12:], off, pos, st[:2])


def test_scan_validation_comes_before_the_device():
    lib = _lib.load()
    x, target = _model()
    p = plm._ptr
    keep = []

    def call(L=4, q=3, sites=(0, 2), letters=None, opts=True, res=True, hist=False, kept=False, **kw):
        s = np.asarray(sites, np.int32)
        f = dict(n_scan_sites=len(s), flags=0, sites=s.ctypes.data, letter_offsets=None, letters=None, first=0, count=1,
                 edges=None, n_edges=0, use_threshold=0, threshold=0.0, capacity=0)
        if letters is not None:
            lo = np.zeros(len(letters) + 1, np.int32)
            lo[1:] = np.cumsum([len(l) for l in letters])
            let = np.array([a for l in letters for a in l], np.int8)
            keep.extend([lo, let])
            f.update(letter_offsets=lo.ctypes.data, letters=let.ctypes.data)
        if "edges" in kw and kw["edges"] is not None:
            e = np.asarray(kw.pop("edges"), np.float64)
            keep.append(e)
            f.update(edges=e.ctypes.data, n_edges=len(e))
        f.update(kw)
        o, r = _lib.PlmScanOpts(**f), _lib.PlmScanResult()
        h, ki, ke = np.zeros(2000, np.uint64), np.zeros(64, np.int64), np.zeros((64, 3))
        keep.extend([s, h, ki, ke])
        if hist:
            r.histogram = h.ctypes.data
        if kept:
            r.kept_index, r.kept_energies = ki.ctypes.data, ke.ctypes.data
        return lib.plm_mutant_scan(p(x), L, q, p(target), C.byref(o) if opts else None, 0, None, C.byref(r) if res else None)

    assert call(opts=False) == EINVAL and call(res=False) == EINVAL
    assert call(q=1) == EUNSUPPORTED and call(q=33) == EUNSUPPORTED and call(L=1) == EINVAL
    assert call(sites=()) == EINVAL and call(sites=(0, 4)) == EINVAL and call(sites=(-1,)) == EINVAL
    assert call(sites=(1, 2, 1)) == EINVAL                                  # a site twice
    assert call(flags=1) == EINVAL
    assert call(letters=[[0, 1], []]) == EINVAL and call(letters=[[0, 3], [1]]) == EINVAL
    assert call(letters=[[0, -1], [1]]) == EINVAL and call(letters=[[1, 1], [0]]) == EINVAL
    assert call(first=-1) == EINVAL and call(count=-1) == EINVAL
    assert call(first=9, count=1) == EINVAL and call(first=5, count=5) == EINVAL and call(first=10, count=0) == EINVAL
    assert call(edges=[0.0, 1.0]) == EINVAL and call(hist=True) == EINVAL   # one without the other
    assert call(edges=[1.0, 0.0], hist=True) == EINVAL and call(edges=[0.0, float("nan")], hist=True) == EINVAL
    assert call(edges=np.zeros(1025), hist=True) == EINVAL and call(n_edges=-1) == EINVAL
    assert call(use_threshold=1, threshold=float("nan")) == EINVAL
    assert call(use_threshold=1, capacity=-1) == EINVAL and call(use_threshold=1, capacity=4) == EINVAL
    # the limits: 8 sites, fewer than 2^62 combinations
    x12, t12 = _model(12, 3)
    big = lambda **kw: lib.plm_mutant_scan(p(x12), 12, 3, p(t12), C.byref(kw["o"]), 0, None, C.byref(_lib.PlmScanResult()))
    s9 = np.arange(9, dtype=np.int32)
    assert big(o=_lib.PlmScanOpts(n_scan_sites=9, sites=s9.ctypes.data, count=1)) == EUNSUPPORTED
    x8 = np.zeros(8 * 32 + 28 * 1024, np.float32)
    t8, s8 = np.zeros(8, np.int8), np.arange(8, dtype=np.int32)

    def library(q, k):
        o = _lib.PlmScanOpts(n_scan_sites=k, sites=s8.ctypes.data, count=1)
        return lib.plm_mutant_scan(p(x8), 8, q, p(t8), C.byref(o), 0, None, C.byref(_lib.PlmScanResult()))

    assert 32 ** 8 < 2 ** 62 and library(32, 8) != EUNSUPPORTED            # 2^40: allowed
    if lib.plm_device_count() <= 0:                                         # valid calls: no CPU path
        assert call() == EDEVICE and call(first=8, count=1) == EDEVICE and call(first=9, count=0) == EDEVICE
        assert call(sites=(3, 1)) == EDEVICE and call(letters=[[2, 0], [1]]) == EDEVICE
        assert call(edges=[0.0, 0.0, 1.0], hist=True) == EDEVICE
        assert call(use_threshold=1, threshold=float("-inf")) == EDEVICE
        assert call(use_threshold=1, capacity=4, kept=True) == EDEVICE
        assert library(32, 8) == EDEVICE
    with pytest.raises(ValueError):
        plm.mutant_scan(target, 3, x[:12].reshape(4, 3), x[12:], [0, 1], letters=[[0]])


def test_scan_digits_follow_itertools_product():
    sizes = [2, 3, 1, 4]
    want = np.array(list(itertools.product(*[range(n) for n in sizes])))
    assert np.array_equal(plm.scan_digits(np.arange(24), sizes), want)
    assert plm.scan_digits(np.array([23]), sizes).tolist() == [[1, 2, 0, 3]]


# ---- the twin against the reference's fixture ----------------------------------------------------------------------

def test_the_twin_agrees_with_the_reference_fixture():
    """every row of tests/golden/mutation_table_L24.npz within 2 n_terms 2^-53 sum_abs, the rejected rows NaN"""
    z = np.load(GOLDEN_TABLE)
    m, target = golden_model()
    n = len(z["offsets"]) - 1
    lens = np.diff(z["offsets"])
    assert 290 <= n <= 310 and set(range(7)) | {12, 24} <= set(lens.tolist())
    out, status, n_terms, sum_abs = mt.mutant_effects(target, m["q"], m["hi"], m["jij"], z["offsets"], z["positions"],
                                                      z["states"], info=True)
    rejected = np.isnan(z["delta"][:, 0])
    assert np.array_equal(rejected, (status != 0) | z["from_mismatch"]) and 6 <= rejected.sum() <= 12
    assert {mt.EPOSITION, mt.ESTATE} <= set(status.tolist()) and z["from_mismatch"].any()
    ok = ~rejected
    err = np.abs(out[ok] - z["delta"][ok])
    print("largest |twin - reference| %.3g, largest share of the bound %.3g" % (
        err.max(), (err.max(axis=1) / np.maximum(mt.bound(n_terms, sum_abs)[ok], 1e-300)).max()))
    assert (err <= mt.bound(n_terms, sum_abs)[ok, None]).all()
    assert np.array_equal(out[ok & (lens == 0)], np.zeros(((ok & (lens == 0)).sum(), 3)))
    # the single tables are the M = 1 rows
    tab = mt.single_tables(target, m["q"], m["hi"], m["jij"])
    one, _ = mt.mutant_effects(target, m["q"], m["hi"], m["jij"], [0, 1], [5], [7])
    assert np.array_equal(one[0], [tab[5, 7, 0] + tab[5, 7, 1], tab[5, 7, 0], tab[5, 7, 1]])
    assert not tab[np.arange(24), target].any()


def test_the_twin_scan_is_the_twin_effects_over_the_product():
    x, target = _model(5, 4)
    h, J = x[:20].reshape(5, 4), x[20:]
    target = np.array([1, 0, 3, 2, 1], np.int8)
    letters = [[2, 0], [1, 3, 0]]
    res = mt.mutant_scan(target, 4, h, J, [3, 0], letters=letters, first=1, count=4, energies=True, edges=[-1.0, 0.0, 1.0],
                         threshold=0.0, info=True)
    combos = list(itertools.product(*letters))[1:5]
    for row, (a, b) in zip(res["energies"], combos):
        want, _, _ = mt.delta(target.astype(int), *mt.dense(h, J, 4), [3, 0], [a, b])
        assert np.array_equal(row, want)
    assert res["n_combinations"] == 6 and res["histogram"].sum() == 4 and res["n_kept"] == (res["energies"][:, 0] >= 0).sum()
    assert np.array_equal(res["kept_index"], 1 + np.nonzero(res["energies"][:, 0] >= 0)[0])
    # ranges deep inside a library are decoded, not walked to: the same members
    assert mt.scan_variants(4, [3, 0, 1], first=7, count=40) == mt.scan_variants(4, [3, 0, 1], first=7, count=40, product_limit=0)
    assert mt.scan_variants(4, [3, 0], letters, 1, 4) == mt.scan_variants(4, [3, 0], letters, 1, 4, product_limit=0)


# ---- the model level ---------------------------------------------------------------------------------------------

def _toy(segments=False):
    rng = np.random.default_rng(3)
    L, q = 4, 3
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = np.zeros((L, L, q, q), np.float32)
    iu, ju = np.triu_indices(L, 1)
    blocks = rng.normal(scale=0.5, size=(len(iu), q, q)).astype(np.float32)
    J[iu, ju], J[ju, iu] = blocks, blocks.transpose(0, 2, 1)
    index = [("A", 10), ("A", 11), ("B", 3), ("B", 4)] if segments else np.array([10, 11, 13, 14])
    return SimpleNamespace(J_ij=J, h_i=h, alphabet=np.array(list("-AC")), target_seq=np.array(list("CA-C")),
                           index_list=index, L=L, q=q)


def test_parse_mutations_plain_model():
    m = _toy()
    rows = ["C10A", "wild", "WT", "", "A11C,-13A", "C14-,C10C", "C12A", "A10C", "C10X", "C10A,A11C,C99A"]
    off, pos, st, bad = model_accel.parse_mutations(m, rows)
    assert off.dtype == np.int64 and pos.dtype == np.int32 and st.dtype == np.int8 and bad.dtype == bool
    assert bad.tolist() == [False] * 6 + [True] * 4           # unknown position, wrong from-letter, unknown letter, late bad entry
    assert off.tolist() == [0, 1, 1, 1, 1, 3, 5, 5, 5, 5, 5]
    assert pos.tolist() == [0, 1, 2, 3, 0] and st.tolist() == [1, 2, 1, 0, 2]
    # substitution lists, as CouplingsModel.delta_hamiltonian takes them
    off2, pos2, st2, bad2 = model_accel.parse_mutations(m, [[(10, "C", "A")], [], [(11, "A", "C"), (13, "-", "A")]])
    assert off2.tolist() == [0, 1, 1, 3] and pos2.tolist() == [0, 1, 2] and not bad2.any()
    with pytest.raises(ValueError):
        model_accel.parse_mutations(m, ["CxA"])               # the reference's int() fails the same way
    assert model_accel.extract_mutations("K50R,I100V") == [(50, "K", "R"), (100, "I", "V")]
    assert model_accel.extract_mutations("K50R", offset=2) == [(52, "K", "R")] and model_accel.extract_mutations("Wt") == []


def test_parse_mutations_segment_model():
    m = _toy(segments=True)
    off, pos, st, bad = model_accel.parse_mutations(m, ["C10A", "-3A,A11C", "C4A", "C10A"], segments=["A", "B,A", "A", "B"])
    assert bad.tolist() == [False, False, True, True] and off.tolist() == [0, 1, 3, 3, 3]
    assert pos.tolist() == [0, 2, 1] and st.tolist() == [1, 1, 2]
    off, pos, st, bad = model_accel.parse_mutations(m, ["-3A,C4A", "C10A", "wild"], segments="B")
    assert bad.tolist() == [False, True, False] and pos.tolist() == [2, 3]
    # more substitutions than segments: the rest is dropped, as the reference's zip drops it
    off, pos, st, bad = model_accel.parse_mutations(m, ["C10A,A11C"], segments=["A"])
    assert off.tolist() == [0, 1] and not bad.any()
    off, pos, st, bad = model_accel.parse_mutations(m, [[(("B", 4), "C", "A")]])
    assert pos.tolist() == [3] and not bad.any()


def test_delta_hamiltonians_and_scan_library_on_the_twin(monkeypatch):
    _twins(monkeypatch)
    m = _toy()
    jij = model_accel._pairs_from_dense(m.J_ij)
    target = np.array([2, 1, 0, 2])
    d = model_accel.delta_hamiltonians(m, [[(10, "C", "A"), (13, "-", "C")], [], [(10, "A", "C")], [(10, "C", "A"), (10, "C", "-")]])
    want, _, _ = mt.delta(target, *mt.dense(m.h_i, jij, 3), [0, 2], [1, 2])
    assert np.array_equal(d[0], want) and np.array_equal(d[1], np.zeros(3))
    assert np.isnan(d[2]).all() and np.isnan(d[3]).all()       # wrong from-letter; a position twice (refused, not doubled)
    lib = model_accel.scan_library(m, [13, 10], exclude="-", top=3)
    assert list(lib.columns) == ["index", "letters", "mutant", "dH", "dH_J", "dH_h"] and len(lib) == 3
    full = mt.mutant_scan(target, 3, m.h_i, jij, [2, 0], letters=[[1, 2], [1, 2]], energies=True)["energies"]
    order = np.lexsort((np.arange(4), -full[:, 0]))[:3]
    assert lib["index"].tolist() == order.tolist() and np.array_equal(lib[["dH", "dH_J", "dH_h"]].to_numpy(), full[order])
    combos = list(itertools.product("AC", "AC"))
    assert lib["letters"].tolist() == ["".join(combos[k]) for k in order]
    names = {"AA": "-13A,C10A", "AC": "-13A", "CA": "-13C,C10A", "CC": "-13C"}
    assert lib["mutant"].tolist() == [names[s] for s in lib["letters"]]
    everything = model_accel.scan_library(m, [10], exclude="", top=10)
    assert len(everything) == 3 and "wild" in everything["mutant"].tolist()
    with pytest.raises(ValueError):
        model_accel.scan_library(m, [12])
    with pytest.raises(ValueError):
        model_accel.scan_library(m, [10], exclude="X")


def test_top_combinations_on_the_twin(monkeypatch):
    """the histogram refinement and the walk in ranges give what a sort of all energies gives"""
    _twins(monkeypatch)
    rng = np.random.default_rng(8)
    L, q = 5, 4
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    target = rng.integers(0, q, L).astype(np.int8)
    sites = [4, 0, 2, 1]
    full = mt.mutant_scan(target, q, h, J, sites, energies=True)["energies"]
    for top, keep in ((7, None), (7, 7), (30, 40), (256, None), (1000, None)):
        idx, en = plm.top_combinations(target, q, h, J, sites, top=top, max_keep=keep)
        order = np.lexsort((np.arange(256), -full[:, 0]))[:top]
        assert np.array_equal(idx, order) and np.array_equal(en, full[order]), (top, keep)
    # exact ties: no couplings, two letters with the same field at every site; more tie than max_keep allows
    h[:, 1] = h[:, 2]
    target[:] = 0
    J[:] = 0
    full = mt.mutant_scan(target, q, h, J, sites, letters=[[1, 2]] * 4, energies=True)["energies"]
    assert len(set(full[:, 0].tolist())) == 1
    for keep, chunk in ((None, 1 << 24), (4, 5)):
        idx, en = plm.top_combinations(target, q, h, J, sites, letters=[[1, 2]] * 4, top=6, max_keep=keep, chunk=chunk)
        assert idx.tolist() == [0, 1, 2, 3, 4, 5] and np.array_equal(en, full[:6])
    with pytest.raises(ValueError):
        plm.top_combinations(target, q, h, J, sites, top=0)


# ---- the command line --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv", [
    ["m", "-o", "x"],                                          # neither --table nor --scan
    ["m", "--table", "t", "--scan", "1", "-o", "x"],
    ["m", "--table", "t"],                                     # no -o
    ["m", "--table", "t", "-o", "x", "--hamiltonian", "other"],
    ["m", "--table", "t", "-o", "x", "--histogram", "10"],
    ["m", "--scan", "1,x", "-o", "x"],
    ["m", "--scan", "1,1", "-o", "x"],
    ["m", "--scan", "1,2,3,4,5,6,7,8,9", "-o", "x"],
    ["m", "--scan", "1", "-o", "x", "--top", "0"],
    ["m", "--scan", "1", "-o", "x", "--histogram", "0"],
    ["m", "--scan", "1", "-o", "x", "--independent"],
])
def test_arguments_that_are_refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        mutate.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def _run_table(tmp_path):
    import pandas as pd
    z = np.load(GOLDEN_TABLE)
    m, target = golden_model()
    rows = slice(0, 120)
    table = pd.DataFrame({"mutant": z["mutants"][rows], "measured": np.arange(120.0)})
    src, dst = str(tmp_path / "in.csv"), str(tmp_path / "out.csv")
    table.to_csv(src, index=False)
    assert mutate.main([GOLDEN_MODEL, "--table", src, "-o", dst, "--independent"]) == 0
    empty_is_nan = {"prediction_epistatic": [""], "prediction_independent": [""]}
    got = pd.read_csv(dst, keep_default_na=False, na_values=empty_is_nan)
    assert list(got.columns) == ["mutant", "measured", "prediction_epistatic", "prediction_independent"]
    assert got["mutant"].tolist() == table["mutant"].tolist() and got["measured"].tolist() == table["measured"].tolist()
    want = z["delta"][rows, 0]
    ep = got["prediction_epistatic"].to_numpy(float)
    assert np.array_equal(np.isnan(ep), np.isnan(want)) and np.isnan(want).sum() >= 3
    # the CSV round-trips doubles exactly; the bound is the twin's, as in the GPU tests
    _, _, n_terms, sum_abs = mt.mutant_effects(target, m["q"], m["hi"], m["jij"], z["offsets"][:121], z["positions"],
                                               z["states"], info=True)
    bound = mt.bound(n_terms, sum_abs)[~np.isnan(want)]
    assert (np.abs(ep[~np.isnan(want)] - want[~np.isnan(want)]) <= bound).all()
    ind = got["prediction_independent"].to_numpy(float)
    assert np.array_equal(np.isnan(ind), np.isnan(want)) and np.abs(ind[~np.isnan(want)]).max() > 0
    assert mutate.main([GOLDEN_MODEL, "--table", src, "-o", dst, "--hamiltonian", "couplings"]) == 0
    got = pd.read_csv(dst, keep_default_na=False, na_values=empty_is_nan)
    assert (np.abs(got["prediction_epistatic"].to_numpy(float)[~np.isnan(want)] - z["delta"][rows, 1][~np.isnan(want)])
            <= bound).all()
    return m, target


def _run_scan(tmp_path, m, target):
    import pandas as pd
    dst = str(tmp_path / "scan.csv")
    index = [int(p) for p in m["index_list"]]
    assert mutate.main([GOLDEN_MODEL, "--scan", "%d,%d" % (index[20], index[2]), "-o", dst, "--top", "5", "--histogram", "8"]) == 0
    got = pd.read_csv(dst, keep_default_na=False)
    hist = pd.read_csv(dst + ".hist.csv")
    letters = [list(range(1, 21))] * 2
    full = mt.mutant_scan(target, m["q"], m["hi"], m["jij"], [20, 2], letters=letters, energies=True)["energies"]
    order = np.lexsort((np.arange(400), -full[:, 0]))[:5]
    assert got["index"].tolist() == order.tolist()
    info = mt.mutant_scan(target, m["q"], m["hi"], m["jij"], [20, 2], letters=letters, info=True)
    bound = mt.bound(info["n_terms"], info["sum_abs"])[order]
    assert (np.abs(got[["dH", "dH_J", "dH_h"]].to_numpy(float) - full[order]) <= bound[:, None]).all()
    first = got.iloc[0]
    a, b = m["alphabet"][1 + order[0] // 20], m["alphabet"][1 + order[0] % 20]
    assert first["letters"] == a + b
    assert len(hist) == 8 and hist["count"].sum() == 400 and hist["lower"].iloc[0] == pytest.approx(full[:, 0].min())
    assert hist["upper"].iloc[-1] == pytest.approx(full[:, 0].max()) and hist["count"].iloc[-1] >= 1


def test_command_line_on_the_twin(monkeypatch, tmp_path):
    _twins(monkeypatch)
    m, target = _run_table(tmp_path)
    _run_scan(tmp_path, m, target)


@pytest.mark.gpu
def test_command_line_on_the_gpu(tmp_path):
    m, target = _run_table(tmp_path)
    _run_scan(tmp_path, m, target)
