"""plm_cross_identities / plm_redundancy_filter on the GPU against the numpy twin (tests/identity_twin.py): every integer
output equal, no tolerance.  Inputs are planted families (identity_twin.planted_families): identities on both sides of
the threshold, exact duplicates, a pair exactly at the threshold, rows of only gaps.

Which launch a case takes (csrc/plm_identity.hip): rows up to 768 sites with the denominators columns / shorter run
the register-resident kernel k_ident_reg (L = 1 .. 768 below), longer rows and the denominator both the column-chunked
k_ident_chunk (L = 769, 1025, 20 000, and every "both" case); the filter adds k_ident_bits and k_ident_resolve."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_twin as twin  # noqa: E402

from evcouplings_amd import alignment_accel, plm, seqfilter  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("best_index", "best_match", "best_denom", "n_within")
LENGTHS = [1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 300, 768, 769, 1025]
SHAPES = [(1, 1), (63, 65), (64, 64), (257, 255), (300, 513)]
# (q, gap state): the alphabets and gap states of the issue; every one meets every denominator it allows below
ALPHABETS = [(2, 0), (21, 0), (32, 5), (21, 5), (32, 0), (2, None), (21, None), (32, None)]


def _two_sets(n_a, n_b, L, q, gap, seed, threshold=0.8):
    rows = twin.planted_families(n_a + n_b, L, q, seed, gap_state=gap, threshold=threshold,
                                 n_families=max(1, min(n_a, n_b) // 6))
    a, b = rows[:n_a].copy(), rows[n_a:].copy()
    if n_b > 2:
        b[n_b - 1] = b[0]       # two equal rows of b: whoever is nearest to them must name the smaller index
        a[0] = b[0]
    return a, b


def _assert_equal(got, want, what):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))
    np.testing.assert_array_equal(got["identity"], want["best_match"] / np.maximum(want["best_denom"], 1))


def _check(a, b, threshold, gap, denominator, exclude_self=False, what=""):
    want = twin.cross_identities(a, b, threshold, gap, denominator, exclude_self)
    got = plm.cross_identities(a, b, threshold=threshold, gap_state=gap, denominator=denominator,
                               exclude_self=exclude_self)
    _assert_equal(got, want, "%s L=%d %dx%d gap=%s %s" % (what, a.shape[1], len(a), len(b), gap, denominator))
    return got


@pytest.mark.parametrize("L", LENGTHS)
def test_cross_shape_matrix(L):
    """Every row length with every pair of set sizes and every denominator; the alphabet and gap state rotate so that
    over the matrix each of them meets each denominator (a denominator that needs a gap state takes the next
    alphabet that has one)."""
    li = LENGTHS.index(L)
    for si, (n_a, n_b) in enumerate(SHAPES):
        for di, denominator in enumerate(twin.DENOMS):
            k = li + 2 * si + 3 * di
            q, gap = ALPHABETS[k % len(ALPHABETS)]
            if denominator != "columns" and gap is None:
                q, gap = ALPHABETS[k % 5]
            a, b = _two_sets(n_a, n_b, L, q, gap, seed=1000 * li + 10 * si + di)
            _check(a, b, 0.8, gap, denominator, what="q=%d" % q)


def test_the_rotation_covers_every_alphabet_with_every_denominator():
    seen = set()
    for li in range(len(LENGTHS)):
        for si in range(len(SHAPES)):
            for di, denominator in enumerate(twin.DENOMS):
                k = li + 2 * si + 3 * di
                q, gap = ALPHABETS[k % len(ALPHABETS)]
                if denominator != "columns" and gap is None:
                    q, gap = ALPHABETS[k % 5]
                seen.add((q, gap, denominator))
    for q, gap in ALPHABETS:
        for denominator in twin.DENOMS:
            if denominator == "columns" or gap is not None:
                assert (q, gap, denominator) in seen


def test_planted_inputs_hold_the_cases_they_promise():
    a, b = _two_sets(63, 65, 100, 21, None, seed=5)
    r = _check(a, b, 0.8, None, "columns")
    assert r["best_index"][0] == 0 and r["best_match"][0] == 100            # b[0] == b[64]: the tie goes to index 0
    assert (r["n_within"] > 0).any() and (r["n_within"] == 0).any()         # both sides of the threshold
    m, _, _, _ = twin.pair_counts(a, b)
    assert (m == 80).any()                                                  # a pair exactly at the threshold
    a, b = _two_sets(63, 65, 100, 21, 5, seed=6)
    r = _check(a, b, 0.8, 5, "shorter")
    assert (a == 5).all(axis=1).any() or (b == 5).all(axis=1).any()         # a row of only gaps
    assert (r["best_denom"] == 0).any() or (b == 5).all(axis=1).any()


@pytest.mark.parametrize("L,denominator,gap", [(33, "columns", None), (300, "shorter", 0), (100, "both", 5),
                                               (769, "columns", 0), (64, "shorter", 5)])
def test_exclude_self_on_and_off(L, denominator, gap):
    a = twin.planted_families(300, L, 21, seed=L, gap_state=gap)
    on = _check(a, a, 0.8, gap, denominator, exclude_self=True)
    off = _check(a, a, 0.8, gap, denominator, exclude_self=False)
    assert (on["best_index"] != np.arange(300)).all()
    by_default = plm.cross_identities(a, threshold=0.8, gap_state=gap, denominator=denominator)     # b=None
    _assert_equal(by_default, on, "b=None")
    if gap is None:
        np.testing.assert_array_equal(off["n_within"], on["n_within"] + 1)
    one = plm.cross_identities(a[:1], threshold=0.8, gap_state=gap, denominator=denominator)
    assert (one["best_index"][0], one["best_match"][0], one["best_denom"][0], one["n_within"][0]) == (-1, 0, 0, 0)


def test_long_rows():
    """L = 20 000 through the column-chunked form, 64 x 64 rows."""
    for gap, denominator in ((None, "columns"), (0, "both"), (0, "shorter")):
        a, b = _two_sets(64, 64, 20000, 21, gap, seed=77)
        _check(a, b, 0.8, gap, denominator)


def test_states_up_to_126():
    rng = np.random.default_rng(3)
    a = rng.integers(100, 127, size=(70, 130)).astype(np.int8)
    b = a[rng.permutation(70)[:40]].copy()
    b[rng.random(b.shape) < 0.1] = 126
    for gap, denominator in ((None, "columns"), (126, "both"), (126, "shorter"), (100, "columns")):
        _check(a, b, 0.8, gap, denominator)


@pytest.mark.parametrize("L,denominator,gap", [(300, "columns", None), (300, "shorter", 0), (769, "columns", 0),
                                               (100, "both", 0)])
def test_the_split_of_b_changes_nothing(monkeypatch, L, denominator, gap):
    a, b = _two_sets(257, 255, L, 21, gap, seed=L + 1)
    want = twin.cross_identities(a, b, 0.8, gap, denominator)
    for tper in (1, 32, 100, len(b)):
        monkeypatch.setenv("PLM_IDENT_TPER", str(tper))
        got = plm.cross_identities(a, b, threshold=0.8, gap_state=gap, denominator=denominator)
        _assert_equal(got, want, "PLM_IDENT_TPER=%d" % tper)
    monkeypatch.delenv("PLM_IDENT_TPER")
    _assert_equal(plm.cross_identities(a, b, threshold=0.8, gap_state=gap, denominator=denominator), want, "default")


def test_counts_equal_the_reweighting_kernel(golden_dir):
    z = np.load(os.path.join(golden_dir, "reweight_freqs.npz"))
    cases = [(z[k[:-4] + "_msa"], float(z[k[:-4] + "_theta"])) for k in sorted(z.files) if k.endswith("_msa")]
    cases.append((twin.planted_families(700, 200, 21, seed=9), 0.8))
    for msa, theta in cases:
        r = plm.cross_identities(msa, msa, threshold=theta, exclude_self=False)
        np.testing.assert_array_equal(r["n_within"], plm.reweight(msa, theta))


def test_matches_equal_the_query_identities_of_alignment_stats():
    a = twin.planted_families(300, 129, 21, seed=11)
    query = a[7]
    r = plm.cross_identities(a, query[None])
    _, _, ident = plm.alignment_stats(a, 0, query=query)
    np.testing.assert_array_equal(r["best_match"], ident)
    assert (r["best_index"] == 0).all() and (r["best_denom"] == 129).all()


def _check_filter(msa, threshold, gap=None, denominator="columns"):
    keep = plm.redundancy_filter(msa, threshold, gap_state=gap, denominator=denominator)
    sim = twin.similarity_matrix(msa, threshold, gap, denominator)
    np.testing.assert_array_equal(keep, twin.greedy_filter(sim))
    assert keep.dtype == bool and keep[0]
    kept = np.flatnonzero(keep)
    pairs = sim[np.ix_(kept, kept)]
    assert not np.triu(pairs, 1).any()                                     # no two kept rows are similar
    for s in np.flatnonzero(~keep):
        assert (sim[s, :s] & keep[:s]).any()                               # every dropped row has an earlier kept one
    return keep


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 700])
def test_redundancy_filter_sizes(n):
    for k, (gap, denominator) in enumerate(((None, "columns"), (0, "shorter"), (5, "both"), (0, "columns"))):
        msa = twin.planted_families(n, 50, 21, seed=100 * n + k, gap_state=gap, n_families=max(1, n // 5))
        keep = _check_filter(msa, 0.8, gap, denominator)
        if n >= 255:
            assert 1 < keep.sum() < n


def test_redundancy_filter_long_rows():
    for gap, denominator in ((None, "columns"), (0, "shorter"), (0, "both")):
        _check_filter(twin.planted_families(300, 769, 21, seed=4, gap_state=gap, n_families=40), 0.8, gap, denominator)


def test_redundancy_filter_extremes():
    rng = np.random.default_rng(8)
    same = np.tile(rng.integers(1, 21, size=(1, 50)), (600, 1)).astype(np.int8)
    assert _check_filter(same, 0.8).sum() == 1
    assert _check_filter(same, 0.8, 0, "shorter").sum() == 1
    unrelated = rng.integers(0, 21, size=(600, 50)).astype(np.int8)
    assert _check_filter(unrelated, 0.8).all()
    assert _check_filter(unrelated, 0.0).sum() == 1                        # threshold 0: everything is similar


def test_redundancy_filter_chain_across_a_block_boundary():
    """Rows 254 .. 258: each 40 of 50 columns of the one before and 30 of the one before that; the filter keeps every
    other one, and the decision about rows 256 .. 258 needs what the block before decided."""
    rng = np.random.default_rng(12)
    msa = rng.integers(0, 10, size=(600, 50))
    order = rng.permutation(50)
    for k in range(1, 5):
        msa[254 + k] = msa[254 + k - 1]
        cols = order[10 * (k - 1):10 * k]
        msa[254 + k, cols] = 10 + k                                        # states no other row has
    keep = _check_filter(msa.astype(np.int8), 0.8)
    np.testing.assert_array_equal(keep[254:259], [True, False, True, False, True])


class _FakeAlignment:
    """The attributes of the reference's Alignment that alignment_accel reads."""

    def __init__(self, mapped, gap):
        self.matrix_mapped, self.alphabet_map, self._match_gap = mapped, {"-": gap}, "-"

    def select(self, sequences=None):
        return _FakeAlignment(self.matrix_mapped[sequences], self.alphabet_map["-"])


def test_alignment_accel_wrappers():
    a, b = _two_sets(63, 65, 100, 21, 0, seed=21)
    r = alignment_accel.nearest_identities(_FakeAlignment(a, 0), _FakeAlignment(b, 0), threshold=0.8)
    _assert_equal(r, twin.cross_identities(a, b, 0.8, 0, "columns"), "nearest_identities")
    sel = alignment_accel.filter_redundant(_FakeAlignment(a, 0), 0.8, denominator="shorter")
    np.testing.assert_array_equal(sel.matrix_mapped, a[twin.redundancy_filter(a, 0.8, 0, "shorter")])


def _example_a2m(golden_dir, tmp_path):
    z = np.load(os.path.join(golden_dir, "example_aln.npz"))
    path = str(tmp_path / "example_aln.a2m")
    with open(path, "w") as f:
        for name, row in zip(z["ids"].tolist(), z["chars_full"]):
            f.write(">%s\n%s\n" % (name, row.tobytes().decode("ascii")))
    return path, [str(x) for x in z["ids"]]


@pytest.mark.parametrize("columns", ["first", "a2m"])
def test_run_hhfilter_drop_in(golden_dir, tmp_path, columns):
    path, ids = _example_a2m(golden_dir, tmp_path)
    out = alignment_accel.run_hhfilter(path, str(tmp_path / "sub" / "filtered.a3m"), threshold=90, columns=columns)
    assert out == str(tmp_path / "sub" / "filtered.a3m")
    _, chars = seqfilter.read_alignment(path)
    states = seqfilter.match_states(chars, seqfilter.match_columns(chars, columns))
    keep = twin.redundancy_filter(states, 0.9, seqfilter.GAP, "shorter")
    kept_ids, _ = seqfilter.alignment_io.read_fasta_records(out)
    assert kept_ids == [i for i, k in zip(ids, keep) if k] and kept_ids[0] == ids[0]
    assert 1 < len(kept_ids) < len(ids)


def test_command_line(golden_dir, tmp_path):
    path, ids = _example_a2m(golden_dir, tmp_path)
    out, report = str(tmp_path / "f.a3m"), str(tmp_path / "r.csv")
    assert seqfilter.main([path, "-o", out, "--id", "90", "--columns", "a2m", "--denominator", "columns"]) == 0
    _, chars = seqfilter.read_alignment(path)
    states = seqfilter.match_states(chars, seqfilter.match_columns(chars, "a2m"))
    keep = twin.redundancy_filter(states, 0.9, seqfilter.GAP, "columns")
    assert seqfilter.alignment_io.read_fasta_records(out)[0] == [i for i, k in zip(ids, keep) if k]
    sub = str(tmp_path / "kept.a2m")                                        # the kept rows, still rectangular
    with open(sub, "wb") as f:
        for s in np.flatnonzero(keep):
            f.write(b">" + ids[s].encode() + b"\n" + chars[s].tobytes() + b"\n")
    assert seqfilter.main([sub, "--against", path, "--report", report, "--id", "80"]) == 0
    lines = open(report).read().split()
    assert lines[0] == "id,nearest_id,identity,n_within" and len(lines) == 1 + keep.sum()
    want = twin.cross_identities(states[keep], states, 0.8, seqfilter.GAP, "columns")
    for line, bi, bm, bd, nw in zip(lines[1:], want["best_index"], want["best_match"], want["best_denom"], want["n_within"]):
        name, near, identity, n_within = line.split(",")
        assert near == ids[bi] and int(n_within) == nw and abs(float(identity) - bm / max(bd, 1)) < 1e-6
