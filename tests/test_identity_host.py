"""CPU-side checks of the pairwise identities and the redundancy filter: the numpy twin (tests/identity_twin.py) against
literal loops and against the reference's recorded cluster sizes, the A3M writer against the reference's reader, the
run_hhfilter rebinding, and the argument checks of the library that run before it looks for a device."""
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_twin as twin  # noqa: E402
import refstubs  # noqa: E402

from evcouplings_amd import _lib, alignment_accel, plm, seqfilter  # noqa: E402

GAP = 0
#        a: the start of a chain; b: 8 of 10 columns of a (exactly at 0.8); c: 8 of b, 6 of a; a again; only gaps;
#        a with two gaps (8 matches of 8 jointly ungapped columns)
HAND = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 9, 1],
                 [1, 2, 3, 4, 5, 6, 7, 8, 2, 2],
                 [1, 2, 3, 4, 5, 6, 3, 3, 2, 2],
                 [1, 2, 3, 4, 5, 6, 7, 8, 9, 1],
                 [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                 [0, 2, 3, 4, 5, 6, 7, 8, 9, 0]], dtype=np.int8)


def _loops(a, b, threshold, gap_state, denominator, exclude_self):
    """The definitions of include/plm_hip.h as literal Python loops."""
    L = a.shape[1]
    out = []
    for s in range(len(a)):
        best, cnt = (-1, 0, 0), 0
        for t in range(len(b)):
            if exclude_self and s == t:
                continue
            m = both = 0
            for i in range(L):
                gapped = gap_state is not None and (a[s][i] == gap_state or b[t][i] == gap_state)
                both += not gapped
                m += (not gapped) and a[s][i] == b[t][i]
            res_s = sum(1 for v in a[s] if gap_state is None or v != gap_state)
            res_t = sum(1 for v in b[t] if gap_state is None or v != gap_state)
            d = {"columns": L, "both": both, "shorter": min(res_s, res_t)}[denominator]
            if denominator == "columns":
                cnt += m >= math.ceil(threshold * L - 1e-9)
            else:
                cnt += d > 0 and m >= math.ceil(threshold * d - 1e-9)
            if best[0] < 0 or m * max(best[2], 1) > best[1] * max(d, 1):
                best = (t, m, d)
        out.append(best + (cnt,))
    return np.array(out)


@pytest.mark.parametrize("denominator,gap_state", [("columns", None), ("columns", GAP), ("both", GAP), ("shorter", GAP)])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_twin_equals_the_literal_loops_on_hand_written_rows(denominator, gap_state, exclude_self):
    want = _loops(HAND, HAND, 0.8, gap_state, denominator, exclude_self)
    got = twin.cross_identities(HAND, HAND, 0.8, gap_state, denominator, exclude_self)
    for k, name in enumerate(("best_index", "best_match", "best_denom", "n_within")):
        np.testing.assert_array_equal(got[name], want[:, k], err_msg=name)


def test_hand_written_rows_mean_what_their_comment_says():
    r = twin.cross_identities(HAND, HAND, 0.8, None, "columns", exclude_self=True)
    assert r["best_index"][0] == 3 and r["best_match"][0] == 10            # the duplicate
    assert r["best_index"][3] == 0                                         # and back: the smallest index of a tie
    m, both, res, _ = twin.pair_counts(HAND, HAND, GAP)
    assert m[0, 1] == 8 and m[1, 2] == 8 and m[0, 2] == 6                  # a ~ b (exactly at 0.8), b ~ c, a !~ c
    assert m[4].sum() == 0 and res[4] == 0 and both[4].sum() == 0          # the row of gaps matches nothing, itself included
    assert m[0, 5] == 8 and both[0, 5] == 8
    g = twin.cross_identities(HAND, HAND, 0.8, GAP, "shorter", exclude_self=False)
    assert g["best_denom"][4] == 0 and g["best_match"][4] == 0 and g["best_index"][4] == 0 and g["n_within"][4] == 0
    b = twin.cross_identities(HAND[5:], HAND[:1], 0.8, GAP, "both")
    assert (b["best_match"][0], b["best_denom"][0], b["n_within"][0]) == (8, 8, 1)
    c = twin.cross_identities(HAND[5:], HAND[:1], 0.81, GAP, "columns")
    assert (c["best_match"][0], c["best_denom"][0], c["n_within"][0]) == (8, 10, 0)


def test_greedy_filter_keeps_the_ends_of_a_chain():
    keep = twin.redundancy_filter(HAND[:4], 0.8)
    np.testing.assert_array_equal(keep, [True, False, True, False])         # b falls to a; c only had b; the duplicate
    sim = twin.similarity_matrix(HAND[:4], 0.8)
    want = []
    for s in range(4):
        want.append(not any(want[t] and sim[s, t] for t in range(s)))
    np.testing.assert_array_equal(keep, want)
    # one column more than the pair at the threshold has: nothing but the duplicate is similar
    np.testing.assert_array_equal(twin.redundancy_filter(HAND[:4], 0.81), [True, True, True, False])


def test_twin_counts_equal_the_recorded_cluster_sizes(golden_dir):
    """a against itself, all columns, no gap state, self included: the reference's num_cluster_members."""
    z = np.load(os.path.join(golden_dir, "reweight_freqs.npz"))
    cases = sorted(k[:-4] for k in z.files if k.endswith("_msa"))
    assert cases
    for c in cases:
        msa = z[c + "_msa"]
        r = twin.cross_identities(msa, msa, float(z[c + "_theta"]), None, "columns", exclude_self=False)
        np.testing.assert_array_equal(r["n_within"], z[c + "_counts"], err_msg=c)


@pytest.mark.skipif(not refstubs.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("columns", ["first", "a2m"])
def test_written_a3m_reads_back_through_the_reference(golden_dir, tmp_path, columns):
    refstubs.install()
    from evcouplings.align.alignment import Alignment
    z = np.load(os.path.join(golden_dir, "example_aln.npz"))
    ids = [str(x) for x in z["ids"]]
    chars = z["chars_full"].view(np.uint8).reshape(z["chars_full"].shape)
    cols = seqfilter.match_columns(chars, columns)
    assert cols.sum() == (423 if columns == "first" else 420)              # three insert columns, lowercase in the first row
    if columns == "a2m":
        np.testing.assert_array_equal(cols, z["keep_cols"])
    states = seqfilter.match_states(chars, cols)
    keep = twin.redundancy_filter(states, 0.9, seqfilter.GAP, "shorter")
    assert keep[0] and 1 < keep.sum() < len(keep)
    path = seqfilter.write_a3m(str(tmp_path / "out.a3m"), ids, chars, cols, keep)
    with open(path) as f:
        back = Alignment.from_file(f, "a3m")
    assert list(back.ids) == [i for i, k in zip(ids, keep) if k]
    first = back.matrix[0]
    match = np.array([c == c.upper() for c in first])                      # the reader keeps the first row's inserts
    assert match.sum() == cols.sum()
    want = np.char.upper(z["chars_full"][keep][:, cols].astype("U1"))
    want[want == "."] = "-"
    np.testing.assert_array_equal(back.matrix[:, match], want)


def _fake_modules():
    ali = types.ModuleType("fake_alignment")
    for name in alignment_accel._NAMES:
        setattr(ali, name, object())
    tools = types.ModuleType("fake_tools")
    tools.run_hhfilter = object()
    return ali, tools


def test_install_rebinds_run_hhfilter_only_when_asked():
    ali, tools = _fake_modules()
    original = tools.run_hhfilter
    alignment_accel.install(ali)
    assert tools.run_hhfilter is original and ali.num_cluster_members is alignment_accel.num_cluster_members
    alignment_accel.uninstall(ali)
    alignment_accel.install(ali, redundancy_filter=True, tools_module=tools)
    assert tools.run_hhfilter is alignment_accel.run_hhfilter
    alignment_accel.uninstall(ali)
    assert tools.run_hhfilter is original and ali.num_cluster_members is not alignment_accel.num_cluster_members


@pytest.mark.skipif(not refstubs.reference_available(), reason="reference tree not present")
def test_install_rebinds_the_reference_tools_module():
    refstubs.install()
    import evcouplings.align.alignment as ref_ali
    import evcouplings.align.tools as ref_tools
    original = ref_tools.run_hhfilter
    try:
        alignment_accel.install()
        assert ref_tools.run_hhfilter is original
        alignment_accel.install(redundancy_filter=True)
        assert ref_tools.run_hhfilter is alignment_accel.run_hhfilter
    finally:
        alignment_accel.uninstall()
    assert ref_tools.run_hhfilter is original and ref_ali.map_matrix is not alignment_accel.map_matrix


def test_run_hhfilter_checks_its_arguments_like_the_reference(tmp_path):
    from evcouplings_amd.tools import ResourceError
    with pytest.raises(ValueError):
        seqfilter.run_hhfilter(str(tmp_path / "x.a2m"), str(tmp_path / "y.a3m"), columns="all")
    with pytest.raises(ResourceError):
        alignment_accel.run_hhfilter(str(tmp_path / "missing.a2m"), str(tmp_path / "y.a3m"))


def test_no_cpu_fallback_without_a_gpu():
    if _lib.load().plm_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.PlmError):
        plm.cross_identities(HAND, HAND[:2])
    with pytest.raises(_lib.PlmError):
        plm.redundancy_filter(HAND, 0.8)


@pytest.mark.parametrize("value", ["0", "abc", "-3", "12x", ""])
def test_a_bad_split_hook_is_refused_before_the_device_is_looked_at(monkeypatch, value):
    monkeypatch.setenv("PLM_IDENT_TPER", value)
    for call in (lambda: plm.cross_identities(HAND, HAND[:2]), lambda: plm.redundancy_filter(HAND, 0.8)):
        with pytest.raises(_lib.PlmError) as err:
            call()
        assert err.value.code == -1 and "PLM_IDENT_TPER" in str(err.value)


def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    def einval(call, word):
        with pytest.raises(_lib.PlmError) as err:
            call()
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    empty = np.zeros((0, 10), np.int8)
    einval(lambda: plm.cross_identities(empty, HAND), "empty")
    einval(lambda: plm.cross_identities(HAND, empty), "empty")
    einval(lambda: plm.redundancy_filter(empty, 0.8), "empty")
    einval(lambda: plm.cross_identities(HAND, HAND, denominator="both"), "gap state")
    einval(lambda: plm.redundancy_filter(HAND, 0.8, denominator="shorter"), "gap state")
    einval(lambda: plm.cross_identities(HAND, HAND, gap_state=127), "gap state")
    einval(lambda: plm.cross_identities(HAND, HAND, threshold=float("nan")), "finite")
    einval(lambda: plm.cross_identities(np.full((2, 10), 127, np.int8), HAND), "0..126")
    with pytest.raises(ValueError):
        plm.cross_identities(HAND, HAND, denominator="longer")
    with pytest.raises(ValueError):
        plm.cross_identities(HAND, HAND[:, :5])
