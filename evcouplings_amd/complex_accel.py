"""
Inter-protein energies and paralog matching from a model fitted on a concatenated alignment (DESIGN_NEXT_ROWS.md
section 9.23): the consumer of a two-segment fit that the reference's `protein_complex` pipeline lacks.  The reference
pairs one sequence of A with one of B per species by genome distance or by best hit to the query
(complex/protocol.py:218, :367); here the model itself says which A goes with which B (Bitbol et al. 2016, Gueudre et
al. 2016):

    E(s,t) = sum_{i in A} sum_{j in B} J_ij(a_si, b_tj)

for every candidate pair, by `plm.cross_energies` on the GPU, then one assignment problem per species
(`plm.group_assignment`) or the pairs that are each other's best partner.

A model is a dict as `model_io.read_model_file` returns it, or an object with `J_ij`, `index_list` and `alphabet`
(the reference's CouplingsModel / MultiSegmentCouplingsModel, `sample.model_from_file`).  The two sides are named by
segment identifiers, resolved through an `index_list` of (segment, position) entries as `model_accel.parse_mutations`
resolves positions, or by `sites_a` / `sites_b`, 0-based indices into the model's sites.
"""
import numpy as np

from evcouplings_amd import model_accel, plm

PAIR_COLUMNS = ["id_1", "id_2", "species", "energy", "gap"]


def _model_parts(model):
    """(jij i<j blocks, L, q, index_list, alphabet) of a model-file dict or a model object"""
    if isinstance(model, dict):
        return np.asarray(model["jij"]), int(model["L"]), int(model["q"]), model["index_list"], model["alphabet"]
    J = np.asarray(model.J_ij)
    return model_accel._pairs_from_dense(J), J.shape[0], J.shape[2], model.index_list, model.alphabet


def _segment_of(entry):
    return entry[0] if isinstance(entry, (tuple, list, np.ndarray)) and len(entry) == 2 else None


def resolve_sites(index_list, segment_a=None, segment_b=None, sites_a=None, sites_b=None):
    """The 0-based model sites of the two sides.  Explicit site lists win; else the sites whose `index_list` entry is
    (segment, position) with the named segment; with neither, the first two segments of the index list in order."""
    entries = [model_accel._hashable(e) for e in index_list]
    segments = [_segment_of(e) for e in entries]
    named = list(dict.fromkeys(s for s in segments if s is not None))

    def side(sites, segment, default_rank, what):
        if sites is not None:
            return np.asarray(sites, dtype=np.int64).ravel()
        if segment is None:
            if len(named) < 2:
                raise ValueError("the model has no segments: give sites_a and sites_b")
            segment = named[default_rank]
        found = np.array([k for k, s in enumerate(segments) if s == segment], dtype=np.int64)
        if not found.size:
            raise ValueError("segment %r (%s) is not in the model's index_list (segments: %r)" % (segment, what, named))
        return found

    return side(sites_a, segment_a, 0, "A"), side(sites_b, segment_b, 1, "B")


def _code(alphabet):
    letters = np.array(list(alphabet) if isinstance(alphabet, str) else alphabet).astype("U1")
    return {a: k for k, a in enumerate(letters)}


def _states(seqs, code, L, what):
    """sequences as strings, a letter matrix or a state matrix -> int8 states (n, L)"""
    if len(seqs) and isinstance(seqs[0], (str, bytes)):
        seqs = [list(s.decode() if isinstance(s, bytes) else s) for s in seqs]
    mat = np.asarray(seqs)
    if mat.size == 0:
        mat = mat.reshape(0, L)
    if mat.ndim != 2 or mat.shape[1] != L:
        raise ValueError("%s must hold sequences of %d sites (got shape %r)" % (what, L, mat.shape))
    return np.ascontiguousarray(model_accel._to_states(mat, code))


def _inter_model(model, segment_a, segment_b, sites_a, sites_b, gauge, skip_gap):
    jij, L, q, index_list, alphabet = _model_parts(model)
    sa, sb = resolve_sites(index_list, segment_a, segment_b, sites_a, sites_b)
    code = _code(alphabet)
    skip = None
    if skip_gap:
        if "-" not in code:
            raise ValueError("the model's alphabet has no gap letter to skip")
        skip = code["-"]
    return plm.inter_blocks(jij, L, q, sa, sb, gauge=gauge), code, skip


def interaction_energies(model, seqs_a, seqs_b, segment_a=None, segment_b=None, sites_a=None, sites_b=None,
                         a_offsets=None, b_offsets=None, gauge="zero_sum", skip_gap=False, matrix=True, best=True, device=0):
    """
    E(s,t) between the sequences seqs_a of side A and seqs_b of side B (letters or states, one column per model site of
    the side) under the inter block of `model`: the dict of `plm.cross_energies` -- all against all, or by groups with
    a_offsets / b_offsets.  gauge: see `plm.inter_blocks`; skip_gap leaves out every term with a gap on either side.
    """
    jab, code, skip = _inter_model(model, segment_a, segment_b, sites_a, sites_b, gauge, skip_gap)
    a = _states(seqs_a, code, jab.shape[0], "seqs_a")
    b = _states(seqs_b, code, jab.shape[1], "seqs_b")
    return plm.cross_energies(jab, a, b, a_offsets=a_offsets, b_offsets=b_offsets, skip_state=skip, matrix=matrix, best=best,
                              device=device)


def _by_species(species_a, species_b):
    """rows of both sides whose species occurs on both, sorted by species (stable), and the group offsets"""
    sp_a, sp_b = np.asarray(species_a).astype(str), np.asarray(species_b).astype(str)
    common = np.intersect1d(sp_a, sp_b)
    keep_a, keep_b = np.nonzero(np.isin(sp_a, common))[0], np.nonzero(np.isin(sp_b, common))[0]
    keep_a = keep_a[np.argsort(sp_a[keep_a], kind="stable")]
    keep_b = keep_b[np.argsort(sp_b[keep_b], kind="stable")]
    ao = np.concatenate([[0], np.searchsorted(sp_a[keep_a], common, side="right")]).astype(np.int64)
    bo = np.concatenate([[0], np.searchsorted(sp_b[keep_b], common, side="right")]).astype(np.int64)
    return common, keep_a, keep_b, ao, bo


def match_by_species(model, alignment_a, alignment_b, species_a, species_b, method="assignment", ids_a=None, ids_b=None,
                     segment_a=None, segment_b=None, sites_a=None, sites_b=None, gauge="zero_sum", skip_gap=False,
                     min_gap=None, device=0):
    """
    Pair the sequences of alignment_a with those of alignment_b inside every species by their inter-protein energy.
    alignment_a / alignment_b: letters or states, one row per sequence, one column per model site of the side;
    species_a / species_b: one label per row; ids_a / ids_b: one identifier per row (default: the row numbers).
    Both sides are sorted by species, one `plm.cross_energies` call scores every candidate pair, then
      method="assignment"       the exact assignment per species (`plm.group_assignment`): min(n_a, n_b) pairs
      method="reciprocal_best"  the pairs that are each other's best partner -- the energy analogue of the reference's
                                best_reciprocal_matching; from the best-partner arrays alone, no pair matrix.
    Returns a DataFrame with the columns id_1, id_2, species, energy, gap, where
    gap = E(s,t) - max(best alternative in row s, best alternative in column t), +inf without an alternative; with
    min_gap only the pairs with gap >= min_gap are kept.  The first two columns are what the reference's
    write_concatenated_alignment(id_pairing, ...) takes.  A species present on one side only produces no rows.
    """
    import pandas as pd
    if method not in ("assignment", "reciprocal_best"):
        raise ValueError("method must be 'assignment' or 'reciprocal_best' (got %r)" % (method,))
    jab, code, skip = _inter_model(model, segment_a, segment_b, sites_a, sites_b, gauge, skip_gap)
    a = _states(alignment_a, code, jab.shape[0], "alignment_a")
    b = _states(alignment_b, code, jab.shape[1], "alignment_b")
    if len(species_a) != len(a) or len(species_b) != len(b):
        raise ValueError("one species label per sequence is needed")
    ids_a = np.arange(len(a)) if ids_a is None else np.asarray(ids_a)
    ids_b = np.arange(len(b)) if ids_b is None else np.asarray(ids_b)
    if len(ids_a) != len(a) or len(ids_b) != len(b):
        raise ValueError("one identifier per sequence is needed")
    common, keep_a, keep_b, ao, bo = _by_species(species_a, species_b)
    if not len(common):
        return pd.DataFrame({c: [] for c in PAIR_COLUMNS})
    assignment = method == "assignment"
    res = plm.cross_energies(jab, a[keep_a], b[keep_b], a_offsets=ao, b_offsets=bo, skip_state=skip, matrix=assignment,
                             best=True, device=device)
    rows, cols = res["rows_best"], res["cols_best"]
    group_of_a = np.repeat(np.arange(len(common)), np.diff(ao))
    if assignment:
        partner, _ = plm.group_assignment(res["matrix"], ao, bo, maximize=True)
        s = np.nonzero(partner >= 0)[0]
        t = partner[s]
        g = group_of_a[s]
        energy = res["matrix"][res["block_offsets"][g] + (s - ao[g]) * (bo[g + 1] - bo[g]) + (t - bo[g])]
    else:
        s = np.nonzero((rows["index"] >= 0) & (cols["index"][np.maximum(rows["index"], 0)] == np.arange(len(rows))))[0]
        t = rows["index"][s]
        g = group_of_a[s]
        energy = rows["best"][s]
    alt_row = np.where(rows["index"][s] == t, rows["second"][s], rows["best"][s])
    alt_col = np.where(cols["index"][t] == s, cols["second"][t], cols["best"][t])
    with np.errstate(invalid="ignore"):
        gap = energy - np.maximum(alt_row, alt_col)
    out = pd.DataFrame({"id_1": ids_a[keep_a][s], "id_2": ids_b[keep_b][t], "species": common[g], "energy": energy,
                        "gap": gap}, columns=PAIR_COLUMNS)
    if min_gap is not None:
        out = out[out["gap"] >= float(min_gap)].reset_index(drop=True)
    return out
