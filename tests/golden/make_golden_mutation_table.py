#!/usr/bin/env python3
"""
Golden vectors of the reference's mutation scoring (run in the build container only; the reference does not exist on the
GPU box).  Input: tests/golden/hip_fit_L24.model, read by the reference's own plmc_v2 reader.  Every row is scored by
the reference's own `CouplingsModel.delta_hamiltonian` (couplings/model.py:672-712, the loop `_delta_hamiltonian`
:112-176), the call `predict_mutation_table` makes per table row; rows on which it raises ValueError are stored with NaN,
as `predict_mutation_table` stores them.  The model's float32 h_i array is widened to float64 first (same values; see
main()), so the whole loop is float64 arithmetic on float32 values.  numba is absent, so the @jit loop runs as plain Python under the identity stub
of tests/refstubs.py.  No reference source is written into this repo; only the arrays are committed.

About 300 variants: every M from 0 to 6, a few with M = 12 and M = 24 (every site), substitutions to the target's own
letter, the first and the last site, and rows the reference rejects (a position or a letter the model does not have, a
from-letter that is not the target's).  Stored:
  mutants        the rows in the notation of the mutate stage ("K50R,I100V", "wild"; positions in the model's numbering)
  offsets, positions, states   the same rows in CSR form with 0-based sites and states; an unknown position is stored as
                 site L and an unknown letter as state q (both outside the model)
  from_mismatch  rows rejected for their from-letter alone (their CSR entries are valid)
  delta          n x 3 (dH, dH_J, dH_h) of the reference, NaN for the rejected rows

Usage:  python tests/golden/make_golden_mutation_table.py      (writes tests/golden/mutation_table_L24.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refstubs  # noqa: E402


def build_rows(m, rng):
    """[(list of (position, from, to)), ...] in the model's numbering"""
    L, letters = m.L, list(m.alphabet)
    index, target = list(m.index_list), list(m.target_seq)

    def row(sites, wild_type_share=0.0):
        subs = []
        for s in sites:
            to = target[s] if rng.random() < wild_type_share else letters[rng.integers(len(letters))]
            subs.append((int(index[s]), target[s], to))
        return subs

    rows = []
    for M in range(0, 7):
        for r in range(40):
            sites = rng.choice(L, M, replace=False)
            if M and r % 8 == 0:
                sites[0] = 0 if 0 not in sites else sites[0]                 # the first site
            if M and r % 8 == 1:
                sites[-1] = L - 1 if L - 1 not in sites else sites[-1]       # the last site
            rows.append(row(sites, wild_type_share=0.3 if r % 5 == 0 else 0.0))
    for r in range(6):
        rows.append(row(rng.choice(L, 12, replace=False), wild_type_share=0.25 * (r % 2)))
    for r in range(4):
        rows.append(row(rng.permutation(L) if r % 2 else np.arange(L), wild_type_share=0.25 * (r // 2)))
    rows.append(row(np.arange(L), wild_type_share=1.0))                      # every site to its own letter
    rejected = [
        [(int(index[0]) - 1, "A", "C")],                                     # position before the model
        [(int(index[-1]) + 7, "A", "C")],                                    # position after it
        [(int(index[3]), target[3], "X")],                                   # letter outside the alphabet
        [(int(index[3]), target[3], "b")],
        [(int(index[5]), letters[(letters.index(target[5]) + 1) % len(letters)], "W")],     # from-letter mismatch
        row([2, 9]) + [(int(index[-1]) + 1, "A", "C")],                      # one bad entry after good ones
        row([4]) + [(int(index[11]), target[11], "Z")] + row([7]),
        row([1]) + [(int(index[8]), letters[(letters.index(target[8]) + 3) % len(letters)], "K")] + row([20]),
    ]
    at = [3, 50, 97, 140, 171, 222, 260, len(rows)]
    for k, rej in zip(at, rejected):
        rows.insert(k, rej)
    return rows


def main():
    refstubs.install()
    from evcouplings.couplings.model import CouplingsModel
    m = CouplingsModel(os.path.join(HERE, "hip_fit_L24.model"))
    # The plmc_v2 reader leaves h_i a float32 array beside the float64 J_ij.  Without numba the loop's `delta_hi += ...`
    # then turns its float64 accumulator into a float32 one (numpy >= 2 scalar promotion), which numba does not do.  The
    # same values in a float64 array give the loop the float64 arithmetic on float32 values that J_ij already has.
    m.h_i = m.h_i.astype(np.float64)
    rows = build_rows(m, np.random.default_rng(2024))
    L, q = m.L, m.num_symbols
    delta = np.full((len(rows), 3), np.nan)
    offsets, positions, states, mismatch, strings = [0], [], [], [], []
    for r, subs in enumerate(rows):
        try:
            delta[r] = m.delta_hamiltonian(subs)
        except ValueError:
            pass
        bad_from = False
        for pos, a_from, a_to in subs:
            site = m.index_map.get(pos, L)
            positions.append(site)
            states.append(m.alphabet_map.get(a_to, q))
            bad_from |= site < L and a_from != m.target_seq[site]
        mismatch.append(bad_from and all(p < L for p in positions[offsets[-1]:]) and all(s < q for s in states[offsets[-1]:]))
        offsets.append(len(positions))
        strings.append(",".join("%s%d%s" % (a, p, b) for p, a, b in subs) or ("wild", "wt", "WT", "")[r % 4])
    out = os.path.join(HERE, "mutation_table_L24.npz")
    np.savez_compressed(out, mutants=np.array(strings), offsets=np.array(offsets, np.int64),
                        positions=np.array(positions, np.int32), states=np.array(states, np.int8),
                        from_mismatch=np.array(mismatch, bool), delta=delta)
    n_nan = int(np.isnan(delta[:, 0]).sum())
    print("wrote %s (%d bytes): %d rows, %d rejected" % (out, os.path.getsize(out), len(rows), n_nan))


if __name__ == "__main__":
    main()
