#!/usr/bin/env python3
"""
Timing probe of the mutation-table and library-scan entry points (DESIGN_NEXT_ROWS.md section 9.16); run by hand on the
GPU, not a test.  Host clocks around calls that end in a device synchronise; kernel times come from a second run under
`rocprofv3 --kernel-trace --stats -- python tests/probes/mutants_probe.py --quick`.

  tables  L = 300, q = 21: 10^6 variants with M <= 3 and 10^5 with M = 10 through plm.mutant_effects, beside the only
          path there was before it: every variant expanded to a full sequence and scored by plm.hamiltonians (minus the
          target's energy).  Host parsing (model_accel.parse_mutations of the strings) is timed apart, and so is a call
          with no variants (model upload, single tables: the share of a call that does not depend on the table).
  scans   20^4 and 20^6 combinations, histogram only and top = 1000 (plm.top_combinations).
"""
import argparse
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, __file__.rsplit("/tests/", 1)[0])
from evcouplings_amd import model_accel, plm  # noqa: E402


def clock(fn, reps=3):
    fn()                                                       # warm-up: code objects, first allocations
    best = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        best.append(time.perf_counter() - t)
    return min(best), float(np.median(best)), out


def table(rng, L, q, n, m_max, exact):
    """n variants in CSR form: M = m_max substitutions each, or 1 .. m_max; distinct positions start, start + 7, ..."""
    M = np.full(n, m_max) if exact else rng.integers(1, m_max + 1, n)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum(M)
    rows = np.repeat(np.arange(n), M)
    within = np.arange(offsets[-1]) - offsets[rows]
    positions = ((rng.integers(0, L, n)[rows] + 7 * within) % L).astype(np.int32)
    return offsets, positions, rng.integers(0, q, positions.size).astype(np.int8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one repetition of everything (for a profiler run)")
    ap.add_argument("--tiny", action="store_true", help="toy sizes, to rehearse the script")
    ap.add_argument("--tables-only", action="store_true", help="skip the scans")
    a = ap.parse_args()
    reps = 1 if a.quick or a.tiny else 3
    L, q = 80 if a.tiny else 300, 21
    rng = np.random.default_rng(0)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = (0.1 * rng.normal(size=(L * (L - 1) // 2, q, q))).astype(np.float32)
    target = rng.integers(1, q, L).astype(np.int8)
    alphabet = np.array(list("-ACDEFGHIKLMNPQRSTVWY"))
    t_model, _, _ = clock(lambda: plm.mutant_effects(target, q, h, J, [0], [], [], tables=True), reps)
    print("model upload + single tables (no variants), L=%d: %.1f ms" % (L, 1e3 * t_model))
    for n, m_max, exact in ((1000, 3, False), (100, 10, True)) if a.tiny else ((1000000, 3, False), (100000, 10, True)):
        off, pos, st = table(rng, L, q, n, m_max, exact)
        t_fast, med, (out, status) = clock(lambda: plm.mutant_effects(target, q, h, J, off, pos, st), reps)
        assert not status.any()
        print("mutant_effects: %d variants, M %s %d: %.1f ms best, %.1f ms median (%.1f ms beyond the model's share), %.2e variants/s"
              % (n, "=" if exact else "<=", m_max, 1e3 * t_fast, 1e3 * med, 1e3 * (t_fast - t_model), n / t_fast))

        def expanded():
            t0 = time.perf_counter()
            seqs = np.tile(target, (n, 1))
            rows = np.repeat(np.arange(n), np.diff(off))
            seqs[rows, pos] = st
            t1 = time.perf_counter()
            H = plm.hamiltonians(np.vstack([target[None], seqs]), q, h, J)
            return t1 - t0, time.perf_counter() - t1, H[1:] - H[0]

        expanded()
        t_exp, t_ham, d = min((expanded() for _ in range(reps)), key=lambda r: r[0] + r[1])
        print("  expanded to sequences + plm.hamiltonians: %.1f ms expansion + %.1f ms call; largest |difference| of the two dH %.2e"
              % (1e3 * t_exp, 1e3 * t_ham, np.abs(d[:, 0] - out[:, 0]).max()))
        # host parsing of the same table written as strings (a tenth of it: the time is linear)
        k = n // 10
        tgt = alphabet[target]
        strings = [",".join("%s%d%s" % (tgt[p], p + 1, alphabet[s]) for p, s in zip(pos[off[v]:off[v + 1]], st[off[v]:off[v + 1]]))
                   for v in range(k)]
        model = SimpleNamespace(h_i=h, alphabet=alphabet, target_seq=tgt, index_list=np.arange(1, L + 1))
        t0 = time.perf_counter()
        parsed = model_accel.parse_mutations(model, strings)
        t_parse = time.perf_counter() - t0
        assert np.array_equal(parsed[1], pos[:off[k]]) and not parsed[3].any()
        print("  parse_mutations of %d rows: %.1f ms (%.1f us per row, %.0f ms for the table)" % (k, 1e3 * t_parse, 1e6 * t_parse / k,
                                                                                           1e3 * t_parse * n / k))
    if a.tables_only:
        return
    letters = [list(range(1, 21))]
    for k in (2,) if a.tiny else (4, 6):
        sites = list(range(10, 10 + 11 * k, 11))
        total = 20 ** k
        edges = np.linspace(-40, 40, 1024)
        t_hist, med, res = clock(lambda: plm.mutant_scan(target, q, h, J, sites, letters=letters * k, edges=edges), reps)
        assert int(res["histogram"].sum()) == total
        print("scan 20^%d, histogram only: %.1f ms best, %.1f ms median (%.1f ms beyond the model's share), %.2e combinations/s"
              % (k, 1e3 * t_hist, 1e3 * med, 1e3 * (t_hist - t_model), total / t_hist))
        t_top, med, (idx, en) = clock(lambda: plm.top_combinations(target, q, h, J, sites, letters=letters * k, top=1000), reps)
        print("scan 20^%d, top 1000 (extremes, histograms, compaction): %.1f ms best, %.1f ms median; best dH %.3f"
              % (k, 1e3 * t_top, 1e3 * med, en[0, 0]))
        if k == 4:
            t_en, _, res = clock(lambda: plm.mutant_scan(target, q, h, J, sites, letters=letters * k, energies=True), reps)
            print("scan 20^4 with all energies returned: %.1f ms" % (1e3 * t_en))


if __name__ == "__main__":
    main()
