"""
The alignments on which the reweighting kernels are compared with the oracle (numpy only; no GPU, no library).

One builder for tests/test_reweight_cases_host.py (which proves on the CPU that the cases have pairs where a wrong kernel
would show) and tests/test_gpu_reweight.py (which runs them).  A case is an (msa, theta, flags) triple made
deterministically from its name; flags = PLM_FLAG_IGNORE_GAPS (2) | PLM_CONV_* bits, as plm_reweight_ex takes them.

Construction
  background   rows uniform over the states 1..20: pairwise identity about 5 %, far below every threshold used, so that
               most (wave, partner row) combinations of k_reweight_reg leave early.
  stars        a centre row and satellites copied from it whose identity to the centre, by the rule of the case's
               convention, is exactly thr + 1, thr or thr - 1 (k = +1, 0, -1; in plain mode: limit - 1, limit, limit + 1
               differing sites, limit = L - T).  The differing sites follow a layout: `tail` (the last sites of the row:
               a wave must not leave early), `head` (the first: a lane is over the limit after one chunk, its wave is
               not), `spread` (evenly spaced: every chunk and half chunk holds some), `last` (site L - 1 and random ones).
  placement    every (layout, k) is planted once per placement class: centre and satellite inside one 64-row wave among
               strangers, in different waves of one 256-row tile, across rows 255 | 256, and at rows 0 and N - 1; above
               N = 1000 also between random rows of the whole alignment (T ranges longer than one row).
  tail star    centre 40 with satellites in rows 41.. that differ in tail sites only and hold no gaps: its count is
               1 + #(satellites with k >= 0), a closed form that does not go through the oracle.
  -g overlays  in gap mode the centres get gaps (one of them followed by state 1, the borrow regression of zero_bytes),
               the satellites gap/gap, residue/gap and gap/residue sites, the other rows 3 % gaps; one row is all gaps
               and one is gapped exactly where its centre is not (n_both = 0).  Under PLM_CONV_G_UNGAPPED_LENGTH the
               satellites' gap counts differ, so n_both differs from pair to pair.
  state range  states up to 126 (`state-*`, which the library refuses) or 123 (`state123-*`, exact counts): satellites one
               site beyond the limit whose next row holds the top state in its first 32 bytes, and in gap mode
               satellites that hold top - 2 where the centre has a gap.
"""
import math
import zlib
from functools import lru_cache

import numpy as np

FLAG_IGNORE_GAPS = 2
CONV_F32, CONV_GAPS_IDENTICAL, CONV_UNGAPPED = 32, 64, 128
CONV_MASK = 32 | 64 | 128 | 256 | 512
LAYOUTS = ("tail", "head", "spread", "last")


def theta_grid(L):
    """searched for a float32 threshold that differs (bit 32): theta L an integer k in 0.5 L .. 0.95 L, or k +- 1e-6.
    The two rules part where float32 rounds (1 - (1 - theta)) L across an integer the other rule stays short of; for
    L = 65 and 130 no theta with two or three decimals does that."""
    return [(k + e) / L for k in range((L + 1) // 2, int(0.95 * L) + 1) for e in (0.0, 1e-6, -1e-6)]


def threshold(L, theta, conv=0):
    """identities a pair needs on the full length: ceil(theta L - 1e-9), or what a float32 plmc makes of -t 1-theta"""
    if conv & CONV_F32:
        t = np.float32(1.0 - theta)
        return int(np.ceil((np.float32(1.0) - t) * np.float32(L)))
    return int(math.ceil(theta * L - 1e-9))


def f32_theta(L):
    hits = [theta for theta in theta_grid(L) if threshold(L, theta, CONV_F32) != threshold(L, theta)]
    assert hits, "no theta of the grid separates the two thresholds at L = %d" % L
    return min(hits, key=lambda theta: abs(theta - 0.6))          # the one nearest the 0.6 of the other conventions


class Case:
    def __init__(self, name, **kw):
        self.name = name
        self.N = self.L = 0
        self.theta = 0.8
        self.flags = 0
        self.top = 20                 # largest state drawn
        self.reject = False           # holds states the library refuses
        self.background = "uniform"
        self.layouts = LAYOUTS
        self.family = ""
        self.__dict__.update(kw)
        self.gaps = bool(self.flags & FLAG_IGNORE_GAPS)
        self.conv = self.flags & CONV_MASK
        self.T = threshold(self.L, self.theta, self.conv)
        self.limit = min(max(self.L - self.T, 0), self.L)
        self.msa = None
        self.planted = []             # (centre, satellite, layout, k): identity = threshold + k by the case's rule
        self.tail_star = None         # (centre, [(satellite, k)])
        self.background_rows = np.zeros(0, np.int64)      # rows that are neither centre nor satellite
        self.beyond = []              # state range: (centre, satellite) one site beyond the limit, see module docstring

    # ---- the per-pair rule of the case's convention (oracle/plm_oracle.c reweight / reweight_gaps, restated) ----
    def pair_stats(self, a, B):
        """identities of row a with every row of B and the identities each pair needs"""
        B = np.atleast_2d(B)
        eq = B == a[None, :]
        if not self.gaps or ((self.conv & CONV_GAPS_IDENTICAL) and not (self.conv & CONV_UNGAPPED)):
            return eq.sum(axis=1), np.full(B.shape[0], self.T)
        ident = (eq & (a != 0)[None, :]).sum(axis=1)
        if self.conv & CONV_UNGAPPED:
            nb = ((a != 0)[None, :] & (B != 0)).sum(axis=1)
            return ident, np.ceil(self.theta * nb.astype(np.float64) - 1e-9).astype(np.int64)
        return ident, np.full(B.shape[0], self.T)

    def neighbours(self, s):
        """rows in the cluster of row s, by the rule above (the row itself always)"""
        ident, thr = self.pair_stats(self.msa[s], self.msa)
        hit = ident >= thr
        hit[s] = True
        return np.flatnonzero(hit)


def _params():
    P = {}

    def add(name, **kw):
        assert name not in P
        P[name] = kw

    G = FLAG_IGNORE_GAPS
    modes = (("plain", 0), ("gap", G))
    for L in (1, 2, 32, 33, 64, 65, 96, 97, 128, 129, 256, 257, 384, 385, 512, 513, 640, 768, 769, 1024):
        for mode, f in modes:
            add("sweep-L%d-%s" % (L, mode), family="sweep", N=400, L=L, theta=0.8, flags=f)
    for L in (512, 768, 800):
        for mode, f in modes:
            add("trange-L%d-%s" % (L, mode), family="trange", N=3000, L=L, theta=0.8, flags=f)
    for L in (40, 400):
        for N in (1, 2, 255, 256, 257):
            for mode, f in modes:
                add("tile-N%d-L%d-%s" % (N, L, mode), family="tile", N=N, L=L, theta=0.8, flags=f)
    for L in (25, 65, 130, 800):
        for conv in (128, 64, 64 | 128, 32, 32 | 128):
            theta = f32_theta(L) if conv & 32 else 0.6
            add("conv%d-L%d" % (conv, L), family="conv", N=300, L=L, theta=theta, flags=conv | (G if conv & (64 | 128) else 0))
    for L in (40, 385):
        for mode, f in modes:
            add("thr-zero-L%d-%s" % (L, mode), family="thr", N=400, L=L, theta=0.0, flags=f)
            add("thr-one-L%d-%s" % (L, mode), family="thr", N=400, L=L, theta=1.0, flags=f)
            add("thr-T1-L%d-%s" % (L, mode), family="thr", N=400, L=L, theta=0.5 / L, flags=f, background="classes")
            add("thr-integral-L%d-%s" % (L, mode), family="thr", N=400, L=L, theta=0.8, flags=f)
    for L in (8, 20, 72, 136, 64):
        for mode, f in modes:
            add("state-L%d-%s" % (L, mode), family="state", N=130, L=L, theta=0.5, flags=f, top=126, reject=True)
            add("state123-L%d-%s" % (L, mode), family="state", N=130, L=L, theta=0.5, flags=f, top=123)
    return P


PARAMS = _params()
NAMES = list(PARAMS)


def _background(c, rng):
    N, L = c.N, c.L
    if c.background == "classes":
        # 20 classes of rows: two rows of one class are equal, rows of two classes differ at every site; then up to
        # three sites per row are redrawn.  With T = 1 a uniform background would make every pair a neighbour.
        shift = rng.integers(0, 20, L)
        msa = (1 + (np.arange(N)[:, None] % 20 + shift[None, :]) % 20).astype(np.int8)
        for s in range(N):
            sites = rng.integers(0, L, rng.integers(0, 4))
            msa[s, sites] = rng.integers(1, 21, sites.size)
        return msa
    if c.top > 20:
        # the whole admitted range, the four largest states over-represented (half of all cells)
        low = rng.integers(0, c.top - 3, (N, L))
        high = rng.integers(c.top - 3, c.top + 1, (N, L))
        return np.where(rng.random((N, L)) < 0.5, high, low).astype(np.int8)
    return rng.integers(1, 21, (N, L)).astype(np.int8)


def _classes(c, rng):
    """placement classes: (tag, centre, candidate satellite rows)"""
    N = c.N
    cls = []
    if N > 128:
        cls.append(("wave", 70, [r for r in range(64, 128) if r != 70]))
    if N > 200:
        cls.append(("tile", 10, list(range(129, min(N, 255), 2))))
    if N == 257:                  # row 256 is the other side of the tile edge and row N - 1: the centre of both stars
        cls.append(("edge", 256, list(range(255, 215, -1))))
        cls.append(("ends", 256, [0, 1, 2, 3]))
        return cls
    if N > 256:
        cls.append(("edge", 255, list(range(256, min(N, 300)))))
    cls.append(("ends", 0, list(range(N - 1, max(N - 41, 63), -1))))
    if N > 1000:
        for k in range(6):
            rows = rng.permutation(np.arange(320, N - 41))
            cls.append(("far%d" % k, int(rows[0]), [int(r) for r in rows[1:201]]))
    return cls


def _other_state(c, rng, old):
    new = rng.integers(1, c.top + 1, old.shape)
    return np.where(new == old, old % c.top + 1, new).astype(np.int8)


def _sites(layout, cand, d, L, rng):
    if d == 0:
        return cand[:0]
    if layout == "tail":
        return cand[-d:]
    if layout == "head":
        return cand[:d]
    if layout == "spread":
        return cand[(np.arange(d) * cand.size) // d]
    rest = cand[cand != L - 1]
    if rest.size == cand.size:
        return rng.permutation(rest)[:d]
    return np.concatenate([[L - 1], rng.permutation(rest)[:d - 1]])


def _satellite(c, rng, msa, centre, protected, layout, k, j=0, overlay=False):
    """a copy of row `centre` at identity threshold + k by the case's rule, or None where that cannot be had"""
    a = msa[centre]
    sat = a.copy()
    free = np.ones(c.L, bool)
    free[list(protected)] = False
    if overlay:
        cg = np.flatnonzero(a == 0)
        if j % 2 and cg.size:                                          # a residue against the centre's gap
            sel = cg[::2]
            sat[sel] = rng.integers(1, c.top + 1, sel.size)
        if c.conv & CONV_UNGAPPED:
            g = (j % 5) * max(1, c.L // 16)                            # n_both differs from pair to pair
        else:
            g = min(j % 4, c.limit // 3)
        res = np.flatnonzero((a != 0) & free)
        sat[rng.permutation(res)[:min(g, res.size // 2)]] = 0          # a gap against the centre's residue
    ident, thr = c.pair_stats(a, sat)
    d = int(ident[0] - thr[0]) - k
    same = (sat == a) & free
    if c.gaps:
        same &= a != 0
    cand = np.flatnonzero(same)
    if d < 0 or d > cand.size:
        return None
    sites = _sites(layout, cand, d, c.L, rng)
    sat[sites] = _other_state(c, rng, sat[sites])
    return sat


@lru_cache(maxsize=None)
def build(name):
    """the case of that name; built once and shared, its alignment read-only"""
    c = _build(name)
    c.msa.flags.writeable = False
    return c


def _build(name):
    c = Case(name, **PARAMS[name])
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    N, L = c.N, c.L
    msa = _background(c, rng)
    c.msa = msa
    if N == 1:
        return c
    if N == 2:                      # the one pair there is: at the threshold (L = 40), one below it (L = 400)
        k = 0 if L == 40 else -1
        msa[1] = _satellite(c, rng, msa, 0, (), "tail", k)
        c.planted.append((0, 1, "tail", k))
        c.layouts = ()
        return c
    cls = _classes(c, rng)
    used = {40} | {centre for _, centre, _ in cls}
    state_rows = set(range(5, 38)) if c.family == "state" else set()
    used |= state_rows

    # ---- gaps of the centres (gap mode): one gap followed by state 1 inside a dword, others at random
    protected = {centre: set() for _, centre, _ in cls}
    if c.gaps:
        ngc = min(4, c.limit // 3) if c.T > 1 else 0        # (T <= 1: a protected identity would keep a pair from 0)
        for _, centre, _ in cls:
            if ngc >= 1 and L >= 8:
                i = int(rng.integers(0, L - 1))
                i -= 1 if i % 4 == 3 else 0
                msa[centre, i], msa[centre, i + 1] = 0, 1
                protected[centre].add(i + 1)
                others = [s for s in rng.permutation(L)[:ngc + 1] if s not in (i, i + 1)][:ngc - 1]
                msa[centre, others] = 0

    # ---- the stars: every (layout, k) once per placement class
    reps = 4 if N < 200 else 8 if N < 1000 else 24
    pools = [list(rows) for _, _, rows in cls]
    j = 0
    for layout in c.layouts:
        for k in (1, 0, -1):
            for rep in range(reps):
                j += 1
                for q in range(len(cls)):
                    ci = (rep + q) % len(cls)
                    pool = [r for r in pools[ci] if r not in used and 0 <= r < N]
                    if pool:
                        break
                else:
                    continue
                centre, row = cls[ci][1], pool[0]
                sat = _satellite(c, rng, msa, centre, protected[centre], layout, k, j, overlay=c.gaps)
                if sat is None:
                    continue
                msa[row] = sat
                used.add(row)
                c.planted.append((centre, row, layout, k))

    # ---- the tail star: no gaps, tail sites only
    if N > 64:
        sats = []
        for n, k in enumerate((1, 0, -1, 1, 0, -1)):
            sat = _satellite(c, rng, msa, 40, (), "tail", k)
            if sat is not None:
                msa[41 + n] = sat
                used.add(41 + n)
                sats.append((41 + n, k))
        c.tail_star = (40, sats)

    # ---- state range: what lies next to the values the kernels fill with
    if c.family == "state":
        for n in range(8):                                   # centre 5, satellites 20, 22, ..: one site beyond the limit,
            t = 20 + 2 * n                                   # the row after each holds the top state early
            sat = _satellite(c, rng, msa, 5, (), LAYOUTS[n % 4], -1)
            if sat is None:
                continue
            msa[t] = sat
            msa[t + 1, rng.integers(0, min(L, 32))] = c.top
            c.beyond.append((5, t))
        if c.gaps:                                           # centre 6 has a gap where satellites 8.. hold top - 2
            g0 = int(rng.integers(0, L))
            msa[6, g0] = 0
            for n in range(8):
                sat = _satellite(c, rng, msa, 6, (g0,), LAYOUTS[n % 4], -1)
                if sat is None:
                    continue
                sat[g0] = c.top - 2
                msa[8 + n] = sat
                c.beyond.append((6, 8 + n))

    # ---- gap mode: gaps in the other rows, an all-gap row, a row gapped wherever its centre is not
    if c.gaps:
        rest = np.array([r for r in range(N) if r not in used])
        if rest.size > 2:
            msa[rest[0]] = 0
            centre = cls[0][1]
            msa[rest[1]] = np.where(msa[centre] != 0, 0, rng.integers(1, 21, L)).astype(np.int8)
            used |= {int(rest[0]), int(rest[1])}
            body = rest[2:]
            holes = rng.random((body.size, L)) < 0.03
            msa[body] = np.where(holes, 0, msa[body])
    c.background_rows = np.array([r for r in range(N) if r not in used], dtype=np.int64)
    return c


def oracle_counts(oracle, case):
    """what the case's counts must be: oracle.reweight / reweight_gaps under the case's conventions"""
    oracle.set_conventions(case.conv)
    try:
        return (oracle.reweight_gaps if case.gaps else oracle.reweight)(case.msa, case.theta)
    finally:
        oracle.set_conventions(0)
