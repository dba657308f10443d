"""
GPU: the field solver of the variable-projection fit stage by stage against tests/field_solver_twin.py.
Every stage is fed with what the GPU produced before it, so that a failure names its kernel:
  counts    k_site_counts                    hcnt against the twin's f64 counts, within N 2^-53 sum(w)
  partials  k_hpass<Q, WRITE_RT, STATS, XACT>  gpart / dpart / hpart (and, residual role, the -log P partials) of every
                                             (block, tile) in the three roles and both arithmetics, against the twin; what
                                             a launch does not own stays unwritten (0xFF prefill of the probe), padding
                                             sites are exactly zero
  solve     k_hsolve                         from the GPU's raw partials the twin predicts hinv, g2_site, the summed norm
                                             and the stepped fields (fresh and cached inverses, update = 0, cap binding)
  chain     vp_chain / ctx_eval_vp_enqueue / ctx_eval_vp_finish / k_vp_check / k_fields_to_x
                                             the reported norm is the twin's at the returned fields, the stop rule, the
                                             distance to h*, x = f32(fields), planes and gradient those of the returned
                                             point (oracle), both values of final_skip, a continued chain
  quiet     PlmVpState::quiet                a block at h* is flagged, stops moving, and keeps its share of the norm
through the diagnostic entry points plm_ctx_field_position / plm_ctx_field_solve.  No entry of any comparison is excluded.

Tolerances of the pass partials.  Yardstick: the twin evaluated in float32 (f32 potentials and softmax, f64 accumulation);
e32 = its largest miss against the f64 twin per tile; the GPU may miss by K e32; the second-order sums (hpart and the
diagonal sums dpart, which k_hsolve uses interchangeably) by K e32 + 2^-24 sum_tile w; the -log P partials by K e32 +
2^-23 of the partial; in the plain arithmetic everything + 3e-11 N L max(1, |x|) (the host's model of the forward
GEMM's error, fwd_noise of plm_ctx_optimize).  K = the next power of two above twice the worst ratio observed on an
MI355X (every test prints its ratios before it asserts), over all roles:
    gradient sums, tiles     1      2      33     65     130    258
      accurate               8.7    8.0    10.4   11.1   12.9   10.5      -> K = 32
      plain                  8.7    0      0      0      0      0         -> K = 32   (without its allowance 13.1 at most)
    diagonal / Hessian / -log P: 0 in every case with their derivable terms; without them
      diagonal sums          31.6   14.9   10.9   11.0   11.7   10.1
      Hessian sums           28.8   7.6    10.1   7.7    9.4    8.4
      -log P                 15.9   181    199    1.8e3  5.6e4  2.0e3
Two of these are findings above 16, explained from k_hpass and not adopted into K: (1) the observed state's P is rebuilt as
1 - sum of the others (exact where P is near 1, the case the gradient needs), an ABSOLUTE error of 2^-24 per sequence where
the f32 twin has a relative one -- with one sequence in a tile and P_x = 0.04 that is 31.6 e32 in sum w P_a^2, and it is
what the 2^-24 sum_tile w term covers; (2) the -log P terms are formed from the hardware's log2 (one ulp, the same sign in
every sequence) and added up in f32 per thread before the f64 sum over the workgroup: a coherent error of up to 1.2 x 2^-24 of
the partial, against a twin whose f64-accumulated miss averages out -- hence the 2^-23 term (one ulp of the partial; the GPU
used up to 0.6 of it, and up to 0.93 of the 2^-24 sum_tile w term of the diagonal sums).
Solve: the GPU's hinv within 10x (observed: 4.7x) the gap between the twin's Gauss-Jordan inverse and numpy.linalg.inv of
the same matrices -- the largest gap of the call relative to the inverse's largest entry: site by site the two routes share
most of their rounding (see check_solve) --, the stepped fields within the same multiple times |g|_1, plus the rounding of
the f64 gradient sums themselves.  (The scales k_hsolve puts on the sampled sums -- nstiles / nsamp, 4 above 21 states -- are
applied by the twin as by the kernel, but the Sinkhorn rescaling divides any common factor out again: a wrong scale would
not show in hinv beyond rounding, a wrong tile, row part, diagonal source or state would.)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_solver_twin as tw  # noqa: E402

from evcouplings_amd._lib import PlmError  # noqa: E402
from evcouplings_amd.synthetic import synthetic_msa  # noqa: E402

pytestmark = pytest.mark.gpu
PLM_EINVAL, PLM_EUNSUPPORTED = -1, -4
LAM = 0.01
K_ACCURATE, K_PLAIN = 32.0, 32.0          # see the module docstring

SMALL = [(1, 2), (257, 17)]
LARGE = [(8193, 16), (16385, 16), (33025, 16)]
CASES = ([(N, L, q, False) for (N, L) in SMALL for q in (4, 5, 20, 21, 32, 7, 25)] + [(N, L, 21, True) for (N, L) in SMALL]
         + [(N, L, q, False) for (N, L) in LARGE for q in (21, 32)] + [(65793, 16, 21, False)])


def case_id(c):
    return "N%d-L%d-q%d%s" % (c[0], c[1], c[2], "-gaps" if c[3] else "")


@pytest.fixture(scope="module")
def plm():
    from evcouplings_amd import plm as _plm
    assert _plm.device_count() >= 1, "no gfx950 device: the HIP path has no fallback"
    return _plm


def edge_msa(N, L, q, seed):
    """the planted alignment, with (N >= 257, L >= 4) a state no sequence carries at site 2 and a state carried only by
    sequence 256 -- tile 1, never a sampled one -- at site 3"""
    msa, _ = synthetic_msa(N, L, seed=seed, q=q)
    if N >= 257 and L >= 4 and q >= 4:
        col = msa[:, 2]
        col[col == q - 1] = 1
        col = msa[:, 3]
        col[col == 2] = 1
        col[256] = 2
    return msa


class Case:
    """one alignment resident on the GPU with weights from reweight, a point x = scale * normal, and the twin's sums there
    (computed once, never changed)"""

    def __init__(self, plm, N, L, q, gap, scale=0.1, seed=7):
        self.N, self.L, self.q, self.gap = N, L, q, gap
        self.Q, self.T, self.B = tw.q_template(q), tw.n_tiles(N), (L + 15) // 16
        self.S, self.a0, self.qm = 16 * self.B, (1 if gap else 0), (q - 1 if gap else q)
        self.live = tw.live_states(q, gap)
        self.msa = edge_msa(N, L, q, seed + N + q)
        self.ctx = plm.PlmContext(self.msa, q=q, lambda_h=LAM, ignore_gaps=gap)
        assert self.ctx.field_dims() == (self.Q, self.T, self.B)
        self.w = self.ctx.reweight()[0]
        rng = np.random.default_rng(seed)
        self.x = (scale * rng.normal(size=plm.n_params(L, self.qm))).astype(np.float32)
        self.ctx.set_x(self.x)
        self.xnorm = float(np.sqrt((self.x.astype(np.float64) ** 2).sum()))
        self.fwd_noise = 3e-11 * N * L * max(1.0, self.xnorm)
        HJ, self.h = tw.potentials(self.msa, self.x, q, gap)
        self.s64 = tw.tile_sums(HJ, self.h, self.msa, self.w, q, gap)
        self.s32 = tw.tile_sums(HJ, self.h, self.msa, self.w, q, gap, dtype=np.float32)
        self.HJ = HJ if N <= 1024 else None

    def sums_at(self, h, dtype=np.float64):
        return tw.tile_sums(self.HJ, h, self.msa, self.w, self.q, self.gap, dtype=dtype)

    def fields_of(self, x):
        """(S, Q): the f64 fields k_h64_init makes of the canonical f32 vector x"""
        h = np.zeros((self.S, self.Q))
        h[:self.L, self.a0:self.q] = np.asarray(x[:self.L * self.qm], np.float32).astype(np.float64).reshape(self.L, self.qm)
        return h

    def with_fields(self, h):
        x = self.x.copy()
        x[:self.L * self.qm] = np.asarray(h)[:self.L, self.a0:self.q].ravel()
        return x

    def tiles(self, part):
        """[block][tile][16][X] -> ([tile][L][X], the padding sites' part)"""
        s = tw.sites_of(part)
        return s[:self.L].transpose(1, 0, 2), s[self.L:]


_cases = {}


@pytest.fixture(scope="module")
def cases(plm):
    def get(key, **kw):
        k = (key, tuple(sorted(kw.items())))
        if k not in _cases:
            _cases[k] = Case(plm, *key, **kw)
        return _cases[k]
    yield get
    for c in _cases.values():
        c.ctx.close()
    _cases.clear()


def k_of(accurate):
    return K_ACCURATE if accurate else K_PLAIN


def per_tile(gpu, t64, t32):
    T, n = t64.shape[0], int(np.prod(t64.shape[1:]))
    return (np.abs(gpu - t64).reshape(T, n).max(axis=1, initial=0.0), np.abs(t32 - t64).reshape(T, n).max(axis=1, initial=0.0))


def report(stage, c, role, accurate, err, e32, extra):
    """worst ratio (err - extra) / e32 over the tiles, printed before anything is asserted"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e32 > 0, np.maximum(err - extra, 0.0) / e32, np.where(err - extra > 0, np.inf, 0.0))
        raw = np.where(e32 > 0, err / e32, 0.0)
        share = np.where(np.asarray(extra) > 0, err / np.where(np.asarray(extra) > 0, extra, 1.0), 0.0)
    print("\nRATIO %-5s %-22s %-8s %-8s worst=%.3g (tile %d of %d; without the allowance %.3g; err / allowance %.3g) "
          "max_err=%.3g max_e32=%.3g allowance=%.3g"
          % (stage, case_id((c.N, c.L, c.q, c.gap)), role, "accurate" if accurate else "plain", r.max(), int(r.argmax()),
             len(r), raw.max(), np.max(share), err.max(), e32.max(), np.max(extra)))
    return float(r.max())


# ---------------------------------------------------------------- counts
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_counts(cases, key):
    c = cases(key)
    out = c.ctx.field_position("stats", update=False)
    want = c.s64["cnt"].sum(axis=0)
    wsum = float(c.w.astype(np.float64).sum())
    err = np.abs(out["hcnt"][:c.L] - want).max()
    print("COUNTS %s max err %.3g bound %.3g" % (case_id(key), err, c.N * 2.0 ** -53 * wsum))
    assert err <= c.N * 2.0 ** -53 * wsum
    assert not out["hcnt"][c.L:].any()
    assert not out["hcnt"][:, ~c.live].any()


# ---------------------------------------------------------------- pass partials
@pytest.mark.parametrize("accurate", [False, True], ids=["plain", "accurate"])
@pytest.mark.parametrize("role", ["stats", "hessian", "residual"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_pass_partials(cases, key, role, accurate):
    c = cases(key)
    K, noise = k_of(accurate), (0.0 if accurate else c.fwd_noise)
    out = c.ctx.field_position(role, accurate=accurate, update=False, prefill=True)
    sampled = np.zeros(c.T, bool)
    sampled[::tw.SAMPLE] = True
    g, gpad = c.tiles(out["gpart"])
    d, dpad = c.tiles(out["dpart"])
    hp, hpad = c.tiles(out["hpart"])
    checks = []
    # gradient sums: every tile, every role
    err, e32 = per_tile(g, c.s64["g"], c.s32["g"])
    report("grad", c, role, accurate, err, e32, noise)
    checks.append(("gpart", err, K * e32 + noise))
    assert not gpad.any(), "padding sites of the gradient sums are not zero"
    assert not g[:, :, ~c.live].any(), "dead states carry gradient sums"
    if role == "hessian":
        own_d = np.ones(c.T, bool) if c.Q > 21 else ~sampled
        err, e32 = per_tile(d[own_d], c.s64["d"][own_d], c.s32["d"][own_d])
        if own_d.any():
            extra = noise + 2.0 ** -24 * c.s64["wsum"][own_d]
            report("diag", c, role, accurate, err, e32, extra)
            checks.append(("dpart", err, K * e32 + extra))
        assert np.isnan(d[~own_d]).all() and np.isnan(dpad[:, ~own_d]).all(), "diagonal sums written on a sampled tile"
        assert not dpad[:, own_d].any()
        M = tw.tri_to_full(hp[sampled].astype(np.float64), c.Q)
        M32 = c.s32["M"]
        err, e32 = per_tile(M, c.s64["M"], M32)
        extra = noise + 2.0 ** -24 * c.s64["wsum"][sampled]
        report("hess", c, role, accurate, err, e32, extra)
        checks.append(("hpart", err, K * e32 + extra))
        assert np.isnan(hp[~sampled]).all() and np.isnan(hpad[:, ~sampled]).all(), "Hessian sums written off the sampled tiles"
        assert not hpad[:, sampled].any()
    else:
        assert np.isnan(out["dpart"]).all() and np.isnan(out["hpart"]).all()
    if role == "residual":
        nll = out["nll_part"]                                                            # [block][tile]
        n64 = np.stack([c.s64["nll"][:, 16 * b:16 * b + 16].sum(axis=1) for b in range(c.B)])
        n32 = np.stack([c.s32["nll"][:, 16 * b:16 * b + 16].sum(axis=1) for b in range(c.B)])
        err, e32 = np.abs(nll - n64).max(axis=0), np.abs(n32 - n64).max(axis=0)
        # the -log P terms come from the hardware's f32 log2 (accurate to one ulp, not half of one) and are accumulated
        # in f32 per thread before the f64 sum over the workgroup: one f32 ulp of the partial itself on top of K e32
        extra = noise + 2.0 ** -23 * np.abs(n64).max(axis=0)
        report("nll", c, role, accurate, err, e32, extra)
        checks.append(("nll", err, K * e32 + extra))
    else:
        assert np.isnan(out["nll_part"]).all()
    assert np.isnan(out["h64"][1]).all(), "an unchained position touched the second field buffer"
    assert np.array_equal(out["h64"][0][:c.L], c.fields_of(c.x)[:c.L]), "update = 0 moved a field"
    for name, err, bound in checks:
        bound = np.broadcast_to(bound, err.shape)
        if len(err):
            k = int((err - bound).argmax())
            assert err[k] <= bound[k], "%s: tile %d misses the twin by %.3g, bound %.3g" % (name, k, err[k], bound[k])


# ---------------------------------------------------------------- solve
def check_solve(c, out, h_start, full, inv_prev=None, update=True, tag=""):
    """k_hsolve against the twin's prediction from the GPU's own partials; -> the prediction"""
    L, Q = c.L, c.Q
    gp, dp, hp = tw.sites_of(out["gpart"]), tw.sites_of(out["dpart"]), tw.sites_of(out["hpart"])
    pred = tw.predict_solve(gp, dp, hp, out["hcnt"], h_start, LAM, c.a0, full, inv_prev, update)
    gr = pred["gr"]
    # rounding of the f64 gradient sums: T + 3 additions on the magnitudes that cancel in them
    dgr = (c.T + 3) * 2.0 ** -53 * (np.abs(gp).sum(axis=1) + 2 * LAM * np.abs(h_start))
    dg2 = (2 * np.abs(gr) * dgr + dgr ** 2).sum(axis=1) + Q * 2.0 ** -52 * pred["g2_site"]
    e = np.abs(out["g2_site"] - pred["g2_site"])
    print("SOLVE%s %s g2_site: worst share of its bound %.3g" % (tag, case_id((c.N, c.L, c.q, c.gap)),
                                                               np.max(e[:L] / np.maximum(dg2[:L], 1e-300))))
    assert (e[:L] <= dg2[:L]).all()
    assert not out["g2_site"][L:].any()
    tot = out["g2_site"].sum()
    assert abs(out["g2_sum"][0] - tot) <= c.S * 2.0 ** -53 * tot
    gapv = np.zeros(c.S)
    if full:
        # the yardstick of the call: the largest gap of its sites relative to the inverse's largest entry.  (Site by site
        # the two routes share most of their rounding and now and then agree 30-170 times better than either is right --
        # a one-ulp change of H then moves the inverse by 50-170 of THAT site's gap: measured on the CPU, N = 8193.)
        site_gap = tw.inverse_gap(pred["H"], pred["inv"])
        scale = np.abs(pred["inv"]).max(axis=(1, 2))
        gapv = (site_gap[:L] / scale[:L]).max() * scale
        e = np.abs(out["hinv"] - pred["inv"]).max(axis=(1, 2))
        print("SOLVE%s hinv: worst ratio to the call's Gauss-Jordan / LU gap %.3g (to the site's own gap %.3g)"
              % (tag, np.max(e[:L] / gapv[:L]), np.max(e[:L] / site_gap[:L])))
        assert (e[:L] <= 10 * gapv[:L]).all()
    elif inv_prev is not None:
        assert np.array_equal(out["hinv"][:L], inv_prev[:L]), "a position without Hessian sums rewrote the cached inverses"
    inv = np.abs(pred["inv"][:L]) if pred["inv"] is not None else np.zeros((L, Q, Q))
    ddh = (10 * gapv[:L, None] * np.abs(gr[:L]).sum(axis=1, keepdims=True) + np.einsum("sab,sb->sa", inv, dgr[:L])
           + Q * 2.0 ** -52 * np.einsum("sab,sb->sa", inv, np.abs(gr[:L])))
    bound = np.where(pred["cap"][:L, None] < 1, 2.0, 1.0) * ddh + 2.0 ** -51 * (np.abs(h_start[:L]) + tw.CAP)
    e = np.abs(out["h64"][0][:L] - pred["h_new"][:L])
    if update:
        print("SOLVE%s fields: worst share of the bound %.3g, capped sites %d" % (tag, np.max(e / bound),
                                                                                 int((pred["cap"][:L] < 1).sum())))
        assert (e <= bound).all()
        assert not (out["h64"][0][:L] - h_start[:L])[:, ~c.live].any(), "a dead state's field moved"
    else:
        assert np.array_equal(out["h64"][0][:L], h_start[:L])
    return pred


SOLVE_CASES = [(257, 17, 21, False), (257, 17, 32, False), (257, 17, 7, False), (257, 17, 21, True), (8193, 16, 21, False),
               (65793, 16, 21, False), (8193, 16, 32, False)]


@pytest.mark.parametrize("key", SOLVE_CASES, ids=case_id)
def test_solve_fresh_inverse(cases, key):
    """0.1 normal (the case's own point): Hessian position, fresh inverse, step; then update = 0"""
    c = cases(key)
    c.ctx.set_x(c.x)
    h0 = c.fields_of(c.x)
    out = c.ctx.field_position("hessian", accurate=True, update=True)
    check_solve(c, out, h0, full=True)
    x1 = c.ctx.get_x()
    assert np.array_equal(x1[:c.L * c.qm].reshape(c.L, c.qm), out["h64"][0][:c.L, c.a0:c.q].astype(np.float32))
    assert np.array_equal(x1[c.L * c.qm:], c.x[c.L * c.qm:])
    c.ctx.set_x(c.x)
    out0 = c.ctx.field_position("hessian", accurate=True, update=False)
    check_solve(c, out0, h0, full=True, update=False, tag="(update=0)")
    assert np.array_equal(c.ctx.get_x(), c.x)
    assert np.array_equal(out0["hinv"][:c.L], out["hinv"][:c.L]) and np.array_equal(out0["gpart"], out["gpart"])


@pytest.mark.parametrize("key", [(257, 17, 21, False), (257, 17, 21, True), (257, 17, 32, False)], ids=case_id)
def test_solve_far_start_caps_the_step(cases, key):
    c = cases(key)
    rng = np.random.default_rng(31)
    h = c.fields_of(c.x)
    h[:c.L, c.a0:c.q] = (8.0 * rng.normal(size=(c.L, c.qm))).astype(np.float32)
    c.ctx.set_x(c.with_fields(h))
    for accurate in (False, True):
        c.ctx.set_x(c.with_fields(h))
        out = c.ctx.field_position("hessian", accurate=accurate, update=True)
        pred = check_solve(c, out, h, full=True, tag="(8 normal, %s)" % ("accurate" if accurate else "plain"))
        assert (pred["cap"][:c.L] < 1).any(), "the cap does not bind at this start"
        move = np.abs(out["h64"][0][:c.L] - h[:c.L]).max(axis=1)
        assert (move <= tw.CAP * (1 + 2.0 ** -50)).all()
        assert np.allclose(move[pred["cap"][:c.L] < 1], tw.CAP, rtol=2.0 ** -48, atol=0)
    c.ctx.set_x(c.x)


@pytest.mark.parametrize("key", [(257, 17, 21, False), (257, 17, 21, True), (257, 17, 5, False)], ids=case_id)
def test_solve_near_the_optimum_and_cached_inverse(cases, key):
    c = cases(key)
    hstar, _, _ = tw.solve_exact(c.HJ, c.h, c.msa, c.w, c.q, LAM, c.gap, tol=1e-9)
    xs = c.with_fields(hstar)
    hs = c.fields_of(xs)
    c.ctx.set_x(xs)
    out = c.ctx.field_position("hessian", accurate=True, update=True)
    pred = check_solve(c, out, hs, full=True, tag="(near h*)")
    assert np.sqrt(pred["g2_sum"]) < 1e-3 * np.sqrt(c.N * c.L), "not near the optimum"
    # a cached inverse: the next positions at another point step with what the Hessian position left
    inv0 = out["hinv"].copy()
    rng = np.random.default_rng(32)
    h1 = hs.copy()
    h1[:c.L, c.a0:c.q] = (hs[:c.L, c.a0:c.q] + 0.05 * rng.normal(size=(c.L, c.qm))).astype(np.float32)
    for role in ("stats", "residual"):
        for accurate in (False, True):
            c.ctx.set_x(c.with_fields(h1))
            o = c.ctx.field_position(role, accurate=accurate, update=True)
            check_solve(c, o, h1, full=False, inv_prev=inv0, tag="(cached, %s)" % role)
    c.ctx.set_x(c.x)


# ---------------------------------------------------------------- chain
def twin_norm(c, fields, accurate):
    """|grad_h f| of the twin at the GPU's fields, and how far the GPU's own norm may be from it: the partials' bound
    summed over the tiles (every entry), in norm over the L Q entries"""
    h = fields[:c.L]
    s64, s32 = c.sums_at(h), c.sums_at(h, np.float32)
    g = tw.field_gradient(s64, h, LAM, c.live)
    e32 = np.abs(s32["g"] - s64["g"]).reshape(c.T, -1).max(axis=1).sum()
    delta = np.sqrt(c.L * c.Q) * k_of(accurate) * e32 + (0.0 if accurate else c.fwd_noise)
    return float(np.sqrt((g * g).sum())), float(delta)


def check_chain(c, oracle64, r, tol, accurate, tag):
    L, qm = c.L, c.qm
    norm, delta = twin_norm(c, r["fields"], accurate)
    floor = 2e-7 * np.sqrt(float(c.w.astype(np.float64).sum()) * L * c.q)
    print("CHAIN %s %s: passes=%d done=%d cont=%d final_skip=%d want_rt=%d cur=%d |g_h| gpu=%.4e twin=%.4e delta=%.2e "
          "tol=%.3e floor=%.2e quiet=%s" % (case_id((c.N, c.L, c.q, c.gap)), tag, r["passes"], r["done"], r["continuations"],
                                            r["final_skip"], r["want_rt"], r["cur"], np.sqrt(r["gh2"]), norm, delta, tol,
                                            floor, r["quiet"][:c.B].tolist()))
    assert abs(np.sqrt(r["gh2"]) - norm) <= delta
    if r["done"] and norm > floor:
        assert norm <= tol
    hstar, nstar, _ = tw.solve_exact(c.HJ, r["fields"][:L], c.msa, c.w, c.q, LAM, c.gap, tol=1e-10)
    assert np.sqrt(((r["fields"][:L] - hstar) ** 2).sum()) <= (norm + nstar) / (2 * LAM)
    x = c.ctx.get_x()
    assert np.array_equal(x[:L * qm].reshape(L, qm), r["fields"][:L, c.a0:c.q].astype(np.float32))
    assert np.array_equal(x[L * qm:], c.x[L * qm:])
    # planes and gradient are those of the returned point: the oracle at get_x(), tolerances of test_eval_matches_oracle
    ev = oracle64.eval_gaps if c.gap else oracle64.eval
    fx_o, nll_o, g_o = ev(c.msa, c.w.astype(np.float64), c.q, LAM, c.ctx.lambda_j, x.astype(np.float64))
    assert r["fx"] == pytest.approx(fx_o, rel=2e-6)
    assert r["nll"] == pytest.approx(nll_o, rel=2e-6)
    g = c.ctx.get_g()
    gj, gj_o = g[L * qm:], g_o[L * qm:]
    np.testing.assert_allclose(gj, gj_o, atol=2e-5 * np.abs(gj_o).max(), rtol=2e-5)
    assert not g[:L * qm].any(), "the reduced gradient has a field part"


@pytest.mark.parametrize("key", [(257, 17, 21, False), (257, 17, 21, True), (257, 17, 32, False)], ids=case_id)
def test_chain(cases, oracle64, key):
    c = cases(key)
    tols = {"loose": 1e-2 * max(1.0, c.xnorm), "default": 0.1 * 1e-3 * max(1.0, c.xnorm)}
    # two starts: the case's own point (0.1 normal: every chain runs out of positions and is continued) and one a step
    # away from the optimum (chains that end inside their positions, in either role)
    hstar, _, _ = tw.solve_exact(c.HJ, c.h, c.msa, c.w, c.q, LAM, c.gap, tol=1e-9)
    near = np.zeros((c.S, c.Q))
    near[:c.L] = np.where(c.live, hstar + 1e-3 * np.random.default_rng(61).normal(size=hstar.shape), 0.0)
    starts = {"0.1 normal": c.x, "near h*": c.with_fields(near)}
    skips, conts = set(), set()
    for sname, x0 in starts.items():
        for tname, tol in tols.items():
            for c_prev in (0, 2):
                for fresh in (True, False):
                    for accurate in (False, True):
                        c.ctx.set_x(x0)
                        if not fresh:      # inverses cached by a Hessian position at the same point
                            c.ctx.field_position("hessian", accurate=accurate, update=False)
                        r = c.ctx.field_solve(tol, vp_c_prev=c_prev, invalidate=fresh, accurate=accurate)
                        check_chain(c, oracle64, r, tol, accurate, "%s %s c_prev=%d %s %s" % (
                            sname, tname, c_prev, "fresh" if fresh else "cached", "accurate" if accurate else "plain"))
                        assert r["done"]
                        skips.add(r["final_skip"])
                        conts.add(min(r["continuations"], 1))
    assert skips == {0, 1}, "only final_skip = %s occurred" % sorted(skips)
    assert conts == {0, 1}, "chains continued by the host: only %s occurred" % sorted(conts)
    c.ctx.set_x(c.x)


@pytest.mark.parametrize("key", [(257, 17, 21, False), (257, 17, 32, False)], ids=case_id)
def test_chain_that_runs_out_of_positions_is_continued(cases, oracle64, key):
    c = cases(key)
    rng = np.random.default_rng(41)
    h = c.fields_of(c.x)
    h[:c.L, c.a0:c.q] = (8.0 * rng.normal(size=(c.L, c.qm))).astype(np.float32)
    c.ctx.set_x(c.with_fields(h))
    tol = 0.1 * 1e-3 * max(1.0, c.xnorm)
    r = c.ctx.field_solve(tol, vp_c_prev=0, invalidate=True, accurate=False)
    check_chain(c, oracle64, r, tol, False, "far start")
    assert r["continuations"] >= 1
    c.ctx.set_x(c.x)


# ---------------------------------------------------------------- quiet blocks
def test_quiet_block_stops_moving_and_keeps_its_share(cases, oracle64):
    c = cases((257, 32, 21, False))
    hstar, _, _ = tw.solve_exact(c.HJ, c.h, c.msa, c.w, c.q, LAM, c.gap, tol=1e-10)
    rng = np.random.default_rng(51)
    h = c.fields_of(c.with_fields(hstar))                     # block 0 at h* (rounded to f32), block 1 perturbed
    h[16:c.L] = (h[16:c.L] + 0.5 * rng.normal(size=(c.L - 16, c.Q))).astype(np.float32)
    x0 = c.with_fields(h)
    tol = 0.1 * 1e-3 * max(1.0, c.xnorm)
    c.ctx.set_x(x0)
    first = c.ctx.field_position("hessian", accurate=False, update=True)      # the chain's first position, unchained
    c.ctx.set_x(x0)
    r = c.ctx.field_solve(tol, vp_c_prev=2, invalidate=True, accurate=False)
    check_chain(c, oracle64, r, tol, False, "quiet")
    moved = np.abs(r["fields"][:16] - h[:16]).max()
    print("QUIET passes=%d quiet=%s block 0 moved by %.3e from its input, by %.3e from the first position's step"
          % (r["passes"], r["quiet"][:2].tolist(), moved, np.abs(r["fields"][:16] - first["h64"][0][:16]).max()))
    assert r["passes"] >= 3, "the chain was too short to skip anything"
    assert r["quiet"][0] == 1
    # The flag is raised by k_vp_check BEHIND the first position's Newton step (every site steps at every position), so
    # the fields the block keeps are those of that step -- the same launches as the unchained Hessian position above,
    # bit for bit -- not the ones it came with (measured: 4.2e-6 from the input, 0 from that step); from then on
    # nothing moves it, whatever the other block does.
    assert np.array_equal(r["fields"][:16], first["h64"][0][:16]), "a quiet block moved after it was flagged"
    # ... and that one step is no longer than |g| / (2 lambda_h) of the block's gradient at the input (H >= 2 lambda_h)
    assert moved <= np.sqrt(first["g2_site"][:16].sum()) / (2 * LAM)
    c.ctx.set_x(c.x)


# ---------------------------------------------------------------- errors
def test_refusals(plm, cases):
    c = cases((257, 17, 21, False))
    lib = c.ctx.lib
    with plm.PlmContext(c.msa, q=21, lambda_h=LAM, n_shards=2, shard=0) as sharded:
        sharded.set_weights(c.w)
        for call in (lambda: sharded.field_position("stats"), lambda: sharded.field_solve(1e-3)):
            with pytest.raises(PlmError) as e:
                call()
            assert e.value.code == PLM_EUNSUPPORTED
    with plm.PlmContext(c.msa, q=21, lambda_h=LAM, joint=True) as joint:
        joint.set_weights(c.w)
        for call in (lambda: joint.field_position("stats"), lambda: joint.field_solve(1e-3)):
            with pytest.raises(PlmError) as e:
                call()
            assert e.value.code == PLM_EINVAL
    assert lib.plm_ctx_field_position(c.ctx._h, 0, 0, 0, 0, None) == PLM_EINVAL
    assert lib.plm_ctx_field_solve(c.ctx._h, 1e-3, 0, 0, 0, None, None, 0) == PLM_EINVAL
    from evcouplings_amd import _lib
    buf = _lib.PlmFieldBuffers()                               # every pointer NULL
    assert lib.plm_ctx_field_position(c.ctx._h, 0, 0, 0, 0, buf) == PLM_EINVAL
    with plm.PlmContext(c.msa, q=21, lambda_h=LAM) as fresh:   # no cached inverse yet: a step without Hessian sums is refused
        fresh.set_weights(c.w)
        with pytest.raises(PlmError) as e:
            fresh.field_position("stats", update=True)
        assert e.value.code == PLM_EINVAL
