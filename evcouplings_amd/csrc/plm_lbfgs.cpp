// plm_lbfgs.cpp -- More'-Thuente line search and L-BFGS pair history of lbfgs_minimize (plm_lbfgs.h; the iteration that
// plm_ctx_optimize and plm_ar_fit run is plm_lbfgs_driver.h): scalar host code, and the two host-only diagnostic entries that run it without a device.
#include "../../include/plm_hip.h"
#include "plm_lbfgs.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

int plm_fail(int code, const char *fmt, ...);   // plm_host.cpp: records the message for plm_last_error()

// ---- More'-Thuente trial-step update (More' & Thuente 1994, sec. 4); scalar host code -------
int mt_update(double *stx, double *fx, double *dx, double *sty, double *fy, double *dy, double *stp, double fp,
              double dp, double tmin, double tmax, int *brackt) {
    if (*brackt && (*stp <= std::min(*stx, *sty) || *stp >= std::max(*stx, *sty))) return -1;
    if (*dx * (*stp - *stx) >= 0.0 || tmax < tmin) return -1;
    const double sgnd = dp * (*dx / std::fabs(*dx));
    double stpf, stpc, stpq, gamma, p, q, r, s, theta;
    bool bound;
    if (fp > *fx) {
        bound = true;
        theta = 3.0 * (*fx - fp) / (*stp - *stx) + *dx + dp;
        s = std::max(std::fabs(theta), std::max(std::fabs(*dx), std::fabs(dp)));
        gamma = s * std::sqrt((theta / s) * (theta / s) - (*dx / s) * (dp / s));
        if (*stp < *stx) gamma = -gamma;
        p = (gamma - *dx) + theta;
        q = ((gamma - *dx) + gamma) + dp;
        r = p / q;
        stpc = *stx + r * (*stp - *stx);
        stpq = *stx + ((*dx / ((*fx - fp) / (*stp - *stx) + *dx)) / 2.0) * (*stp - *stx);
        stpf = (std::fabs(stpc - *stx) < std::fabs(stpq - *stx)) ? stpc : stpc + (stpq - stpc) / 2.0;
        *brackt = 1;
    } else if (sgnd < 0.0) {
        bound = false;
        theta = 3.0 * (*fx - fp) / (*stp - *stx) + *dx + dp;
        s = std::max(std::fabs(theta), std::max(std::fabs(*dx), std::fabs(dp)));
        gamma = s * std::sqrt((theta / s) * (theta / s) - (*dx / s) * (dp / s));
        if (*stp > *stx) gamma = -gamma;
        p = (gamma - dp) + theta;
        q = ((gamma - dp) + gamma) + *dx;
        r = p / q;
        stpc = *stp + r * (*stx - *stp);
        stpq = *stp + (dp / (dp - *dx)) * (*stx - *stp);
        stpf = (std::fabs(stpc - *stp) > std::fabs(stpq - *stp)) ? stpc : stpq;
        *brackt = 1;
    } else if (std::fabs(dp) < std::fabs(*dx)) {
        bound = true;
        theta = 3.0 * (*fx - fp) / (*stp - *stx) + *dx + dp;
        s = std::max(std::fabs(theta), std::max(std::fabs(*dx), std::fabs(dp)));
        gamma = s * std::sqrt(std::max(0.0, (theta / s) * (theta / s) - (*dx / s) * (dp / s)));
        if (*stp > *stx) gamma = -gamma;
        p = (gamma - dp) + theta;
        q = (gamma + (*dx - dp)) + gamma;
        r = p / q;
        if (r < 0.0 && gamma != 0.0) stpc = *stp + r * (*stx - *stp);
        else stpc = (*stp > *stx) ? tmax : tmin;
        stpq = *stp + (dp / (dp - *dx)) * (*stx - *stp);
        if (*brackt) stpf = (std::fabs(*stp - stpc) < std::fabs(*stp - stpq)) ? stpc : stpq;
        else stpf = (std::fabs(*stp - stpc) > std::fabs(*stp - stpq)) ? stpc : stpq;
    } else {
        bound = false;
        if (*brackt) {
            theta = 3.0 * (fp - *fy) / (*sty - *stp) + *dy + dp;
            s = std::max(std::fabs(theta), std::max(std::fabs(*dy), std::fabs(dp)));
            gamma = s * std::sqrt((theta / s) * (theta / s) - (*dy / s) * (dp / s));
            if (*stp > *sty) gamma = -gamma;
            p = (gamma - dp) + theta;
            q = ((gamma - dp) + gamma) + *dy;
            r = p / q;
            stpf = *stp + r * (*sty - *stp);
        } else {
            stpf = (*stp > *stx) ? tmax : tmin;
        }
    }
    if (fp > *fx) {
        *sty = *stp; *fy = fp; *dy = dp;
    } else {
        if (sgnd < 0.0) { *sty = *stx; *fy = *fx; *dy = *dx; }
        *stx = *stp; *fx = fp; *dx = dp;
    }
    stpf = std::max(tmin, std::min(tmax, stpf));
    *stp = stpf;
    if (*brackt && bound) {
        const double lim = *stx + 0.66 * (*sty - *stx);
        *stp = (*sty > *stx) ? std::min(lim, *stp) : std::max(lim, *stp);
    }
    return 0;
}

// ---- the line search ------------------------------------------------------------------------------------------------
void MtSearch::start(double finit_, double dginit_, double step) {
    finit = finit_;
    dginit = dginit_;
    dgtest = ftol * dginit;
    step0 = step;
    brackt = 0, stage1 = 1, count = 0, uinfo = 0;
    width = stpmax - stpmin, prev_width = 2.0 * width;
    stx = 0, fxx = finit, dgx = dginit, sty = 0, fy = finit, dgy = dginit, stp = step;
}

double MtSearch::next() {
    if (brackt) { stmin = std::min(stx, sty); stmax = std::max(stx, sty); }
    else { stmin = stx; stmax = stp + 4.0 * (stp - stx); }
    stp = std::max(stpmin, std::min(stpmax, stp));
    if ((brackt && (stp <= stmin || stmax <= stp || count >= max_ls - 1 || uinfo)) ||
        (brackt && stmax - stmin <= xtol * stmax))
        stp = stx;
    return stp;
}

int MtSearch::feed(double fx, double dg) {
    if (!std::isfinite(fx) || !std::isfinite(dg)) {
        // the trial left the region where the objective is representable: the interpolation formulas
        // of mt_update are meaningless on it (NaN steps).  Make the trial the far end of the bracket
        // with a finite stand-in value and bisect towards the best point found so far.
        if (count < 64) { trace[count][0] = stp; trace[count][1] = INFINITY; trace[count][2] = 0; }
        if (++count >= max_ls) return -5;
        sty = stp;
        fy = fxx + std::fabs(fxx) + 1.0;
        dgy = std::fabs(dgx);
        brackt = 1;
        stp = stx + 0.5 * (stp - stx);
        width = std::fabs(sty - stx);
        prev_width = 2.0 * width;
        return 0;
    }
    const double ftest1 = finit + stp * dgtest;
    // the value the search works with: the evaluated one, or inside the noise band the derivative-implied one
    const double f_implied = finit + 0.5 * stp * (dginit + dg);
    const bool noisy = std::fabs(fx - finit) <= flat_rel * std::fabs(finit) &&
                       std::fabs(fx - f_implied) > 0.5 * std::fabs(f_implied - finit) + 1e-12 * std::fabs(finit);
    const double fl = noisy ? f_implied : fx;
    if (count < 64) { trace[count][0] = stp; trace[count][1] = fx - finit; trace[count][2] = dg; }
    count++;
    if (brackt && (stp <= stmin || stmax <= stp || uinfo)) return -1;
    if (stp == stpmax && fl <= ftest1 && dg <= dgtest) return -2;
    if (stp == stpmin && (ftest1 < fl || dgtest <= dg)) return -3;
    if (brackt && stmax - stmin <= xtol * stmax) return -4;
    if (count >= max_ls) return -5;
    if ((fl <= ftest1 || (!noisy && fx <= finit + epsf * std::fabs(finit))) && std::fabs(dg) <= gtol * (-dginit))
        return 1;
    if (stage1 && fl <= ftest1 && std::min(ftol, gtol) * dginit <= dg) stage1 = 0;
    if (stage1 && ftest1 < fl && fl <= fxx) {
        double fm = fl - stp * dgtest, fxm = fxx - stx * dgtest, fym = fy - sty * dgtest;
        double dgm = dg - dgtest, dgxm = dgx - dgtest, dgym = dgy - dgtest;
        uinfo = mt_update(&stx, &fxm, &dgxm, &sty, &fym, &dgym, &stp, fm, dgm, stmin, stmax, &brackt);
        fxx = fxm + stx * dgtest; fy = fym + sty * dgtest;
        dgx = dgxm + dgtest; dgy = dgym + dgtest;
    } else {
        uinfo = mt_update(&stx, &fxx, &dgx, &sty, &fy, &dgy, &stp, fl, dg, stmin, stmax, &brackt);
    }
    if (brackt) {
        if (0.66 * prev_width <= std::fabs(sty - stx)) stp = stx + 0.5 * (sty - stx);
        prev_width = width;
        width = std::fabs(sty - stx);
    }
    return 0;
}

void MtSearch::dump_failure(int iteration, int lsrc) const {
    fprintf(stderr, "[plm] line search failed at iteration %d: code %d, finit=%.6f dginit=%.6e step0=%.3e brackt=%d stx=%.6e sty=%.6e\n", iteration, -lsrc, finit, dginit, step0, brackt, stx, sty);
    for (int t = 0; t < count && t < 64; t++)
        fprintf(stderr, "[plm]   trial %d: stp=%.9e  f-f0=%.6e  dg=%.6e\n", t, trace[t][0], trace[t][1], trace[t][2]);
}

// ---- the pair history -----------------------------------------------------------------------------------------------
// Two-loop recursion of L-BFGS (Nocedal 1980) in coefficient space: with the Gram matrix of {s_j, y_j, g} the direction
//     p = sum_j cs[j] s_j + D^-1 (sum_j cy[j] y_j + cg g)      (D^-1 = I without preconditioning)
// needs no pass over the vectors.  The history is a ring of m physical slots; the LIVE pairs are the `stored` slots before
// `end` in ring order (newest = end - 1).  That is not always the physical range 0..stored-1: when a noise-dominated pair
// is skipped on a full ring (LbfgsHistory::admit), the dead slot is `end` -- wherever the ring stands.  Inputs and outputs
// are indexed by PHYSICAL slot: SY[i*m+j] = s_i.y_j, YDY[i*m+j] = y_i.D^-1 y_j, Sg[i] = s_i.g, YDg[i] = y_i.D^-1 g,
// gDg = g.D^-1 g; cs / cy get zeros in dead slots; *dg = g.p.  Exported for the host-side test (tests/test_host_layer.py).
extern "C" void plm_lbfgs_coefficients(int m, int stored, int end, const double *SY, const double *YDY, const double *Sg,
                                       const double *YDg, double gDg, double *cs, double *cy, double *cg_out,
                                       double *dg_out) {
    std::vector<double> alpha(m, 0.0);
    std::vector<int> live(stored);                       // newest first
    for (int i = 0; i < stored; i++) live[i] = lbfgs_live_slot(m, end, i);
    for (int j = 0; j < m; j++) cs[j] = cy[j] = 0.0;
    double cg = -1.0;
    // first loop (newest -> oldest): q = cg g + sum cy y lives in the plain space, only s_i.q is needed (cs is still zero)
    for (int i = 0; i < stored; i++) {
        const int j = live[i];
        double v = cg * Sg[j];
        for (int k : live) v += cy[k] * SY[j * m + k];
        alpha[j] = v / SY[j * m + j];
        cy[j] -= alpha[j];
    }
    if (stored > 0) {
        const int newest = live[0];
        const double gamma = SY[newest * m + newest] / YDY[newest * m + newest];
        cg *= gamma;
        for (int k : live) cy[k] *= gamma;
    }
    // second loop (oldest -> newest): r = sum cs s + D^-1 (cg g + sum cy y)
    for (int i = stored - 1; i >= 0; i--) {
        const int j = live[i];
        double v = cg * YDg[j];
        for (int k : live) v += cs[k] * SY[k * m + j] + cy[k] * YDY[j * m + k];
        cs[j] += alpha[j] - v / SY[j * m + j];
    }
    double dg = cg * gDg;
    for (int k : live) dg += cs[k] * Sg[k] + cy[k] * YDg[k];
    *cg_out = cg;
    *dg_out = dg;
}

LbfgsHistory::LbfgsHistory(int m_) : m(m_), SY(m_ * m_, 0.0), YDY(m_ * m_, 0.0), Sg(m_, 0.0), YDg(m_, 0.0), cs(m_), cy(m_) {}

void LbfgsHistory::coefficients(double *cg, double *dginit) {
    plm_lbfgs_coefficients(m, stored, end, SY.data(), YDY.data(), Sg.data(), YDg.data(), gDg, cs.data(), cy.data(), cg,
                           dginit);
}

void LbfgsHistory::absorb(const double *md, int nbv, int nst) {
    const int e = end;
    for (int j = 0; j < nst; j++) {
        SY[e * m + j] = md[0 * nbv + nst + j];            // s_e . y_j
        SY[j * m + e] = md[1 * nbv + j];                  // s_j . y_e
        YDY[e * m + j] = YDY[j * m + e] = md[1 * nbv + nst + j];
        Sg[j] = md[2 * nbv + j];
        YDg[j] = md[2 * nbv + nst + j];
    }
    gDg = md[2 * nbv + 2 * nst];
    gg = md[2 * nbv + 2 * nst + 1];
}

void LbfgsHistory::reset() {
    stored = 0;
    end = 0;
    anchored = false;
}

LbfgsAdmission LbfgsHistory::admit(const double *md, int nbv, int nst, bool vp, bool straddle, bool debug) {
    const int e = end;
    // Curvature pair of the accepted step (slot e).  s.y > 0 always holds under the Wolfe conditions -- for exact
    // gradients.  Near the noise floor of the evaluation (config 3: error 1e-3 |x| at a stop rule of 1e-3) steps
    // get so short that y = H s + (difference of two evaluation errors) is mostly the latter: s.y is then a tiny
    // number of either sign, 1 / s.y blows the two-loop coefficients up (seen with PLM_DEBUG: directions whose
    // g.d disagreed in sign with the value the coefficients imply, a unit step raising f by 8e14) and the fit
    // ends in a line-search failure.  For a convex quadratic cos(s, H s) >= 2 sqrt(k) / (1 + k) with k the
    // condition number (0.12 at the headline's 120 : 3.5e4; the field part of s lowers it to ~0.04), a pair of
    // pure noise has cos ~ 1 / sqrt(P) = 2e-4: pairs below 1e-3 are not stored (the history keeps its other
    // pairs; the slot is written again by the next iteration -- with a pair over the longer baseline from the
    // anchor, see `anchored`).
    // Variable projection: y has no field part (the reduced gradient's is zero), the curvature information of the pair
    // lives in the couplings -- but s carries the CHANGE OF THE OPTIMAL FIELDS as well, which enters no product of the
    // two-loop recursion and only lowers cos(s, y) (0.12 -> 0.04 at the headline; at N = 500 000 below the admission
    // rule: every pair of the accurate phase was skipped and the history went stale, NOTES_r06.md).  The rule looks at
    // the coupling part of s.
    const double ss_full = md[0 * nbv + e], ss_h = vp ? std::min(ss_full, std::max(0.0, md[3 * nbv])) : 0.0;
    const double sy = SY[e * m + e], ss = std::max(ss_full - ss_h, 1e-300), yy = md[1 * nbv + nst + e];
    if (debug)
        fprintf(stderr, "[plm]        pair: s.y = %.4e, |s| = %.4e (couplings %.4e), |y| = %.4e, cos = %.3e; history %d pair(s)%s%s\n",
                sy, std::sqrt(ss_full), std::sqrt(ss), std::sqrt(yy), sy / std::sqrt(std::max(1e-300, ss * yy)), stored,
                anchored ? ", anchored" : "", straddle ? ", straddle" : "");
    if (straddle) {
        // y = g_accurate(x) - g_plain(previous x) carries the DIFFERENCE of the two evaluations' errors (~3e-11 N L
        // |x|): not a curvature pair.  It is dropped (slot e, the oldest pair once the ring is full, goes with it);
        // the next pair starts from this point, whose gradient is the accurate one.
        stored = std::min(stored, m - 1);
        anchored = false;
        return {LBFGS_PAIR_STRADDLE, false};
    } else if (sy > 0 && sy * sy >= 1e-6 * ss * yy) {
        stored = nst;
        end = (end + 1) % m;
        anchored = false;
        return {LBFGS_PAIR_STORED, false};
    } else if (sy > 0) {       // noise-dominated pair: skipped; slot e (the oldest pair once the ring is full) is gone
        stored = std::min(stored, m - 1);
        // keep the point the pair started from: (xp, gp) is overwritten by the next swap
        const bool copy = !anchored;
        anchored = true;
        return {LBFGS_PAIR_SKIPPED, copy};
    } else {                   // slot e now holds a rejected pair: restart the history
        reset();
        return {LBFGS_HISTORY_RESTARTED, false};
    }
}

// ---- host-only diagnostic entries (include/plm_hip.h): no device is initialised ---------------------------------------
extern "C" int plm_linesearch_run(plm_phi_cb phi, void *user, double finit, double dginit, double step0, int32_t *code,
                                  int32_t *n_trials, double *stp, double *trace) {
    if (!phi || !code || !n_trials || !stp || !trace) return plm_fail(PLM_EINVAL, "NULL argument");
    if (!std::isfinite(finit) || !(step0 > 0)) return plm_fail(PLM_EINVAL, "need a finite f(0) and a positive first step");
    *n_trials = 0;
    *stp = 0.0;
    // what plm_ctx_optimize does before it searches: a direction that does not descend ends the fit with reason 10
    if (!(dginit < 0)) { *code = -10; return PLM_OK; }
    MtSearch ls;
    ls.start(finit, dginit, step0);
    int lsrc;
    do {
        const double t = ls.next();
        double dg = 0;
        const double fx = phi(t, &dg, user);
        lsrc = ls.feed(fx, dg);
    } while (lsrc == 0);
    *code = lsrc;
    *n_trials = ls.count;
    // a failed search takes no step: the optimiser goes back to the point it started from
    *stp = lsrc < 0 ? 0.0 : ls.stp;
    for (int t = 0; t < ls.count; t++)
        for (int k = 0; k < 3; k++) trace[3 * t + k] = ls.trace[t][k];
    return PLM_OK;
}

extern "C" int plm_lbfgs_admit(int32_t m, int32_t *stored, int32_t *end, int32_t *anchored, double *SY, double *YDY,
                               double *Sg, double *YDg, double *gDg, double *gg, const double *md, int32_t nbv,
                               int32_t nst, int32_t vp, int32_t straddle, int32_t *outcome, int32_t *copy_anchor) {
    if (!stored || !end || !anchored || !SY || !YDY || !Sg || !YDg || !gDg || !gg || !md || !outcome || !copy_anchor)
        return plm_fail(PLM_EINVAL, "NULL argument");
    if (m < 1 || m > 20) return plm_fail(PLM_EINVAL, "%d history slots, need 1..20", (int)m);
    if (*stored < 0 || *stored > m) return plm_fail(PLM_EINVAL, "need 0 <= stored <= m (m = %d, stored = %d)", (int)m, (int)*stored);
    if (*end < 0 || *end >= m) return plm_fail(PLM_EINVAL, "ring slot %d outside 0..%d", (int)*end, (int)m - 1);
    LbfgsHistory h(m);
    h.stored = *stored;
    h.end = *end;
    h.anchored = *anchored != 0;
    if (nst != h.nst() || nbv != 2 * nst + 2)
        return plm_fail(PLM_EINVAL, "the Gram pass of %d stored pair(s) has nst = %d and nbv = %d, not %d and %d", (int)*stored,
                        h.nst(), 2 * h.nst() + 2, (int)nst, (int)nbv);
    if (h.end >= nst) return plm_fail(PLM_EINVAL, "the new pair's slot %d is not among the %d slots of the basis", h.end, (int)nst);
    std::copy(SY, SY + m * m, h.SY.begin());
    std::copy(YDY, YDY + m * m, h.YDY.begin());
    std::copy(Sg, Sg + m, h.Sg.begin());
    std::copy(YDg, YDg + m, h.YDg.begin());
    h.gDg = *gDg;
    h.gg = *gg;
    h.absorb(md, nbv, nst);
    const LbfgsAdmission a = h.admit(md, nbv, nst, vp != 0, straddle != 0, false);
    std::copy(h.SY.begin(), h.SY.end(), SY);
    std::copy(h.YDY.begin(), h.YDY.end(), YDY);
    std::copy(h.Sg.begin(), h.Sg.end(), Sg);
    std::copy(h.YDg.begin(), h.YDg.end(), YDg);
    *gDg = h.gDg;
    *gg = h.gg;
    *stored = h.stored;
    *end = h.end;
    *anchored = h.anchored ? 1 : 0;
    *outcome = a.outcome;
    *copy_anchor = a.copy_anchor ? 1 : 0;
    return PLM_OK;
}
