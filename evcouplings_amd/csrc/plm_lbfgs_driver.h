// plm_lbfgs_driver.h -- the L-BFGS iteration around MtSearch and LbfgsHistory (plm_lbfgs.h), written once for every
// optimiser of the library: plm_ctx_optimize (plm_host.cpp) and plm_ar_fit (plm_ar.hip).  Host code only, no kernel.
// The two-loop recursion (Nocedal 1980) is evaluated in coefficient space ("vector-free" L-BFGS, Chen et al. 2014): every
// inner product it needs is an entry of the Gram matrix of {s_j, y_j, g}, refreshed by ONE pass over the history per
// trial (k_sy_multidot), and the direction is ONE fused linear combination (k_multiaxpy).  Vectors stay in HBM; what is
// particular to an objective -- its evaluation, its norms, its stop rule -- is a member function of the Problem:
//
//   int start(LbfgsHistory &, LbfgsOutcome *)   f and g at the start point: fx, nll, cond of the outcome; gDg, gg of the history
//   LbfgsVectors vectors()                      the buffers as they stand now
//   double first_step(LbfgsHistory &)           length of a first step along the steepest descent (at the start, after a restart)
//   void swap_points()                          (x, g) <-> (xp, gp), and whatever travels with them
//   int begin_search()                          after the swap, before the first trial is evaluated
//   int evaluate_trial(nbv, gram_pass)          f and g at x; gram_pass() enqueues the pair and the Gram rows, in the same fetch
//   double search_dg0(dg_gram)                  g.d at step 0 for the search (asked after the first trial's fetch)
//   void trial_values(&fx, &nll, &dg)           what the last evaluate_trial brought back
//   int after_search(k, ls, dg, gg_trial, nbv, gram_pass, out, &straddle)   the accepted trial, before its rows are absorbed
//   void accepted_norms(hist, &cond, &xx, &hh)  |g| / max(1, |x|), x.x, x.x over the fields at the accepted point
//   int converged(&cond, &done)                 the stop rule
//   int anchor_buffers()                        xa, ga exist from here on
//   bool vp, debug                              for LbfgsHistory::admit; debug also asks for MtSearch::dump_failure
#pragma once
#include "plm_internal.h"
#include "plm_host_util.h"
#include "plm_lbfgs.h"

#include <chrono>

struct LbfgsLimits {
    int m;              // history slots
    double eps;         // the iteration is not entered when cond at the start point is <= eps
    int max_iter;       // 0: no limit
    plm_iter_cb cb;     // after every accepted step; a non-zero return cancels the fit
    void *user;
    double t0;          // lbfgs_now() the callback's seconds count from
};
struct LbfgsOutcome {
    int k = 0, status = PLM_STATUS_CONVERGED, ls_reason = 0;
    double fx = 0, nll = 0, cond = 0;   // at the last accepted point
};
struct LbfgsVectors {
    float *x, *g, *xp, *gp, *xa, *ga, *dir, *S, *Y;   // xa, ga: the anchor (LbfgsHistory::anchored)
    int64_t n, nh;                    // entries; leading entries that are fields (plm_launch_sy_multidot)
    const float *dinv;                // H0 diagonal, or null
    double *scratch, *md, *ex;        // device: scratch and the two outputs of plm_launch_sy_multidot
    const double *h_md;               // host copy of md once evaluate_trial has returned
    hipStream_t st;
};

inline double lbfgs_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class Problem> int lbfgs_minimize(Problem &p, const LbfgsLimits &lim, LbfgsOutcome *out) {
    LbfgsHistory hist(lim.m);      // the ring of pairs and the Gram matrix of {s_j, y_j, g}
    PLM_TRY(p.start(hist, out));
    if (!(out->cond > lim.eps)) return PLM_OK;
    int &k = out->k, restarts = 0;
    double step = p.first_step(hist);
    for (k = 1;; k++) {
        LbfgsVectors v = p.vectors();
        double cg, dg_gram;
        hist.coefficients(&cg, &dg_gram);
        if (!(dg_gram < 0)) { out->status = PLM_STATUS_LINESEARCH; out->ls_reason = 10; k--; break; }
        PlmVecList B;
        PlmCoefList C;
        const int first_weighted = lbfgs_direction_basis(v.S, v.Y, v.g, v.n, lim.m, hist.stored, hist.end, hist.cs.data(),
                                                         hist.cy.data(), cg, &B, &C);
        // the direction and, in the same pass, the first trial point x + stp0 p -- written where the trial points are
        // built after the swap below (today's xp: the point before the accepted one, not needed any more unless it is
        // still the anchor of the next pair, which lives in its own buffers then)
        const float stp0 = (float)std::max(MtSearch::stpmin, std::min(MtSearch::stpmax, step));
        PLM_HIP(plm_launch_multiaxpy_trial(v.dir, B, C, v.n, v.dinv, first_weighted, v.x, stp0, v.xp, v.st));
        p.swap_points();      // the accepted point moves to (xp, gp); trial points are built in (x, g)
        v = p.vectors();
        PLM_TRY(p.begin_search());
        const double finit = out->fx, nllinit = out->nll;
        // Speculate that a trial point is accepted (it is, 97 % of the time): form its (s, y) pair in slot `end` -- the
        // slot the next pair goes to anyway; a rejected trial is simply overwritten by the next one -- and run the Gram
        // pass (rows for s, y, g) behind its evaluation, so that ONE host synchronisation per trial brings back f, the
        // directional derivative and everything the next direction needs.
        float *s_new = v.S + (size_t)hist.end * v.n, *y_new = v.Y + (size_t)hist.end * v.n;
        const int nst = hist.nst();
        unsigned long long wb;                        // basis vectors that enter products in the H0 metric: Y, g
        unsigned wq;                                  // queries y_new and g
        lbfgs_gram_basis(v.S, v.Y, v.g, v.n, nst, &B, &wb, &wq);      // v.g: the buffer the trial gradients land in
        auto gram_pass = [&]() {
            return plm_launch_sy_multidot(s_new, y_new, v.x, hist.anchored ? v.xa : v.xp, v.g, hist.anchored ? v.ga : v.gp,
                                          v.dir, B, v.n, v.nh, v.scratch, v.md, v.ex, v.dinv, wq, wb, v.st);
        };
        MtSearch ls = {};
        int lsrc;
        double dg = 0;
        for (bool first = true;; first = false) {
            if (!first) PLM_HIP(plm_launch_lincomb(v.x, 1.f, v.xp, (float)ls.next(), v.dir, v.n, v.st));
            PLM_TRY(p.evaluate_trial(B.n, gram_pass));
            if (first) {
                const double dginit = p.search_dg0(dg_gram);
                if (!(dginit < 0)) { lsrc = -10; break; }
                ls.start(finit, dginit, step);
                ls.next();      // the first trial point came with the direction: (float)next() == stp0
            }
            p.trial_values(&out->fx, &out->nll, &dg);
            if ((lsrc = ls.feed(out->fx, dg)) != 0) break;
        }
        if (lsrc < 0 && p.debug) ls.dump_failure(k, lsrc);
        if (lsrc < 0) {
            p.swap_points();      // the last accepted point is still in (xp, gp): make it current again
            out->fx = finit;
            out->nll = nllinit;
            k--;
            if (hist.stored > 0 && restarts < 2) {
                // a stale quasi-Newton model is the usual reason near the f32 floor: drop the history
                // and retry from steepest descent before giving up
                restarts++;
                hist.reset();
                step = p.first_step(hist);
                continue;
            }
            out->status = PLM_STATUS_LINESEARCH;
            out->ls_reason = -lsrc;
            break;
        }
        restarts = 0;
        // the pair of the accepted point already sits in slot `end` and its Gram rows in h_md (see above)
        const double *md = v.h_md;
        const int nbv = B.n;
        bool straddle = false;              // this step's pair would difference gradients of two arithmetics
        PLM_TRY(p.after_search(k, ls, dg, md[2 * nbv + 2 * nst + 1], nbv, gram_pass, out, &straddle));
        hist.absorb(md, nbv, nst);
        double xx, hh;
        p.accepted_norms(hist, &out->cond, &xx, &hh);
        // a non-zero return cancels the fit (a pipeline's SIGTERM / SIGINT handler, evcouplings/utils/pipeline.py:476-545,
        // raised inside a Python callback): the point reached so far stays with the problem
        if (lim.cb && lim.cb(k, lbfgs_now() - lim.t0, out->cond, out->fx, out->nll, std::sqrt(hh),
                             std::sqrt(std::max(0.0, xx - hh)), lim.user) != 0) {
            out->status = PLM_STATUS_INTERRUPTED;
            break;
        }
        bool done = false;
        PLM_TRY(p.converged(&out->cond, &done));
        if (done) { out->status = PLM_STATUS_CONVERGED; break; }
        if (lim.max_iter > 0 && k >= lim.max_iter) { out->status = PLM_STATUS_MAXITER; break; }
        // the pair of the accepted step: stored, dropped as a straddle, skipped as noise, or the history restarted
        if (hist.admit(md, nbv, nst, p.vp, straddle, p.debug).copy_anchor) {
            // keep the point the pair started from: (xp, gp) is overwritten by the next swap
            PLM_TRY(p.anchor_buffers());
            v = p.vectors();
            PLM_HIP(hipMemcpyAsync(v.xa, v.xp, sizeof(float) * v.n, hipMemcpyDeviceToDevice, v.st));
            PLM_HIP(hipMemcpyAsync(v.ga, v.gp, sizeof(float) * v.n, hipMemcpyDeviceToDevice, v.st));
        }
        step = 1.0;
    }
    return PLM_OK;
}
