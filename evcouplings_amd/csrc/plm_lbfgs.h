// plm_lbfgs.h -- the scalar side of the optimiser: More'-Thuente line search and the L-BFGS pair history.
// Host arithmetic in double only: no HIP header, no plm_ctx.  lbfgs_minimize (plm_lbfgs_driver.h) drives both with what
// the device pass brings back, for plm_ctx_optimize (plm_host.cpp) and plm_ar_fit (plm_ar.hip) alike; plm_linesearch_run /
// plm_lbfgs_admit (include/plm_hip.h) run them for the CPU tests.
#ifndef PLM_LBFGS_H
#define PLM_LBFGS_H

#include <vector>

// ---- More'-Thuente trial-step update (More' & Thuente 1994, sec. 4); scalar host code -------
int mt_update(double *stx, double *fx, double *dx, double *sty, double *fy, double *dy, double *stp, double fp,
              double dp, double tmin, double tmax, int *brackt);

// the i-th newest LIVE slot of a ring of m history slots whose next pair goes to `end` (i = 0: slot end - 1)
inline int lbfgs_live_slot(int m, int end, int i) { return (end + m - 1 - i) % m; }

// One line search of lbfgs_minimize: start(), then next() -> evaluate the trial -> feed() until feed() is non-zero.
struct MtSearch {
    // Defaults follow libLBFGS (ftol 1e-4, gtol 0.9, <= 20 trial steps)
    static constexpr int max_ls = 20;
    static constexpr double ftol = 1e-4, gtol = 0.9, xtol = 1e-7, stpmin = 1e-20, stpmax = 1e20;
    // f is an f64 sum of ~N L f32 terms: its rounding noise is ~1e-10 |f| (measured: 2e-3 at f = 2.8e7, N = 100 000),
    // while the gradient -- exact integer sums of 24-bit residuals since round 3 -- is good to a few 1e-4 of |x|.  Near
    // the optimum of a large problem the decrease of an iteration (stp |g.d| / 2) falls below that noise before the stop
    // rule is met; a More'-Thuente search fed with such values interpolates on noise (seen at config 3: trials that
    // wander between two step lengths until the bracket collapses, accepted steps that raise f).  Two devices:
    //  * approximate Wolfe (Hager & Zhang 2005), as in the f32 oracle build: a trial whose f did not rise beyond
    //    epsf |f0| passes the sufficient-decrease test;
    //  * where |f(trial) - f(0)| is inside flat_rel |f(0)| AND the evaluated value contradicts what the derivatives
    //    imply, f(0) + stp (g0.d + g.d) / 2 (trapezoid: exact for a quadratic), by more than half of that implied change,
    //    the search works with the implied value -- then the sufficient-decrease test is H&Z's derivative form
    //    g.d <= (2 ftol - 1) g0.d and the cubic steps see consistent data.  Small problems never get there (their f is
    //    good to ~1e-10 |f| too, and that is far below their decreases).
    static constexpr double epsf = 1e-6, flat_rel = 4e-9;

    double finit, dginit, dgtest, step0;   // f and g.d at step 0, ftol * dginit, the first trial step
    int brackt, stage1, count, uinfo;
    double width, prev_width;
    double stx, fxx, dgx, sty, fy, dgy, stp, stmin, stmax;
    double trace[64][3];                   // per trial: stp, f - f0 (INFINITY: not finite), g.d

    void start(double finit_, double dginit_, double step);
    // the step to evaluate next: the interval, the clamp and the "fall back to stx" rule
    double next();
    // (f, g.d) at the step next() returned.  0: go on; 1: accepted (stp is the step); < 0: failed, minus the reason
    // (1 step left the bracket / no progress, 2 stpmax, 3 stpmin, 4 bracket below xtol, 5 max_ls trials)
    int feed(double fx, double dg);
    // PLM_DEBUG report of a failed search
    void dump_failure(int iteration, int lsrc) const;
};

// outcome of LbfgsHistory::admit
enum { LBFGS_PAIR_STORED = 0, LBFGS_PAIR_STRADDLE = 1, LBFGS_PAIR_SKIPPED = 2, LBFGS_HISTORY_RESTARTED = 3 };
struct LbfgsAdmission {
    int outcome;
    bool copy_anchor;   // the caller must copy the point the pair started from into the anchor buffers now
};

// The pair history as the host sees it: a ring of m physical slots and the Gram matrix of {s_j, y_j, g}.
struct LbfgsHistory {
    int m;
    // Gram matrix pieces, indexed by history slot: SY[i][j] = s_i.y_j, YDY[i][j] = y_i.D^-1 y_j, Sg = s_i.g,
    // YDg = y_i.D^-1 g, gDg = g.D^-1 g, gg = g.g (stop rule)
    std::vector<double> SY, YDY, Sg, YDg;
    double gDg = 0, gg = 0;
    std::vector<double> cs, cy;
    // the LIVE pairs are the `stored` slots before `end` (lbfgs_live_slot); the next pair goes into slot `end`
    int stored = 0, end = 0;
    // The next pair is (x - anchor, g - g(anchor)).  The anchor is the previous accepted point (xp, gp) -- unless the
    // pair(s) since were skipped as noise (admit): then it stays where the last STORED pair ended, in its own buffers,
    // so that the difference is taken over a longer baseline, where H s outgrows the evaluation error again.
    bool anchored = false;

    explicit LbfgsHistory(int m_);
    // number of slots in the basis of the Gram pass that carries the next pair
    int nst() const { return m < stored + 1 ? m : stored + 1; }
    // p = sum cs[j] s_j + D^-1 (sum cy[j] y_j + cg g): two-loop recursion in coefficient space over the LIVE pairs
    // (after a skipped pair on a full ring the dead slot is `end` itself, not the highest physical slot); *dginit = g.p
    void coefficients(double *cg, double *dginit);
    // the Gram rows of the accepted point's pair (slot `end`) out of the pass's results md [3 nbv + 1]
    void absorb(const double *md, int nbv, int nst);
    // decides what becomes of the pair in slot `end`; debug: the PLM_DEBUG line about the pair
    LbfgsAdmission admit(const double *md, int nbv, int nst, bool vp, bool straddle, bool debug);
    // drop every pair (a failed line search on a stale model, a rejected pair)
    void reset();
};

#endif  // PLM_LBFGS_H
