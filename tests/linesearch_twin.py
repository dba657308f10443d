"""float64 twin of the optimiser's line search and pair admission (evcouplings_amd/csrc/plm_lbfgs.cpp), written from the
rules: More' & Thuente 1994, section 4 (the safeguarded trial-step selection, the modified function of the first stage, the
0.66 width rule) plus the library's two deviations ("Noise rules": the approximate-Wolfe allowance and the noise
band with the derivative-implied value) and the bisection away from a non-finite trial.  Plain Python floats (IEEE
double) and only + - * / sqrt abs min max in the library's operation order, so the library must agree exactly: same exit
code, same number of trials, bit-equal steps.  Every trial is tagged with the branches it took.

No GPU and no library: tests/test_linesearch_host.py runs the library's own code (plm_linesearch_run, plm_lbfgs_admit)
against this.
"""
import math

import numpy as np

FTOL, GTOL, XTOL, STPMIN, STPMAX, MAX_LS = 1e-4, 0.9, 1e-7, 1e-20, 1e20, 20
EPSF, FLAT_REL = 1e-6, 4e-9
INF = float("inf")


def _cubic_gamma(theta, d1, d2, clamp=False):
    s = max(abs(theta), max(abs(d1), abs(d2)))
    rad = (theta / s) * (theta / s) - (d1 / s) * (d2 / s)
    if clamp:
        rad = max(0.0, rad)
    return s * math.sqrt(rad)


def trial_step(I, fp, dp, tmin, tmax):
    """Section 4 of the paper: I = dict(stx, fx, dx, sty, fy, dy, stp, brackt) is updated in place with the new
    interval and the next trial step; returns (0 | -1, case tag, whether the 0.66 safeguard moved the step)."""
    stx, fx, dx, sty, fy, dy, stp, brackt = (I[k] for k in ("stx", "fx", "dx", "sty", "fy", "dy", "stp", "brackt"))
    if brackt and (stp <= min(stx, sty) or stp >= max(stx, sty)):
        return -1, "outside", False
    if dx * (stp - stx) >= 0.0 or tmax < tmin:
        return -1, "no_descent", False
    sgnd = dp * (dx / abs(dx))
    if fp > fx:
        # case 1: a higher value.  The minimum is bracketed; the cubic step if it is closer to stx than the quadratic
        # one, else their average
        tag, bound = "case1", True
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        gamma = _cubic_gamma(theta, dx, dp)
        if stp < stx:
            gamma = -gamma
        p = (gamma - dx) + theta
        q = ((gamma - dx) + gamma) + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
        stpf = stpc if abs(stpc - stx) < abs(stpq - stx) else stpc + (stpq - stpc) / 2.0
        brackt = 1
    elif sgnd < 0.0:
        # case 2: a lower value, derivatives of opposite sign.  Bracketed; the cubic or the secant step, whichever is
        # farther from stp
        tag, bound = "case2", False
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        gamma = _cubic_gamma(theta, dx, dp)
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = ((gamma - dp) + gamma) + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = 1
    elif abs(dp) < abs(dx):
        # case 3: a lower value, same sign, the derivative shrinks.  The cubic step only if it tends to infinity in the
        # direction of the step (or its minimum lies beyond stp); closest to stp when bracketed, farthest when not
        tag, bound = ("case3_bracketed" if brackt else "case3_open"), True
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        gamma = _cubic_gamma(theta, dx, dp, clamp=True)
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = (gamma + (dx - dp)) + gamma
        r = p / q
        if r < 0.0 and gamma != 0.0:
            stpc = stp + r * (stx - stp)
        else:
            stpc = tmax if stp > stx else tmin
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        if brackt:
            stpf = stpc if abs(stp - stpc) < abs(stp - stpq) else stpq
        else:
            stpf = stpc if abs(stp - stpc) > abs(stp - stpq) else stpq
    else:
        # case 4: a lower value, same sign, the derivative does not shrink.  The cubic step through (sty, stp) when
        # bracketed, else the end of the allowed interval
        tag, bound = ("case4_bracketed" if brackt else "case4_open"), False
        if brackt:
            theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
            gamma = _cubic_gamma(theta, dy, dp)
            if stp > sty:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dy
            r = p / q
            stpf = stp + r * (sty - stp)
        else:
            stpf = tmax if stp > stx else tmin
    # the interval that contains a minimiser
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0.0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    stpf = max(tmin, min(tmax, stpf))
    stp = stpf
    if brackt and bound:
        # a step chosen by extrapolation, or close to the far end: at most 0.66 of the way from stx to sty
        lim = stx + 0.66 * (sty - stx)
        stp = min(lim, stp) if sty > stx else max(lim, stp)
    I.update(stx=stx, fx=fx, dx=dx, sty=sty, fy=fy, dy=dy, stp=stp, brackt=brackt)
    return 0, tag, stp != stpf


def line_search(phi, finit, dginit, step0):
    """phi(stp) -> (f, f').  Returns (code, n_trials, stp, trace [(stp, f - f0, f')], tags [set per trial]); code 1:
    accepted, -1 .. -5 as the library's, -10: dginit is not negative.  stp is 0 after a failure."""
    if not dginit < 0:
        return -10, 0, 0.0, [], []
    dgtest = FTOL * dginit
    I = dict(stx=0.0, fx=finit, dx=dginit, sty=0.0, fy=finit, dy=dginit, stp=step0, brackt=0)
    stage1, count, uinfo = 1, 0, 0
    width = STPMAX - STPMIN
    prev_width = 2.0 * width
    trace, tags = [], []

    def done(code):
        return code, count, (I["stp"] if code == 1 else 0.0), trace, tags

    while True:
        brackt, stx, sty = I["brackt"], I["stx"], I["sty"]
        if brackt:
            stmin, stmax = min(stx, sty), max(stx, sty)
        else:
            stmin, stmax = stx, I["stp"] + 4.0 * (I["stp"] - stx)
        stp = max(STPMIN, min(STPMAX, I["stp"]))
        # nothing more to gain from the interval: the best point so far is evaluated once more (and then fails or passes)
        if (brackt and (stp <= stmin or stmax <= stp or count >= MAX_LS - 1 or uinfo)) or \
                (brackt and stmax - stmin <= XTOL * stmax):
            stp = stx
        I["stp"] = stp
        fx, dg = phi(stp)
        tag = set()
        tags.append(tag)
        if not math.isfinite(fx) or not math.isfinite(dg):
            # beyond the representable region: the trial becomes the far end of the bracket with a finite stand-in, the
            # next trial halves the distance to the best point
            tag.add("nonfinite")
            trace.append((stp, INF, 0.0))
            count += 1
            if count >= MAX_LS:
                return done(-5)
            I.update(sty=stp, fy=I["fx"] + abs(I["fx"]) + 1.0, dy=abs(I["dx"]), brackt=1, stp=stx + 0.5 * (stp - stx))
            width = abs(I["sty"] - stx)
            prev_width = 2.0 * width
            continue
        ftest1 = finit + stp * dgtest
        f_implied = finit + 0.5 * stp * (dginit + dg)          # trapezoid rule on the two derivatives
        noisy = abs(fx - finit) <= FLAT_REL * abs(finit) and \
            abs(fx - f_implied) > 0.5 * abs(f_implied - finit) + 1e-12 * abs(finit)
        fl = f_implied if noisy else fx
        if noisy:
            tag.add("noisy")
        trace.append((stp, fx - finit, dg))
        count += 1
        if brackt and (stp <= stmin or stmax <= stp or uinfo):
            return done(-1)
        if stp == STPMAX and fl <= ftest1 and dg <= dgtest:
            return done(-2)
        if stp == STPMIN and (ftest1 < fl or dgtest <= dg):
            return done(-3)
        if brackt and stmax - stmin <= XTOL * stmax:
            return done(-4)
        if count >= MAX_LS:
            return done(-5)
        if (fl <= ftest1 or (not noisy and fx <= finit + EPSF * abs(finit))) and abs(dg) <= GTOL * (-dginit):
            if not fl <= ftest1:
                tag.add("epsf_accept")
            elif noisy:
                tag.add("noisy_accept")
            return done(1)
        if stage1 and fl <= ftest1 and min(FTOL, GTOL) * dginit <= dg:
            stage1 = 0
            tag.add("left_stage1")
        if stage1 and ftest1 < fl and fl <= I["fx"]:
            # first stage: the step is chosen for the modified function psi(t) = f(t) - f(0) - ftol f'(0) t
            tag.add("modified")
            stx, sty = I["stx"], I["sty"]
            M = dict(I, fx=I["fx"] - stx * dgtest, fy=I["fy"] - sty * dgtest, dx=I["dx"] - dgtest, dy=I["dy"] - dgtest)
            uinfo, case, limited = trial_step(M, fl - stp * dgtest, dg - dgtest, stmin, stmax)
            I.update(M, fx=M["fx"] + M["stx"] * dgtest, fy=M["fy"] + M["sty"] * dgtest, dx=M["dx"] + dgtest,
                     dy=M["dy"] + dgtest)
        else:
            uinfo, case, limited = trial_step(I, fl, dg, stmin, stmax)
        tag.add(case)
        if limited:
            tag.add("limit066")
        if I["brackt"]:
            # the interval must shrink to 0.66 of its length of two trials ago, else it is halved
            if 0.66 * prev_width <= abs(I["sty"] - I["stx"]):
                I["stp"] = I["stx"] + 0.5 * (I["sty"] - I["stx"])
                tag.add("bisect066")
            prev_width = width
            width = abs(I["sty"] - I["stx"])


# ---- the pair history ------------------------------------------------------------------------------------------------
STORED, STRADDLE, SKIPPED, RESTARTED = 0, 1, 2, 3


def absorb_admit(state, md, vp, straddle):
    """The rules of the history ("Noise rules", and section 6): the Gram rows of the accepted step's pair -- it sits in slot
    `end` -- are copied out of md [3 nbv + 1] (rows of the queries s, y, g over the basis S[0..nst), Y[0..nst), g, g;
    last entry: the fields' share of s.s), then
      * a straddle pair is dropped: slot `end` (the oldest pair once the ring is full) is gone, the anchor is released;
      * a pair with s.y > 0 and cos(s, y) >= 1e-3 (variable projection: over the coupling part of s) is stored: the
        ring advances;
      * a pair with s.y > 0 below that is skipped: slot `end` is gone as well, and the point the pair started from is
        kept as the anchor of the next pair -- copied once, at the first skip in a row;
      * s.y <= 0 restarts the history.
    state: dict(m, stored, end, anchored, SY, YDY, Sg, YDg, gDg, gg).  Returns (new state, outcome, copy_anchor)."""
    m, stored, end, anchored = state["m"], state["stored"], state["end"], state["anchored"]
    SY, YDY, Sg, YDg = (np.array(state[k], np.float64) for k in ("SY", "YDY", "Sg", "YDg"))
    nst = min(m, stored + 1)
    nbv = 2 * nst + 2
    assert len(md) == 3 * nbv + 1 and end < nst
    e = end
    for j in range(nst):
        SY[e, j] = md[0 * nbv + nst + j]
        SY[j, e] = md[1 * nbv + j]
        YDY[e, j] = YDY[j, e] = md[1 * nbv + nst + j]
        Sg[j] = md[2 * nbv + j]
        YDg[j] = md[2 * nbv + nst + j]
    gDg, gg = float(md[2 * nbv + 2 * nst]), float(md[2 * nbv + 2 * nst + 1])
    ss_full = float(md[0 * nbv + e])
    ss_h = min(ss_full, max(0.0, float(md[3 * nbv]))) if vp else 0.0
    sy, ss, yy = float(SY[e, e]), max(ss_full - ss_h, 1e-300), float(md[1 * nbv + nst + e])
    copy_anchor = False
    if straddle:
        outcome, stored, anchored = STRADDLE, min(stored, m - 1), False
    elif sy > 0 and sy * sy >= 1e-6 * ss * yy:
        outcome, stored, end, anchored = STORED, nst, (end + 1) % m, False
    elif sy > 0:
        outcome, stored = SKIPPED, min(stored, m - 1)
        copy_anchor, anchored = not anchored, True
    else:
        outcome, stored, end, anchored = RESTARTED, 0, 0, False
    new = dict(m=m, stored=stored, end=end, anchored=anchored, SY=SY, YDY=YDY, Sg=Sg, YDg=YDg, gDg=gDg, gg=gg)
    return new, outcome, copy_anchor
