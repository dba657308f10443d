"""
CPU: the optimiser's line search and pair admission (evcouplings_amd/csrc/plm_lbfgs.cpp -- the code plm_ctx_optimize runs,
reached through the host-only entries plm_linesearch_run and plm_lbfgs_admit) against the float64 twin written from the
rules, tests/linesearch_twin.py.

The twin uses the library's operation order and only + - * / sqrt abs min max, and the host build contracts nothing into
fused multiply-adds, so the agreement asked for is exact: same exit code, same number of trials, bit-equal steps.  The twin
tags the branches every trial takes; the case list as a whole must reach all of them (test_case_list_reaches_every_branch
checks that on the twin alone).

Admission: every case builds the Gram pass of an accepted step from explicit vectors, lets the library and the twin
absorb and admit the pair, compares the whole state, and then feeds plm_lbfgs_coefficients with the result -- slots outside
the live set filled with NaN -- which must give the dense two-loop recursion over exactly the live pairs.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linesearch_twin as tw  # noqa: E402
from test_host_layer import _two_loop_dense  # noqa: E402
from test_lbfgs_vector_twin_host import coefficients  # noqa: E402

INF = float("inf")


# ---- one-dimensional functions: phi(t) -> (f, f') ----------------------------------------------------------------------
def quadratic(f0, g0, c):
    return lambda t: (f0 + g0 * t + 0.5 * c * t * t, g0 + c * t)


def more_thuente_2(f0, b=0.004):          # (t + b)^5 - 2 (t + b)^4, table 2 of the paper, shifted to f(0) = f0
    return lambda t: (f0 + (t + b) ** 5 - 2 * (t + b) ** 4 - (b ** 5 - 2 * b ** 4), 5 * (t + b) ** 4 - 8 * (t + b) ** 3)


def concave_start(f0):                    # the slope steepens before a quartic turns it round
    return lambda t: (f0 - t - t * t + 0.05 * t ** 4, -1 - 2 * t + 0.2 * t ** 3)


def wavy(f0, a, w):
    return lambda t: (f0 - t + a * math.sin(w * t) + 0.05 * t * t, -1 + a * w * math.cos(w * t) + 0.1 * t)


def walled(f0, g0, c, t_max):             # not representable beyond t_max
    q = quadratic(f0, g0, c)
    return lambda t: q(t) if t <= t_max else (INF, 0.0)


def cliff(f0, t_jump):                    # a descent whose slope never flattens, then a jump: no Wolfe point exists
    return lambda t: (f0 - t, -1.0) if t < t_jump else (f0 + 10.0, -1.0)


def kink(t):
    return abs(t - 0.3) * 2.0, (-2.0 if t < 0.3 else 2.0)


def shallow_rise(f0, a, b):               # a (-t e^-t + b t): far beyond the dip f sits a little ABOVE f(0), almost flat
    return lambda t: (f0 + a * (-t * math.exp(-t) + b * t), a * ((t - 1) * math.exp(-t) + b))


def noise_floor(f0, g0, c, bumps):
    """|f| ~ 1e7: the true change g0 t + c t^2 / 2 (~1e-3) is far below 4e-9 |f|, the derivatives are exact, and the
    values carry evaluation noise (`bumps`, picked by the step) that contradicts them"""
    def phi(t):
        k = int(round(t * 1e6)) % len(bumps)
        return f0 + g0 * t + 0.5 * c * t * t + bumps[k], g0 + c * t
    return phi


def _case(phi, step0, f0=None):
    f, g = phi(0.0)
    return phi, (f if f0 is None else f0), g, step0


LS_CASES = {
    "quadratic_short_step": _case(quadratic(0.0, -1.0, 1.0), 1e-3),
    "quadratic_long_step": _case(quadratic(100.0, -1.0, 1.0), 10.0),
    "quadratic_exact_step": _case(quadratic(100.0, -1.0, 1.0), 1.0),
    "curvature_met_with_equality": _case(quadratic(0.0, -1.0, 1.0), 0.1),      # f'(0.1) = -0.9 = -gtol |f'(0)| exactly
    "quadratic_barely_lower": _case(quadratic(100.0, -1.0, 1.0), 1.9999),       # lower, but not by ftol: modified function
    "mt2_short_step": _case(more_thuente_2(0.0), 1e-3),
    "mt2_long_step": _case(more_thuente_2(100.0), 10.0),
    "mt2_longer_step": _case(more_thuente_2(100.0), 50.0),
    "concave_short_step": _case(concave_start(0.0), 1e-3),
    "concave_long_step": _case(concave_start(100.0), 10.0),
    "wavy": _case(wavy(3.0, 0.15, 6.0), 0.05),
    "wavy_step_held_at_two_thirds": _case(wavy(100.0, 0.1, 5.0), 0.3),           # the 0.66 safeguard of the trial step binds
    "wall_long_step": _case(walled(100.0, -1.0, 0.2, 2.0), 10.0),
    "wall_longer_step": _case(walled(0.0, -1.0, 0.2, 2.0), 50.0),
    "nothing_representable": _case(walled(100.0, -1.0, 0.2, 0.0), 1.0),
    "cliff": _case(cliff(0.0, 0.7), 1.0),
    "kink": _case(kink, 1.0, f0=0.6),
    "unbounded_below": _case(lambda t: (5.0 - t, -1.0), 1.0),
    "approximate_wolfe": _case(shallow_rise(1e3, 0.01, 0.01), 8.0),
    "noise_accepts_first_trial": _case(noise_floor(1e7, -1e-3, 1e-3, [0.01]), 1.0, f0=1e7),
    "noise_after_a_long_step": _case(noise_floor(1e7, -1e-3, 1e-3, [0.01, -0.02, 0.005]), 2.5, f0=1e7),
    "noise_short_step": _case(noise_floor(1e7, -1e-3, 1e-3, [0.01, -0.02, 0.005]), 0.3, f0=1e7),
    "no_descent": (quadratic(1.0, 0.5, 1.0), 1.0, 0.5, 1.0),
}

BRANCHES = {"case1", "case2", "case3_open", "case3_bracketed", "case4_open", "case4_bracketed", "modified", "left_stage1",
            "limit066", "bisect066", "nonfinite", "noisy", "noisy_accept", "epsf_accept"}


def test_case_list_reaches_every_branch():
    """on the twin alone: all four cases of the trial-step rule (the third and fourth bracketed and not), the modified
    function and the leaving of it, the 0.66 safeguard of the step and the 0.66 bisection, the non-finite branch, the noise band with acceptance through the
    derivative-implied value, the approximate-Wolfe acceptance, and exit codes 1, -5, -1 and -10"""
    seen, codes = set(), set()
    for name, (phi, f0, g0, s0) in LS_CASES.items():
        code, n, stp, trace, tags = tw.line_search(phi, f0, g0, s0)
        assert len(trace) == len(tags) == n
        seen |= set().union(*tags) if tags else set()
        codes.add(code)
    assert BRANCHES <= seen, BRANCHES - seen
    assert {1, -5, -1, -10} <= codes, codes


def test_twin_accepts_a_trial_that_meets_the_curvature_condition_with_equality():
    phi, f0, g0, s0 = LS_CASES["curvature_met_with_equality"]
    assert abs(phi(s0)[1]) == tw.GTOL * -g0
    assert tw.line_search(phi, f0, g0, s0)[:3] == (1, 1, s0)


def test_twin_bisects_towards_the_best_point_when_a_trial_is_not_finite():
    phi, f0, g0, s0 = LS_CASES["wall_long_step"]
    code, n, stp, trace, tags = tw.line_search(phi, f0, g0, s0)
    steps = [t[0] for t in trace]
    assert steps[:3] == [10.0, 5.0, 2.5] and trace[0][1] == INF and "nonfinite" in tags[0]      # stx = 0: halved each time
    assert code == 1 and stp == steps[-1] <= 2.0


def test_twin_noise_band_works_with_the_implied_value():
    """the evaluated value ROSE by 0.01 (inside 4e-9 |f|) where the derivatives say it fell: accepted all the same, and
    the same values outside the band (|f| = 1e3) are a plain failure of the sufficient-decrease test"""
    phi, f0, g0, s0 = LS_CASES["noise_accepts_first_trial"]
    code, n, stp, trace, tags = tw.line_search(phi, f0, g0, s0)
    assert (code, n, stp) == (1, 1, 1.0) and trace[0][1] > 0 and tags[0] == {"noisy", "noisy_accept"}
    code, n, stp, trace, tags = tw.line_search(noise_floor(1e3, -1e-3, 1e-3, [0.01]), 1e3, g0, s0)
    assert not any("noisy" in t for t in tags) and (code != 1 or stp != 1.0)


@pytest.mark.parametrize("name", list(LS_CASES))
def test_library_line_search_is_the_twin_bit_for_bit(name):
    from evcouplings_amd import plm
    phi, f0, g0, s0 = LS_CASES[name]
    code, n, stp, trace, tags = tw.line_search(phi, f0, g0, s0)
    lcode, ln, lstp, ltrace = plm.linesearch_run(phi, f0, g0, s0)
    assert (lcode, ln) == (code, n), (lcode, ln, code, n, [sorted(t) for t in tags])
    ref = np.array(trace, np.float64).reshape(-1, 3)
    assert ltrace.shape == ref.shape
    assert ltrace.tobytes() == ref.tobytes(), (ltrace - ref, [sorted(t) for t in tags])
    assert np.float64(lstp).tobytes() == np.float64(stp).tobytes()
    assert (lstp == ltrace[-1, 0]) if code == 1 else (lstp == 0.0)      # a failed search takes no step


def test_line_search_refuses_invalid_arguments():
    import ctypes as C
    from evcouplings_amd import _lib
    lib = _lib.load()
    cb = _lib.PHI_CB(lambda t, d, u: 0.0)
    code, n, stp = C.c_int32(77), C.c_int32(77), C.c_double(77.0)
    trace = np.full(60, np.nan)
    args = lambda f0, s0, tr: (cb, None, f0, -1.0, s0, C.byref(code), C.byref(n), C.byref(stp), tr)
    for bad in (args(INF, 1.0, trace.ctypes.data), args(1.0, 0.0, trace.ctypes.data), args(1.0, -1.0, trace.ctypes.data),
                args(1.0, 1.0, None)):
        assert lib.plm_linesearch_run(*bad) == -1 and lib.plm_last_error()
        assert (code.value, n.value, stp.value) == (77, 77, 77.0) and np.isnan(trace).all()


# ---- the pair history ------------------------------------------------------------------------------------------------
N_VEC, NH = 30, 6


def _ring(m, stored, end, anchored, precond, seed):
    """a history at (stored, end) from explicit vectors: Gram pieces of the live slots, NaN everywhere else"""
    rng = np.random.default_rng(seed)
    n = N_VEC
    A = rng.normal(size=(n, n))
    H = A @ A.T + n * np.eye(n)
    S = rng.normal(size=(m, n))
    Y = S @ H
    dinv = 1.0 / np.diag(H) if precond else np.ones(n)
    live = [(end - 1 - i) % m for i in range(stored)]
    dead = [j for j in range(m) if j not in live]
    S[dead] = Y[dead] = np.nan
    g_old = rng.normal(size=n)
    state = dict(m=m, stored=stored, end=end, anchored=anchored, SY=S @ Y.T, YDY=(Y * dinv) @ Y.T, Sg=S @ g_old,
                 YDg=(Y * dinv) @ g_old, gDg=float((g_old * dinv) @ g_old), gg=float(g_old @ g_old))
    return rng, H, S, Y, dinv, state


def _gram_pass(S, Y, s_new, y_new, g, e, nst, dinv):
    """md of the pass behind an accepted point: queries (s, y, g) over the basis S[0..nst), Y[0..nst), g, g with the new
    pair in slot e; the metric on (y, g) x (Y's, first g); last entry: s.s over the first NH entries"""
    basis = [(s_new if i == e else S[i], False) for i in range(nst)] + [(y_new if i == e else Y[i], True) for i in range(nst)]
    basis += [(g, True), (g, False)]
    md = [float(((qv * dinv) if (wq and wb) else qv) @ bv) for qv, wq in ((s_new, False), (y_new, True), (g, True))
          for bv, wb in basis]
    return np.array(md + [float(s_new[:NH] @ s_new[:NH])])


def _pair(kind, rng, H):
    n = N_VEC
    s = rng.normal(size=n)
    if kind == "curvature":
        y = H @ s
    elif kind == "noise":                 # s.y > 0 but cos(s, y) ~ 1e-5: orthogonal to s up to a sliver
        r = rng.normal(size=n)
        r -= (r @ s) / (s @ s) * s
        y = 100.0 * r + 1e-3 * s
    elif kind == "negative":
        y = -(H @ s)
    elif kind == "field_heavy":           # cos over the whole s is below 1e-3, over the coupling part well above
        s[:NH] = 0.0
        y = H @ s
        y[:NH] = 0.0                      # the reduced gradient has no field part
        s[:NH] = 3e4 * rng.normal(size=NH)
    return s, y


# (m, stored, end, anchored, pair, vp, straddle) -> (outcome, stored, end, anchored, copy_anchor)
ADMIT_CASES = {
    "store_filling": ((6, 2, 2, False, "curvature", False, False), (tw.STORED, 3, 3, False, False)),
    "store_first": ((6, 0, 0, False, "curvature", True, False), (tw.STORED, 1, 1, False, False)),
    "store_full_wraps": ((4, 4, 3, False, "curvature", False, False), (tw.STORED, 4, 0, False, False)),
    "store_releases_anchor": ((6, 3, 3, True, "curvature", False, False), (tw.STORED, 4, 4, False, False)),
    "store_after_skip_on_full_ring": ((4, 3, 1, True, "curvature", False, False), (tw.STORED, 4, 2, False, False)),
    "straddle_full": ((4, 4, 2, False, "curvature", False, True), (tw.STRADDLE, 3, 2, False, False)),
    "straddle_filling": ((6, 2, 2, False, "curvature", False, True), (tw.STRADDLE, 2, 2, False, False)),
    "straddle_releases_anchor": ((6, 2, 2, True, "noise", False, True), (tw.STRADDLE, 2, 2, False, False)),
    "skip_first": ((6, 3, 3, False, "noise", False, False), (tw.SKIPPED, 3, 3, True, True)),
    "skip_second_in_a_row": ((6, 3, 3, True, "noise", False, False), (tw.SKIPPED, 3, 3, True, False)),
    "skip_full_kills_slot_end": ((4, 4, 1, False, "noise", False, False), (tw.SKIPPED, 3, 1, True, True)),
    "skip_full_precond": ((4, 4, 2, False, "noise", False, False, True), (tw.SKIPPED, 3, 2, True, True)),
    "negative_curvature_restarts": ((6, 4, 4, True, "negative", False, False), (tw.RESTARTED, 0, 0, False, False)),
    "field_heavy_vp_stores": ((6, 2, 2, False, "field_heavy", True, False), (tw.STORED, 3, 3, False, False)),
    "field_heavy_joint_skips": ((6, 2, 2, False, "field_heavy", False, False), (tw.SKIPPED, 2, 2, True, True)),
}


@pytest.mark.parametrize("name", list(ADMIT_CASES))
def test_pair_admission_follows_the_rules_and_leaves_a_usable_history(name):
    from evcouplings_amd import plm
    (m, stored, end, anchored, kind, vp, straddle, *rest), expected = ADMIT_CASES[name]
    precond = bool(rest and rest[0])
    rng, H, S, Y, dinv, state = _ring(m, stored, end, anchored, precond, seed=sorted(ADMIT_CASES).index(name))
    s_new, y_new = _pair(kind, rng, H)
    g = rng.normal(size=N_VEC)
    nst = min(m, stored + 1)
    md = _gram_pass(S, Y, s_new, y_new, g, end, nst, dinv)
    assert np.isfinite(md).all()                         # the pass reads live slots and the new pair only
    if kind == "field_heavy":                            # the case sits astride the 1e-3 line
        sy, yy, ss = s_new @ y_new, y_new @ y_new, s_new @ s_new
        assert sy / math.sqrt(ss * yy) < 1e-3 < sy / math.sqrt((ss - md[-1]) * yy)
    new_t, outcome_t, copy_t = tw.absorb_admit(state, md, vp, straddle)
    new_l, outcome_l, copy_l = plm.lbfgs_admit(state, md, vp=vp, straddle=straddle)
    assert (outcome_t, new_t["stored"], new_t["end"], new_t["anchored"], copy_t) == expected
    assert (outcome_l, new_l["stored"], new_l["end"], new_l["anchored"], copy_l) == expected
    for k in ("SY", "YDY", "Sg", "YDg"):
        assert new_l[k].tobytes() == new_t[k].tobytes(), k           # NaN of the dead slots included
    assert (new_l["gDg"], new_l["gg"]) == (new_t["gDg"], new_t["gg"]) == (float((g * dinv) @ g), float(g @ g))
    # the direction of the next iteration: exactly the live pairs, whatever the dead slots hold
    S2, Y2 = S.copy(), Y.copy()
    S2[end], Y2[end] = s_new, y_new
    stored2, end2 = new_l["stored"], new_l["end"]
    live = [(end2 - 1 - i) % m for i in range(stored2)]
    dead = [j for j in range(m) if j not in live]
    SY, YDY, Sg, YDg = (new_l[k].copy() for k in ("SY", "YDY", "Sg", "YDg"))
    SY[dead, :] = SY[:, dead] = YDY[dead, :] = YDY[:, dead] = np.nan
    Sg[dead] = YDg[dead] = np.nan
    cs, cy, cg, dg = coefficients(m, stored2, end2, SY, YDY, Sg, YDg, new_l["gDg"])
    assert np.all(cs[dead] == 0) and np.all(cy[dead] == 0)
    direction = dinv * (cg * g) + sum(cs[j] * S2[j] + dinv * (cy[j] * Y2[j]) for j in live)
    assert np.isfinite(direction).all()
    ref = _two_loop_dense(g, [(S2[j], Y2[j]) for j in reversed(live)], dinv if precond else None)
    np.testing.assert_allclose(direction, ref, rtol=1e-9, atol=1e-12)
    assert dg == pytest.approx(g.dot(ref), rel=1e-9) and dg < 0


def test_pair_admission_refuses_an_inconsistent_history():
    from evcouplings_amd import _lib, plm
    def blank(m, stored, end):
        nst = min(m, stored + 1)
        state = dict(m=m, stored=stored, end=end, anchored=False, SY=np.ones((m, m)), YDY=np.ones((m, m)), Sg=np.ones(m),
                     YDg=np.ones(m), gDg=1.0, gg=1.0)
        return state, np.ones(3 * (2 * nst + 2) + 1)

    assert plm.lbfgs_admit(*blank(4, 2, 2))[1] == tw.STORED
    # m outside 1..20, stored > m, end outside the ring, a pair that is not in the basis of the pass
    for bad in ((0, 0, 0), (21, 0, 0), (4, 5, 0), (4, 2, 4), (4, 2, -1), (6, 1, 3)):
        with pytest.raises(_lib.PlmError, match="error -1"):
            plm.lbfgs_admit(*blank(*bad))
