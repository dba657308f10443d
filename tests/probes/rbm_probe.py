#!/usr/bin/env python3
"""Speed of the restricted Boltzmann machine (plm_rbm_*, DESIGN_NEXT_ROWS.md section 9.22) at L = 300, q = 21, M = 128,
N = 50 000 sequences.  A probe, not a test; it reads nothing outside the tree.

  fit      one epoch of plm_rbm_fit with C = 4096 chains and k = 2 steps, split into data statistics, chain steps, model
           statistics (with the trace row) and update by the device events of plm_rbm_fit_result.phase_ms, over enough
           epochs for a window of about a second
  step     one block-Gibbs step of 65 536 chains: the difference of two plm.rbm_sample calls with B_LONG and B_SHORT steps
           (host clock, same start, so uploads, the expansion and the download cancel), next to one plm.sample sweep of
           the same number of chains timed the same way in the same process, as the yardstick of the machine
  bounds   for each group of kernels the bytes that must move and the operations, from the shapes alone, the time the
           bounding peak (HBM copy rate, FP32 or FP64 vector rate) would need, and that time over the measured one
  twin     one step and one epoch of the numpy twin at a reduced size on the host, as context only

    python tests/probes/rbm_probe.py [OUT.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

L, Q, M, N = 300, 21, 128, 50000
C_FIT, K_FIT, C_STEP = 4096, 2, 65536
HBM = 6.29e12             # bytes / s, the measured copy rate of an MI355X
VALU32 = 78.6e12          # float32 vector instructions x lanes / s: 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz (an FMA counts once)
VALU64 = 39.3e12          # float64: half of that


def problem(seed=0):
    rng = np.random.default_rng(seed)
    fi = rng.dirichlet(np.full(Q, 0.3), size=L)                    # a few frequent letters per site, as in a family
    msa = np.stack([rng.choice(Q, size=N, p=fi[i]) for i in range(L)], axis=1).astype(np.int8)
    g = np.log(fi + 1e-3).astype(np.float32)
    c = rng.normal(0.0, 0.5, M).astype(np.float32)
    W = rng.normal(0.0, 1.0 / np.sqrt(L), (M, L, Q)).astype(np.float32)
    return msa, np.ones(N, np.float32), g, c, W


def fit_phases(pb):
    msa, w, g, c, W = pb
    run = lambda E: plm.rbm_fit(msa, w, Q, g, c, W, C_FIT, E, steps_per_epoch=K_FIT, lr=0.01, seed=1, phase_times=True)
    run(1)                                                         # warm-up: code objects, allocator
    first = run(2)["phase_ms"].sum() / 2
    E = int(min(200, max(4, np.ceil(1000.0 / max(first, 0.1)))))
    t0 = time.perf_counter()
    ms = run(E)["phase_ms"] / E
    wall = time.perf_counter() - t0
    names = ("data_statistics", "chain_steps", "model_statistics", "update")
    out = dict(epochs=E, call_seconds=wall, **{k: float(v) for k, v in zip(names, ms)})
    print("fit: L=%d q=%d M=%d N=%d C=%d k=%d, %d epochs in one call of %.2f s; per epoch by device events: data statistics "
          "%.3f ms, chain steps %.3f ms (%.3f per step), model statistics %.3f ms, update %.3f ms"
          % (L, Q, M, N, C_FIT, K_FIT, E, wall, ms[0], ms[1], ms[1] / K_FIT, ms[2], ms[3]), flush=True)
    return out


def _per_unit(call, short, guess_ms):
    """milliseconds per step (or sweep) from the difference of two calls; the long one is sized for about a second"""
    call(short)                                                    # warm-up
    t0 = time.perf_counter()
    call(short)
    a = time.perf_counter() - t0
    t0 = time.perf_counter()
    call(short + 8)
    b = time.perf_counter() - t0
    per = max((b - a) / 8, guess_ms * 1e-3 / 100)
    long = short + int(min(2000, max(8, np.ceil(1.0 / per))))
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        call(short)
        a = time.perf_counter() - t0
        t0 = time.perf_counter()
        call(long)
        b = time.perf_counter() - t0
        ts.append(1e3 * (b - a) / (long - short))
    return dict(median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts), reps=3, window_units=long - short)


def step_and_sweep(pb):
    _, _, g, c, W = pb
    rng = np.random.default_rng(5)
    x0 = rng.integers(0, Q, (C_STEP, L)).astype(np.int8)
    step = _per_unit(lambda B: plm.rbm_sample(g, c, W, Q, C_STEP, burn_in=B, seed=2, start=x0), 2, 5.0)
    print("step: one block-Gibbs step of %d chains: %.3f ms (min %.3f, max %.3f; window of %d steps)"
          % (C_STEP, step["median_ms"], step["min_ms"], step["max_ms"], step["window_units"]), flush=True)
    J = rng.normal(0.0, 0.05, (L * (L - 1) // 2, Q, Q)).astype(np.float32)
    sweep = _per_unit(lambda B: plm.sample(g, J, Q, C_STEP, burn_in=B, seed=2, start=x0, energies=False), 2, 50.0)
    print("yardstick: one plm.sample sweep of %d chains at the same L and q: %.3f ms (min %.3f, max %.3f; window of %d sweeps)"
          % (C_STEP, sweep["median_ms"], sweep["min_ms"], sweep["max_ms"], sweep["window_units"]), flush=True)
    return step, sweep


def bounds(fit, step):
    """bytes and operations from the shapes alone; the share is the bounding time over the measured time"""
    nv4 = (Q + 3) // 4 * 4
    n_par = L * Q + M + M * L * Q
    rows = {}

    def row(name, measured_ms, bytes_, ops, rate, what):
        t_b, t_o = bytes_ / HBM, ops / rate
        bound = max(t_b, t_o)
        rows[name] = dict(bytes=bytes_, operations=ops, bound_ms=1e3 * bound, bound_by="HBM" if t_b >= t_o else what,
                          measured_ms=measured_ms, share=1e3 * bound / measured_ms if measured_ms > 0 else None)
        print("bounds: %-18s %.3e bytes, %.3e operations (%s): the peak needs %.4f ms (%s), measured %.3f ms, share %.1f %%"
              % (name, bytes_, ops, what, 1e3 * bound, rows[name]["bound_by"], measured_ms,
                 100 * rows[name]["share"] if rows[name]["share"] else float("nan")), flush=True)

    # one step of C chains: M L float32 adds for the inputs, M L 4NV adds and as many selects for the logits; the tables
    # (Wt, Wv) come from the caches, the chain states are read and written once per launch
    row("block_gibbs_step", step["median_ms"], 2.0 * C_STEP * L, C_STEP * (M * L + 2.0 * M * L * nv4), VALU32, "float32 VALU")
    # data statistics: inputs (N M L float64 adds) + the one-hot product (N M L float64 adds); I and p are written and
    # read back once, the alignment is read
    row("data_statistics", fit["data_statistics"], N * L + 4.0 * 8 * N * M + 8.0 * M * L * Q, 2.0 * N * M * L, VALU64,
        "float64 VALU")
    row("chain_steps_fit", fit["chain_steps"], 2.0 * C_FIT * L, K_FIT * C_FIT * (M * L + 2.0 * M * L * nv4), VALU32,
        "float32 VALU")
    row("model_statistics", fit["model_statistics"], C_FIT * L + 4.0 * 8 * C_FIT * M + 8.0 * M * L * Q + 16.0 * n_par,
        2.0 * C_FIT * M * L, VALU64, "float64 VALU")
    row("update", fit["update"], (4 + 4 + 8 + 8) * n_par, 4.0 * n_par, VALU64, "float64 VALU")
    return rows


def twin_context():
    import rbm_twin as tw
    rng = np.random.default_rng(1)
    C, n = 256, 1000
    g, c, W = tw.random_model(L, Q, M, seed=3, sd_w=1.0 / np.sqrt(L))
    x = rng.integers(0, Q, (C, L))
    t0 = time.perf_counter()
    tw.step(x, g, c, W, 1, 0, np.arange(C))
    t_step = time.perf_counter() - t0
    msa = rng.integers(0, Q, (n, L))
    t0 = time.perf_counter()
    tw.statistics(msa, np.ones(n), c, W, Q, float(n))
    t_stat = time.perf_counter() - t0
    print("twin (numpy, this host, context only): one step of %d chains %.1f ms = %.1f s per 65 536 chains; the statistics "
          "of %d sequences %.1f ms = %.1f s per 50 000" % (C, 1e3 * t_step, t_step * C_STEP / C, n, 1e3 * t_stat, t_stat * N / n),
          flush=True)
    return dict(step_ms_256_chains=1e3 * t_step, statistics_ms_1000_sequences=1e3 * t_stat)


if __name__ == "__main__":
    pb = problem()
    fit = fit_phases(pb)
    step, sweep = step_and_sweep(pb)
    out = dict(shape=dict(L=L, q=Q, M=M, N=N, C_fit=C_FIT, k=K_FIT, C_step=C_STEP), fit_epoch_ms=fit, step=step,
               sample_sweep=sweep, bounds=bounds(fit, step), twin=twin_context())
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
