#!/usr/bin/env python3
"""
bench.py -- L-BFGS iterations/s of the MI355X pseudo-likelihood Potts solver on the
BASELINE.json headline workload (synthetic MSA, L=300, q=21, N=50 000).

    python bench.py --gpus N --steps K --warmup W          (N > 1: starts the N ranks itself)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one L-BFGS iteration of the fit as the library runs it by default (variable projection:
every trial evaluation = forward GEMM, Newton solve of the fields, residual pass, backward GEMM, assemble;
line-search evaluations and the two-loop recursion included) on the alignment already resident in HBM.  W warm-up iterations are followed by
exactly K timed iterations, bracketed by barrier + device synchronise; a fit that converges before (~170 iterations at
the headline) starts over from its start point with the clock stopped.  Rank 0 prints one JSON line.  With N > 1 the sites of the ONE problem -- and with them the parameters, the gradient and the L-BFGS
state -- are sharded across the ranks (strong scaling); per evaluation two neighbour all-to-alls (coupling halo,
gradient halo) and scalar all-reduces over RCCL (evcouplings_amd/dist.py).

    --dump-outputs DIR   after the timed steps, what they computed as DIR/<name>.npy (see dump_outputs); the inputs
                         are the same from run to run with the same arguments, so two builds compare output for output
    --full               also the extra blocks below, each a run of its own (one GPU); a plain run sets up, warms up,
                         times the K steps, dumps if asked and prints the headline line only

Extra blocks on the same line (--full):
  roofline      dominant kernel (HIP events inside the library, on the stream it launches on)
  cpu_baseline  the oracle's float32/OpenMP build timed on this host on a bounded sample
  value_plmc_unit   joint L-BFGS iterations/s: plmc's own unit (value counts variable-projection iterations)
  fit           (run_plmc_hip_default: A2M file -> run_plmc_hip, reference defaults -> _ECs.txt + .model, wall-clock split)
                wall-clock of whole fits: the reference's default 100 iterations, to |g|/|x| < 1e-3, and a short leg of
                the joint L-BFGS path (plmc's algorithm) whose iterations/s shares its unit with cpu_baseline.value
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HEADLINE = dict(L=300, N=50000, q=21, seed_offset=1)
PEAK_F16_MFMA_TFLOPS = 2500.0     # dense, MI355X_MICROARCH.md
PEAK_I8_MFMA_TOPS = 5000.0        # dense int8, 2 x the f16 rate (MI355X_MICROARCH.md)
PEAK_F32_VALU_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0
VALU_CLK_PER_WAVE_INSTR = 4.3     # measured, scripts/ubench/valu_rate.hip -> profiles/r05_valu_rate_ubench.txt


def reweight_executed_fraction(msa, theta, n_waves=24, n_partners=1500, seed=7):
    """Share of the 32-site half chunks k_reweight_reg really compares: a wave of 64 consecutive
    sequences walks a partner row in 32-site steps and leaves it once ALL 64 running mismatch counts are past the
    allowed L - T (padding sites of the last half chunk always match).  Host emulation of that rule on a random sample
    of (wave, later partner) pairs of this alignment -- measurement bookkeeping only, the counts come from the kernel."""
    N, L = msa.shape
    T = int(np.ceil(theta * L - 1e-9))
    allowed = L - T
    nh = (L + 31) // 32
    rng = np.random.default_rng(seed)
    done, total = 0, 0
    for w0 in rng.choice(max(1, N // 64 - 1), size=min(n_waves, max(1, N // 64 - 1)), replace=False):
        rows = msa[w0 * 64:(w0 + 1) * 64]                                  # (64, L)
        lo = w0 * 64 + 1                                                   # the kernel compares partners t > s only
        if lo >= N:
            continue
        ts = rng.integers(lo, N, size=min(n_partners, N - lo))
        mism = (rows[None, :, :] != msa[ts][:, None, :])                   # (P, 64, L)
        pad = nh * 32 - L
        if pad:
            mism = np.concatenate([mism, np.zeros(mism.shape[:2] + (pad,), bool)], axis=2)
        run = mism.reshape(len(ts), 64, nh, 32).sum(3).cumsum(2)          # running counts after each half chunk
        far = (run > allowed).all(1)                                       # (P, nh): every lane past the limit
        first = np.where(far.any(1), far.argmax(1) + 1, nh)                # half chunks executed before the exit
        done += int(first.sum())
        total += len(ts) * nh
    return done / max(1, total)


def usable_cores():
    """Cores this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def pmc_traffic_bytes(kernel):
    """HBM bytes per launch of `kernel` (prefix match on the instantiation name, e.g. "k_fwd<21_3>") from the
    newest committed PMC summary, or None."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_counters.csv")))
    if not files:
        return None
    vals = {}
    with open(files[-1]) as f:
        for row in csv.reader(l for l in f if not l.startswith("#")):
            if len(row) >= 3 and row[0].startswith(kernel):
                vals.setdefault(row[1], float(row[2]))
    if "FETCH_SIZE" not in vals or "WRITE_SIZE" not in vals:
        return None
    return (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0


def pmc_traffic_per_evaluation():
    """HBM bytes of one whole objective+gradient evaluation as the fit runs it: per-launch traffic of every kernel in
    the newest committed PMC summary (2*FETCH + WRITE KiB) x that kernel's launches per evaluation in the newest
    committed rocprofv3 kernel-trace statistics of a bench run (launches / launches of k_bwd, which runs once per
    evaluation).  Returns (bytes, {kernel: bytes}) or (None, {})."""
    import csv
    import glob
    pmc = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_counters.csv")))
    stats = sorted(glob.glob(os.path.join(ROOT, "profiles", "*kernel_stats.csv")))
    if not pmc or not stats:
        return None, {}
    tr = {}
    with open(pmc[-1]) as f:
        for row in csv.reader(l for l in f if not l.startswith("#")):
            if len(row) >= 3 and row[1] in ("FETCH_SIZE", "WRITE_SIZE"):
                tr.setdefault(row[0], {})[row[1]] = float(row[2])
    calls = {}
    with open(stats[-1]) as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("void ", "").split("(")[0].replace(", ", "_")
            calls[name] = calls.get(name, 0) + int(row["Calls"])
    n_eval = sum(v for k, v in calls.items() if k.startswith("k_bwd"))
    if not n_eval:
        return None, {}
    per = {}
    for k, v in tr.items():
        if k in calls and "FETCH_SIZE" in v and "WRITE_SIZE" in v:
            per[k] = (2.0 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024.0 * calls[k] / n_eval
    return (sum(per.values()) if per else None), per


COUPLING_SAMPLE = 4_000_000       # entries of the coupling block dump_outputs writes (float32: 16 MB)


def dump_outputs(path, x, res, L, q):
    """What a caller of the timed path receives after its last step, as float32 / float64 .npy files in `path`:
      fields.npy            (L, q) float32   h_i(a) of the parameter vector x
      couplings_sample.npy  float32          J entries of x at a fixed sample of positions (sorted, seed 0) when the
                                             coupling block is longer than COUPLING_SAMPLE, else the whole block
      iterations.npy        (K, 4) float64   per timed iteration: iteration number, |g|/max(1,|x|), objective, NLL
      fx.npy                (1,) float64     objective at the returned x
    The wall-clock column of the iteration table is left out: it differs from run to run."""
    os.makedirs(path, exist_ok=True)
    nf = L * q
    J = x[nf:]
    if J.size > COUPLING_SAMPLE:
        J = J[np.sort(np.random.default_rng(0).choice(J.size, COUPLING_SAMPLE, replace=False))]
    np.save(os.path.join(path, "fields.npy"), np.ascontiguousarray(x[:nf], dtype=np.float32).reshape(L, q))
    np.save(os.path.join(path, "couplings_sample.npy"), np.ascontiguousarray(J, dtype=np.float32))
    table = np.array([(r[0], r[2], r[3], r[4]) for r in res["table"]], dtype=np.float64).reshape(-1, 4)
    np.save(os.path.join(path, "iterations.npy"), table)
    np.save(os.path.join(path, "fx.npy"), np.array([res["fx"]], dtype=np.float64))


def relaunch_under_torchrun(n_gpus, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks here (one per GPU, rendezvous on 127.0.0.1 --
    the container's hostname may not resolve) and hand their exit code back.  Rank 0 prints the JSON line."""
    import socket
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rc = 1
    for attempt in range(3):          # the port is found by bind-and-release: retry if somebody took it in between
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
        run = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, text=True)
        sys.stderr.write(run.stderr or "")
        rc = run.returncode
        if rc == 0 or "ddress already in use" not in (run.stderr or ""):
            break
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-seqs", type=int, default=HEADLINE["N"])
    ap.add_argument("--n-sites", type=int, default=HEADLINE["L"])
    ap.add_argument("--no-fit", action="store_true", help="skip the whole-fit timing")
    ap.add_argument("--fit-cap", type=int, default=4000, help="iteration cap of the fit-to-epsilon leg")
    ap.add_argument("--joint-fit-cap", type=int, default=300,
                    help="iteration cap of the joint L-BFGS leg (PLM_FLAG_JOINT_LBFGS, plmc's algorithm; 0 = skip)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg")
    ap.add_argument("--full", action="store_true",
                    help="also the roofline, the whole-fit legs and the CPU baseline (one GPU; --no-fit / --no-cpu "
                         "leave legs out)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the timed steps computed as DIR/<name>.npy (with N > 1 ranks: DIR/rank<r>/)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(relaunch_under_torchrun(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but the launcher started %d ranks" % (args.gpus, world))
    if os.environ.get("PLM_BENCH_LAUNCH_ONLY"):
        # launcher check (tests/test_host_layer.py, no GPU needed): every rank joins a gloo group, rank 0 reports
        import torch.distributed as dist
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo", rank=rank, world_size=world)
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"launch_only": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup}))
        return

    import torch
    from evcouplings_amd import plm
    from evcouplings_amd.synthetic import synthetic_msa, BASE_SEED
    # PLM_DIST_BACKEND=gloo: collectives staged through host memory and ranks folded onto the visible GPUs --
    # exercises this multi-rank flow on a single-GPU box (never used for a reported number)
    backend = os.environ.get("PLM_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, rank=rank, world_size=world)

    q, L, N = HEADLINE["q"], args.n_sites, args.n_seqs
    msa, _ = synthetic_msa(N, L, seed=BASE_SEED + HEADLINE["seed_offset"])
    lam_j = plm.default_lambda_j(L, q)

    # --- set-up (untimed): upload, reweight, marginals, start point ------------------------
    t_setup = time.time()
    native = False
    # epsilon = the production stop rule (it also selects the 24-bit residual planes; a fit asked to go below 1e-4 would
    # run 32-bit ones).  The headline fit reaches it in ~170 iterations; a longer window starts the fit over (run_steps)
    ctx1 = plm.PlmContext(msa, q=q, lambda_h=0.01, lambda_j=lam_j, device=local_rank, max_iter=args.warmup,
                          epsilon=1e-3)
    w, counts, n_eff = ctx1.reweight()
    ctx1.marginals(pairs=False)
    ctx1.set_x(None)
    if world > 1:
        # sharded-state mode: parameters, gradient and L-BFGS state split by owning site block; per
        # evaluation two all-to-alls of neighbour blocks + scalar all-reduces over RCCL
        from evcouplings_amd.dist import (make_torch_collective, make_host_staged_collective, negotiate_native_rccl,
                                          share_rccl_id)
        x0 = ctx1.get_x()
        ctx1.close()
        ctx = plm.PlmContext(msa, q=q, lambda_h=0.01, lambda_j=lam_j, device=local_rank, n_shards=world,
                             shard=rank, max_iter=args.warmup, epsilon=1e-3, sharded_state=True)
        native = backend == "nccl" and negotiate_native_rccl(device=local_rank)
        if native:
            ctx.attach_rccl(share_rccl_id())       # collectives issued by the library on its own stream
        else:
            ctx.set_collective(make_torch_collective() if backend == "nccl" else
                               make_host_staged_collective(device=local_rank))
        ctx.set_weights(w)
        ctx.set_x(x0)
    else:
        ctx = ctx1
    t_setup = time.time() - t_setup

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # --- warm-up: W iterations; timed: exactly K more iterations ---------------------------
    import ctypes as C
    from evcouplings_amd import _lib

    def run_iters(k):
        # re-create the problem's iteration cap through a fresh optimise call from the current x
        ctx._set_max_iter(k)
        return ctx.optimize()

    def run_steps(k):
        """Exactly k L-BFGS iterations from the current x; returns (result, seconds).  A fit that stops before k (at the
        headline it converges after ~170) starts over from its start point -- the set-up's x, set outside the clock --
        so that a step is always an iteration of the fit.  `seconds` covers the optimise calls only; `result` sums
        iterations and evaluations and joins the iteration tables, its other entries are those of the last call."""
        sync()
        res, secs, restarted = None, 0.0, False
        while res is None or res["iters"] < k:
            if res is not None:
                ctx.set_x(None if world == 1 else x0)
                sync()
                restarted = True
            t = time.perf_counter()
            r = run_iters(k - (res["iters"] if res else 0))
            sync()
            secs += time.perf_counter() - t
            if r["iters"] == 0 and restarted:
                raise SystemExit("the fit stopped at its start point: %s" % r["status_msg"])
            if res is not None:
                r.update(iters=res["iters"] + r["iters"], n_evals=res["n_evals"] + r["n_evals"],
                         table=res["table"] + r["table"])
            res = r
        return res, secs

    if args.warmup > 0:
        run_steps(args.warmup)
    res, dt = run_steps(args.steps)
    if dist is not None:
        tt = torch.tensor([dt], device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    assert res["iters"] == args.steps, res
    if args.dump_outputs:
        dump_outputs(args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, "rank%d" % rank),
                     ctx.get_x(), res, L, q)

    out = {
        "metric": "plmc L-BFGS iterations/sec (PLM fit, synthetic MSA)",
        "value": args.steps / dt,
        "unit": "iterations/s",
        "evaluations_per_s": res["n_evals"] / dt,
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32 (forward: f16 hi/lo split couplings on the 2:4 sparse MFMA, f32 accumulation -- in the last "
                 "iterations of a fit 39-bit fixed-point couplings as five int8 digit planes, exact; backward: 24-bit "
                 "fixed-point residuals as three int8 digit planes on the int8 MFMA (32-bit / four there), exact int32 "
                 "accumulation; f64 reductions and field solves).  "
                 "tests/test_gpu_scale.py prints the error of a float32 CPU build beside the HIP error at every stop point",
        "data": "synthetic",
        "config": {"workload": "headline: synthetic MSA L=%d q=%d N=%d, theta=0.8, lambda_h=0.01, lambda_J=%.1f"
                               % (L, q, N, lam_j),
                   "n_eff": n_eff,
                   # the stop rule of the timed contexts: it selects the digit planes of the backward GEMM (3 above 1e-4,
                   # 4 below) and scales the field solver's tolerance.  BENCH r01 / r02 ran these iterations at 1e-12
                   # (4 planes, tighter field solves): their `value` is not like-for-like with r03+.
                   "epsilon": 1e-3, "bwd_digit_planes": 3,
                   "parallelism": "single GPU" if world == 1 else "sites + state sharded x%d (%s)" % (
                       world, ("RCCL all-to-all, issued by the library on its stream" if native
                               else "RCCL all-to-all via torch.distributed callbacks") if backend == "nccl"
                       else "gloo, host-staged: flow test only"),
                   "evals_per_iteration": res["n_evals"] / max(1, res["iters"]),
                   "solver": "variable projection (default): one step = one L-BFGS iteration over the couplings with the "
                             "fields solved by Newton at every trial point; reaches epsilon in ~170 such iterations "
                             "where the joint L-BFGS of round 1 (83 it/s) needed > 6000 -- see fit.*"},
    }

    if args.full and rank == 0 and world == 1:
        # --- roofline of the dominant kernel (HIP events on the library's stream) ----------
        solver = ctx.solver_stats()      # field solver of the timed window (HIP events inside the library)
        km = ctx.time_kernels(reps=5)
        # `fields`: what the field solver of an evaluation REALLY cost in the timed window (its whole chain of passes,
        # HIP events around it in every evaluation); time_kernels' own figure -- one Newton step + the residual pass --
        # is kept as fields_one_step.  `total` = the evaluation as the timed window ran it.
        km["fields_one_step"] = km["fields"]
        # the two GEMMs: their average launch duration INSIDE the timed window (HIP events on the library's stream around
        # the forward and the backward GEMM of every evaluation, plm_ctx_solver_stats); time_kernels' figures -- the same
        # launches in isolation, a host synchronisation between repetitions -- are kept as *_isolated
        km["forward_isolated"], km["backward_isolated"] = km["forward"], km["backward"]
        if solver.get("gemm_evaluations", 0) > 0:
            km["forward"], km["backward"] = solver["forward_ms_per_evaluation"], solver["backward_ms_per_evaluation"]
            km["gemm_evaluations_timed"] = solver["gemm_evaluations"]
        if solver["evaluations"] > 0:
            km["fields"] = solver["field_ms_per_evaluation"]
            km["total"] = km["expand"] + km["forward"] + km["fields"] + km["backward"] + km["assemble"]
        km["field_passes_per_evaluation"] = solver["passes_per_evaluation"]
        dom = "forward" if km["forward"] >= km["backward"] else "backward"
        t_dom = km[dom] * 1e-3
        flops_dense = 2.0 * N * (L * q) ** 2            # one one-hot GEMM (flops_dense / 2)
        flops_alg = 1.0 * N * L * (L - 1) * q           # gathered adds of one half (flops_alg / 2)
        nb16, nu = (L + 15) // 16, (L + 31) // 32
        # executed MFMA flops of the launch: f16 hi + lo planes, K and N padded to the tile grid
        if dom == "forward":
            flops_exec = 2.0 * 2 * ((N + 255) // 256 * 256) * (nu * 32 * q) * (nb16 * 16 * q)
        else:
            # backward: three int8 digit planes of the 24-bit fixed-point residuals, M and N padded to the tile grid
            # (k_bwd_w: workgroup tile 28 x 9 fragments)
            flops_exec = 2.0 * 3 * ((N + 255) // 256 * 256) * ((nb16 * q + 7 + 27) // 28 * 28 * 16) * (
                (nb16 * q + 8) // 9 * 9 * 16)
        P = L * q + L * (L - 1) // 2 * q * q
        bytes_alg = N * L + 4 * N + 8 * P
        achieved = flops_alg / t_dom / 1e12
        out["roofline"] = {
            "kernel": "k_fwd_w" if dom == "forward" else "k_bwd_w",
            "bound": "mfma",
            # SURVEY.md 8(d) primary figure: useful gathered adds of this half of the evaluation against the f32
            # vector peak (the one-hot GEMM formulation does q x redundant flops on the matrix cores to get there)
            "achieved": achieved,
            "peak": PEAK_F32_VALU_TFLOPS,
            "unit": "TFLOP/s",
            "frac": achieved / PEAK_F32_VALU_TFLOPS,
            # the same accounting for a whole STEP: both halves of every evaluation the step made (flops_alg x
            # evaluations per iteration) over the measured ms_per_step -- what is left of `frac` once the field solver,
            # the L-BFGS vector kernels and the host are counted
            "frac_per_step": 2.0 * flops_alg * (res["n_evals"] / max(1, res["iters"])) / (dt / args.steps) / 1e12 / PEAK_F32_VALU_TFLOPS,
            "definition": "SURVEY 8(d) primary: flops_alg/2 = N*L*(L-1)*q gathered adds per launch / HIP-event time "
                          "/ 157.3 TFLOP/s f32 vector peak",
            "traffic": pmc_traffic_bytes("k_fwd_w" if dom == "forward" else "k_bwd_w"),
            "traffic_note": "HBM bytes per launch from the newest committed rocprofv3 PMC passes (profiles/*pmc_counters.csv:"
                            " 2*FETCH_SIZE + WRITE_SIZE KiB, gfx950 FETCH_SIZE correction of MI355X_MICROARCH.md); "
                            "not re-collected by this run",
            "onehot_dense_tflops": flops_dense / t_dom / 1e12,
            "onehot_dense_frac_of_f16_mfma": flops_dense / t_dom / 1e12 / PEAK_F16_MFMA_TFLOPS,
            "executed_mfma_tflops": flops_exec / t_dom / 1e12,
            # forward: f16 planes on the (2:4 sparse) f16 MFMA; backward: int8 planes on the int8 MFMA (~5 POP/s dense)
            "executed_mfma_frac_of_peak": flops_exec / t_dom / 1e12 / (PEAK_F16_MFMA_TFLOPS if dom == "forward"
                                                                          else PEAK_I8_MFMA_TOPS),
            "eval_hbm_alg_bytes": bytes_alg,
            "eval_hbm_alg_frac": bytes_alg / (km["total"] * 1e-3) / 1e9 / PEAK_HBM_GBS,
            "kernel_ms": km,
        }
        tr = out["roofline"]["traffic"]
        if tr:
            # the north-star's "gradient kernel >= 40 % of HBM roofline", in the only sense a measured number can
            # have: HBM bytes the dominant kernel really moved per launch / its time / 8 TB/s.  The kernel is
            # MFMA-bound (intensity ~1 100 flop/B), so this figure is small by construction.
            out["roofline"]["measured_hbm_frac"] = tr / t_dom / 1e9 / PEAK_HBM_GBS
            out["roofline"]["measured_hbm_frac_note"] = ("north-star 'HBM roofline' figure of the dominant kernel: PMC "
                                                         "bytes per launch / HIP-event time / 8 TB/s")
        tot, per = pmc_traffic_per_evaluation()
        if tot:
            out["roofline"]["traffic_eval_total"] = tot
            out["roofline"]["traffic_eval_over_alg"] = tot / bytes_alg
            out["roofline"]["traffic_eval_by_kernel"] = {k: round(v) for k, v in sorted(per.items(), key=lambda kv: -kv[1])[:8]}
            out["roofline"]["traffic_eval_note"] = ("HBM bytes of ONE evaluation of the fit's pipeline: per-launch PMC "
                                                    "traffic x launches per evaluation (committed profiles/, not "
                                                    "re-collected); ratio to eval_hbm_alg_bytes = wasted re-reads")
        pairs = float(N) * (N - 1) / 2
        exe = reweight_executed_fraction(msa, 0.8)
        # three VALU instructions (v_xad_u32, v_and_b32, v_bcnt_u32_b32) per dword of 4 sites, 64 sequences per
        # wave-instruction, rows padded to 32-site half chunks; measured issue rate of exactly this triple with every
        # operand in registers: 4.3 clocks per wave-instruction per SIMD (profiles/r05_valu_rate_ubench.txt), 2.4 GHz
        instr_full = pairs * (((L + 31) // 32) * 8) * 3 / 64
        floor_full = instr_full * VALU_CLK_PER_WAVE_INSTR / (256 * 4 * 2.4e9) * 1e3
        out["roofline"]["reweight"] = {
            "ms": km["reweight"], "byte_compares_per_s": pairs * L / (km["reweight"] * 1e-3),
            "executed_fraction": exe,
            "executed_byte_compares_per_s": exe * pairs * ((L + 31) // 32 * 32) / (km["reweight"] * 1e-3),
            "valu_floor_ms_full_rows": floor_full,
            "valu_floor_ms": exe * floor_full,
            "frac_of_valu_floor": exe * floor_full / km["reweight"],
            "note": "symmetric: N(N-1)/2 sequence pairs.  The kernel leaves a partner row once all 64 sequences of a wave "
                    "are past the allowed mismatches (looked at every 32 sites): executed_fraction = share of the 32-site "
                    "half chunks it really compares, from a host emulation of that rule on a sample of (wave, partner) "
                    "pairs of THIS alignment.  Floor = executed instructions at the MEASURED 4.3 clocks per "
                    "wave-instruction per SIMD (not the 2 clocks earlier rounds assumed)"}
        # --- whole fit: (a) the reference's default 100 iterations, (b) to |g|/|x| < 1e-3 -------------------
        if not args.no_fit:
            t1 = time.perf_counter()
            fit = plm.fit(msa, q, lambda_h=0.01, lambda_j=lam_j, max_iter=100, epsilon=1e-3, device=local_rank,
                          want_fij=False)
            out["fit"] = {"reference_default_100_iterations": {
                "seconds_total": time.perf_counter() - t1, "iterations": fit["iters"], "evaluations": fit["n_evals"],
                "status": fit["status_msg"], "final_cond": fit["table"][-1][2], "seconds": fit["seconds"]}}
            t1 = time.perf_counter()
            fit = plm.fit(msa, q, lambda_h=0.01, lambda_j=lam_j, max_iter=args.fit_cap, epsilon=1e-3,
                          device=local_rank, want_fij=False)
            reach = {}
            for thr in (1.0, 1e-1, 1e-2, 3e-3, 1e-3):
                hit = [r for r in fit["table"] if r[2] < thr]
                reach["%g" % thr] = {"iteration": hit[0][0], "seconds": hit[0][1]} if hit else None
            out["fit"]["to_epsilon_1e-3"] = {
                "seconds_total": time.perf_counter() - t1, "iterations": fit["iters"], "evaluations": fit["n_evals"],
                "status": fit["status_msg"], "converged": fit["status"] == 0, "final_cond": fit["table"][-1][2],
                "iterations_per_s": fit["iters"] / max(1e-9, fit["seconds"]["optimize"]),
                "iteration_cap": args.fit_cap, "first_time_cond_below": reach, "seconds": fit["seconds"],
                "note": "cond = |g|/max(1,|x|); default solver = variable projection (fields by Newton per trial "
                        "point, L-BFGS over the couplings).  --joint-fit-cap K additionally times the joint L-BFGS "
                        "path that libLBFGS-based plmc takes"}
            if args.joint_fit_cap > 0:
                t1 = time.perf_counter()
                fit = plm.fit(msa, q, lambda_h=0.01, lambda_j=lam_j, max_iter=args.joint_fit_cap, epsilon=1e-3,
                              device=local_rank, want_fij=False, joint=True)
                out["fit"]["joint_lbfgs"] = {
                    "seconds_total": time.perf_counter() - t1, "iterations": fit["iters"],
                    "evaluations": fit["n_evals"], "status": fit["status_msg"], "final_cond": fit["table"][-1][2],
                    "iterations_per_s": fit["iters"] / max(1e-9, fit["seconds"]["optimize"]),
                    "evaluations_per_s": fit["n_evals"] / max(1e-9, fit["seconds"]["optimize"]),
                    "note": "plmc's algorithm (L-BFGS over fields and couplings together): THIS iterations/s shares its "
                            "unit with cpu_baseline.value; one of `value`'s variable-projection iterations is worth "
                            "~20 of these"}
                # the plmc-comparable rate next to the headline value, so the record carries both
                out["joint_lbfgs_iterations_per_s"] = out["fit"]["joint_lbfgs"]["iterations_per_s"]
                # `value` counts variable-projection iterations (one is worth ~20 of plmc's); THIS is the figure in plmc's
                # own unit -- joint L-BFGS iterations per second -- and the only one to read beside cpu_baseline.value
                out["value_plmc_unit"] = out["fit"]["joint_lbfgs"]["iterations_per_s"]
                out["value_plmc_unit_note"] = "joint L-BFGS iterations/s (PLM_FLAG_JOINT_LBFGS, plmc's algorithm); same unit as cpu_baseline.value"
        # --- the reference's DEFAULT mode: plmc -g / ignore_gaps (config/sample_config_monomer.txt:155), 20 model
        # states, lambda_J scaled with q - 1 = 19 (couplings/protocol.py:159-165): kernel times and the fit to epsilon
        if not args.no_fit:
            lam_g = plm.default_lambda_j(L, q - 1)
            with plm.PlmContext(msa, q=q, lambda_h=0.01, lambda_j=lam_g, device=local_rank, max_iter=args.fit_cap,
                                epsilon=1e-3, ignore_gaps=True) as cg:
                cg.reweight()
                cg.marginals(pairs=False)
                cg.set_x(None)
                t1 = time.perf_counter()
                rg = cg.optimize()
                tg = time.perf_counter() - t1
                kg = cg.time_kernels(reps=5)
            out["fit"]["ignore_gaps"] = {
                "seconds_optimize": tg, "iterations": rg["iters"], "evaluations": rg["n_evals"], "status": rg["status_msg"],
                "converged": rg["status"] == 0, "final_cond": rg["table"][-1][2], "iterations_per_s": rg["iters"] / max(1e-9, tg),
                "lambda_J": lam_g, "kernel_ms": kg,
                "backward_frac_of_f32_peak": 1.0 * N * L * (L - 1) * (q - 1) / (kg["backward"] * 1e-3) / 1e12 / PEAK_F32_VALU_TFLOPS,
                "note": "plmc -g semantics of DESIGN.md 2b on the headline alignment (the path every default pipeline run "
                        "takes): the 21-state kernel instantiations with the gap state masked out of every softmax and "
                        "structurally zero in parameters and gradient; 20 useful states per site"}
        # --- the boundary itself, as a pipeline user calls it: A2M FILE -> run_plmc_hip with the reference's default
        # settings (ignore_gaps: True, iterations: 100; config/sample_config_monomer.txt:149-155) -> _ECs.txt + .model
        if not args.no_fit:
            import shutil
            import tempfile
            from evcouplings_amd import tools
            from evcouplings_amd.synthetic import msa_to_a2m
            tmp = tempfile.mkdtemp(prefix="plm_bench_")
            try:
                ali = msa_to_a2m(msa, os.path.join(tmp, "headline.a2m"))
                ec_file, model_file = os.path.join(tmp, "headline_ECs.txt"), os.path.join(tmp, "headline.model")
                t1 = time.perf_counter()
                r, raw, _ = tools.infer_to_files(ali, ec_file, model_file, focus_seq="SYN/1-%d" % L, theta=0.8,
                                                 ignore_gaps=True, iterations=100, lambda_h=0.01,
                                                 lambda_J=plm.default_lambda_j(L, q - 1))
                wall = time.perf_counter() - t1
                sec = raw["seconds"]
                out["fit"]["run_plmc_hip_default"] = {
                    "seconds_wall": wall, "seconds_read_alignment": sec["read_alignment"],
                    "seconds_library": sec["library"], "seconds_optimize": sec["optimize"],
                    "seconds_write_files": sec["write_files"], "iterations": int(raw["iters"]),
                    "status": r.optimization_status, "alignment_bytes": os.path.getsize(ali),
                    "model_bytes": os.path.getsize(model_file), "ec_lines": sum(1 for _ in open(ec_file)),
                    "note": "evcouplings_amd.tools.run_plmc_hip's body (infer_to_files) on the headline alignment written "
                            "as an A2M file: reference defaults ignore_gaps=True, iterations=100, lambda_J = 0.01 (q-1)(L-1); "
                            "wall-clock from the file path going in to _ECs.txt + plmc_v2 .model on disk (tmpfs or disk "
                            "of this box), PCIe and file I/O included"}
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        # --- CPU baseline: oracle f32 + OpenMP on a bounded sample --------------------------
        if not args.no_cpu:
            # one OpenMP thread per usable core (the box shows 256 CPUs but runs under a 16-core quota)
            os.environ["OMP_NUM_THREADS"] = str(usable_cores())
            os.environ.setdefault("OMP_PROC_BIND", "false")
            from oracle.oracle import Oracle
            orc = Oracle("f32")
            orc.set_num_threads(usable_cores())
            ns = min(N, 1500)
            sub = np.ascontiguousarray(msa[:ns])
            wsub = w[:ns].astype(np.float32)
            x = np.zeros(plm.n_params(L, q), np.float32)
            orc.eval(sub, wsub, q, 0.01, lam_j, x)      # touch
            reps, t2 = 0, time.perf_counter()
            while reps < 2 or time.perf_counter() - t2 < 6.0:
                orc.eval(sub, wsub, q, 0.01, lam_j, x)
                reps += 1
            per_eval_full = (time.perf_counter() - t2) / reps * (N / ns)
            # ten L-BFGS iterations of the oracle's own joint optimiser on the same sample
            t2 = time.perf_counter()
            f10 = orc.fit(sub, q, lambda_j=lam_j, max_iter=10, epsilon=1e-12, want_fij=False)
            per_iter_full = (time.perf_counter() - t2) / max(1, f10["iters"]) * (N / ns)
            # reweighting: O(N^2 L); a 6000-sequence sample scaled by the pair count
            nr = min(N, 6000)
            t2 = time.perf_counter()
            orc.reweight(np.ascontiguousarray(msa[:nr]), 0.8)
            rew_full = (time.perf_counter() - t2) * (float(N) * (N - 1)) / (float(nr) * (nr - 1))
            model = "unknown"
            try:
                for line in open("/proc/cpuinfo"):
                    if line.startswith("model name"):
                        model = line.split(":", 1)[1].strip()
                        break
            except OSError:
                pass
            out["cpu_baseline"] = {
                "value": 1.0 / per_iter_full, "unit": "iterations/s (joint L-BFGS: compare with joint_lbfgs_iterations_per_s)",
                "cores": orc.num_threads(),
                "kind": "port", "cpu_model": model,
                "seconds_per_evaluation": per_eval_full, "seconds_per_iteration": per_iter_full,
                "seconds_reweighting": rew_full,
                "sample": "plmc-equivalent OpenMP restatement (oracle, float32): 10 joint L-BFGS iterations and %d "
                          "objective+gradient evaluations on the first %d of %d sequences (L=%d), scaled by N/%d; "
                          "reweighting of the first %d sequences scaled by the number of pairs" % (
                              reps, ns, N, L, ns, nr),
            }
    if rank == 0:
        out["setup_seconds"] = t_setup
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
