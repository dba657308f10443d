/*
 * plm_hip.h -- C ABI of libplm_hip.so, the MI355X (gfx950) pseudo-likelihood Potts solver
 * that replaces the external `plmc` process behind EVcouplings' couplings stage.
 *
 * Nothing like this ABI exists in the reference: its boundary for this path is a
 * subprocess (evcouplings/couplings/tools.py:202-266 builds the argv, :266 launches it,
 * :286 parses stderr).  Each entry point below names the piece of that boundary it
 * replaces.  All functions return PLM_OK (0) or a negative PLM_E* code, never throw and
 * never abort; plm_last_error() holds a message for the calling thread.  Host buffers are
 * caller-owned; the library owns its device memory.  No torch types cross this boundary.
 *
 * Parameter-vector layout ("canonical", identical to the order of the plmc_v2 `.model`
 * file, evcouplings/couplings/model.py:355-389):
 *     x = [ h_i(a) : i<L, a<q ] ++ [ J_ij(a,b) : pairs i<j row-major, a<q (site i), b<q (site j) ]
 */
#ifndef PLM_HIP_H
#define PLM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libplm_hip.so is built with -fvisibility=hidden: the declarations between this push and the pop at the end of the
 * file are its whole dynamic symbol table (tests/test_abi.py compares `nm -D` with this header). */
#pragma GCC visibility push(default)

#define PLM_ABI_VERSION 2   /* 2: plm_iter_cb returns int (cancellation), PLM_STATUS_INTERRUPTED, lambda_group */

#define PLM_OK 0
#define PLM_EINVAL (-1)      /* bad argument (NULL, size <= 0, state outside 0..q-1, ...) */
#define PLM_ENOMEM (-2)      /* host or device allocation failed, or the problem needs more device memory than is free (checked up front) */
#define PLM_EDEVICE (-3)     /* HIP runtime error / no gfx950 device */
#define PLM_EUNSUPPORTED (-4)/* alphabet size outside 2..32 (any size in that range runs, padded to 4 / 5 / 20 / 21 / 32) */
#define PLM_ENUMERIC (-5)    /* NaN/Inf met in objective */
#define PLM_ECALLBACK (-6)   /* exchange / collective callback or an RCCL call reported failure */

/* optimisation end states (plm_result_t.status) -> "Gradient optimization: (.+)" line that
 * tools.py:56,99 parses */
#define PLM_STATUS_CONVERGED 0
#define PLM_STATUS_MAXITER 1
#define PLM_STATUS_LINESEARCH 2
#define PLM_STATUS_INTERRUPTED 3   /* the iteration callback asked to stop; the result holds the point reached so far */

typedef struct plm_ctx plm_ctx_t;

/* One inference problem.  Mirrors the plmc options run_plmc() can set
 * (tools.py:126-130, 222-259): -t theta, -s scale, -lh, -le, -m iterations. */
typedef struct {
    int32_t n_seqs;      /* N  valid sequences */
    int32_t n_sites;     /* L  model columns */
    int32_t n_states;    /* q  alphabet size, gap first (alignment.py:25-26) */
    const int8_t *msa;   /* host, row-major N x L, values 0..q-1 */
    double theta_id;     /* identity threshold (0.8); cluster if ident >= ceil(theta*L - 1e-9) */
    double scale;        /* cluster weight scale (plmc -s), w_s = scale / cluster size */
    double lambda_h;     /* L2 strength on fields */
    double lambda_j;     /* L2 strength on couplings, as passed to plmc -le (already scaled
                            by (q-1)(L-1), protocol.py:179) */
    int32_t max_iter;    /* L-BFGS iterations; 0 = until converged */
    double epsilon;      /* stop when |g| / max(1,|x|) < epsilon.  Also selects the precision of the backward GEMM's
                            fixed-point residuals at context creation: 24 bits (three int8 digit planes), or 32 bits
                            (four planes, 4/3 of the cost) when 0 < epsilon < 1e-4 */
    int32_t lbfgs_m;     /* history length; 0 = default (6) */
    int32_t n_shards;    /* site shards (GPUs); 1 = single GPU */
    int32_t shard;       /* this process' shard index */
    int32_t flags;       /* PLM_FLAG_* */
    double lambda_group; /* run_plmc's lambda_g (plmc -lg, tools.py:252-253): group regulariser on the coupling blocks,
                            lambda_group * sum_{i<j} sqrt(|J_ij|_F^2 + PLM_GROUP_DELTA^2); 0 = none */
} plm_problem_t;
/* smoothing of the group norm at the origin (the start point is J = 0, where the bare norm has no gradient) */
#define PLM_GROUP_DELTA 1e-4

#define PLM_FLAG_NONE 0
#define PLM_FLAG_VERBOSE 1
/* plmc -g / run_plmc(ignore_gaps=True) (tools.py:222-224): state 0 (the gap) is excluded from the
 * model.  Sites where a sequence has a gap contribute no conditional, gapped neighbours no coupling,
 * identities for reweighting count only non-gap matches, frequencies are normalised over ungapped
 * sequences.  All arrays keep the q-state layout of the alphabet; every entry that involves state 0
 * is zero (the Python host drops them and writes a (q-1)-state model file).  DESIGN.md section 2b. */
#define PLM_FLAG_IGNORE_GAPS 2
/* n_shards > 1 only (at most 16): parameters, gradient and L-BFGS state are split over the shards instead of
 * replicated: a shard's fields, the block pairs inside its site blocks and half of every
 * rectangle of block pairs it shares with another shard.  Needs a plm_collective_cb; per evaluation two all-to-alls
 * (couplings, gradient fragments; every rank exchanges with every other) and one scalar all-reduce replace the
 * all-gather of whole gradient slabs; the fitted parameters are assembled with one PLM_COLL_ALLREDUCE_F32 of the
 * canonical vector. */
#define PLM_FLAG_SHARDED_STATE 4
/* L-BFGS with a diagonal initial Hessian (inverse Hessian diagonal of the independent-site model) instead of the
 * textbook scalar one.  Same optimum (strictly convex objective), different path.  Measured on MI355X: fewer
 * iterations on short alignments, MORE at L = 300 -- opt-in. */
#define PLM_FLAG_PRECOND 8
/* Optimise fields and couplings jointly with L-BFGS, as libLBFGS-based plmc does, instead of the default variable
 * projection (fields solved exactly by Newton for every trial couplings, L-BFGS over the couplings only:
 * DESIGN.md section 2c).  Same objective, same optimum; the joint path needs ~10-20x more iterations to reach
 * |g|/|x| < epsilon.  With max_iter far below convergence (the reference default 100) the two paths stop at
 * different points.  The Python boundary exposes it as solver="joint" / PLM_HIP_SOLVER=joint / plmc_hip --solver joint.
 * (lambda_h = 0 always runs this path: the per-site Hessians of the field solver are then singular.) */
#define PLM_FLAG_JOINT_LBFGS 16
/* plm_fit / plm_fit_sharded / plm_fit_sharded_rccl with PLM_FLAG_IGNORE_GAPS only: the result arrays come back in the
 * (q-1)-state layout plmc -g itself writes -- fi, hi: [L][q-1]; fij, jij: [L(L-1)/2][q-1][q-1] -- instead of the q-state
 * layout with zero entries for the gap state.  The entries are dropped on the device before the download (the Python host
 * used to drop them with two strided copies of the pair arrays: 30 ms of a -g fit at the headline). */
#define PLM_FLAG_COMPACT_GAPS 1024
/* ---- convention switches ---------------------------------------------------------------------------------------
 * plmc is not available to this project, so a few of its conventions cannot be checked; each
 * is a switch here (same bits in the oracle, oracle/plm_oracle.c), so that a plmc binary on a future host pins the
 * path by choosing bits, not by changing code.  Defaults (bit clear) are the documented ones of DESIGN.md section 2.
 *   PLM_CONV_THRESHOLD_F32      SURVEY App. D-1: the cluster threshold as a float32 plmc would evaluate what run_plmc
 *                               sends it (-t 1-theta): ident >= (float)(1 - (float)(1 - theta)) * L, instead of the
 *                               integer rule ceil(theta * L - 1e-9).  Identical for theta = 0.8 and every L <= 2000.
 *   PLM_CONV_G_GAPS_IDENTICAL   -g: two gaps at a position count as identical in reweighting, as without -g (plmc's
 *                               usage text describes -g as excluding the gap from the POTENTIAL calculations only);
 *                               default: only non-gap matches count.
 *   PLM_CONV_G_UNGAPPED_LENGTH  -g: the identity threshold applies to the positions where both sequences are
 *                               ungapped, ident >= ceil(theta * n_both - 1e-9), instead of the full length.
 *   PLM_CONV_G_FREQ_TOTAL       -g: f_i and f_ij are normalised by N_eff (all sequences), so they sum to the ungapped
 *                               fraction of a site / pair; default: normalised over the ungapped sequences.
 *   PLM_CONV_FN_NO_GAP          SURVEY App. D-3: the Frobenius norm of a coupling block (zero-sum gauge over all q
 *                               states) sums the non-gap states only; default: all q states, as the reference's
 *                               CouplingsModel does (couplings/model.py:792).  No effect with -g (no gap state). */
#define PLM_CONV_THRESHOLD_F32 32
#define PLM_CONV_G_GAPS_IDENTICAL 64
#define PLM_CONV_G_UNGAPPED_LENGTH 128
#define PLM_CONV_G_FREQ_TOTAL 256
#define PLM_CONV_FN_NO_GAP 512
#define PLM_CONV_MASK (32 | 64 | 128 | 256 | 512)

/* Per-iteration progress: the 7 columns of plmc's stderr table that
 * parse_plmc_log() collects (tools.py:59-83): iter time cond fx -loglk ||h|| ||e||.
 * Return 0 to go on; any other value cancels the fit after this iteration (status PLM_STATUS_INTERRUPTED, the result
 * arrays hold the point reached).  This is how the signal handlers a pipeline installs around the stage
 * (evcouplings/utils/pipeline.py:476-545: SIGTERM / SIGINT -> sys.exit) reach a running fit: the plmc child process
 * was killed by the signal itself, an in-process solver has to be told. */
typedef int (*plm_iter_cb)(int32_t iter, double secs, double cond, double fx, double nll,
                           double norm_h, double norm_e, void *user);

/* Exchange step of the site-sharded evaluation: every shard has
 * written `bytes_per_shard` bytes at  dev_buf + shard * bytes_per_shard ; on return the
 * whole buffer (n_shards * bytes_per_shard) must hold every shard's part.  The Python host
 * implements it with torch.distributed.all_gather_into_tensor (RCCL).  Called on the
 * context's stream after a stream synchronise; return 0 on success. */
typedef int (*plm_exchange_cb)(void *dev_buf, size_t bytes_per_shard, int32_t n_shards,
                               int32_t shard, void *user);

/* Collectives of the sharded-state mode, implemented by the host with torch.distributed (RCCL).
 * All buffers are device pointers of this library; counts are BYTES per rank (arrays of n_shards).
 *   PLM_COLL_ALLTOALL      send -> recv with per-rank byte counts, messages in rank order
 *   PLM_COLL_ALLREDUCE_F64 in-place sum over ranks of send_counts[0] bytes of doubles at `send`
 *   PLM_COLL_ALLREDUCE_F32 in-place sum over ranks of send_counts[0] bytes of floats at `send`
 * Called after the context's stream has been synchronised; must return 0 on success with the result
 * visible to later work on that stream. */
#define PLM_COLL_ALLTOALL 1
#define PLM_COLL_ALLREDUCE_F64 2
#define PLM_COLL_ALLREDUCE_F32 3
/*   PLM_COLL_BROADCAST     send_counts[0] bytes at `send` travel from rank recv_counts[0] to every rank (in place).
 *                          Rounds 2-5 assembled the fitted parameters with two broadcasts per shard; since round 6 (a
 *                          shard's entries are no longer contiguous in the canonical order) that is one
 *                          PLM_COLL_ALLREDUCE_F32 of the canonical vector.  The operation stays part of the contract. */
#define PLM_COLL_BROADCAST 4
typedef int (*plm_collective_cb)(int32_t op, void *send, void *recv, const int64_t *send_counts,
                                 const int64_t *recv_counts, int32_t n_shards, int32_t shard, void *user);

typedef struct {
    float *weights;      /* [N]            or NULL */
    float *fi;           /* [L*q]          or NULL */
    float *fij;          /* [L(L-1)/2*q*q] or NULL (i<j blocks, [a][b]) */
    float *hi;           /* [L*q]          or NULL */
    float *jij;          /* [L(L-1)/2*q*q] or NULL */
    float *fn;           /* [L*L]          or NULL */
    float *cn;           /* [L*L]          or NULL */
    float n_eff;
    int32_t iters_done;
    int32_t n_evals;
    int32_t status;      /* PLM_STATUS_* */
    double fx;           /* final objective */
    double seconds_reweight, seconds_marginals, seconds_optimize, seconds_total;
    char status_msg[128];
} plm_result_t;

/* -- library ---------------------------------------------------------------------------- */
int plm_version(void);                 /* PLM_ABI_VERSION */
int plm_device_count(void);            /* visible gfx950 devices, or PLM_EDEVICE */
const char *plm_strerror(int code);
const char *plm_last_error(void);      /* thread-local message of the last failure */

/* -- whole stage: replaces the `plmc` child process (tools.py:266) ----------------------- */
/* Reweight -> marginals -> L-BFGS on the symmetric L2-regularised pseudo-likelihood ->
 * zero-sum gauge / Frobenius / APC scores.  `stream` is a hipStream_t (0 = null stream);
 * `device` the HIP device ordinal.  exchange/exchange_user are only used when
 * problem->n_shards > 1. */
int plm_fit(const plm_problem_t *problem, plm_result_t *result, int device, void *stream,
            plm_iter_cb iter_cb, void *iter_user, plm_exchange_cb exchange, void *exchange_user);

/* Same stage with problem->flags & PLM_FLAG_SHARDED_STATE: every rank calls it with its shard index;
 * all ranks return the same full result arrays. */
int plm_fit_sharded(const plm_problem_t *problem, plm_result_t *result, int device, void *stream,
                    plm_iter_cb iter_cb, void *iter_user, plm_collective_cb collective, void *collective_user);

/* The same with the collectives issued by the library itself: RCCL calls on the context's stream (one process per
 * GPU, ranks = shards), no host callback and no stream synchronisation around a collective.  Rank 0 creates an id
 * (plm_rccl_unique_id), the host hands its PLM_RCCL_ID_BYTES bytes to every rank by its own means (MPI, a file,
 * torch.distributed), then every rank calls plm_fit_sharded_rccl -- or plm_ctx_attach_rccl on a resident context
 * (a collective call: all ranks, each with its GPU current).  librccl is resolved at run time (a copy already in
 * the process first, then /opt/rocm's; PLM_RCCL_LIB overrides).  plm_rccl_selftest runs every collective on a
 * one-rank communicator. */
#define PLM_RCCL_ID_BYTES 128
int plm_rccl_unique_id(void *id_out);
int plm_rccl_runtime_version(void);          /* NCCL version code of the resolved library, 0 if none */
int plm_rccl_selftest(int device, void *stream);
/* Every rank of a prospective communicator: form it from `rccl_id`, exchange one all-to-all and one all-reduce, check
 * the data, destroy it.  PLM_OK on this rank = the library-issued transport works here (dist.py negotiates the ranks'
 * verdicts and falls back to the callback transport if any of them failed). */
int plm_rccl_probe(const void *rccl_id, int32_t nranks, int32_t rank, int device, void *stream);
/* The rank-local half of the probe (device, librccl, buffer, upload) with no communicator call in it.  A rank that
 * failed these steps inside plm_rccl_probe would leave its peers blocked in the communicator call: run this on every
 * rank and agree on the verdicts first. */
int plm_rccl_probe_local(int32_t nranks, int device, void *stream);
int plm_fit_sharded_rccl(const plm_problem_t *problem, plm_result_t *result, int device, void *stream,
                         plm_iter_cb iter_cb, void *iter_user, const void *rccl_id);

/* -- fine-grained, host buffers (parity tests) ------------------------------------------- */
/* plmc sequence reweighting; twin: align/alignment.py:1193-1233.  counts[s] = cluster size.
 * States are 0..PLM_REWEIGHT_MAX_STATE (0..123): the compare kernels fill with the bytes 124..127 (a lane's own gaps
 * under -g, the words past the end of a row, padded columns and rows) and count on no alignment byte having such a
 * value; an alignment that holds one is refused with PLM_EINVAL, the message names the value and the limit. */
#define PLM_REWEIGHT_MAX_STATE 123
int plm_reweight(const int8_t *msa, int32_t n_seqs, int32_t n_sites, double theta_id,
                 int32_t *counts_out);
/* the same with plmc -g semantics and / or PLM_CONV_* switches: flags = PLM_FLAG_IGNORE_GAPS | PLM_CONV_... */
int plm_reweight_ex(const int8_t *msa, int32_t n_seqs, int32_t n_sites, double theta_id, int32_t flags,
                    int32_t *counts_out);
/* plmc marginals; twins: align/alignment.py:1079-1153.  weights need not be normalised. */
int plm_marginals(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites,
                  int32_t n_states, float *fi_out, float *fij_out);
/* plmc objective + gradient at x (canonical layout). */
int plm_eval(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites,
             int32_t n_states, double lambda_h, double lambda_j, const float *x, double *fx_out,
             double *nll_out, float *g_out);
/* plmc EC scoring; twins: couplings/model.py:179-233, 744-775, 790-793.  fn/cn dense LxL. */
int plm_scores(const float *jij, int32_t n_sites, int32_t n_states, float *fn_out,
               float *cn_out);
/* the same with PLM_CONV_FN_NO_GAP in flags: state 0 left out of the Frobenius norm */
int plm_scores_ex(const float *jij, int32_t n_sites, int32_t n_states, int32_t flags, float *fn_out, float *cn_out);

/* ---- statistical energies under a fitted model -------------------
 * Replace the numba loops of evcouplings/couplings/model.py that the mutate stage and
 * CouplingsModel.hamiltonians / .single_mut_mat call:
 *   plm_hamiltonians  <->  _hamiltonians(sequences, J_ij, h_i)              model.py:25-60
 *   plm_potentials    <->  the sums of _single_mutant_hamiltonians           model.py:63-109
 * seqs: n x n_sites int8 states 0..q-1 (row-major); x_canonical: the model in the canonical
 * layout (h [L][q], then J pair blocks i<j row-major [q][q] -- the plmc_v2 .model order).
 * energies_out: n x 3 doubles (H, H_J, H_h) with H_J = sum_{i<j} J_ij(x_i,x_j), H_h = sum_i h_i(x_i).
 * potentials_out: n x n_sites x q floats, HJ[s][i][a] = sum_{j != i} J_ij(a, x_sj); the single-mutant
 * matrix of a sequence is dJ(i,a) = HJ[i][a] - HJ[i][x_i], dh(i,a) = h_i(a) - h_i(x_i).            */
int plm_hamiltonians(const int8_t *seqs, int32_t n, int32_t n_sites, int32_t n_states,
                     const float *x_canonical, int device, void *stream, double *energies_out);
int plm_potentials(const int8_t *seqs, int32_t n, int32_t n_sites, int32_t n_states,
                   const float *x_canonical, int device, void *stream, float *potentials_out);

/* ---- analysis of a fitted model: the numeric rest of CouplingsModel (DESIGN_NEXT_ROWS.md section 9.5) ---------
 * float64 throughout, host buffers in and out.  Dense [L][L][q][q] inputs are read in their i<j blocks only (the row
 * tails J[i, i+1:], L-1 copies into a compact device buffer).  PLM_EUNSUPPORTED for q outside 2..32; PLM_ENOMEM before
 * any allocation when the device lacks the memory.
 * plm_model_pair_scores replaces CouplingsModel._calculate_ecs's arithmetic (evcouplings/couplings/model.py:777-799):
 *   the zero-sum gauge over all q states (_zero_sum_gauge, model.py:180-233), fn = its Frobenius norm, and
 *   mi = sum_{f_ij(a,b) > 0} f_ij(a,b) log(f_ij(a,b) / (f_i(a) f_j(b))) -- +inf where f_ij > 0 meets f_i f_j = 0.
 *   jij_full, fij_full: dense [L][L][q][q] doubles, only i<j blocks read; fi: [L][q]; fn_out, mi_out: [L][L],
 *   symmetric, zero diagonal.                                                                                    */
int plm_model_pair_scores(const double *jij_full, const double *fij_full, const double *fi, int32_t n_sites,
                          int32_t n_states, int device, void *stream, double *fn_out, double *mi_out);
/* the same with flags: PLM_MODEL_FI_PRODUCT_F32 rounds f_i(a) f_j(b) to float32 before the division -- what numpy's
 * outer product gives for the float32 f_i a plmc_v2 .model file holds (model.py:797 np.dot of two float32 rows) */
#define PLM_MODEL_FI_PRODUCT_F32 1
int plm_model_pair_scores_ex(const double *jij_full, const double *fij_full, const double *fi, int32_t n_sites,
                             int32_t n_states, int32_t flags, int device, void *stream, double *fn_out, double *mi_out);
/* plm_double_mutants replaces CouplingsModel.double_mut_mat (model.py:715-742):
 *   D[i][j][a][b] = smm[i][a] + smm[j][b] + J_ij(a,b) - J_ij(a,t_j) - J_ij(t_i,b) + J_ij(t_i,t_j), D[j][i] = D[i][j]^T,
 *   zero diagonal blocks.  smm: [L][q] single-mutant dH of the target; target: L states 0..q-1;
 *   dmm_out: dense [L][L][q][q].                                                                                 */
int plm_double_mutants(const double *jij_full, const double *smm, const int8_t *target, int32_t n_sites,
                       int32_t n_states, int device, void *stream, double *dmm_out);
/* plm_independent_fields replaces the per-site fmin_bfgs of CouplingsModel.to_independent_model (model.py:882-927):
 *   h_i = argmin_x n_eff (log sum_a exp x_a - f_i.x) + lambda_h |x|^2, by damped Newton to |g|_inf <= 1e-12 max(1, n_eff).
 *   fi: [L][q]; h_out: [L][q]; iters_out: [L] Newton steps per site, may be NULL.  PLM_EINVAL for lambda_h <= 0 (the
 *   optimum need not exist); PLM_ENUMERIC if a site does not converge within the step cap (h_out holds the last iterates). */
int plm_independent_fields(const double *fi, int32_t n_sites, int32_t n_states, double lambda_h, double n_eff,
                           int device, void *stream, double *h_out, int32_t *iters_out);

/* ---- sampling from a fitted model: Gibbs sampler (DESIGN_NEXT_ROWS.md section 9.6) --------------------------------
 * Draws sequences from P(x) ~ exp beta (sum_i h_i(x_i) + sum_{i<j} J_ij(x_i, x_j)); nothing in the reference does this
 * (its loops stop at _hamiltonians / _delta_hamiltonian, couplings/model.py:25-177).  C independent chains; one sweep
 * visits the sites 0 .. L-1 in that order and draws x_ci ~ softmax_a beta (h_i(a) + sum_{j != i} J_ij(a, x_cj)) over the
 * allowed states; fixed sites are skipped.  Random numbers: Philox4x32-10, counter (chain, 0, sweep, site), key (seed low,
 * seed high); sweep counts from 0 across burn-in, thinning and snapshots; u = ((word0 >> 8) + 0.5) 2^-24 (below 1 in float32 too); with
 * e_a = exp(beta U_a - max) over the allowed states in state order and running sum S_a the new state is the first allowed
 * a with S_a > u S_last.  start == NULL: chain c starts from one such draw per site of softmax beta h_i with sweep index
 * 0xFFFFFFFF.  U accumulates in float32 over j = 0 .. L-1.  The result depends on (seed, chain index, model, options)
 * only: not on n_chains, the device or the run.
 * x_canonical: as plm_hamiltonians (q in 2..32, else PLM_EUNSUPPORTED; any n_sites >= 1 whose chain states fit the LDS:
 * 20 480, the tiled form up to about 2 500 and the slower direct form beyond, see plm_sample_plan).  samples_out: K x C x L states; energies_out: K x C x 3 doubles (H, H_J, H_h) of the snapshots at beta = 1,
 * what plm_hamiltonians returns for those rows, or NULL.  PLM_ENOMEM before any allocation, and before any array is
 * read, when the device cannot hold the expanded couplings (L^2 q ceil4(q) floats), the chain states and the outputs.
 * In plm_sample, plm_bm_fit and plm_ais an out-of-memory error that HIP reports only at a call after the allocations is
 * PLM_ENOMEM too (it was PLM_EDEVICE), as in plm_ctx_create.
 * PLM_EINVAL: start states outside 0..q-1, or not allowed at a site that is not fixed; no allowed state; beta not
 * finite or <= 0. */
typedef struct {
    int32_t  n_chains;      /* C >= 1, independent chains                                            */
    int32_t  burn_in;       /* full sweeps before the first snapshot, >= 0                           */
    int32_t  n_snapshots;   /* K >= 1 snapshots of all chains                                        */
    int32_t  thin;          /* sweeps between snapshots, >= 1 (ignored when K == 1)                  */
    float    beta;          /* inverse temperature, > 0, finite                                      */
    uint64_t seed;
    const int8_t  *start;   /* NULL, or C x L states: initial state of every chain                   */
    const uint8_t *fixed;   /* NULL, or L flags: sites that are never resampled                      */
    const uint8_t *allowed; /* NULL, or q flags: states that may be drawn (at least one set)         */
} plm_sample_opts;
int plm_sample(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_sample_opts *opts,
               int device, void *stream, int8_t *samples_out /* K x C x L */, double *energies_out /* K x C x 3 or NULL */);

/* The launch plan plm_sample and plm_bm_fit choose for a shape: which form of the sweep, and for the tiled form the tile
 * of chains per workgroup and the chunk of sites staged in LDS at a time.  n_cu > 0: the plan on a device with that many
 * compute units, pure host code (no device is needed); n_cu <= 0: on the current device.  For the direct form `tile` is
 * the chains per workgroup (256 / group size, the group being the power of two >= q, at least 2) and jc is 0.  The
 * environment variables PLM_SAMPLE_FORM=tiled|direct, PLM_SAMPLE_TILE=64|128|256 and PLM_SAMPLE_JC=1|2|4|8|12|16
 * (measurements and tests only; every plan returns the same states) are honoured as the two calls honour them: a tile or
 * chunk whose plan fails the planner's checks (jc q nv <= 8 tile, lds_bytes <= 163840) is PLM_EINVAL, never launched.
 * PLM_EUNSUPPORTED: q outside 2..32, or no form holds the chain states of a workgroup in LDS. */
typedef struct {
    int32_t direct;        /* 1: the direct form (lanes = chain x state), 0: the tiled form            */
    int32_t tile;          /* chains per workgroup                                                      */
    int32_t jc;            /* sites per staged chunk (tiled form)                                       */
    int32_t nv;            /* ceil(q / 4): float4 per row of the expanded couplings                     */
    int32_t n_workgroups;  /* ceil(n_chains / tile)                                                     */
    int64_t lds_bytes;     /* dynamic LDS of a workgroup                                                */
} plm_sample_plan_info;
int plm_sample_plan(int32_t n_sites, int32_t n_states, int32_t n_chains, int32_t n_cu, plm_sample_plan_info *out);

/* ---- Boltzmann-machine refinement of a model (DESIGN_NEXT_ROWS.md section 9.7) -------------------------------------
 * Plain gradient ascent on the likelihood of target frequencies, the model's own marginals estimated by persistent Gibbs
 * chains.  x_start: canonical parameters as for plm_hamiltonians; fi [L][q] and fij [L(L-1)/2][q][q] (pair blocks in the
 * canonical order): the targets.  Chains begin at opts->start, or from the sampler's start rule at x_start.  Local epoch
 * e = 0 .. n_epochs - 1, global epoch g = first_epoch + e:
 *   1. the couplings are expanded as for plm_sample
 *   2. every chain makes sweeps_per_epoch sweeps of plm_sample's contract (beta = 1, all states allowed, no fixed sites)
 *      with the sweep indices g k .. g k + k - 1
 *   3. exact int32 counts n_i(a), n_ij(a, b) over the chains; p = (float)n / (float)C
 *   4. trace row e = (max |fi - pi|, max |fij - pij|, rms of fij - pij over all pair entries, lr_g) with lr_g = lr when
 *      lr_decay_after == 0 or g + 1 <= lr_decay_after, else (float)((double)lr lr_decay_after / (g + 1))
 *   5. tol > 0 and both maxima <= tol: stop before the update (PLM_STATUS_CONVERGED, epochs_done = e); the callback
 *      returning non-zero stops the same way (PLM_STATUS_INTERRUPTED)
 *   6. x <- x + lr_g ((f - p) - 2 lambda x) elementwise in float32 (lambda_h on fields, lambda_j on couplings; both on
 *      the per-sequence scale, the plmc value over N_eff); lr_g == 0 leaves x as it is
 * After n_epochs updates the status is PLM_STATUS_MAXITER.  The counts are integers, so the result is bitwise
 * reproducible and depends on the arguments only.  Every output pointer may be NULL.  PLM_EINVAL: NULL arguments, sizes
 * below 1, negative or non-finite lr, lambda_h, lambda_j or tol, start states outside 0..q-1, (first_epoch + n_epochs)
 * sweeps_per_epoch at or above 2^32 - 1; PLM_EUNSUPPORTED: q outside 2..32; PLM_ENOMEM before any array is read. */
typedef struct {
    int32_t  n_chains;          /* C >= 1 persistent chains                                              */
    int32_t  n_epochs;          /* E >= 1 epochs of this call                                            */
    int32_t  sweeps_per_epoch;  /* k >= 1                                                                */
    int32_t  first_epoch;       /* e0 >= 0: global number of this call's first epoch (continuation)      */
    float    lr;                /* step, >= 0                                                            */
    int32_t  lr_decay_after;    /* T >= 0: the step decays as T / (g + 1) after global epoch T - 1       */
    float    lambda_h;          /* >= 0, per-sequence scale                                              */
    float    lambda_j;          /* >= 0, per-sequence scale                                              */
    float    tol;               /* >= 0; 0: never stop early                                             */
    uint64_t seed;
    const int8_t *start;        /* NULL, or C x L states                                                 */
} plm_bm_opts;
typedef struct {
    float  *x_out;       /* canonical parameters after the last applied update                           */
    float  *pi_out;      /* [L][q]            model frequencies of the last epoch that ran               */
    float  *pij_out;     /* [L(L-1)/2][q][q]                                                             */
    int8_t *chains_out;  /* C x L states of the last epoch that ran                                      */
    double *trace;       /* n_epochs x 4, one row per epoch that ran                                     */
    int32_t epochs_done; /* updates applied                                                              */
    int32_t status;      /* PLM_STATUS_MAXITER, PLM_STATUS_CONVERGED or PLM_STATUS_INTERRUPTED           */
} plm_bm_result;
/* Called once per epoch after its trace row is known and before its update, with the global epoch number. */
typedef int (*plm_bm_epoch_cb)(int32_t epoch, double max_dfi, double max_dfij, double rms_dfij, double lr, void *user);
int plm_bm_fit(int32_t n_sites, int32_t n_states, const float *fi, const float *fij, const float *x_start,
               const plm_bm_opts *opts, int device, void *stream, plm_bm_epoch_cb cb, void *user, plm_bm_result *result);

/* ---- log Z by annealed importance sampling (DESIGN_NEXT_ROWS.md section 9.8) ---------------------------------------
 * Estimates the partition function of the model (h, J) of plm_sample along the path
 *   p_beta(x) ~ exp(sum_i h_i(x_i) + beta sum_{i<j} J_ij(x_i, x_j)),
 * from the independent-site model of the fields (beta = 0: sampled exactly, log Z_0 = sum_i log sum_a exp h_i(a)) to the
 * couplings scaled by the last beta.  Schedule: K + 1 float32 values beta_0 = 0 <= beta_1 <= ... <= beta_K, all finite;
 * betas == NULL: beta_k = (float)((double)k / K).  beta_K need not be 1: the result is log Z of the model with the
 * couplings scaled by beta_K, so every prefix of a schedule is a schedule.
 * Chain c starts from plm_sample's start rule at beta = 1 with all states allowed.  E = 1/2 sum_i (double)U_i[x_i] there,
 * U_i[a] = sum_{j != i} J_ij(a, x_j) in float32 from 0 over j = 0 .. L-1.  Step k = 1 .. K: log w += ((double)beta_k -
 * (double)beta_{k-1}) E, then sweeps_per_temp = n sweeps with the indices (k-1) n .. k n - 1; a site update draws (the draw
 * and the Philox counter of plm_sample) on fadd(h_i(a), fmul(beta_k, U_i[a])) and adds (double)U_i[a_new] -
 * (double)U_i[a_old] to E in float64.
 *   log_z = log_z0 + m + log((1/C) sum_c exp(log_w[c] - m)), m = max log_w, summed in chain order in float64
 *   ess = (sum w)^2 / sum w^2, log_z_se = std(w, ddof = 1) / (sqrt(C) mean w) with w = exp(log_w - m); 0 for C = 1
 * log_w[c] depends on (seed, c, model, schedule, n) only: not on C, the launch plan or steps_per_launch.  The steps run in
 * launches of at most steps_per_launch steps (0: about a second each); cb, if given, is called between launches and
 * cancels by returning non-zero: status PLM_STATUS_INTERRUPTED, log_z, log_z_se and ess NaN, the arrays hold the state
 * reached after steps_done steps.  PLM_EINVAL (before the device is looked at): NULL opts or result, sizes below 1, a
 * schedule that does not start at 0, decreases or holds a non-finite value, K n >= 2^32 - 1; PLM_EUNSUPPORTED: q outside
 * 2..32; PLM_ENOMEM before any array is read. */
typedef struct {
    int32_t n_chains;          /* C >= 1                                                               */
    int32_t n_temps;           /* K >= 1 annealing steps                                               */
    int32_t sweeps_per_temp;   /* n >= 1                                                               */
    int32_t steps_per_launch;  /* 0 = default; any value gives the same bits                           */
    const float *betas;        /* NULL, or K + 1 values as defined above                               */
    uint64_t seed;
} plm_ais_opts;
typedef struct {
    double log_z, log_z0, log_z_se, ess;
    double *log_w;             /* [C] or NULL                                                          */
    double *e_j;               /* [C] tracked coupling energy of the final states, or NULL             */
    int8_t *states;            /* C x L final states, or NULL                                          */
    int32_t steps_done;
    int32_t status;            /* PLM_STATUS_CONVERGED when all K steps ran, else PLM_STATUS_INTERRUPTED */
} plm_ais_result;
typedef int (*plm_ais_cb)(int32_t steps_done, int32_t n_steps, void *user);
int plm_ais(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_ais_opts *opts, int device,
            void *stream, plm_ais_cb cb, void *user, plm_ais_result *result);

/* ---- parallel tempering: replica-exchange Gibbs sampling (DESIGN_NEXT_ROWS.md section 9.9) -------------------------
 * Samples the family of plm_ais, p_beta(x) ~ exp(sum_i h_i(x_i) + beta sum_{i<j} J_ij(x_i, x_j)), at the R inverse
 * temperatures of a ladder at once, and lets neighbouring temperatures exchange.  Ladder: R >= 1 float32 values
 * 0 <= beta_0 <= ... <= beta_{R-1}, all finite; beta_0 need not be 0 and equal neighbours are allowed.
 * Walkers: C independent ladders of R walkers.  Walker w = l R + s is slot s of ladder l, and chain w of the random
 * numbers.  It carries its states, its tracked coupling energy E (float64) and its rung rho(w) in 0..R-1.  States never
 * move between walkers: an exchange swaps rungs.  Per ladder the maps rung_of_slot and slot_of_rung are inverses.
 * Start, start == NULL: rho(l R + s) = s; states from plm_sample's start rule at beta = 1 with all states allowed (sweep
 * index 0xFFFFFFFF), E = 1/2 sum_i (double)U_i[x_i] from the measuring pass, all exactly as plm_ais.  start (C R x L
 * states) given: rho from start_rungs (NULL: rho = s) and E from the measuring pass, or, with start_e, E as given: the
 * bit-exact continuation of an earlier call from its walkers, rungs and walker_e with first_round moved on.
 * Round: the global round number is g = first_round + the local number.
 *   1. n = sweeps_per_round sweeps with the sweep indices g n .. g n + n - 1.  A site update of walker w is the one of
 *      plm_ais at beta = beta_rho(w): U in float32 from 0 over j = 0 .. L-1, j != i; arg_a = fadd(h_i(a), fmul(beta, U_a));
 *      the draw of plm_sample on arg with beta = 1; Philox counter (w, 0, sweep, site); E += (double)U[a_new] -
 *      (double)U[a_old].
 *   2. one exchange pass of parity p = g mod 2: for every ladder l and every r = p (mod 2) with r + 1 < R, a =
 *      slot_of_rung[r], b = slot_of_rung[r + 1], Delta = ((double)beta_{r+1} - (double)beta_r) (E_a - E_b) (the two
 *      differences, then one product, each rounded once), u = plm_sample's uniform of Philox word 0 at counter
 *      (l, 1, g, r), same key, widened to double; accept iff Delta >= 0 or u < exp(Delta) in float64.  On acceptance the
 *      two walkers swap rungs and accepts[r] goes up by one.  (The fields cancel in Delta: E holds the coupling part.)
 * Schedule: burn_in rounds, then K = n_snapshots snapshots thin rounds apart: snapshot k is taken after burn_in + k thin
 * rounds of the call (with burn_in = 0 snapshot 0 is the start); the call runs burn_in + (K - 1) thin rounds.  A snapshot
 * holds, in rung order, the states and E of the walker at every rung: samples K x C x R x L, e_j K x C x R; with
 * all_rungs == 0 rung R - 1 only: K x C x L and K x C.  attempts[r] = C x the rounds of the call whose parity is r mod 2.
 * Ladder l depends on (seed, l, model, ladder, n, first_round and the start of that ladder) only: not on C, the launch
 * plan or the run.  cb, if given, is called between rounds and cancels by returning non-zero: status
 * PLM_STATUS_INTERRUPTED, rounds_done rounds ran, walkers, rungs, walker_e, accepts and attempts hold the state reached,
 * snapshots not yet taken are zero.  Every output pointer may be NULL.
 * PLM_EINVAL (before the device is looked at): NULL opts or result, sizes below 1, burn_in or first_round below 0, thin
 * below 1; a ladder that is NULL, decreases, is negative or holds a non-finite value; (first_round + rounds + 1) n at or
 * above 2^32 - 1; start_rungs without start, start_e without both; C R L at or above 2^31.  PLM_EUNSUPPORTED: q outside
 * 2..32.  PLM_ENOMEM before any array is read; then PLM_EINVAL for start states outside 0..q-1 and for start_rungs that
 * are not a permutation of 0..R-1 within each ladder. */
typedef struct {
    int32_t n_ladders;         /* C >= 1 independent ladders                                           */
    int32_t n_rungs;           /* R >= 1 temperatures                                                  */
    int32_t burn_in;           /* rounds before the first snapshot, >= 0                               */
    int32_t n_snapshots;       /* K >= 1                                                               */
    int32_t thin;              /* rounds between snapshots, >= 1                                       */
    int32_t sweeps_per_round;  /* n >= 1                                                               */
    int32_t first_round;       /* >= 0: global number of this call's first round (continuation)        */
    int32_t all_rungs;         /* 0: snapshots hold rung R - 1 only; else every rung                   */
    const float *betas;        /* R values as defined above                                            */
    uint64_t seed;
    const int8_t  *start;       /* NULL, or C R x L states of the walkers                              */
    const int32_t *start_rungs; /* NULL, or C R rungs of the walkers                                   */
    const double  *start_e;     /* NULL, or C R tracked energies of the walkers                        */
} plm_pt_opts;
typedef struct {
    int8_t  *samples;          /* K x C x (R or 1) x L states in rung order, or NULL                   */
    double  *e_j;              /* K x C x (R or 1) tracked coupling energies of those rows, or NULL    */
    int64_t *accepts;          /* [R - 1] accepted exchanges between the rungs r and r + 1, or NULL    */
    int64_t *attempts;         /* [R - 1] attempted ones, or NULL                                      */
    int8_t  *walkers;          /* C R x L final states of the walkers, or NULL                         */
    int32_t *rungs;            /* C R final rungs of the walkers, or NULL                              */
    double  *walker_e;         /* C R final tracked energies of the walkers, or NULL                   */
    int32_t rounds_done;
    int32_t status;            /* PLM_STATUS_CONVERGED when all rounds ran, else PLM_STATUS_INTERRUPTED */
} plm_pt_result;
typedef int (*plm_pt_cb)(int32_t rounds_done, int32_t n_rounds, void *user);
int plm_pt(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_pt_opts *opts, int device,
           void *stream, plm_pt_cb cb, void *user, plm_pt_result *result);

/* ---- simulated annealing and greedy ascent (DESIGN_NEXT_ROWS.md section 9.13) --------------------------------------
 * Searches for sequences of high statistical energy H(x) = sum_i h_i(x_i) + sum_{i<j} J_ij(x_i, x_j) (P(x) ~ exp H(x):
 * higher is better) of the model of plm_sample.  C independent chains; a sweep visits the sites 0 .. L-1 in that order and
 * skips the fixed ones.  A site update computes U_a = h_i(a) + sum_{j != i} J_ij(a, x_j) in float32, from the field over
 * j = 0 .. L-1, as plm_sample does, and is one of two kinds:
 *   annealing at beta   the draw of plm_sample on U with that beta and the allowed mask, Philox counter (chain, 0, sweep,
 *                       site), key (seed low, seed high): bit for bit the update of plm_sample at that beta, sweep and seed
 *   greedy              a* = the first allowed state in state order with the largest U over the allowed states; the chain
 *                       moves to a* iff U[a*] > U[x_i] in float32 (a tie never moves); no random numbers
 * and after either gain += (double)U[a_new] - (double)U[a_old] in float64: the change of H up to the rounding of the two
 * float32 sums, 0 when nothing moved.
 * Schedule: 1. the start: opts->start, or (NULL) plm_sample's start rule at beta = 1 with the allowed mask and sweep index
 * 0xFFFFFFFF; gain = 0; checkpoint 0: best = the start, best_gain = 0, best_at = 0.  2. step k = 1 .. K: n =
 * sweeps_per_step annealing sweeps at betas[k-1] with the sweep indices first_sweep + (k-1) n + s, then checkpoint k: if
 * gain > best_gain (strictly) the chain's states go to best, best_gain = gain, best_at = k.  3. at most G = max_greedy
 * greedy sweeps, numbered from 1: a chain that completes a sweep without a move is converged and never moves again;
 * last_move[c] is the number of the last greedy sweep in which chain c moved (0: none), converged[c] = 1 iff it completed
 * some sweep without a move.  With G >= 1 checkpoint K + 1 follows, under the same rule.
 * Chain c depends on (seed, c, model, options, its start) only: not on C, the launch plan, the device or how the schedule
 * is cut into launches.  The steps run in launches of at most steps_per_launch steps (0: about a second each) and the
 * greedy sweeps in launches of at most that many steps' sweeps; cb, if given, is called after a launch of annealing steps
 * while work remains (further steps, or the greedy phase) and cancels by returning non-zero: status
 * PLM_STATUS_INTERRUPTED, the greedy phase does not run, the arrays hold the state reached after steps_done steps,
 * last_move and converged are zero.  energies / best_energies: (H, H_J, H_h) of states / best, what plm_hamiltonians
 * returns for those rows (for n_sites == 1: (h(x), 0, h(x)), as plm_sample).
 * PLM_EINVAL (before the device is looked at): NULL opts or result, n_sites or n_chains or sweeps_per_step below 1,
 * n_steps, max_greedy or steps_per_launch below 0, n_steps == 0 with max_greedy == 0, betas NULL with n_steps > 0 or given
 * with n_steps == 0, a beta that is not finite or <= 0, first_sweep + K n at or above 2^32 - 1, no allowed state;
 * PLM_EUNSUPPORTED: q outside 2..32.  PLM_ENOMEM before any array of the model or the start is read (the expanded table,
 * the canonical vector, 2 C L states, 28 C bytes of scalars); then PLM_EINVAL for n_chains x n_sites at or above 2^31 and
 * for start states outside 0..q-1 or not allowed at a site that is not fixed. */
typedef struct {
    int32_t  n_chains;          /* C >= 1                                                               */
    int32_t  n_steps;           /* K >= 0 annealing steps                                               */
    int32_t  sweeps_per_step;   /* n >= 1                                                               */
    int32_t  max_greedy;        /* G >= 0; K == 0 and G == 0 together: PLM_EINVAL                       */
    uint32_t first_sweep;       /* sweep index of the first annealing sweep (continuation)              */
    int32_t  steps_per_launch;  /* 0 = default; any value gives the same bits                           */
    const float *betas;         /* K values, finite and > 0, in any order (reheating is allowed); NULL iff K == 0 */
    uint64_t seed;
    const int8_t  *start;       /* NULL, or C x L states                                                */
    const uint8_t *fixed;       /* NULL, or L flags; as plm_sample: a fixed site keeps what the start gave it */
    const uint8_t *allowed;     /* NULL, or q flags, at least one set                                   */
} plm_anneal_opts;
typedef struct {
    int8_t  *states;        /* C x L final states                                                       */
    double  *gain;          /* [C] tracked H(final) - H(start)                                          */
    int8_t  *best;          /* C x L states at the best checkpoint                                      */
    double  *best_gain;     /* [C]                                                                      */
    int32_t *best_at;       /* [C] checkpoint 0 .. K + 1                                                */
    int32_t *last_move;     /* [C]                                                                      */
    uint8_t *converged;     /* [C]                                                                      */
    double  *energies;      /* C x 3 (H, H_J, H_h) of `states`                                          */
    double  *best_energies; /* C x 3 of `best`                                                          */
    int32_t steps_done;     /* annealing steps that ran                                                 */
    int32_t status;         /* PLM_STATUS_CONVERGED: all K steps and the greedy phase ran; else PLM_STATUS_INTERRUPTED */
} plm_anneal_result;        /* every pointer may be NULL */
typedef int (*plm_anneal_cb)(int32_t steps_done, int32_t n_steps, void *user);
int plm_anneal(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_anneal_opts *opts, int device,
               void *stream, plm_anneal_cb cb, void *user, plm_anneal_result *result);

/* ---- mean-field direct coupling analysis ---------------------------
 * Replaces the arithmetic of evcouplings/couplings/mean_field.py:163-222 (MeanFieldDCA.fit: weights,
 * frequencies, pseudo-count regularisation :717-790, covariance matrix :897-940, J = -C^-1 :204-210 and
 * :943-975, fields :977-1014) and :792-893 (direct_information).  All outputs are caller-allocated host
 * buffers; any pointer may be NULL to skip that output.                                                */
typedef struct {
    float *weights;     /* n_seqs                    1 / cluster size                                    */
    float n_eff;
    float *fi;          /* n_sites * q               raw frequencies                                     */
    float *fij;         /* pairs * q * q             raw pair frequencies, i<j blocks row-major           */
    double *hi;         /* n_sites * q               fields                                              */
    double *jij_full;   /* n_sites^2 * q^2           dense couplings [i][j][a][b], diagonal blocks included
                                                     (what reshape_invC_to_4d returns)                   */
    float *jij;         /* pairs * q * q             the i<j blocks in the .model file's precision        */
    double *di;         /* n_sites^2                 direct information, symmetric, zero diagonal         */
} plm_mf_result_t;
int plm_meanfield(const int8_t *msa, int32_t n_seqs, int32_t n_sites, int32_t n_states, double theta_id,
                  double pseudo_count, int device, void *stream, plm_mf_result_t *out);
/* Direct information of every pair from given couplings and frequencies: replaces
 * evcouplings/couplings/mean_field.py:842-893 direct_information(J_ij, f_i).  jij_full: dense
 * [L][L][q][q] doubles (only i<j blocks are read); fi: [L][q] doubles; di_out: [L][L] doubles.       */
int plm_direct_information(const double *jij_full, const double *fi, int32_t n_sites, int32_t n_states,
                           int device, void *stream, double *di_out);

/* ---- alignment statistics of the upstream align stage -----------------------------
 * One pass over an integer-coded alignment (n x n_sites, row-major, states 0..126) for the quantities
 * evcouplings/align/protocol.py:806-1016 (modify_alignment) filters and reports on:
 *   seq_gaps[s]   = #{i : msa[s][i] == gap_state}        Alignment.count("-", axis="seq")  (alignment.py:707-747)
 *   col_gaps[i]   = #{s : msa[s][i] == gap_state}        Alignment.count(gap, axis="pos")
 *   ident[s]      = #{i : msa[s][i] == query[i]}         identities_to_seq(seq, matrix)    (alignment.py:1157-1190)
 * Raw integer counts (the reference normalises on the host); any output pointer may be NULL, query may be NULL
 * when ident is.                                                                                              */
int plm_alignment_stats(const int8_t *msa, int32_t n_seqs, int32_t n_sites, int32_t gap_state, const int8_t *query,
                        int32_t *seq_gaps, int32_t *col_gaps, int32_t *ident, int device, void *stream);

/* ---- pairwise identities between two sets of sequences, and the greedy redundancy filter built on them -------------
 * For rows s of a and t of b over the n_sites columns (states 0..126, row-major):
 *   m(s,t) = #{columns where both rows hold the same state}; with a gap state, a column where either row has the gap
 *            is no match (gap_state = -1: gaps are ordinary states)
 *   d(s,t) = PLM_IDENT_DENOM_COLUMNS: n_sites;  _BOTH: #{columns where neither row has the gap};
 *            _SHORTER: min(residues of s, residues of t)            (_BOTH and _SHORTER need a gap state)
 *   similar: _COLUMNS: m >= ceil(threshold * n_sites - 1e-9), the threshold of plm_reweight (a == b, no gap state:
 *            n_within equals its counts); _BOTH / _SHORTER: d > 0 and m >= ceil(threshold * d - 1e-9)
 *   nearest: the pair with the largest m / d, compared exactly (m1 d2 against m2 d1 in 64 bits; d = 0 is identity 0),
 *            ties to the smallest t.
 * plm_cross_identities: best_index / best_match / best_denom [n_a] describe the nearest row of b (index -1, 0, 0 when
 * exclude_self leaves no partner), n_within [n_a] counts the similar rows; exclude_self (a and b hold the same rows)
 * skips t == s in both.  Any output may be NULL.  The result does not depend on how the rows of b are split over
 * workgroups; PLM_IDENT_TPER (rows of b per workgroup, an integer >= 1; measurements and tests) forces the split.
 * plm_redundancy_filter: keep_out[0] = 1, keep_out[s] = 1 iff no kept t < s is similar to s (exclude_self is ignored),
 * exactly the sequential definition; n_kept may be NULL.  Device memory is O(n_seqs n_sites), no pair matrix.
 * PLM_EINVAL (before the device is looked at): NULL inputs or opts, an empty set or one of more than 2^30 rows, states
 * outside 0..126, gap_state outside -1..126, an unknown denominator or one that needs a gap state without one, a
 * threshold that is not finite, a PLM_IDENT_TPER that is no positive integer.  PLM_ENOMEM before any allocation.     */
#define PLM_IDENT_DENOM_COLUMNS 0
#define PLM_IDENT_DENOM_BOTH 1
#define PLM_IDENT_DENOM_SHORTER 2
typedef struct {
    int32_t gap_state;      /* -1: none */
    int32_t denominator;    /* PLM_IDENT_DENOM_* */
    int32_t exclude_self;   /* cross call with a == b */
    double threshold;
} plm_ident_opts;
int plm_cross_identities(const int8_t *a, int32_t n_a, const int8_t *b, int32_t n_b, int32_t n_sites,
                         const plm_ident_opts *opts, int32_t *best_index, int32_t *best_match, int32_t *best_denom,
                         int32_t *n_within, int device, void *stream);
int plm_redundancy_filter(const int8_t *msa, int32_t n_seqs, int32_t n_sites, const plm_ident_opts *opts,
                          uint8_t *keep_out, int32_t *n_kept, int device, void *stream);

/* ---- three-site counts, frequencies and connected correlations of an alignment ---------------------------------------
 * msa: n_seqs x n_sites int8, row-major, states 0..q-1, 2 <= q <= 32, n_sites >= 3.  weights: n_seqs floats, finite,
 * >= 0, not all zero; NULL = every weight is 1.  The weights enter as fixed-point integers, computed on the host in
 * double arithmetic: e = the largest integer <= 30 with max(w) 2^e <= 2^30, wq_n = llrint((double)w_n 2^e) (NULL: wq_n =
 * 1), W = sum_n wq_n (returned in *total; W = 0, possible when only tiny weights sit next to huge ones, is PLM_EINVAL).
 * For a triplet i < j < k:
 *   count_ijk(a,b,c) = sum_n wq_n [x_ni = a, x_nj = b, x_nk = c], an exact integer (u64);
 *   the lower-order counts are its exact integer marginals (count_ij(a,b) = sum_c count_ijk(a,b,c), ...);
 *   f = count / W in float64, at every order;
 *   C_ijk(a,b,c) = f_ijk - f_ij(a,b) f_k(c) - f_ik(a,c) f_j(b) - f_jk(b,c) f_i(a) + 2 f_i(a) f_j(b) f_k(c) in float64;
 *   norm2 = sum C^2 and maxabs = max |C| over the cells where none of a, b, c equals skip_state (-1: over all cells),
 *   argmax = a q^2 + b q + c of a cell that attains maxabs.
 * The counts are accumulated in integers: no output depends on the launch plan, on how the sequences are split over
 * workgroups or on the order of arrival.  PLM_TRIPLET_PLAN forces the plan (measurements and tests): a comma-separated
 * list of w32 / w64 (counter width; w32 is refused when W >= 2^32), n<int> (sequences per workgroup of the listed
 * call), c<int> (c values per counting pass, 1..32), k<int> (workgroups sharing the k range of one (i, j) of the scan,
 * 1..65535), u (the scan through the kernels of the listed call).
 * plm_triplet_stats: the listed triplets [T][3] int32, i < j < k (a triplet may be listed twice).  counts [T][q][q][q]
 *   u64, freq / connected [T][q][q][q] f64; an output is written when its pointer is not NULL and its bit is in want.
 * plm_triplet_scan: every i < j < k among `sites` (n_sel >= 3 strictly ascending site indices; NULL = all sites, n_sel
 *   ignored), lexicographic in the positions of the selection: norm2, maxabs [C(n_sel,3)] f64, argmax [C(n_sel,3)]
 *   int32; any of them may be NULL.
 * PLM_EINVAL (with a message, before the device is looked at): NULL msa, opts or triplets; n_seqs < 1; n_sites < 3; q
 * outside 2..32; a state outside 0..q-1; a triplet that is not i < j < k inside 0..n_sites-1; n_triplets < 1; sites not
 * strictly ascending, out of range, or fewer than 3 (or so many that the triplets pass 2^31 - 1); skip_state outside
 * -1..q-1; a weight that is negative or not finite; W = 0; a malformed PLM_TRIPLET_PLAN.  PLM_ENOMEM before any
 * allocation when images plus outputs (T q^3 8 bytes per wanted array of the listed call) do not fit.               */
#define PLM_TRIPLET_COUNTS 1
#define PLM_TRIPLET_FREQ 2
#define PLM_TRIPLET_CONNECTED 4
typedef struct {
    int32_t skip_state;   /* -1: none; else 0..q-1, left out of norm2 / maxabs / argmax only */
    int32_t want;         /* PLM_TRIPLET_COUNTS | _FREQ | _CONNECTED  (listed call)            */
} plm_triplet_opts;
int plm_triplet_stats(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                      const int32_t *triplets, int32_t n_triplets, const plm_triplet_opts *opts, uint64_t *counts,
                      double *freq, double *connected, uint64_t *total, int device, void *stream);
int plm_triplet_scan(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                     const int32_t *sites, int32_t n_sel, const plm_triplet_opts *opts, double *norm2, double *maxabs,
                     int32_t *argmax, uint64_t *total, int device, void *stream);

/* ---- principal components of an alignment, and projections on them ------------------------------------------------------
 * msa, weights, wq_n and W as in the three-site section above (same quantisation rule, same errors; n_sites >= 1 here).
 *   f_i(a)       = count_i(a) / W in float64, count_i(a) = sum_n wq_n [x_ni = a] an exact integer; returned in mean [L][q];
 *   phi_n[(i,a)] = [x_ni = a] - f_i(a) for every site i and every state a != skip_state (skip_state = -1 keeps all
 *                  states): D = L q or L (q - 1) features;
 *   C            = (1/W) sum_n wq_n phi_n phi_n^T, never formed;  total_variance = trace C = sum f_i(a) (1 - f_i(a)) over
 *                  the kept features, from the counts;
 *   eigenvalues  lambda_1 >= ... >= lambda_k, the k largest of C, with orthonormal eigenvectors components [k][L][q] in
 *                  float64 (zeros at the skipped state); the entry of a component with the largest magnitude is positive
 *                  (the smallest index of a tie decides);
 *   t_c(x)       = sum_i v_c[(i, x_i)] - sum_{i,a} f_i(a) v_c[(i,a)], the projection of a sequence x; a skipped state
 *                  contributes 0.  scores [n][k].
 * Method: block subspace iteration with a Rayleigh-Ritz step in float64; b = min(k + oversample, D, 64) columns started
 * from Philox4x32-10 numbers keyed by (seed, feature, column).  An iteration computes U = Phi V and Y = Phi^T diag(wq) U / W,
 * the b x b matrices V^T Y, V^T V, Y^T Y on the device, the b x b eigenproblems on the host (Jacobi), the rotation to the
 * Ritz vectors and the next orthonormal block on the device; one host synchronisation per iteration.  The residuals
 * |C v_c - theta_c v_c| of the Ritz vectors of an iteration are summed directly by the rotation and read with the next
 * iteration's matrices; the loop stops when they are <= tol theta_1 for the first k columns, or after max_iter block
 * products (iterations counts them).  Then the k vectors are made orthonormal to rounding (Gram-Schmidt, twice) and
 * evaluated once more: eigenvalues are their Rayleigh quotients v.Cv / v.v, residuals [k] the absolute norms |C v_c - lambda_c v_c|,
 * converged = 1 iff every residual is <= tol lambda_1.  Running out of iterations is a result (converged = 0), no error.
 * Rank: a direction of the block whose Gram eigenvalue is not above D 2^-44 times the largest is dropped (its column is
 * zero from then on); this is where a block wider than the rank of C (at most min(D, n_seqs - 1)), or C = 0, ends up.  A
 * component beyond that numerical rank -- one whose direction was dropped, or whose Rayleigh quotient is not above
 * D 2^-52 total_variance -- is returned as a unit vector orthogonal to the others with eigenvalue 0 and residual 0.
 * Every float64 sum has one order, fixed by constants of the library (256 sequences per serial slice sum, slices
 * ascending; 32 feature rows per serial chunk sum, chunks ascending): no output bit depends on the launch plan.
 * PLM_PCA_PLAN forces the plan (measurements and tests): a comma-separated list of g<int> (workgroups per site of the
 * Phi^T kernel, 1..65535), s<int> (sequences per workgroup of the Phi V kernel, 1..1048576), r<int> (32-row chunks per
 * workgroup of the b x b products and of the rotation, 1..65535).
 * plm_pca_fit: scores [n_seqs][k] may be NULL, as may total_variance, total, iterations, converged; where given, scores
 *   equals plm_pca_project of the same rows through the returned mean and components, bit for bit.
 * plm_pca_fit_cb: the same with a callback, called once per iteration after its synchronisation with the iteration's
 *   number and the largest relative residual seen (infinity at the first); a non-zero return stops the loop: the outputs
 *   describe the vectors reached, converged = 0 and *status = PLM_STATUS_INTERRUPTED (otherwise _CONVERGED / _MAXITER).
 * plm_pca_project: any n sequences through a given mean [L][q] and components [k][L][q].
 * PLM_EINVAL (with a message, before the device is looked at): NULL inputs; n_seqs, n < 1; n_sites < 1 (or > 65535); q
 * outside 2..32; a state outside 0..q-1; k < 1, k > D or k > 64; oversample < 0; a weight that is negative or not finite;
 * W = 0; tol <= 0; max_iter < 1; skip_state outside -1..q-1; a mean or component that is not finite (plm_pca_project); a
 * malformed PLM_PCA_PLAN.  PLM_ENOMEM before any allocation when the image, U, the blocks and the slice sums do not fit. */
typedef struct {
    int32_t n_components;   /* k >= 1 */
    int32_t oversample;     /* >= 0; default 8 */
    int32_t max_iter;       /* >= 1 */
    int32_t skip_state;     /* -1..q-1 */
    double  tol;            /* > 0 */
    uint64_t seed;
} plm_pca_opts;
typedef int (*plm_pca_cb)(int32_t iteration, double max_relative_residual, void *user);
int plm_pca_fit(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                const plm_pca_opts *opts, double *mean, double *components, double *eigenvalues, double *residuals,
                double *total_variance, uint64_t *total, int32_t *iterations, int32_t *converged, double *scores,
                int device, void *stream);
int plm_pca_fit_cb(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                   const plm_pca_opts *opts, double *mean, double *components, double *eigenvalues, double *residuals,
                   double *total_variance, uint64_t *total, int32_t *iterations, int32_t *converged, double *scores,
                   int device, void *stream, plm_pca_cb cb, void *user, int32_t *status);
int plm_pca_project(const int8_t *seqs, int32_t n, int32_t n_sites, int32_t n_states, const double *mean,
                    const double *components, int32_t k, int32_t skip_state, double *scores, int device, void *stream);

/* ---- residue distance maps of structures, and their minimum over many chains -----------------------------------------
 * The arithmetic of the reference's compare stage (_distances, compare/distances.py:24-88, and the minimum that
 * DistanceMap.aggregate takes over a stack of maps), all in float64.  For a residue pair (i, j):
 *   d2(a, b)  = (dx dx + dy dy) + dz dz over the atoms a of i and b of j, dx = x_a - x_b and so on; every difference,
 *               product and sum is rounded once (no fused multiply-add);
 *   dist(i,j) = min(1e6, sqrt(min over (a, b) of d2)), one correctly rounded square root (sqrt is monotone: this is the
 *               minimum of the distances).  1e6 is the reference's LARGE_DIST; a residue without atoms yields it too.
 * A minimum of correctly rounded values: no output bit depends on the launch plan.  PLM_DIST_PLAN forces the plan
 * (measurements and tests): a comma-separated list of t<int> (residues on the row side of a workgroup's tile: 4, 8, 16,
 * 32 or 64; the column side is 256 / t) and c<int> (atoms of a residue per staging chunk, 1..32).
 * plm_residue_distances: coords [n_atoms][3]; ranges [n_res][2] int32, the first and last atom of a residue, inclusive;
 *   ranges may overlap, leave atoms out, and be empty (last < first, whatever the two values are).  coords_j == NULL and
 *   ranges_j == NULL (n_atoms_j, n_res_j ignored): the symmetric call on axis i alone; only the pairs i <= j are
 *   computed and stored at both places, so the output is exactly symmetric, and equal bit for bit to the call with the
 *   chain on both axes.  dist_out [n_res_i][n_res_j].
 * plm_distance_maps_aggregate: n_chains chains in one coordinate array and one range array (atom indices count from
 *   the start of the coordinate array); chain c owns the residues chain_offsets[c] .. chain_offsets[c + 1] - 1
 *   (chain_offsets [n_chains + 1], ascending from 0).  slots_i / slots_j [residues]: the row / column of a residue in
 *   the aggregated map, -1 = not in it; slots_j == NULL: slots_i serves both axes.  maps [n_maps][2]: (chain on axis i,
 *   chain on axis j); a chain may be on both axes and in any number of maps.  agg [m_i][m_j]: the minimum of dist over
 *   the maps that cover the cell, NaN where none does; count [m_i][m_j] int32: how many do.  Either may be NULL.  No
 *   n_maps x m_i x m_j array is made: device memory is the inputs plus the outputs.
 * PLM_EINVAL (with a message, before the device is looked at): NULL inputs; only one of coords_j / ranges_j; sizes
 * below 1; a non-empty range that reaches outside the atoms; a coordinate that is not finite; more than 65535 tiles of
 * rows; chain offsets that do not ascend from 0 or hold no residue; a slot outside -1..m-1; two residues of one chain at
 * one slot of an axis; a chain index outside 0..n_chains-1; more than 2^31 - 1 tiles in all; a malformed PLM_DIST_PLAN.
 * PLM_ENOMEM before any allocation.                                                                                  */
int plm_residue_distances(const double *coords_i, int32_t n_atoms_i, const int32_t *ranges_i, int32_t n_res_i,
                          const double *coords_j, int32_t n_atoms_j, const int32_t *ranges_j, int32_t n_res_j,
                          double *dist_out, int device, void *stream);
int plm_distance_maps_aggregate(const double *coords, int32_t n_atoms, const int32_t *ranges, const int32_t *chain_offsets,
                                int32_t n_chains, const int32_t *slots_i, const int32_t *slots_j, int32_t m_i, int32_t m_j,
                                const int32_t *maps, int32_t n_maps, double *agg, int32_t *count, int device,
                                void *stream);

/* ---- alignment input (host code, no device): what plmc does when it reads the file run_plmc names (tools.py:202-262
 * passes only the path).  evcouplings_amd/alignment_io.py states the rules and keeps a pure-Python twin (fallback and
 * test oracle); these two single passes replace its per-line loop and fancy indexing (0.23 -> 0.03 s at the headline).
 *   plm_fasta_split     FASTA / A2M framing of a file image: lines stripped of ASCII whitespace at both ends, empty lines
 *                       skipped, '>' opens a record, a record's data lines are concatenated.  seq_out == NULL: only
 *                       *n_records and *seq_bytes are set (call once to size the buffers, once to fill them);
 *                       hdr_off / hdr_len delimit each id inside buf.  PLM_EINVAL: data before the first header.
 *   plm_encode_columns  out[r][k] = lut256[mat[r][cols[k]]] for a row-major byte matrix (n_rows x width), valid[r] = 1
 *                       iff no entry of the row is negative (a symbol outside the alphabet in a kept column).        */
int plm_fasta_split(const char *buf, int64_t n, int64_t *n_records, int64_t *seq_bytes, int64_t *hdr_off,
                    int32_t *hdr_len, int64_t *seq_len, char *seq_out);
int plm_encode_columns(const uint8_t *mat, int64_t n_rows, int64_t width, const int64_t *cols, int64_t n_cols,
                       const int8_t *lut256, int8_t *out, uint8_t *valid);
/* ... and output (host code): the raw EC file plmc writes and couplings/pairs.py:55-58 reads -- one line per site pair
 * i < j, "index_i A_i index_j A_j 0 cn" with cn as "%.6f"; cn = dense row-major [n_sites][n_sites] doubles.  One buffer, one
 * write instead of 44 850 Python format operations (L = 300); model_io.write_raw_ec_file keeps the Python twin. */
int plm_write_raw_ec_file(const char *path, int32_t n_sites, const int32_t *index_list, const char *target_seq,
                          const double *cn);

/* -- resident-context API (bench / multi-GPU host) ---------------------------------------- */
/* Uploads the alignment once; everything below runs on data resident in HBM. */
int plm_ctx_create(const plm_problem_t *problem, int device, void *stream, plm_ctx_t **out);
void plm_ctx_destroy(plm_ctx_t *ctx);
int plm_ctx_set_exchange(plm_ctx_t *ctx, plm_exchange_cb exchange, void *user);
int plm_ctx_set_collective(plm_ctx_t *ctx, plm_collective_cb collective, void *user);
int plm_ctx_attach_rccl(plm_ctx_t *ctx, const void *rccl_id);   /* ranks = problem.n_shards, rank = problem.shard */
/* change the stop rule / history of later plm_ctx_optimize calls (negative = keep) */
int plm_ctx_set_options(plm_ctx_t *ctx, int32_t max_iter, double epsilon, int32_t lbfgs_m);
/* number of floats of the solver's internal ("native", 16-site blocked) parameter vector */
int64_t plm_ctx_native_size(const plm_ctx_t *ctx);
int plm_ctx_reweight(plm_ctx_t *ctx);                       /* fills device weights, N_eff */
int plm_ctx_set_weights(plm_ctx_t *ctx, const float *weights_host);
int plm_ctx_get_weights(plm_ctx_t *ctx, float *weights_host, int32_t *counts_host, float *n_eff);
int plm_ctx_marginals(plm_ctx_t *ctx, float *fi_host, float *fij_host);
int plm_ctx_set_x(plm_ctx_t *ctx, const float *x_canonical_host);   /* NULL = start point */
int plm_ctx_get_x(plm_ctx_t *ctx, float *x_canonical_host);
int plm_ctx_get_g(plm_ctx_t *ctx, float *g_canonical_host);
/* one objective+gradient evaluation at the resident x; asynchronous unless fx_out != NULL */
int plm_ctx_eval(plm_ctx_t *ctx, double *fx_out, double *nll_out);
int plm_ctx_optimize(plm_ctx_t *ctx, plm_iter_cb cb, void *user, plm_result_t *result);
int plm_ctx_scores(plm_ctx_t *ctx, float *fn_host, float *cn_host);
/* average HIP-event duration (ms) of each kernel of the evaluation pipeline over `reps`
 * evaluations: out_ms[PLM_K_*]; used by bench.py for the roofline block. */
#define PLM_K_EXPAND 0
#define PLM_K_FORWARD 1
#define PLM_K_BACKWARD 2
#define PLM_K_ASSEMBLE 3
#define PLM_K_TOTAL 4
#define PLM_K_REWEIGHT 5
#define PLM_K_FIELDS 6      /* variable-projection fit: Newton passes on the fields + residual pass (0 otherwise) */
#define PLM_K_FORWARD_ACCURATE 7   /* the forward GEMM's accurate instantiation (f64 outer sums): last iterations, plm_eval */
#define PLM_K_LBFGS_VECTOR 8       /* the L-BFGS vector kernels of one iteration (m = 6) on this context's share of the state */
#define PLM_K_COUNT 9
int plm_ctx_time_kernels(plm_ctx_t *ctx, int32_t reps, float *out_ms /* [PLM_K_COUNT] */);
/* The two kinds of position of the field solver's chain, timed alone on this context's site blocks (after
 * plm_ctx_time_kernels, whose forward GEMM left the potentials): out_ms[0] = a Hessian position (pass with gradient,
 * diagonal and sampled Hessian sums + per-site Newton step), out_ms[1] = the closing position (pass that writes the
 * residual planes + gradient sums, norm check).  scripts/shard_compute.py prices a chain of p passes as
 * (p - 1) out_ms[0] + out_ms[1]. */
int plm_ctx_time_field_positions(plm_ctx_t *ctx, int32_t reps, float *out_ms /* [2] */);
/* Field-solver statistics of the last plm_ctx_optimize on this context (variable-projection fits; zeros otherwise),
 * measured with HIP events on the context's stream around the solver of every evaluation: bench.py reports the average
 * field-solver time per evaluation of its timed window from these. */
#define PLM_S_EVALS 0          /* evaluations whose field solver was timed */
#define PLM_S_FIELD_MS 1       /* total milliseconds between the forward GEMM and the backward GEMM of those evaluations */
#define PLM_S_PASSES 2         /* passes over the stored potentials made by the solver's chains (the last, residual-only pass not counted) */
#define PLM_S_CHAIN_SHORT 3    /* evaluations whose chain ran out of positions and had to be continued by the host */
#define PLM_S_GEMM_EVALS 4     /* evaluations (plain arithmetic, chain done at the first look) whose two GEMMs were timed */
#define PLM_S_FWD_MS 5         /* total milliseconds of their forward GEMMs (HIP events on the context's stream, inside the fit) */
#define PLM_S_BWD_MS 6         /* total milliseconds of their backward GEMMs */
#define PLM_S_COUNT 7
int plm_ctx_solver_stats(plm_ctx_t *ctx, double *out /* [PLM_S_COUNT] */);

/* -- field solver, test-facing (DIAGNOSTIC: tests/test_gpu_field_solver.py; no product path calls these) -------------
 * Both run on a single-shard context (PLM_EUNSUPPORTED otherwise) whose fit uses variable projection (PLM_EINVAL for a
 * joint-L-BFGS context or lambda_h = 0), with weights set, in the arithmetic the caller names (accurate = 0: plain, 1:
 * the accurate evaluation's) -- the environment switch is read once at context creation.  Sizes below: Q = the
 * instantiated alphabet (4 / 5 / 20 / 21 / 32), T = sequence tiles of 256, B = 16-site blocks, S = 16 B sites.
 *
 * plm_ctx_field_position: ONE unchained position of the solver at the context's current x.  Stage 1 (expand, forward
 * GEMM into the stored potentials, f64 fields <- x), one pass in the role asked for, then the per-site Newton step
 * without chain state (in place, on field buffer 0), with fresh inverses exactly when the pass carried Hessian sums
 * (PLM_FIELD_ROLE_HESSIAN); the other roles step with the inverses cached by an earlier Hessian position on this
 * context (PLM_EINVAL if update is asked for and none exists).  update = 0: norms only, no field moves.  prefill != 0:
 * the partial-sum buffers, the -log P partials and field buffer 1 are filled with 0xFF bytes (NaN) before the pass, so
 * the caller sees what a launch did not write.  The device buffers come back RAW -- no reduction on the host:
 *   gpart, dpart [B][T][16][Q] f64; hpart [B][T][16][Q (Q + 1) / 2] f32; hcnt [S][Q]; hinv [S][Q][Q]; g2_site [S];
 *   g2_sum [1]; h64 [2][S][Q] (both field buffers); nll_part [B][T] (-log P partials: written by the residual role).
 * Every pointer must be non-NULL and every n_* the element count above (PLM_EINVAL). */
#define PLM_FIELD_ROLE_STATS 0      /* statistics pass: gradient sums */
#define PLM_FIELD_ROLE_HESSIAN 1    /* Hessian position: + diagonal sums, + Hessian sums on every 32nd tile */
#define PLM_FIELD_ROLE_RESIDUAL 2   /* residual-writing pass: gradient sums, residual planes, -log P partials */
typedef struct {
    double *gpart, *dpart;
    float *hpart;
    double *hcnt, *hinv, *g2_site, *g2_sum, *h64, *nll_part;
    int64_t n_gpart, n_hpart, n_hcnt, n_hinv, n_g2_site, n_h64, n_nll_part;   /* n_gpart counts gpart and dpart each */
} plm_field_buffers_t;
int plm_ctx_field_position(plm_ctx_t *ctx, int32_t role, int32_t accurate, int32_t update, int32_t prefill,
                           plm_field_buffers_t *out);
/* plm_ctx_field_solve: the field solver's chain as a variable-projection evaluation of plm_ctx_optimize runs it at the
 * current x (enqueue, one synchronisation, verdict; repeated while the chain ran out of positions), with the squared
 * tolerance tol^2, the pass count of the "previous evaluation" vp_c_prev (0..11) and, invalidate != 0, no cached
 * inverses.  Afterwards plm_ctx_get_x / plm_ctx_get_g hold the evaluation's point (fields solved) and reduced gradient.
 * fields [S][Q]: the chain's current f64 fields (n_fields = S Q). */
#define PLM_FIELD_HIST 24
#define PLM_FIELD_MAXBLK 256
typedef struct {
    double gh2;                 /* squared field-gradient norm the evaluation reports */
    double fx, nll;             /* objective and its -log P part at the returned point */
    int32_t passes, done;       /* the verdict slots as the host read them last */
    int32_t continuations;      /* times the host continued a chain that ran out of positions */
    int32_t final_skip, want_rt, cur, state_passes;   /* the device-side chain state at the end */
    int32_t c_prev_next;        /* the pass count the next evaluation would be planned with */
    double hist[PLM_FIELD_HIST];              /* per pass: squared norm + 1e9 x open sites */
    unsigned char quiet[PLM_FIELD_MAXBLK];    /* 16-site blocks that stopped moving */
} plm_field_solve_t;
int plm_ctx_field_solve(plm_ctx_t *ctx, double tol, int32_t vp_c_prev, int32_t invalidate, int32_t accurate,
                        plm_field_solve_t *result, double *fields, int64_t n_fields);

/* -- L-BFGS vector kernels and H0 diagonal, test-facing (DIAGNOSTIC: tests/test_gpu_lbfgs_vectors.py; no product path
 * calls these) ---------------------------------------------------------------------------------------------------------
 * The plm_lbfgs_* entries run the launchers of the optimiser's vector kernels on HOST vectors, without an alignment or a
 * context: upload, one launch, raw results back.  Before the launch the dot scratch (sized as a context sizes it) and
 * every output buffer are filled with 0xFF bytes (NaN), so a partial sum or an output the kernels fail to write shows
 * in the result.  Vector lengths are multiples of 4.  Invalid arguments: PLM_EINVAL, nothing is launched and no output
 * is touched.
 *
 * plm_lbfgs_gram: the pass plm_ctx_optimize issues behind every trial point.  S, Y [nst][n]: ring slots 0 .. nst-1 of a
 * history of m slots (nst = min(m, stored + 1), at most 20); the new pair s = x - xp, y = g - gp goes to slot `end`
 * (end < nst; the slot's contents on entry are never read) and comes back in s_new, y_new [n].  The basis is the one
 * the optimiser builds (same helper): S[0..nst), Y[0..nst), g, g -- nb = 2 nst + 2 vectors; products of the queries
 * y_new and g with the Y's and the first g carry dinv [n] when it is given (NULL: plain products).
 *   md [3 nb + 1]: md[q nb + k] = <query q, basis k> with q = (s_new, y_new, g); md[3 nb] = s_new.s_new over the first
 *   nh entries;  ex [3] = g.dir, x.x, x.x over the first nh entries.  (nh: a multiple of 4 in 0..n.)
 *
 * plm_lbfgs_direction: dir = sum_j cs[j] s_j + dinv (.) (sum_j cy[j] y_j + cg g) over the `stored` live slots before
 * `end` of S, Y [m][n] (basis order of the optimiser, same helper: live S newest to oldest, live Y likewise, g;
 * coefficients rounded to f32); cs, cy [m] by physical slot as plm_lbfgs_coefficients returns them.  trial != NULL: the
 * fused launch that also writes trial = xacc + stp0 * dir (xacc required); trial == NULL: the plain launch.
 *
 * plm_lbfgs_multidot: out[q nb + k] = <V[q_index[q]], V[b_index[k]]> for nq (1..4) queries and nb (1..42) basis vectors
 * taken from V [nv][n]; bit q of wq and bit k of wb flag the products that carry dinv (both bits set, dinv given).
 * plm_lbfgs_dots: out[p] = <V[a_index[p]], V[b_index[p]]> over the first n entries (n a multiple of 4 in 0..stride) of
 * vectors V [nv][stride], 1..4 pairs.
 * plm_lbfgs_lincomb: out = ca a + cb b, or ca a when b is NULL.
 *
 * plm_ctx_precond_diagonal: the inverse Hessian diagonal of the independent-site model at the start point (the H0 of
 * PLM_FLAG_PRECOND), built by the code plm_ctx_optimize runs, in the canonical layout of plm_ctx_get_x.  Needs the
 * context's marginals; single-shard contexts only (PLM_EINVAL otherwise). */
int plm_lbfgs_gram(int64_t n, int64_t nh, int32_t m, int32_t end, int32_t nst, const float *S, const float *Y,
                   const float *x, const float *xp, const float *g, const float *gp, const float *dir, const float *dinv,
                   int device, float *s_new, float *y_new, double *md, double *ex);
int plm_lbfgs_direction(int64_t n, int32_t m, int32_t stored, int32_t end, const float *S, const float *Y, const float *g,
                        const double *cs, const double *cy, double cg, const float *dinv, const float *xacc, float stp0,
                        int device, float *dir, float *trial);
int plm_lbfgs_multidot(int64_t n, int32_t nv, const float *V, int32_t nq, const int32_t *q_index, int32_t nb,
                       const int32_t *b_index, const float *dinv, uint32_t wq, uint64_t wb, int device, double *out);
int plm_lbfgs_dots(int64_t stride, int32_t nv, const float *V, int32_t npairs, const int32_t *a_index,
                   const int32_t *b_index, int64_t n, int device, double *out);
int plm_lbfgs_lincomb(int64_t n, float ca, const float *a, float cb, const float *b, int device, float *out);
int plm_ctx_precond_diagonal(plm_ctx_t *ctx, float *canonical_out);

/* -- host arithmetic exposed for tests (no device) ------------------------------------------ */
/* Two-loop recursion of L-BFGS in coefficient space over a ring of m history slots, of which the `stored` slots
 * before `end` (ring order, newest = end - 1) are live: direction p = sum_j cs[j] s_j + D^-1 (sum_j cy[j] y_j + cg g).
 * All arrays are indexed by PHYSICAL slot: SY[i*m+j] = s_i.y_j, YDY[i*m+j] = y_i.D^-1 y_j, Sg[i] = s_i.g,
 * YDg[i] = y_i.D^-1 g, gDg = g.D^-1 g; *dg = g.p.  This is the code plm_ctx_optimize runs every iteration. */
void plm_lbfgs_coefficients(int m, int stored, int end, const double *SY, const double *YDY, const double *Sg,
                            const double *YDg, double gDg, double *cs, double *cy, double *cg, double *dg);

/* DIAGNOSTIC (tests/test_linesearch_host.py; no product path calls these, neither initialises a device).
 *
 * plm_linesearch_run: the More'-Thuente line search of plm_ctx_optimize -- same code, same constants (ftol 1e-4,
 * gtol 0.9, xtol 1e-7, steps in 1e-20 .. 1e20, at most PLM_LS_MAX_TRIALS trials, approximate-Wolfe allowance 1e-6 |f0|,
 * noise band 4e-9 |f0|) -- on a function of one variable: phi returns f(stp) and writes f'(stp) to *dphi.  It starts
 * from finit = f(0), dginit = f'(0) and the first trial step step0 > 0.
 *   *code: 1 accepted; -1 the step left the bracket or made no progress, -2 / -3 the largest / smallest step, -4 the
 *   bracket fell below xtol, -5 too many trials; -10 dginit is not negative (no trial is made).  *n_trials: trials
 *   made.  *stp: the accepted step -- 0 after a failure: the optimiser returns to the point it started from.
 *   trace [PLM_LS_MAX_TRIALS][3]: per trial (stp, f - f0, f'); f - f0 is +inf for a trial whose f or f' was not finite.
 *
 * plm_lbfgs_admit: what plm_ctx_optimize does with the curvature pair of an accepted step.  The history is a ring of
 * m (1..20) slots with *stored live pairs before slot *end and the Gram pieces SY, YDY [m][m], Sg, YDg [m], *gDg, *gg
 * laid out as for plm_lbfgs_coefficients.  md [3 nbv + 1] is the result of the Gram pass behind the accepted point as
 * plm_lbfgs_gram returns it (nst = min(m, stored + 1), nbv = 2 nst + 2, the new pair in slot *end).  First the pair's
 * rows are copied into the Gram pieces, then the pair is admitted or not (vp: the rule looks at the coupling part of s,
 * md[3 nbv] being the fields' share of s.s; straddle: the pair differences gradients of two arithmetics).  Everything
 * is updated in place.  *outcome: 0 stored, 1 dropped as a straddle, 2 skipped as noise, 3 history restarted;
 * *copy_anchor: 1 when the optimiser would now copy the pair's starting point into its anchor buffers. */
#define PLM_LS_MAX_TRIALS 20
typedef double (*plm_phi_cb)(double stp, double *dphi, void *user);
int plm_linesearch_run(plm_phi_cb phi, void *user, double finit, double dginit, double step0, int32_t *code,
                       int32_t *n_trials, double *stp, double *trace);
int plm_lbfgs_admit(int32_t m, int32_t *stored, int32_t *end, int32_t *anchored, double *SY, double *YDY, double *Sg,
                    double *YDg, double *gDg, double *gg, const double *md, int32_t nbv, int32_t nst, int32_t vp,
                    int32_t straddle, int32_t *outcome, int32_t *copy_anchor);

/* ---- mutation tables and combinatorial libraries (DESIGN_NEXT_ROWS.md section 9.16) ------------------------------
 * Energy differences relative to a target sequence t: the arithmetic of the reference's `_delta_hamiltonian`
 * (couplings/model.py:112-176) that `predict_mutation_table` (mutate/calculations.py:54-180) calls once per table row,
 * regrouped.  A variant changes sites i_1..i_M to letters a_1..a_M:
 *   S_h[i,a]  = h_i(a) - h_i(t_i)             S_J[i,a] = sum_{j != i} ( J_ij(a, t_j) - J_ij(t_i, t_j) )
 *   E_ij(a,b) = J_ij(a,b) - J_ij(a,t_j) - J_ij(t_i,b) + J_ij(t_i,t_j)
 *   dH_h = sum_m S_h[i_m,a_m]   dH_J = sum_m S_J[i_m,a_m] + sum_{m<n} E_{i_m i_n}(a_m,a_n)   dH = dH_J + dH_h
 * x_canonical: as plm_hamiltonians (float32); all arithmetic is float64, sums in a fixed order, no floating-point
 * atomics: the same input gives the same bits.  Substituting the target's own letter adds 0; M = 0 gives (0, 0, 0).
 *
 * plm_mutant_effects: n_variants variants in CSR form, variant v holding the entries offsets[v] .. offsets[v+1]-1 of
 * positions (0-based sites) and states; n_entries is the length of those two arrays.  out: n_variants x 3 doubles
 * (dH, dH_J, dH_h); status: one byte per variant.  A malformed variant gets NaN in all three and the first of these
 * codes that applies (the kernels check a variant before they load anything through its indices); the call still
 * returns PLM_OK.  A repeated position is refused, where the reference counts it twice.
 * tables_out, if not NULL: [n_sites][n_states][2] doubles (S_J, S_h), the single-mutant matrix in float64.
 * PLM_EINVAL (before the device is looked at): NULL argument, n_sites < 2, n_variants or n_entries < 0, a target
 * state outside 0..q-1, offsets[0] != 0, offsets decreasing, offsets[n_variants] != n_entries;
 * PLM_EUNSUPPORTED: q outside 2..32. */
#define PLM_MUT_OK 0
#define PLM_MUT_ETOOMANY 1    /* more entries than the model has sites */
#define PLM_MUT_EPOSITION 2   /* a position outside 0..n_sites-1 */
#define PLM_MUT_ESTATE 3      /* a state outside 0..n_states-1 */
#define PLM_MUT_EREPEAT 4     /* a position named twice */
int plm_mutant_effects(const float *x_canonical, int32_t n_sites, int32_t n_states, const int8_t *target,
                       int64_t n_variants, const int64_t *offsets, int64_t n_entries, const int32_t *positions,
                       const int8_t *states, int device, void *stream, double *out, uint8_t *status,
                       double *tables_out);

/* plm_mutant_scan: every combination of letters at n_scan_sites (1..8) distinct sites.  Site s takes the letters
 * letters[letter_offsets[s] .. letter_offsets[s+1]-1] (distinct states; letters == NULL: all n_states states at every
 * site, in state order).  The combination index is mixed-radix with the last site fastest (the order of Python's
 * itertools.product); the call covers the indices first .. first+count-1.  Outputs, each optional (NULL / 0):
 *   energies    count x 3 doubles (dH, dH_J, dH_h)
 *   histogram   n_edges+1 counts over the non-decreasing `edges` (at most 1024): a combination falls into the bin whose
 *               number is the count of edges <= dH, found by comparison only (numpy.searchsorted(edges, dH, "right"))
 *   dh_min, dh_max  exact extremes of dH over the range (+inf, -inf for count == 0); always written
 *   kept_index, kept_energies  with use_threshold: the indices with dH >= threshold, ascending, and their energies, at
 *               most `capacity` of them; n_kept is the number that qualified, and when it exceeds capacity the two
 *               buffers are unspecified (call again with room for n_kept)
 * The n_scan_sites single tables and the E tables of the site pairs are gathered once per call into compact tables
 * that the scan reads through the caches.
 * PLM_EINVAL: NULL argument, a site outside the model or named twice, an empty letter list, a letter outside 0..q-1 or
 * named twice at a site, first or count < 0 or a range beyond the last combination, edges decreasing or NaN, more than
 * 1024 edges, histogram without edges or edges without histogram, a NaN threshold, capacity < 0, capacity > 0 without
 * the two buffers; PLM_EUNSUPPORTED: q outside 2..32, more than 8 sites, 2^62 combinations or more. */
#define PLM_SCAN_MAX_SITES 8
#define PLM_SCAN_MAX_EDGES 1024
typedef struct {
    int32_t n_scan_sites;
    int32_t flags;                   /* 0 */
    const int32_t *sites;            /* [n_scan_sites] */
    const int32_t *letter_offsets;   /* [n_scan_sites + 1], read when letters != NULL */
    const int8_t *letters;
    int64_t first, count;
    const double *edges;
    int32_t n_edges;
    int32_t use_threshold;
    double threshold;
    int64_t capacity;
} plm_scan_opts;
typedef struct {
    double *energies;
    uint64_t *histogram;
    int64_t *kept_index;
    double *kept_energies;
    double dh_min, dh_max;
    int64_t n_kept;
    int64_t n_combinations;          /* of the whole library */
} plm_scan_result;
int plm_mutant_scan(const float *x_canonical, int32_t n_sites, int32_t n_states, const int8_t *target,
                    const plm_scan_opts *opts, int device, void *stream, plm_scan_result *result);

/* ---- The autoregressive Potts model (DESIGN_NEXT_ROWS.md section 9.19) -------------------------------------------------
 *     P(x) = prod_i P(x_i | x_<i),   P(x_i = b | x_<i) = softmax_b( h_i(b) + sum_{j<i} J_ji(x_j, b) )
 * (arDCA, Trinquier et al. 2021).  It is normalised by construction: log P(x) is exact, a sample is one pass over the
 * sites, and the fit is a convex problem with exact gradients.
 *
 * Parameters: float32 in the canonical layout of plm_hamiltonians, h [L][q], then the i<j blocks [q][q].  Block (j, i)
 * with j < i sits at the canonical pair index of (j, i); its entry [a][b] couples state a of the EARLIER site j with
 * state b of the LATER site i, and the block enters the conditional of site i only (h_0 alone is the first site's
 * conditional).  These are NOT the symmetric-gauge couplings of a Potts model and must not be read as one.  The sites
 * are taken in the order 0 .. L-1; another order is a permutation of the columns by the caller.
 * q in 2..32 (PLM_EUNSUPPORTED otherwise), L >= 1.  In all four calls the arguments are checked before the device is
 * looked at (PLM_EINVAL: NULL arguments, sizes below 1, n x L at or above 2^31, states outside 0..q-1 and what each call
 * names below), and PLM_ENOMEM is decided before any allocation.
 *
 * plm_ar_logprob: logp_out [n] = log P of each sequence, site_logp_out [n][L] (or NULL) its site terms.  logit_b is
 *   accumulated in float64 from (double) h_i(b) over j = 0 .. i-1 in that order; the log-softmax is taken in float64 (the
 *   maximum, then the sum of exp in state order); log P is the sum of the site terms in site order.  The result depends
 *   on (sequence, model) only, not on n or the place of the sequence in the call.
 *
 * plm_ar_sample: states_out [n_samples][L], one ancestral pass per chain.  Site i of chain c: U_b starts as h_i(b) in
 *   float32 and takes one float32 add per j = 0 .. i-1, in that order, of J_ji(x_cj, b); the new state is the draw of
 *   plm_sample's contract (e_b = exp(beta U_b - max) over the allowed states in state order, the first allowed state
 *   whose running sum exceeds u S_last) with the Philox4x32-10 counter (first_chain + c, 0, 0, i) and the key
 *   (seed low, seed high).  Chain c of any call is the same chain whatever n_samples and however a run is cut into calls
 *   by first_chain.  beta must be finite and > 0; allowed is NULL or q flags, one set at least.  There are no fixed
 *   sites: an autoregressive pass conditions a site on the EARLIER sites only, so fixing a later site would not give
 *   samples of the conditional distribution (that needs the posterior over the earlier sites, which this model does not
 *   factorise).
 *
 * plm_ar_eval: F(x) = -(1/N_eff) sum_s w_s log P(x_s) + lambda_h sum h^2 + lambda_j sum J^2, N_eff = sum_s w_s summed in
 *   float64 in sequence order; nll_out (or NULL) is the first term; g_out (or NULL) the gradient, canonical, double:
 *     dF/dh_i(b)     = -(1/N_eff) sum_s w_s (delta(x_si, b) - p_sib) + 2 lambda_h h_i(b)
 *     dF/dJ_ji(a, b) = -(1/N_eff) sum_s w_s delta(x_sj, a) (delta(x_si, b) - p_sib) + 2 lambda_j J_ji(a, b)
 *   Logits, probabilities, residuals and every sum over sequences are float64, in an order the shape alone fixes, without
 *   floating-point atomics: two calls return the same bytes.  The division by N_eff follows the sum.  PLM_EINVAL for a
 *   weight that is negative or not finite, for weights that sum to zero and for a negative lambda.
 *
 * plm_ar_fit: minimises F over float32 parameters by L-BFGS (More'-Thuente line search, lbfgs_m pairs) from x_start
 *   (NULL: zeros); lambda_h and lambda_j are in per-sequence units, as F is normalised by N_eff.  The gradient is rounded
 *   to float32 once, where it enters the pair history; f, the directional derivatives of the line search and the norms of
 *   the stop rule come from the float64 evaluation.  Status: PLM_STATUS_CONVERGED when |g|_2 <= epsilon max(1, |x|_2) at
 *   the float32 point that is returned, PLM_STATUS_MAXITER after max_iter iterations (0: no limit),
 *   PLM_STATUS_LINESEARCH (ls_reason: the line search's code, 10 for a direction that does not descend),
 *   PLM_STATUS_INTERRUPTED when the callback returned non-zero (x_out is the point of that iteration).  The callback's
 *   arguments are those of plm_fit's.  PLM_EINVAL also for max_iter < 0, an epsilon that is not finite and > 0, lbfgs_m
 *   outside 1..20. */
typedef struct {
    int32_t  n_samples;        /* >= 1 */
    uint32_t first_chain;      /* the chain index of the call's first sample */
    uint64_t seed;
    float    beta;             /* > 0 */
    const uint8_t *allowed;    /* [q] flags or NULL */
} plm_ar_sample_opts;
typedef struct {
    double  lambda_h, lambda_j;
    int32_t max_iter;          /* 0: no limit */
    double  epsilon;
    int32_t lbfgs_m;           /* 1..20 */
} plm_ar_fit_opts;
typedef struct {
    int32_t status;            /* PLM_STATUS_* */
    int32_t iterations;
    int32_t evaluations;
    int32_t ls_reason;         /* with PLM_STATUS_LINESEARCH, else 0 */
    double  fx, nll;           /* F and its first term at x_out */
    double  gnorm, xnorm;      /* |g|_2 and |x|_2 at x_out */
} plm_ar_fit_result;
int plm_ar_logprob(const int8_t *seqs, int32_t n_seqs, int32_t n_sites, int32_t n_states, const float *x_canonical,
                   int device, void *stream, double *logp_out, double *site_logp_out);
int plm_ar_sample(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_ar_sample_opts *opts, int device,
                  void *stream, int8_t *states_out);
int plm_ar_eval(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                double lambda_h, double lambda_j, const float *x_canonical, int device, void *stream, double *fx_out,
                double *nll_out, double *g_out);
int plm_ar_fit(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
               const plm_ar_fit_opts *opts, const float *x_start, plm_iter_cb cb, void *user, int device, void *stream,
               float *x_out, plm_ar_fit_result *result);

/* ---- A restricted Boltzmann machine on an alignment (DESIGN_NEXT_ROWS.md section 9.22) --------------------------------
 * Potts visible units v_i in 0..q-1 at the sites i = 0 .. L-1 and M Bernoulli hidden units h_mu in {0, 1} (Tubiana, Cocco,
 * Monasson 2019):
 *     I_mu(v)   = c_mu + sum_i W_mu,i(v_i)
 *     P(v, h)   ~ exp( sum_i g_i(v_i) + sum_mu h_mu I_mu(v) )
 *     score(v)  = sum_i g_i(v_i) + sum_mu softplus(I_mu(v))            = log P(v) + log Z
 *     P(h_mu = 1 | v) = sigma(I_mu(v)),    P(v_i = a | h) = softmax_a( g_i(a) + sum_mu h_mu W_mu,i(a) )
 * Parameters ("the RBM layout"): one float32 vector, g [L][q], then c [M], then W [M][L][q]: L q + M + M L q values.
 * q in 2..32 (PLM_EUNSUPPORTED otherwise), L >= 1, M >= 1, M L q below 2^31 (and M at most 64 x 65535, else
 * PLM_EUNSUPPORTED).  In all three calls the arguments are checked before the device is looked at (PLM_EINVAL: NULL
 * arguments, sizes below 1, rows x L at or above 2^31, states outside 0..q-1 and what each call names below), and
 * PLM_ENOMEM is decided before any allocation.  log Z is not computed here (plm_rbm_ais, below, estimates it).
 *
 * plm_rbm_score: score_out [n] and inputs_out [n][M] (or NULL), float64.  I_mu is accumulated in float64 from (double) c_mu,
 *   then one add per site i = 0 .. L-1 in that order of (double) W_mu,i(v_i); softplus(I) = max(I, 0) + log1p(exp(-|I|));
 *   the score is one running sum: the fields in site order, then the softplus terms in mu order.  The result depends on
 *   (sequence, model) only, not on n or the place of the row in the call.
 *
 * plm_rbm_sample: block Gibbs sampling with C independent chains; states_out [K][C][L], hidden_out [K][C][M] (or NULL).
 *   Step t of chain c (the steps count from first_step across burn-in, thinning and snapshots, as plm_sample counts its
 *   sweeps: snapshot 0 after burn_in steps, every further one thin steps later):
 *   (a) hidden draw: for every mu, I_mu in float32 is c_mu, then one float32 add per site i = 0 .. L-1 in that order of
 *       W_mu,i(v_i); p = 1 / (1 + expf(-I)); h_mu = 1 iff u < p, u = ((word0 >> 8) + 0.5) 2^-24 (kept below 1) of
 *       Philox4x32-10 with the counter (first_chain + c, 2, t, mu);
 *   (b) visible draw: for every site that is not fixed, U_a = g_i(a), then one float32 add of W_mu,i(a) for every mu with
 *       h_mu = 1, in mu order; the new state is the draw of plm_sample's contract over the allowed states at beta = 1
 *       with the counter (first_chain + c, 0, t, i).
 *   The key is (seed low, seed high).  start == NULL: chain c begins from one such draw per site of softmax g_i with the
 *   counter (first_chain + c, 0, 0xFFFFFFFF, i).  hidden_out holds the h drawn in the step that produced each snapshot
 *   (zeros for a snapshot no step produced: burn_in = 0).  Chain c is the same chain whatever n_chains, the launch plan
 *   (PLM_RBM_WAVES=1|2|4|8 forces the waves that share a tile of 64 chains: measurements and tests only), or how a run is cut into
 *   calls by first_chain, or by first_step with the last states as start.  PLM_EINVAL also: no allowed state, start
 *   states that are not allowed at a site that is not fixed, first_chain + n_chains above 2^32, a step index at or above
 *   2^32 - 1.  PLM_EUNSUPPORTED: the states and hidden units of 64 chains do not fit the LDS of a CU (L / 4 + M / 32
 *   words per chain: L + M / 8 up to about 2 500).
 *
 * plm_rbm_fit: persistent contrastive divergence by plain gradient ascent from x_start (required).  Chains begin at
 *   opts->start, or from the start rule at the parameters of the call's first epoch.  Local epoch e = 0 .. n_epochs - 1,
 *   global epoch g = first_epoch + e:
 *   1. data statistics at the current parameters, float64: p_s,mu = sigma(I_mu(x_s)) with I as in plm_rbm_score;
 *      D_g[i][a] = sum_s w_s delta(x_si, a) / N_eff (computed once), D_c[mu] = sum_s w_s p_s,mu / N_eff,
 *      D_W[mu][i][a] = sum_s (w_s p_s,mu) delta(x_si, a) / N_eff; N_eff = sum_s w_s in sequence order; the division
 *      follows the sum
 *   2. every chain makes steps_per_epoch = k steps of plm_rbm_sample's contract (first_chain = 0, all states allowed, no
 *      fixed sites) with the step indices g k .. g k + k - 1
 *   3. model statistics from the chains' visible states after those steps, Rao-Blackwellised over the hidden units:
 *      p_c,mu = sigma(I_mu(v_c)) in float64; N_g exact counts over C; N_c, N_W as in step 1 with weight 1 and divisor C
 *   4. trace row e = (max |D_g - N_g|, max |D_c - N_c|, max |D_W - N_W|, lr_g, sum_s w_s score(x_s) / N_eff) with
 *      lr_g = lr when lr_decay_after == 0 or g + 1 <= lr_decay_after, else lr lr_decay_after / (g + 1), in float64
 *   5. the callback is called with the global epoch and the row; a non-zero return stops before the update
 *      (PLM_STATUS_INTERRUPTED, epochs_done = e)
 *   6. theta <- (float)( (double) theta + lr_g ((D - N) - (2 lambda) theta) ), lambda = lambda_g on g, 0 on c, lambda_w on
 *      W: every operation in float64, the sum rounded to float32 once
 *   After n_epochs updates the status is PLM_STATUS_MAXITER.  Every sum over sequences or chains is made in an order the
 *   shape alone fixes, without floating-point atomics: two calls return the same bytes, and E epochs equal E1 + E2 epochs
 *   resumed from x_out, chains_out and first_epoch = E1.  Every output pointer may be NULL; data_out and model_out are
 *   the statistics D and N of the last epoch that ran, in the RBM layout.  PLM_EINVAL also: a weight that is negative or
 *   not finite, weights that sum to zero, lr, lambda_g or lambda_w negative or not finite, (first_epoch + n_epochs)
 *   steps_per_epoch at or above 2^32 - 1. */
typedef struct {
    int32_t  n_chains;      /* C >= 1, independent chains                                            */
    int32_t  burn_in;       /* steps before the first snapshot, >= 0                                 */
    int32_t  n_snapshots;   /* K >= 1 snapshots of all chains                                        */
    int32_t  thin;          /* steps between snapshots, >= 1 (unused when K == 1)                    */
    uint32_t first_step;    /* the index of the call's first step                                    */
    uint32_t first_chain;   /* the chain index of the call's first chain                             */
    uint64_t seed;
    const int8_t  *start;   /* NULL, or C x L states                                                 */
    const uint8_t *fixed;   /* NULL, or L flags: sites that are never resampled                      */
    const uint8_t *allowed; /* NULL, or q flags: states that may be drawn (at least one set)         */
} plm_rbm_sample_opts;
typedef struct {
    int32_t  n_chains;          /* C >= 1 persistent chains                                          */
    int32_t  n_epochs;          /* E >= 1 epochs of this call                                        */
    int32_t  steps_per_epoch;   /* k >= 1                                                            */
    int32_t  first_epoch;       /* e0 >= 0: global number of this call's first epoch (continuation)  */
    int32_t  lr_decay_after;    /* T >= 0: the step decays as T / (g + 1) after global epoch T - 1   */
    double   lr;                /* step, >= 0                                                        */
    double   lambda_g;          /* >= 0, on the fields                                               */
    double   lambda_w;          /* >= 0, on the weights                                              */
    uint64_t seed;
    const int8_t *start;        /* NULL, or C x L states                                             */
} plm_rbm_fit_opts;
typedef struct {
    float  *x_out;       /* parameters after the last applied update, RBM layout                     */
    double *data_out;    /* D of the last epoch that ran, RBM layout                                 */
    double *model_out;   /* N of the last epoch that ran, RBM layout                                 */
    int8_t *chains_out;  /* C x L states of the last epoch that ran                                  */
    double *trace;       /* n_epochs x 5, one row per epoch that ran                                 */
    double *phase_ms;    /* NULL, or 4 doubles: milliseconds of (data statistics, chain steps, model  */
                         /* statistics and trace row, update) summed over the epochs whose update    */
                         /* was applied, by device events; a timed fit waits for every epoch         */
    int32_t epochs_done; /* updates applied                                                          */
    int32_t status;      /* PLM_STATUS_MAXITER or PLM_STATUS_INTERRUPTED                             */
} plm_rbm_fit_result;
/* Called once per epoch after its trace row is known and before its update, with the global epoch number. */
typedef int (*plm_rbm_epoch_cb)(int32_t epoch, double max_dg, double max_dc, double max_dw, double lr, double data_score,
                                void *user);
int plm_rbm_score(const int8_t *seqs, int32_t n_seqs, int32_t n_sites, int32_t n_states, int32_t n_hidden,
                  const float *params, int device, void *stream, double *score_out, double *inputs_out);
int plm_rbm_sample(int32_t n_sites, int32_t n_states, int32_t n_hidden, const float *params, const plm_rbm_sample_opts *opts,
                   int device, void *stream, int8_t *states_out, int8_t *hidden_out);
int plm_rbm_fit(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states, int32_t n_hidden,
                const float *x_start, const plm_rbm_fit_opts *opts, int device, void *stream, plm_rbm_epoch_cb cb, void *user,
                plm_rbm_fit_result *result);

/* ---- log Z of the restricted Boltzmann machine by annealed importance sampling (DESIGN_NEXT_ROWS.md section 9.25) ------
 * The model is the RBM above (g [L][q], c [M], W [M][L][q] in the RBM layout, q in 2..32).  The path puts the inverse
 * temperature on the hidden layer only, as plm_ais puts it on the couplings only:
 *     p*_beta(v) = exp( sum_i g_i(v_i) ) prod_mu (1 + exp(beta I_mu(v))),    I_mu(v) = c_mu + sum_i W_mu,i(v_i)
 * beta = 0 is the independent-site model of g, sampled exactly, with log_z0 = M log 2 + sum_i log sum_a exp g_i(a) in
 * float64 on the host.  The schedule is that of plm_ais: K + 1 float32 values beta_0 = 0 <= ... <= beta_K, all finite;
 * betas == NULL: beta_k = (float)((double)k / K).  beta_K need not be 1: the result is log Z of the model with c and W
 * scaled by beta_K, so every prefix of a schedule is a schedule.  plm_ais_opts and plm_ais_cb mean here what they mean
 * for plm_ais.
 * Start: chain c begins from plm_rbm_sample's start rule on g (all states allowed, counter (c, 0, 0xFFFFFFFF, i)) with
 * log w = 0.  Step k = 1 .. K on the current states v:
 *   1. inputs: I_mu = (double)c_mu, then one float64 add per site i = 0 .. L-1 of (double)W_mu,i(v_i): the bits
 *      plm_rbm_score returns in inputs_out
 *   2. weight, on the first sweep of the step only: x_k = (double)beta_k I_mu and x_{k-1} = (double)beta_{k-1} I_mu, one
 *      product each; sp(x) = fmax(x, 0) + log1p(exp(-fabs(x))); term_mu = sp(x_k) - sp(x_{k-1}).  The terms are summed
 *      from 0.0 in mu order inside each chunk of 8 hidden units (mu = 8 j .. 8 j + 7), the chunk sums are added from 0.0
 *      in chunk order, and that sum is added to log w.  No product is fused with a sum.
 *   3. n = sweeps_per_temp sweeps with the sweep indices (k-1) n .. k n - 1; every sweep after the first recomputes I from
 *      the current states.
 *      hidden half: p_mu = sigma(x_k) in float64 (1 / (1 + exp(-x)) for x >= 0, else e / (1 + e) with e = exp(x));
 *        h_mu = ((double)u < p_mu), u the float32 uniform ((word0 >> 8) + 0.5) 2^-24 (kept below 1) of the counter
 *        (c, 2, sweep, mu)
 *      visible half, every site: S_a starts at 0.0f and adds W_mu,i(a) in float32 for every set h_mu in mu order;
 *        arg_a = fadd(g_i(a), fmul(beta_k, S_a)), two roundings; the draw of plm_sample's contract on arg at beta = 1
 *        with the counter (c, 0, sweep, i)
 * log_z, log_z_se and ess are formed from log w as plm_ais forms them.  log w, the states and the hidden units of chain c
 * depend on (seed, c, model, schedule, n) only: not on C, on the waves that share a tile (PLM_RBM_WAVES) or on how the
 * steps are cut into launches (steps_per_launch; 0: about a second each).  cb, if given, is called between launches and
 * cancels by returning non-zero: PLM_STATUS_INTERRUPTED, the three summaries NaN, the arrays of the steps_done steps that
 * ran.  Before the device is looked at: PLM_EINVAL for NULL opts, result or params, the shape checks of plm_rbm_score,
 * C, K or n below 1, steps_per_launch below 0, K n >= 2^32 - 1, C L or C M at or above 2^31 and the schedule checks of
 * plm_ais; PLM_EUNSUPPORTED for q outside 2..32 and when the tile of 64 chains (L / 4 + M / 32 words and M / 8 doubles
 * per chain) does not fit the LDS of a CU.  PLM_ENOMEM is decided before any array but the schedule is read. */
typedef struct {
    double log_z, log_z0, log_z_se, ess;
    double *log_w;             /* [C] or NULL                                                          */
    int8_t *states;            /* C x L final states, or NULL                                          */
    int8_t *hidden;            /* C x M hidden units of the last sweep, or NULL                        */
    int32_t steps_done;
    int32_t status;            /* PLM_STATUS_CONVERGED when all K steps ran, else PLM_STATUS_INTERRUPTED */
} plm_rbm_ais_result;
int plm_rbm_ais(int32_t n_sites, int32_t n_states, int32_t n_hidden, const float *params, const plm_ais_opts *opts,
                int device, void *stream, plm_ais_cb cb, void *user, plm_rbm_ais_result *result);

/* ---- inter-protein coupling energies of two sequence sets, and matching by them (DESIGN_NEXT_ROWS.md section 9.23) ----
 * For a row s of A (n_sites_a states) and a row t of B (n_sites_b states) of the same group
 *     E(s,t) = sum_{i in A} sum_{j in B} J_ij(a_si, b_tj)
 * jab: the inter block of a model alone, [n_sites_a][n_sites_b][q][q] float32, jab[i][j][a][b] = J_ij(a,b), assumed
 * finite (the energy of the inter block alone depends on the gauge: plm.inter_blocks of the Python side extracts it in
 * the zero-sum gauge).  seqs_a [n_a][n_sites_a], seqs_b [n_b][n_sites_b]: states 0..q-1, row-major.
 * Groups: a_offsets and b_offsets [n_groups + 1], non-decreasing from 0 to n_a / n_b; group g pairs the rows
 * a_offsets[g] .. a_offsets[g+1]-1 of A with the rows b_offsets[g] .. b_offsets[g+1]-1 of B; either side may be empty; one
 * group is the all-against-all table.  n_groups = 0 (with n_a = n_b = 0) is PLM_OK and writes nothing.
 * Arithmetic (fixed, so that a twin can follow it to the bit):
 *     V[t][i][a] = sum_j (double) jab[i][j][a][b_tj]     j ascending, float64, from +0.0
 *     E[s][t]    = sum_i V[t][i][a_si]                   i ascending, float64, from +0.0
 * A term whose state equals skip_state is left out (a b_tj in the first sum, an a_si in the second).  Only additions
 * of float32 values widened to double, no floating-point atomics: the result does not depend on tile sizes, on how groups
 * share workgroups, on the chunks of V, or on the device.  PLM_CROSS_TILE (rows of A per workgroup) and PLM_CROSS_VCHUNK
 * (64-row tiles of B per V buffer), positive integers, force the plan: measurements and tests only.
 * Outputs, each optional (but one at least):
 *   matrix_out  the groups' row-major n_a(g) x n_b(g) blocks, concatenated in group order
 *   rows_best   [n_a]: index = the row of B in the row's group with the largest E (a global row index, ties to the smallest
 *               index), best = that E, second = the largest E over the other partners (-inf with one partner; index -1 and
 *               both -inf with none);  cols_best [n_b]: the same for every row of B over the rows of A.
 *               Both are filled only when opts->want_best is not 0.
 * PLM_EINVAL (with a message, before the device is looked at): NULL jab, seqs, offsets or opts; nothing to write; a side
 * with fewer than 1 site; negative counts; offsets that do not start at 0, decrease or end elsewhere than n_a / n_b; a
 * state outside 0..q-1; skip_state outside -1..q-1; a PLM_CROSS_TILE or PLM_CROSS_VCHUNK that is no positive integer.
 * PLM_EUNSUPPORTED: q outside 2..32.  PLM_ENOMEM before any allocation, from jab, the sequences, V and the outputs.
 *
 * plm_group_assignment (host code, no device): per group the exact rectangular linear assignment on `scores` (laid out
 * as matrix_out): min(n_a(g), n_b(g)) pairs with the largest (maximize != 0) or smallest total score, by shortest
 * augmenting paths, O(n^2 m).  partner_of_a [n_a]: the global row of B, or -1; totals [n_groups] or NULL: the sum of the
 * chosen scores, over the rows of A in order.  PLM_EINVAL: NULL arguments, malformed offsets, a score that is not finite. */
typedef struct {
    int32_t skip_state;     /* -1: none; else a term whose a- or b-state equals it is omitted */
    int32_t want_best;      /* fill the best-partner arrays */
} plm_cross_opts;
typedef struct {
    int64_t index;
    double best;
    double second;
} plm_cross_best;
int plm_cross_energies(const float *jab, int32_t n_sites_a, int32_t n_sites_b, int32_t n_states, const int8_t *seqs_a,
                       int64_t n_a, const int8_t *seqs_b, int64_t n_b, int64_t n_groups, const int64_t *a_offsets,
                       const int64_t *b_offsets, const plm_cross_opts *opts, int device, void *stream, double *matrix_out,
                       plm_cross_best *rows_best, plm_cross_best *cols_best);
int plm_group_assignment(const double *scores, int64_t n_groups, const int64_t *a_offsets, const int64_t *b_offsets,
                         int32_t maximize, int64_t *partner_of_a, double *totals);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PLM_HIP_H */
