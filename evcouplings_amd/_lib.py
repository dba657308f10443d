"""
ctypes binding of libplm_hip.so (include/plm_hip.h).

There is deliberately no CPU fallback: if the shared library is missing, or no gfx950
device is visible, every call raises.  The library is built in-tree by
``__graft_entry__.build()`` / ``make -C evcouplings_amd/csrc`` so it travels with the repo.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PLM_HIP_LIB selects another build of the same library (kernel A/B experiments only)
LIB_PATH = os.environ.get("PLM_HIP_LIB") or os.path.join(_HERE, "libplm_hip.so")

PLM_OK = 0
STATUS_CONVERGED, STATUS_MAXITER, STATUS_LINESEARCH, STATUS_INTERRUPTED = 0, 1, 2, 3
ABI_VERSION = 2
K_EXPAND, K_FORWARD, K_BACKWARD, K_ASSEMBLE, K_TOTAL, K_REWEIGHT, K_FIELDS, K_FORWARD_ACCURATE, K_LBFGS_VECTOR, K_COUNT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
S_COUNT = 7

ITER_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                      C.c_double, C.c_double, C.c_void_p)
EXCHANGE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p)
COLLECTIVE_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                            C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_void_p)
COLL_ALLTOALL, COLL_ALLREDUCE_F64, COLL_ALLREDUCE_F32, COLL_BROADCAST = 1, 2, 3, 4


class PlmProblem(C.Structure):
    _fields_ = [
        ("n_seqs", C.c_int32), ("n_sites", C.c_int32), ("n_states", C.c_int32),
        ("msa", C.c_void_p),
        ("theta_id", C.c_double), ("scale", C.c_double),
        ("lambda_h", C.c_double), ("lambda_j", C.c_double),
        ("max_iter", C.c_int32), ("epsilon", C.c_double), ("lbfgs_m", C.c_int32),
        ("n_shards", C.c_int32), ("shard", C.c_int32), ("flags", C.c_int32),
        ("lambda_group", C.c_double),
    ]


class PlmResult(C.Structure):
    _fields_ = [
        ("weights", C.c_void_p), ("fi", C.c_void_p), ("fij", C.c_void_p), ("hi", C.c_void_p),
        ("jij", C.c_void_p), ("fn", C.c_void_p), ("cn", C.c_void_p),
        ("n_eff", C.c_float), ("iters_done", C.c_int32), ("n_evals", C.c_int32),
        ("status", C.c_int32), ("fx", C.c_double),
        ("seconds_reweight", C.c_double), ("seconds_marginals", C.c_double),
        ("seconds_optimize", C.c_double), ("seconds_total", C.c_double),
        ("status_msg", C.c_char * 128),
    ]


class PlmMfResult(C.Structure):
    _fields_ = [
        ("weights", C.c_void_p), ("n_eff", C.c_float), ("fi", C.c_void_p), ("fij", C.c_void_p),
        ("hi", C.c_void_p), ("jij_full", C.c_void_p), ("jij", C.c_void_p), ("di", C.c_void_p),
    ]


class PlmSampleOpts(C.Structure):
    _fields_ = [
        ("n_chains", C.c_int32), ("burn_in", C.c_int32), ("n_snapshots", C.c_int32), ("thin", C.c_int32),
        ("beta", C.c_float), ("seed", C.c_uint64),
        ("start", C.c_void_p), ("fixed", C.c_void_p), ("allowed", C.c_void_p),
    ]


class PlmSamplePlanInfo(C.Structure):
    _fields_ = [
        ("direct", C.c_int32), ("tile", C.c_int32), ("jc", C.c_int32), ("nv", C.c_int32), ("n_workgroups", C.c_int32),
        ("lds_bytes", C.c_int64),
    ]


class PlmBmOpts(C.Structure):
    _fields_ = [
        ("n_chains", C.c_int32), ("n_epochs", C.c_int32), ("sweeps_per_epoch", C.c_int32), ("first_epoch", C.c_int32),
        ("lr", C.c_float), ("lr_decay_after", C.c_int32), ("lambda_h", C.c_float), ("lambda_j", C.c_float),
        ("tol", C.c_float), ("seed", C.c_uint64), ("start", C.c_void_p),
    ]


class PlmBmResult(C.Structure):
    _fields_ = [
        ("x_out", C.c_void_p), ("pi_out", C.c_void_p), ("pij_out", C.c_void_p), ("chains_out", C.c_void_p),
        ("trace", C.c_void_p), ("epochs_done", C.c_int32), ("status", C.c_int32),
    ]


BM_EPOCH_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p)


class PlmAisOpts(C.Structure):
    _fields_ = [
        ("n_chains", C.c_int32), ("n_temps", C.c_int32), ("sweeps_per_temp", C.c_int32), ("steps_per_launch", C.c_int32),
        ("betas", C.c_void_p), ("seed", C.c_uint64),
    ]


class PlmAisResult(C.Structure):
    _fields_ = [
        ("log_z", C.c_double), ("log_z0", C.c_double), ("log_z_se", C.c_double), ("ess", C.c_double),
        ("log_w", C.c_void_p), ("e_j", C.c_void_p), ("states", C.c_void_p),
        ("steps_done", C.c_int32), ("status", C.c_int32),
    ]


AIS_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_int32, C.c_void_p)



class PlmPtOpts(C.Structure):
    _fields_ = [
        ("n_ladders", C.c_int32), ("n_rungs", C.c_int32), ("burn_in", C.c_int32), ("n_snapshots", C.c_int32),
        ("thin", C.c_int32), ("sweeps_per_round", C.c_int32), ("first_round", C.c_int32), ("all_rungs", C.c_int32),
        ("betas", C.c_void_p), ("seed", C.c_uint64),
        ("start", C.c_void_p), ("start_rungs", C.c_void_p), ("start_e", C.c_void_p),
    ]


class PlmPtResult(C.Structure):
    _fields_ = [
        ("samples", C.c_void_p), ("e_j", C.c_void_p), ("accepts", C.c_void_p), ("attempts", C.c_void_p),
        ("walkers", C.c_void_p), ("rungs", C.c_void_p), ("walker_e", C.c_void_p),
        ("rounds_done", C.c_int32), ("status", C.c_int32),
    ]


PT_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_int32, C.c_void_p)


class PlmAnnealOpts(C.Structure):
    _fields_ = [
        ("n_chains", C.c_int32), ("n_steps", C.c_int32), ("sweeps_per_step", C.c_int32), ("max_greedy", C.c_int32),
        ("first_sweep", C.c_uint32), ("steps_per_launch", C.c_int32),
        ("betas", C.c_void_p), ("seed", C.c_uint64),
        ("start", C.c_void_p), ("fixed", C.c_void_p), ("allowed", C.c_void_p),
    ]


class PlmAnnealResult(C.Structure):
    _fields_ = [
        ("states", C.c_void_p), ("gain", C.c_void_p), ("best", C.c_void_p), ("best_gain", C.c_void_p),
        ("best_at", C.c_void_p), ("last_move", C.c_void_p), ("converged", C.c_void_p),
        ("energies", C.c_void_p), ("best_energies", C.c_void_p),
        ("steps_done", C.c_int32), ("status", C.c_int32),
    ]


ANNEAL_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_int32, C.c_void_p)
PHI_CB = C.CFUNCTYPE(C.c_double, C.c_double, C.POINTER(C.c_double), C.c_void_p)
LS_MAX_TRIALS = 20

IDENT_DENOM = {"columns": 0, "both": 1, "shorter": 2}


class PlmIdentOpts(C.Structure):
    _fields_ = [("gap_state", C.c_int32), ("denominator", C.c_int32), ("exclude_self", C.c_int32),
                ("threshold", C.c_double)]


TRIPLET_COUNTS, TRIPLET_FREQ, TRIPLET_CONNECTED = 1, 2, 4


class PlmTripletOpts(C.Structure):
    _fields_ = [("skip_state", C.c_int32), ("want", C.c_int32)]


class PlmPcaOpts(C.Structure):
    _fields_ = [("n_components", C.c_int32), ("oversample", C.c_int32), ("max_iter", C.c_int32),
                ("skip_state", C.c_int32), ("tol", C.c_double), ("seed", C.c_uint64)]


PCA_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_double, C.c_void_p)

FIELD_ROLE_STATS, FIELD_ROLE_HESSIAN, FIELD_ROLE_RESIDUAL = 0, 1, 2
FIELD_HIST, FIELD_MAXBLK = 24, 256


class PlmFieldBuffers(C.Structure):
    _fields_ = [
        ("gpart", C.c_void_p), ("dpart", C.c_void_p), ("hpart", C.c_void_p), ("hcnt", C.c_void_p), ("hinv", C.c_void_p),
        ("g2_site", C.c_void_p), ("g2_sum", C.c_void_p), ("h64", C.c_void_p), ("nll_part", C.c_void_p),
        ("n_gpart", C.c_int64), ("n_hpart", C.c_int64), ("n_hcnt", C.c_int64), ("n_hinv", C.c_int64),
        ("n_g2_site", C.c_int64), ("n_h64", C.c_int64), ("n_nll_part", C.c_int64),
    ]


class PlmFieldSolve(C.Structure):
    _fields_ = [
        ("gh2", C.c_double), ("fx", C.c_double), ("nll", C.c_double),
        ("passes", C.c_int32), ("done", C.c_int32), ("continuations", C.c_int32),
        ("final_skip", C.c_int32), ("want_rt", C.c_int32), ("cur", C.c_int32), ("state_passes", C.c_int32),
        ("c_prev_next", C.c_int32),
        ("hist", C.c_double * FIELD_HIST), ("quiet", C.c_ubyte * FIELD_MAXBLK),
    ]


MUT_OK, MUT_ETOOMANY, MUT_EPOSITION, MUT_ESTATE, MUT_EREPEAT = 0, 1, 2, 3, 4
SCAN_MAX_SITES, SCAN_MAX_EDGES = 8, 1024


class PlmScanOpts(C.Structure):
    _fields_ = [
        ("n_scan_sites", C.c_int32), ("flags", C.c_int32),
        ("sites", C.c_void_p), ("letter_offsets", C.c_void_p), ("letters", C.c_void_p),
        ("first", C.c_int64), ("count", C.c_int64),
        ("edges", C.c_void_p), ("n_edges", C.c_int32), ("use_threshold", C.c_int32),
        ("threshold", C.c_double), ("capacity", C.c_int64),
    ]


class PlmScanResult(C.Structure):
    _fields_ = [
        ("energies", C.c_void_p), ("histogram", C.c_void_p), ("kept_index", C.c_void_p), ("kept_energies", C.c_void_p),
        ("dh_min", C.c_double), ("dh_max", C.c_double), ("n_kept", C.c_int64), ("n_combinations", C.c_int64),
    ]


class PlmArSampleOpts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("first_chain", C.c_uint32), ("seed", C.c_uint64), ("beta", C.c_float),
                ("allowed", C.c_void_p)]


class PlmArFitOpts(C.Structure):
    _fields_ = [("lambda_h", C.c_double), ("lambda_j", C.c_double), ("max_iter", C.c_int32), ("epsilon", C.c_double),
                ("lbfgs_m", C.c_int32)]


class PlmArFitResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("ls_reason", C.c_int32),
                ("fx", C.c_double), ("nll", C.c_double), ("gnorm", C.c_double), ("xnorm", C.c_double)]


class PlmRbmSampleOpts(C.Structure):
    _fields_ = [("n_chains", C.c_int32), ("burn_in", C.c_int32), ("n_snapshots", C.c_int32), ("thin", C.c_int32),
                ("first_step", C.c_uint32), ("first_chain", C.c_uint32), ("seed", C.c_uint64),
                ("start", C.c_void_p), ("fixed", C.c_void_p), ("allowed", C.c_void_p)]


class PlmRbmFitOpts(C.Structure):
    _fields_ = [("n_chains", C.c_int32), ("n_epochs", C.c_int32), ("steps_per_epoch", C.c_int32), ("first_epoch", C.c_int32),
                ("lr_decay_after", C.c_int32), ("lr", C.c_double), ("lambda_g", C.c_double), ("lambda_w", C.c_double),
                ("seed", C.c_uint64), ("start", C.c_void_p)]


class PlmRbmFitResult(C.Structure):
    _fields_ = [("x_out", C.c_void_p), ("data_out", C.c_void_p), ("model_out", C.c_void_p), ("chains_out", C.c_void_p),
                ("trace", C.c_void_p), ("phase_ms", C.c_void_p), ("epochs_done", C.c_int32), ("status", C.c_int32)]


class PlmRbmAisResult(C.Structure):
    _fields_ = [
        ("log_z", C.c_double), ("log_z0", C.c_double), ("log_z_se", C.c_double), ("ess", C.c_double),
        ("log_w", C.c_void_p), ("states", C.c_void_p), ("hidden", C.c_void_p),
        ("steps_done", C.c_int32), ("status", C.c_int32),
    ]


class PlmCrossOpts(C.Structure):
    _fields_ = [("skip_state", C.c_int32), ("want_best", C.c_int32)]


class PlmCrossBest(C.Structure):
    _fields_ = [("index", C.c_int64), ("best", C.c_double), ("second", C.c_double)]


RBM_EPOCH_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p)


# every symbol include/plm_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("plm_version", C.c_int, []),
    ("plm_device_count", C.c_int, []),
    ("plm_strerror", C.c_char_p, [C.c_int]),
    ("plm_last_error", C.c_char_p, []),
    ("plm_fit", C.c_int, [C.POINTER(PlmProblem), C.POINTER(PlmResult), C.c_int, _P, ITER_CB, _P,
                          EXCHANGE_CB, _P]),
    ("plm_fit_sharded", C.c_int, [C.POINTER(PlmProblem), C.POINTER(PlmResult), C.c_int, _P, ITER_CB, _P,
                                  COLLECTIVE_CB, _P]),
    ("plm_fit_sharded_rccl", C.c_int, [C.POINTER(PlmProblem), C.POINTER(PlmResult), C.c_int, _P, ITER_CB, _P, _P]),
    ("plm_rccl_unique_id", C.c_int, [_P]),
    ("plm_rccl_runtime_version", C.c_int, []),
    ("plm_rccl_selftest", C.c_int, [C.c_int, _P]),
    ("plm_ctx_attach_rccl", C.c_int, [_P, _P]),
    ("plm_reweight", C.c_int, [_P, C.c_int32, C.c_int32, C.c_double, _P]),
    ("plm_reweight_ex", C.c_int, [_P, C.c_int32, C.c_int32, C.c_double, C.c_int32, _P]),
    ("plm_marginals", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("plm_eval", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P,
                           C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    ("plm_scores", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    ("plm_scores_ex", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("plm_hamiltonians", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int, _P, _P]),
    ("plm_potentials", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int, _P, _P]),
    ("plm_model_pair_scores", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int, _P, _P, _P]),
    ("plm_model_pair_scores_ex", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int, _P, _P, _P]),
    ("plm_double_mutants", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int, _P, _P]),
    ("plm_independent_fields", C.c_int, [_P, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int, _P, _P, _P]),
    ("plm_sample", C.c_int, [C.c_int32, C.c_int32, _P, C.POINTER(PlmSampleOpts), C.c_int, _P, _P, _P]),
    ("plm_sample_plan", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlmSamplePlanInfo)]),
    ("plm_bm_fit", C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(PlmBmOpts), C.c_int, _P, BM_EPOCH_CB, _P,
                             C.POINTER(PlmBmResult)]),
    ("plm_ais", C.c_int, [C.c_int32, C.c_int32, _P, C.POINTER(PlmAisOpts), C.c_int, _P, AIS_CB, _P,
                          C.POINTER(PlmAisResult)]),
    ("plm_pt", C.c_int, [C.c_int32, C.c_int32, _P, C.POINTER(PlmPtOpts), C.c_int, _P, PT_CB, _P,
                         C.POINTER(PlmPtResult)]),
    ("plm_anneal", C.c_int, [C.c_int32, C.c_int32, _P, C.POINTER(PlmAnnealOpts), C.c_int, _P, ANNEAL_CB, _P,
                             C.POINTER(PlmAnnealResult)]),
    ("plm_meanfield", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int, _P,
                                C.POINTER(PlmMfResult)]),
    ("plm_direct_information", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int, _P, _P]),
    ("plm_alignment_stats", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int, _P]),
    ("plm_cross_identities", C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(PlmIdentOpts), _P, _P, _P, _P,
                                       C.c_int, _P]),
    ("plm_redundancy_filter", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(PlmIdentOpts), _P, _P, C.c_int, _P]),
    ("plm_triplet_stats", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.POINTER(PlmTripletOpts), _P,
                                    _P, _P, C.POINTER(C.c_uint64), C.c_int, _P]),
    ("plm_triplet_scan", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.POINTER(PlmTripletOpts), _P,
                                   _P, _P, C.POINTER(C.c_uint64), C.c_int, _P]),
    ("plm_pca_fit", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlmPcaOpts), _P, _P, _P, _P,
                              C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P,
                              C.c_int, _P]),
    ("plm_pca_fit_cb", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlmPcaOpts), _P, _P, _P, _P,
                                 C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 _P, C.c_int, _P, PCA_CB, _P, C.POINTER(C.c_int32)]),
    ("plm_pca_project", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int, _P]),
    ("plm_residue_distances", C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_int, _P]),
    ("plm_distance_maps_aggregate", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P,
                                              C.c_int32, _P, _P, C.c_int, _P]),
    ("plm_fasta_split", C.c_int, [_P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, _P, _P, _P]),
    ("plm_encode_columns", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, _P]),
    ("plm_write_raw_ec_file", C.c_int, [C.c_char_p, C.c_int32, _P, C.c_char_p, _P]),
    ("plm_ctx_create", C.c_int, [C.POINTER(PlmProblem), C.c_int, _P, C.POINTER(_P)]),
    ("plm_ctx_destroy", None, [_P]),
    ("plm_ctx_set_exchange", C.c_int, [_P, EXCHANGE_CB, _P]),
    ("plm_ctx_set_collective", C.c_int, [_P, COLLECTIVE_CB, _P]),
    ("plm_ctx_set_options", C.c_int, [_P, C.c_int32, C.c_double, C.c_int32]),
    ("plm_ctx_native_size", C.c_int64, [_P]),
    ("plm_ctx_reweight", C.c_int, [_P]),
    ("plm_ctx_set_weights", C.c_int, [_P, _P]),
    ("plm_ctx_get_weights", C.c_int, [_P, _P, _P, C.POINTER(C.c_float)]),
    ("plm_ctx_marginals", C.c_int, [_P, _P, _P]),
    ("plm_ctx_set_x", C.c_int, [_P, _P]),
    ("plm_ctx_get_x", C.c_int, [_P, _P]),
    ("plm_ctx_get_g", C.c_int, [_P, _P]),
    ("plm_ctx_eval", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("plm_ctx_optimize", C.c_int, [_P, ITER_CB, _P, C.POINTER(PlmResult)]),
    ("plm_ctx_scores", C.c_int, [_P, _P, _P]),
    ("plm_ctx_time_kernels", C.c_int, [_P, C.c_int32, _P]),
    ("plm_ctx_time_field_positions", C.c_int, [_P, C.c_int32, _P]),
    ("plm_ctx_solver_stats", C.c_int, [_P, _P]),
    ("plm_ctx_field_position", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlmFieldBuffers)]),
    ("plm_ctx_field_solve", C.c_int, [_P, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlmFieldSolve), _P,
                                      C.c_int64]),
    ("plm_lbfgs_gram", C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P,
                                 C.c_int, _P, _P, _P, _P]),
    ("plm_lbfgs_direction", C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_double, _P, _P,
                                      C.c_float, C.c_int, _P, _P]),
    ("plm_lbfgs_multidot", C.c_int, [C.c_int64, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_uint32, C.c_uint64,
                                     C.c_int, _P]),
    ("plm_lbfgs_dots", C.c_int, [C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, C.c_int, _P]),
    ("plm_lbfgs_lincomb", C.c_int, [C.c_int64, C.c_float, _P, C.c_float, _P, C.c_int, _P]),
    ("plm_ctx_precond_diagonal", C.c_int, [_P, _P]),
    ("plm_rccl_probe", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int, _P]),
    ("plm_rccl_probe_local", C.c_int, [C.c_int32, C.c_int, _P]),
    ("plm_lbfgs_coefficients", None, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, _P, _P,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("plm_linesearch_run", C.c_int, [PHI_CB, _P, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_double), _P]),
    ("plm_lbfgs_admit", C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, _P,
                                  _P, C.POINTER(C.c_double), C.POINTER(C.c_double), _P, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("plm_mutant_effects", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int, _P, _P, _P,
                                     _P]),
    ("plm_mutant_scan", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(PlmScanOpts), C.c_int, _P,
                                  C.POINTER(PlmScanResult)]),
    ("plm_ar_logprob", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int, _P, _P, _P]),
    ("plm_ar_sample", C.c_int, [C.c_int32, C.c_int32, _P, C.POINTER(PlmArSampleOpts), C.c_int, _P, _P]),
    ("plm_ar_eval", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, C.c_int, _P,
                              C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    ("plm_ar_fit", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlmArFitOpts), _P, ITER_CB, _P, C.c_int,
                             _P, _P, C.POINTER(PlmArFitResult)]),
    ("plm_rbm_score", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int, _P, _P, _P]),
    ("plm_rbm_sample", C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(PlmRbmSampleOpts), C.c_int, _P, _P, _P]),
    ("plm_rbm_fit", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(PlmRbmFitOpts), C.c_int, _P,
                              RBM_EPOCH_CB, _P, C.POINTER(PlmRbmFitResult)]),
    ("plm_rbm_ais", C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(PlmAisOpts), C.c_int, _P, AIS_CB, _P,
                              C.POINTER(PlmRbmAisResult)]),
    ("plm_cross_energies", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, _P,
                                     C.POINTER(PlmCrossOpts), C.c_int, _P, _P, _P, _P]),
    ("plm_group_assignment", C.c_int, [_P, C.c_int64, _P, _P, C.c_int32, _P, _P]),
]

_lib = None


class PlmError(RuntimeError):
    """Failure reported by libplm_hip (code + the library's message)."""

    def __init__(self, code, message):
        super().__init__("libplm_hip error %d: %s" % (code, message))
        self.code = code


def load():
    """Load libplm_hip.so and bind every declared symbol.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the PLM solver)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        if os.environ.get("PLM_HIP_LIB") and not hasattr(lib, name):
            continue              # A/B experiments against an older build: tolerate newer symbols
        fn = getattr(lib, name)   # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.plm_version() != ABI_VERSION:
        raise ImportError("libplm_hip ABI version %d, expected %d" % (lib.plm_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != PLM_OK:
        lib = load()
        msg = lib.plm_last_error() or lib.plm_strerror(rc) or b""
        raise PlmError(rc, msg.decode("utf-8", "replace"))
