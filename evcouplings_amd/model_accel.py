"""
GPU statistical energies behind the reference's `CouplingsModel`.

`evcouplings/couplings/model.py` computes Hamiltonians with two numba-compiled loops that its
`CouplingsModel.hamiltonians`, `.single_mut_mat_full`, `.smm`, `.dmm` and the mutate stage call:
`_hamiltonians(sequences, J_ij, h_i)` (model.py:25-60) and
`_single_mutant_hamiltonians(target_seq, J_ij, h_i)` (model.py:63-109).  `install()` rebinds those two
module attributes to wrappers around libplm_hip (`plm_hamiltonians`, `plm_potentials`); signatures, dtypes
and return layouts are the reference's.  There is no CPU fallback: without the library the wrappers raise.
`install(reader=True)` also swaps the class's plmc_v2 reader (L^2 tiny `np.fromfile` calls, model.py:364-389)
for a block-wise one -- host-side format code, same attributes; measured to be no faster (see read_plmc_v2).
`install(analysis=True)` also rebinds the numeric rest of the class (DESIGN_NEXT_ROWS.md section 9.5):
`_calculate_ecs` (FN / MI / CN / the EC table), the `double_mut_mat` property and `to_independent_model`, on
`plm_model_pair_scores`, `plm_double_mutants` and `plm_independent_fields`.  Off by default.
`sample_sequences(model, n)` draws sequences from a model with the library's Gibbs sampler (`plm_sample`,
DESIGN_NEXT_ROWS.md section 9.6); the reference has no sampler, so `install()` has nothing to rebind for it.
`refine_model(model)` refines a model's fields and couplings towards its own `f_i`, `f_ij` with the library's
Boltzmann-machine loop (`plm_bm_fit`, section 9.7), so that its samples reproduce those frequencies.
`log_partition(model)` estimates log Z by annealed importance sampling (`plm_ais`, section 9.8), and
`log_probabilities(model, sequences, log_z)` turns statistical energies into log-probabilities with it.
`optimize_sequences(model, n)` searches a model for its highest-scoring sequences by simulated annealing and greedy
ascent (`plm_anneal`, section 9.13), and `local_optima(model, sequences)` climbs from given sequences.
`install(mutations=True)` also rebinds the mutate stage's `predict_mutation_table` (mutate/calculations.py:54-180, one
`delta_hamiltonian` call per table row) to one `plm_mutant_effects` call per table (section 9.16): `parse_mutations`,
`delta_hamiltonians`, `predict_mutation_table`; `scan_library(model, positions)` ranks every letter combination at a few
positions (`plm_mutant_scan`).  Off by default.
"""
from copy import deepcopy

import numpy as np

_ORIGINAL = {}
_ANALYSIS = {}                 # class -> {attribute name: the class's own attribute before install(analysis=True)}
_ANALYSIS_NAMES = ("_calculate_ecs", "double_mut_mat", "to_independent_model")
_MUTATE = {}                   # module -> its own predict_mutation_table before install(mutations=True)
COMPONENT_TO_INDEX = {"full": 0, "couplings": 1, "fields": 2}
_WILD_TYPE = ("wild", "wt", "")


def _pairs_from_dense(J_ij):
    """dense L x L x q x q (J[j,i] = J[i,j].T) -> the i<j blocks the C ABI takes."""
    L = J_ij.shape[0]
    iu = np.triu_indices(L, 1)
    return np.ascontiguousarray(J_ij[iu], dtype=np.float32)


def hamiltonians(sequences, J_ij, h_i):
    """Drop-in for model._hamiltonians: N x 3 float64 (total, couplings, fields)."""
    from evcouplings_amd import plm
    sequences = np.asarray(sequences)
    L, q = h_i.shape
    return plm.hamiltonians(sequences.astype(np.int8), q, h_i, _pairs_from_dense(J_ij))


def single_mutant_hamiltonians(target_seq, J_ij, h_i):
    """Drop-in for model._single_mutant_hamiltonians: L x q x 3 float64."""
    from evcouplings_amd import plm
    L, q = h_i.shape
    return plm.single_mutant_matrix(np.asarray(target_seq).astype(np.int8), q, h_i, _pairs_from_dense(J_ij))


def sample_sequences(model, n_chains, burn_in=100, n_snapshots=1, thin=1, beta=1.0, seed=0, start=None, fixed=None,
                     exclude="", as_letters=True, energies=False, device=0):
    """
    Draw sequences from P(x) ~ exp beta H(x) of a `CouplingsModel` (anything with `J_ij` [L, L, q, q], `h_i` [L, q],
    `alphabet`, `target_seq` and `index_list`) with the Gibbs sampler of libplm_hip: n_chains independent chains, burn_in
    sweeps, then n_snapshots snapshots thin sweeps apart.
      start    None (one draw per site of softmax beta h_i), "target" (every chain starts from the target sequence), or an
               (n_chains, L) matrix of letters or of states
      fixed    positions in the model's own numbering (`index_list`) that keep the target's residue
      exclude  letters that are never drawn, e.g. "-" for sequences without gaps
    Returns an (n_snapshots * n_chains, L) matrix of letters (as_letters) or of int8 states, snapshots one after the
    other; with energies=True a tuple of that and the (n_snapshots * n_chains, 3) energies (H, H_J, H_h) at beta = 1.
    """
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    letters, x0, flags, allowed = _chain_setup(model, n_chains, start, fixed, exclude, beta, seed, device)
    out, en = plm.sample(h_i, _pairs_from_dense(np.asarray(model.J_ij)), q, n_chains, burn_in=burn_in,
                         n_snapshots=n_snapshots, thin=thin, beta=beta, seed=seed, start=x0, fixed=flags, allowed=allowed,
                         energies=energies, device=device)
    out = out.reshape(-1, L)
    res = letters[out] if as_letters else out
    return (res, en.reshape(-1, 3)) if energies else res


def _to_states(mat, code):
    """A matrix of letters, or of states already, as int8 states."""
    mat = np.asarray(mat)
    if mat.dtype.kind in "iu":
        return mat.astype(np.int8)
    try:
        return np.vectorize(code.__getitem__, otypes=[np.int8])(mat.astype("U1"))
    except KeyError as e:
        raise ValueError("letter %s is not in the model's alphabet" % e)


def _site_flags(model, fixed, L):
    """Positions in the model's own numbering (`index_list`) as L flags, or None when there are none."""
    if fixed is None or not len(fixed):
        return None
    pos = {int(p): k for k, p in enumerate(np.asarray(model.index_list))}
    missing = [p for p in fixed if int(p) not in pos]
    if missing:
        raise ValueError("positions %r are not in the model's index_list" % missing)
    flags = np.zeros(L, np.uint8)
    flags[[pos[int(p)] for p in fixed]] = 1
    return flags


def _allowed_flags(exclude, code, q):
    """The q flags of the states that may be drawn when the letters of `exclude` may not, or None."""
    if not exclude:
        return None
    unknown = [a for a in exclude if a not in code]
    if unknown:
        raise ValueError("excluded letters %r are not in the model's alphabet" % "".join(unknown))
    allowed = np.ones(q, np.uint8)
    allowed[[code[a] for a in exclude]] = 0
    return allowed


def _chain_setup(model, n_chains, start, fixed, exclude, beta, seed, device):
    """What `sample_sequences` and `optimize_sequences` make of their arguments: (the alphabet as an array of letters, the
    start states or None for the start rule, the flags of the fixed sites or None, the flags of the allowed states or
    None).  Fixed sites hold the target's residue in the start states."""
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    letters, code = _letters_and_code(model, q)
    target = _to_states(np.array(list(model.target_seq)), code)
    allowed = _allowed_flags(exclude, code, q)
    flags = _site_flags(model, fixed, L)
    if isinstance(start, str):
        if start != "target":
            raise ValueError('start must be None, "target" or a matrix')
        x0 = np.tile(target, (int(n_chains), 1))
    elif start is not None:
        x0 = _to_states(start, code).reshape(int(n_chains), L).copy()
    elif flags is not None:
        # the start rule knows no fixed sites: draw it, then put the target's residues there
        x0 = plm.sample(h_i, _pairs_from_dense(np.asarray(model.J_ij)), q, n_chains, burn_in=0, beta=beta, seed=seed,
                        allowed=allowed, energies=False, device=device)[0][0]
    else:
        x0 = None
    if flags is not None:
        x0[:, flags.astype(bool)] = target[flags.astype(bool)]
    return letters, x0, flags, allowed


def optimize_sequences(model, n_chains, betas=None, n_steps=100, sweeps_per_step=1, max_greedy=100, seed=0, start=None,
                       fixed=None, exclude="", top=None, as_letters=True, info=False, device=0):
    """
    Search a `CouplingsModel` (as for `sample_sequences`) for sequences of high statistical energy H by simulated
    annealing and greedy ascent (`plm.anneal`, DESIGN_NEXT_ROWS.md section 9.13): n_chains chains make sweeps_per_step
    Gibbs sweeps at every inverse temperature of betas (None: `plm.annealing_schedule(n_steps)`), then at most max_greedy
    greedy sweeps; every chain reports the best state it held at a checkpoint.  start, fixed and exclude mean what they
    mean in `sample_sequences` ("target": every chain starts from the target sequence; fixed positions, in `index_list`
    numbering, keep the target's residue; excluded letters are never proposed).
    Returns (sequences, energies, chains): the distinct best sequences as an (M, L) matrix of letters (as_letters) or of
    int8 states, sorted by H descending (the first chain's on equal H) and cut to `top` rows; their (M, 3) energies
    (H, H_J, H_h); and how many chains ended in each.  With info=True the dict of `plm.anneal` follows.
    """
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    letters, x0, flags, allowed = _chain_setup(model, n_chains, start, fixed, exclude, 1.0, seed, device)
    res = plm.anneal(h_i, _pairs_from_dense(np.asarray(model.J_ij)), q, n_chains, betas=betas, n_steps=n_steps,
                     sweeps_per_step=sweeps_per_step, max_greedy=max_greedy, seed=seed, start=x0, fixed=flags,
                     allowed=allowed, device=device)
    best, en = np.asarray(res["best"]), np.asarray(res["best_energies"])
    _, first, counts = np.unique(best, axis=0, return_index=True, return_counts=True)
    order = sorted(range(len(first)), key=lambda u: (-en[first[u], 0], first[u]))[:top]
    rows = first[order]
    out = best[rows]
    ret = (letters[out.astype(np.int64)] if as_letters else out, en[rows], counts[order])
    return ret + (res,) if info else ret


def local_optima(model, sequences, fixed=None, exclude="", max_sweeps=100, as_letters=True, info=False, device=0):
    """
    The local optimum of H every given sequence runs into under single-site moves (`plm.greedy_ascent`): greedy sweeps
    from each row of `sequences` (an (N, L) matrix of letters of the model's alphabet or of states, or a list of strings;
    for example the natural alignment) until a sweep moves nothing.  Fixed positions (`index_list` numbering) keep the
    residue of the given sequence; excluded letters are never moved to, and a sequence that holds one at a free position
    is refused.
    Returns (optima, energies, mutations, last_move): the (N, L) optima, their (N, 3) energies (H, H_J, H_h), the number
    of positions at which an optimum differs from its start, and the number of the last sweep that moved something (0:
    the sequence is a local optimum itself).  With info=True the dict of `plm.anneal` follows.
    """
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    letters, code = _letters_and_code(model, q)
    if len(sequences) and isinstance(sequences[0], str):
        sequences = [list(s) for s in sequences]
    x0 = _to_states(sequences, code)
    if x0.ndim != 2 or x0.shape[1] != L:
        raise ValueError("sequences must have the model's %d positions" % L)
    res = plm.greedy_ascent(h_i, _pairs_from_dense(np.asarray(model.J_ij)), q, x0, max_sweeps=max_sweeps,
                            fixed=_site_flags(model, fixed, L), allowed=_allowed_flags(exclude, code, q), device=device)
    out = np.asarray(res["states"])
    ret = (letters[out.astype(np.int64)] if as_letters else out, res["energies"], (out != x0).sum(axis=1),
           res["last_move"])
    return ret + (res,) if info else ret


def sample_tempered(model, n_ladders, betas=None, n_rungs=8, beta_max=1.0, burn_in=100, n_snapshots=1, thin=1,
                    sweeps_per_round=1, seed=0, start=None, as_letters=True, energies=False, info=False, device=0):
    """
    Draw sequences of a `CouplingsModel` (as for `sample_sequences`) by parallel tempering (`plm.parallel_tempering`,
    DESIGN_NEXT_ROWS.md section 9.9): n_ladders independent ladders whose walkers exchange between the inverse
    temperatures `betas` on the couplings (None: `plm.tempering_ladder(n_rungs, beta_max)`), burn_in rounds, then
    n_snapshots snapshots thin rounds apart of the walker at the top rung.  With beta_max = 1 these are samples of the
    model itself, as `sample_sequences` draws at beta = 1, from chains that cross between its modes through the upper
    rungs.  All states are allowed at all sites.
      start    None (the sampler's start rule), "target" (every walker starts from the target sequence), or an
               (n_ladders * R, L) matrix of letters or of states
    Returns an (n_snapshots * n_ladders, L) matrix of letters (as_letters) or of int8 states, snapshots one after the
    other; with energies=True followed by the (n_snapshots * n_ladders, 3) energies (H, H_J, H_h) at beta = 1; with
    info=True followed by the dict of `plm.parallel_tempering` (acceptance rates, walkers for a continuation).
    """
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    letters, code = _letters_and_code(model, q)
    if betas is None:
        betas = plm.tempering_ladder(n_rungs, beta_max)
    betas = np.asarray(betas, np.float32).reshape(-1)

    def states(mat):
        return _to_states(mat, code)

    n_walkers = int(n_ladders) * betas.size
    if isinstance(start, str):
        if start != "target":
            raise ValueError('start must be None, "target" or a matrix')
        x0 = (np.tile(states(np.array(list(model.target_seq))), (n_walkers, 1)),)
    elif start is not None:
        x0 = (states(start).reshape(n_walkers, L).copy(),)
    else:
        x0 = None
    res = plm.parallel_tempering(h_i, _pairs_from_dense(np.asarray(model.J_ij)), q, n_ladders, betas, burn_in=burn_in,
                                 n_snapshots=n_snapshots, thin=thin, sweeps_per_round=sweeps_per_round, seed=seed,
                                 start=x0, device=device)
    out = np.asarray(res["samples"]).reshape(-1, L)
    ret = (letters[out.astype(np.int64)] if as_letters else out,)
    if energies:
        ret += (np.asarray(res["energies"]).reshape(-1, 3),)
    if info:
        ret += (res,)
    return ret if len(ret) > 1 else ret[0]


def _letters_and_code(model, q):
    letters = np.array(list(model.alphabet) if isinstance(model.alphabet, str) else model.alphabet).astype("U1")
    if len(letters) != q:
        raise ValueError("the model's alphabet has %d letters, its fields %d states" % (len(letters), q))
    return letters, {a: k for k, a in enumerate(letters)}


def log_partition(model, **kw):
    """
    log Z of a `CouplingsModel` (anything with `J_ij` [L, L, q, q], `h_i` [L, q] and `alphabet`) by annealed importance
    sampling (`plm.log_partition`, DESIGN_NEXT_ROWS.md section 9.8; the keyword arguments are its own).  Returns its dict,
    with `sequences`: the final states of the chains as letters of the model's alphabet.
    """
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    letters, _ = _letters_and_code(model, q)
    res = plm.log_partition(h_i, _pairs_from_dense(np.asarray(model.J_ij)), q, **kw)
    res["sequences"] = letters[np.asarray(res["states"]).astype(np.int64)]
    return res


def log_probabilities(model, sequences, log_z):
    """
    log P(x) = H(x) - log_z of sequences under a `CouplingsModel`, log_z from `log_partition`.  sequences: an (N, L)
    matrix of letters of the model's alphabet or of integer states, or a list of strings.
    """
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    _, code = _letters_and_code(model, q)
    if len(sequences) and isinstance(sequences[0], str):
        sequences = [list(s) for s in sequences]
    mat = np.asarray(sequences)
    if mat.dtype.kind not in "iu":
        try:
            mat = np.vectorize(code.__getitem__, otypes=[np.int8])(mat.astype("U1"))
        except KeyError as e:
            raise ValueError("letter %s is not in the model's alphabet" % e)
    if mat.ndim != 2 or mat.shape[1] != L:
        raise ValueError("sequences must have the model's %d positions" % L)
    if mat.min(initial=0) < 0 or mat.max(initial=0) >= q:
        raise ValueError("states outside 0..%d" % (q - 1))
    return hamiltonians(mat, np.asarray(model.J_ij), h_i)[:, 0] - float(log_z)


def refine_model(model, n_chains=4096, n_epochs=120, sweeps_per_epoch=2, lr=0.5, lr_decay_after=None, lambda_h=None,
                 lambda_j=None, tol=0.0, seed=0, start=None, first_epoch=0, callback=None, device=0):
    """
    Boltzmann-machine refinement (`plm.bm_fit`) of a pseudo-likelihood model towards its own frequencies.  `model` is a
    `CouplingsModel` (`f_i`, `f_ij` and `J_ij` [L, L, q, q], `h_i`, `lambda_h`, `lambda_J`, `N_eff`) or the dict that
    `model_io.read_model_file` returns.  The targets are the model's f_i, f_ij, the start point its h_i, J_ij.  The
    regularisers default to the file's lambda_h / N_eff and lambda_J / N_eff (the plmc penalties on the per-sequence
    scale of the frequencies); lr_decay_after defaults to half the epochs.  Returns the dict of `plm.bm_fit` (hi, and
    jij as i<j blocks).
    """
    from evcouplings_amd import plm
    if isinstance(model, dict):
        fi, fij, hi, jij = model["fi"], model["fij"], model["hi"], model["jij"]
        lam_h, lam_j, n_eff = model["lambda_h"], model["lambda_j"], model["n_eff"]
    else:
        fi, hi = np.asarray(model.f_i), np.asarray(model.h_i)
        fij, jij = _pairs_from_dense(np.asarray(model.f_ij)), _pairs_from_dense(np.asarray(model.J_ij))
        lam_h, lam_j, n_eff = model.lambda_h, model.lambda_J, model.N_eff
    if (lambda_h is None or lambda_j is None) and not float(n_eff) > 0:
        raise ValueError("the model has no N_eff > 0 to scale its regularisers by; pass lambda_h and lambda_j")
    if lambda_h is None:
        lambda_h = max(float(lam_h), 0.0) / float(n_eff)
    if lambda_j is None:
        lambda_j = max(float(lam_j), 0.0) / float(n_eff)
    if lr_decay_after is None:
        lr_decay_after = int(n_epochs) // 2
    q = np.asarray(hi).shape[1]
    return plm.bm_fit(fi, fij, q, hi, jij, n_chains, n_epochs, sweeps_per_epoch=sweeps_per_epoch, lr=lr,
                      lr_decay_after=lr_decay_after, lambda_h=lambda_h, lambda_j=lambda_j, tol=tol, seed=seed, start=start,
                      first_epoch=first_epoch, callback=callback, device=device)


def read_plmc_v2(self, f, precision):
    """
    Drop-in for `CouplingsModel.__read_plmc_v2` (model.py:317-400): same attributes, dtypes and layouts,
    but the L(L-1)/2 pair blocks are read as two contiguous arrays and copied row by row into the dense
    symmetric L x L x q x q float64 arrays instead of L^2 `np.fromfile` calls.  Measured against the
    reference reader: 2.9 s vs 2.8 s at L = 300, 9.8 s vs 10.6 s at L = 600 -- the time goes into filling the
    two dense float64 arrays (2.5 GB at L = 600) with transposed blocks, not into the small reads, so this is
    NOT installed by default (`install(reader=True)` opts in).
    """
    self.L, self.num_symbols, self.N_valid, self.N_invalid, self.num_iter = np.fromfile(f, "int32", 5)
    self.theta, self.lambda_h, self.lambda_J, self.lambda_group, self.N_eff = np.fromfile(f, precision, 5)
    self.alphabet = np.fromfile(f, "S1", self.num_symbols).astype("U1")
    self.weights = np.fromfile(f, precision, self.N_valid + self.N_invalid)
    self._target_seq = np.fromfile(f, "S1", self.L).astype("U1")
    self.index_list = np.fromfile(f, "int32", self.L)
    L, q = int(self.L), int(self.num_symbols)
    self.f_i = np.fromfile(f, precision, L * q).reshape(L, q)
    self.h_i = np.fromfile(f, precision, L * q).reshape(L, q)
    n_pairs = L * (L - 1) // 2
    for name in ("f_ij", "J_ij"):
        blocks = np.fromfile(f, precision, n_pairs * q * q)
        if blocks.size != n_pairs * q * q:
            raise ValueError("truncated plmc_v2 file: %s blocks incomplete" % name)
        blocks = blocks.reshape(n_pairs, q, q)
        dense = np.zeros((L, L, q, q))
        off = 0
        for i in range(L - 1):          # the file's pair order is row-major i<j: row i is one contiguous run
            run = blocks[off:off + L - 1 - i]
            dense[i, i + 1:] = run
            dense[i + 1:, i] = run.transpose(0, 2, 1)
            off += L - 1 - i
        setattr(self, name, dense)
    if self.lambda_h < 0:                # mean-field marker, as in the reference reader (model.py:393-400)
        from evcouplings.couplings.mean_field import MeanFieldCouplingsModel
        self.__class__ = MeanFieldCouplingsModel
        self.transform_from_plmc_model()


def calculate_ecs(self):
    """
    Drop-in for `CouplingsModel._calculate_ecs` (model.py:777-827): FN of the zero-sum-gauged couplings and raw MI of
    every pair from one kernel (plm_model_pair_scores), CN and MI-APC from the object's own `apc`, and the EC table with
    the reference's columns, dtypes, row order (i < j, row-major, hence its index labels) and final
    sort_values(by="cn", ascending=False).  seqdist is NaN when index_list is not numeric, as the reference's
    try/except TypeError gives.
    """
    import pandas as pd
    from evcouplings_amd import plm
    fn, mi = plm.model_pair_scores(self.J_ij, self.f_ij, self.f_i)
    self._fn_scores = fn
    self._mi_scores_raw = mi
    self._cn_scores = self.apc(fn)
    self._mi_scores_apc = self.apc(mi)
    iu, ju = np.triu_indices(self.L, 1)
    index_list, target_seq = np.asarray(self.index_list), np.asarray(self.target_seq)
    idx_i, idx_j = index_list[iu], index_list[ju]
    try:
        seqdist = np.abs(idx_i - idx_j)
    except TypeError:
        seqdist = np.full(len(iu), np.nan)
    self._ecs = pd.DataFrame({
        "i": idx_i, "A_i": target_seq[iu].astype(object), "j": idx_j, "A_j": target_seq[ju].astype(object),
        "seqdist": seqdist, "mi_raw": mi[iu, ju], "mi_apc": self._mi_scores_apc[iu, ju],
        "fn": fn[iu, ju], "cn": self._cn_scores[iu, ju],
    }).sort_values(by="cn", ascending=False)


def _double_mut_mat(self):
    """
    Drop-in for the `CouplingsModel.double_mut_mat` property (model.py:715-742): the L x L x q x q double-mutant
    matrix of the target from plm_double_mutants, cached in `_double_mut_mat`.  Built on `self.single_mut_mat`,
    whatever computes it, so it is consistent with the single-mutant matrix the caller sees.
    """
    if self._double_mut_mat is None:
        from evcouplings_amd import plm
        self._double_mut_mat = plm.double_mutant_matrix(self.J_ij, self.single_mut_mat, self.target_seq_mapped)
    return self._double_mut_mat


double_mut_mat = property(_double_mut_mat)


def to_independent_model(self):
    """
    Drop-in for `CouplingsModel.to_independent_model` (model.py:882-927): the reference's deepcopy / h_i /
    J_ij.fill(0) / _reset_precomputed sequence, with the per-site fmin_bfgs replaced by the exact minimiser of the same
    objective (plm_independent_fields, Newton to |g|_inf <= 1e-12 max(1, N_eff)).  When lambda_h <= 0 the optimum need
    not exist (a state with f_i = 0 drives its field to -inf), so the call goes to the original method, whose
    iteration count bounds it.
    """
    if not float(self.lambda_h) > 0.0:
        return _analysis_original(type(self), "to_independent_model")(self)
    from evcouplings_amd import plm
    h_i, _ = plm.independent_fields(self.f_i, self.lambda_h, self.N_eff)
    c0 = deepcopy(self)
    c0.h_i = h_i
    c0.J_ij.fill(0)
    c0._reset_precomputed()
    return c0


# ---- mutation tables and combinatorial libraries (DESIGN_NEXT_ROWS.md section 9.16) ------------------------------

def _hashable(key):
    if isinstance(key, (list, tuple, np.ndarray)):
        return tuple(_hashable(k) for k in key)
    return key.item() if isinstance(key, np.generic) else key


def _model_maps(model):
    """(index_map, alphabet_map) of a model: its own where it has them (CouplingsModel), else built from `index_list`
    and `alphabet`."""
    index_map = getattr(model, "index_map", None)
    if index_map is None:
        index_map = {_hashable(b): a for a, b in enumerate(model.index_list)}
    alphabet_map = getattr(model, "alphabet_map", None)
    if alphabet_map is None:
        alphabet_map = {a: k for k, a in enumerate(np.asarray(list(model.alphabet)).astype("U1"))}
    return index_map, alphabet_map


def _target_states(model, alphabet_map):
    mapped = getattr(model, "target_seq_mapped", None)
    if mapped is None:
        mapped = [alphabet_map[a] for a in model.target_seq]
    return np.asarray(mapped).astype(np.int8)


def extract_mutations(mutation_string, offset=0, sep=","):
    """"K50R,I100V" -> [(50, "K", "R"), (100, "I", "V")]; "wild", "wt" and "" (any case) -> []: the reference's
    function of that name (mutate/calculations.py:25-51), a ValueError for a position that is no integer included."""
    if mutation_string.lower() in _WILD_TYPE:
        return []
    return [(int(x[1:-1]) + offset, x[0], x[-1]) for x in mutation_string.split(sep)]


def parse_mutations(model, mutants, segments=None):
    """
    A table of mutants as the CSR arrays of `plm.mutant_effects`.  mutants: one entry per row, a string as
    `extract_mutations` takes it or a list of (position, from, to) substitutions as `CouplingsModel.delta_hamiltonian`
    takes it; segments: None, one segment identifier for every substitution, or one comma-separated string per row
    (a substitution of position p in segment s addresses the model position (s, p); substitutions beyond the row's
    segments are dropped, as the reference's zip does).  Positions go through `model.index_map`, letters through
    `model.alphabet_map`.
    Returns (offsets int64 [n + 1], positions int32, states int8, invalid bool [n]): `invalid` marks the rows the
    reference turns into NaN (a position or letter the model does not have, a from-letter that is not the target's);
    they are stored with no substitutions.
    """
    index_map, alphabet_map = _model_maps(model)
    target = model.target_seq
    per_row = segments is not None and not isinstance(segments, str)
    if per_row:
        segments = list(segments)
    offsets, positions, states, invalid = [0], [], [], []
    for r, m in enumerate(mutants):
        subs = extract_mutations(m) if isinstance(m, str) else list(m)
        if per_row:
            subs = [((seg, pos), a, b) for seg, (pos, a, b) in zip(segments[r].split(","), subs)]
        elif segments is not None:
            subs = [((segments, pos), a, b) for pos, a, b in subs]
        row_pos, row_st, bad = [], [], False
        for pos, a_from, a_to in subs:
            try:
                i = index_map[_hashable(pos)]
                row_st.append(alphabet_map[a_to])
            except (KeyError, TypeError):
                bad = True
                break
            if a_from != target[i]:
                bad = True
                break
            row_pos.append(i)
        if bad:
            row_pos, row_st = [], []
        positions.extend(row_pos)
        states.extend(row_st)
        offsets.append(len(positions))
        invalid.append(bad)
    return (np.asarray(offsets, np.int64), np.asarray(positions, np.int32), np.asarray(states, np.int8),
            np.asarray(invalid, bool))


def _effects(model, parsed, device=0):
    """n x 3 (dH, dH_J, dH_h) of parsed rows; NaN where the row is invalid or the library refused it (a position named
    twice, which the reference counts twice)."""
    from evcouplings_amd import plm
    offsets, positions, states, invalid = parsed
    h_i = np.asarray(model.h_i)
    _, alphabet_map = _model_maps(model)
    out, status = plm.mutant_effects(_target_states(model, alphabet_map), h_i.shape[1], h_i,
                                     _pairs_from_dense(np.asarray(model.J_ij)), offsets, positions, states, device=device)
    out = np.array(out, dtype=np.float64)
    out[invalid | (np.asarray(status) != 0)] = np.nan
    return out


def delta_hamiltonians(model, substitutions, device=0):
    """`CouplingsModel.delta_hamiltonian` (model.py:672-712) for a list of substitution lists [(pos, from, to), ...] in one
    GPU call: n x 3 float64 (dH, dH_J, dH_h), NaN rows where the reference raises ValueError."""
    return _effects(model, parse_mutations(model, substitutions), device=device)


def predict_mutation_table(model, table, output_column="prediction_epistatic", mutant_column="mutant", hamiltonian="full",
                           segment=None, parsed=None):
    """
    Drop-in for the reference's `predict_mutation_table` (mutate/calculations.py:54-180): the same arguments, column and
    segment handling, NaN rows and ValueErrors, with one `plm.mutant_effects` call for the whole table in place of one
    `delta_hamiltonian` call per row.  parsed: the return value of `parse_mutations` for this table, to score it with
    several models that share positions, alphabet and target (the epistatic and the independent one) after one parse.
    """
    if hamiltonian not in COMPONENT_TO_INDEX:
        raise ValueError("Invalid selection for hamiltonian. Valid values are: " + ", ".join(COMPONENT_TO_INDEX))
    if not getattr(model, "has_target_seq", True):
        raise ValueError("CouplingsModel object does not have a target sequence (non-focus mode). "
                         "Set target sequence, or rerun inference in focus mode.")
    pred = table.copy()
    if parsed is None:
        parsed = parse_table(model, pred, mutant_column=mutant_column, segment=segment)
    pred.loc[:, output_column] = _effects(model, parsed)[:, COMPONENT_TO_INDEX[hamiltonian]]
    return pred


def parse_table(model, table, mutant_column="mutant", segment=None):
    """`parse_mutations` of a mutant table: the index or `mutant_column`, with the table's own `segment` column if it
    has one without nulls, else the `segment` argument."""
    mutations = table.index if mutant_column is None else table.loc[:, mutant_column]
    if "segment" in table.columns and table.loc[:, "segment"].notnull().all():
        segment = list(table.loc[:, "segment"])
    return parse_mutations(model, list(mutations), segments=segment)


def scan_library(model, positions, exclude="-", top=100, device=0):
    """
    The `top` best members of the combinatorial library that varies the given positions (the model's numbering) of the
    target over every letter not in `exclude`, by exhaustive enumeration on the GPU (`plm.top_combinations`).  Returns a
    DataFrame, best first (ties in library order): `index` (the member's number in `itertools.product` order), `letters`
    (its letters at the positions, in the order given), `mutant` (its substitutions in the notation of the mutate stage,
    "wild" for the target itself) and `dH`, `dH_J`, `dH_h` relative to the target.
    """
    import pandas as pd
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    L, q = h_i.shape
    index_map, alphabet_map = _model_maps(model)
    letters, code = _letters_and_code(model, q)
    try:
        sites = [index_map[_hashable(p)] for p in positions]
    except KeyError as e:
        raise ValueError("position %s is not in the model's index_list" % e)
    allowed = _allowed_flags(exclude, code, q)
    states = np.arange(q) if allowed is None else np.nonzero(allowed)[0]
    lists = [states] * len(sites)
    idx, en = plm.top_combinations(_target_states(model, alphabet_map), q, h_i, _pairs_from_dense(np.asarray(model.J_ij)),
                                   sites, letters=lists, top=top, device=device)
    chosen = letters[states[plm.scan_digits(idx, [len(states)] * len(sites))]].reshape(len(idx), len(sites))
    target = np.asarray(list(model.target_seq)).astype("U1")
    names = [",".join("%s%s%s" % (target[s], p if not isinstance(p, tuple) else p[-1], a)
                      for s, p, a in zip(sites, positions, row) if a != target[s]) or "wild" for row in chosen]
    return pd.DataFrame({"index": idx, "letters": ["".join(row) for row in chosen], "mutant": names,
                         "dH": en[:, 0], "dH_J": en[:, 1], "dH_h": en[:, 2]})


def _analysis_original(cls, name):
    for k in cls.__mro__:
        if k in _ANALYSIS and name in _ANALYSIS[k]:
            return _ANALYSIS[k][name]
    raise AttributeError("%s.%s: model_accel analysis drop-ins are not installed" % (cls.__name__, name))


def install(model_module=None, reader=False, analysis=False, mutations=False):
    """
    Rebind, in evcouplings.couplings.model (or the module object given): the two Hamiltonian loops and,
    if the module has a CouplingsModel class and `reader` is true, its plmc_v2 reader; if `analysis` is true, the
    class's `_calculate_ecs`, `double_mut_mat` and `to_independent_model` (subclasses such as
    MeanFieldCouplingsModel reach them through super() or inheritance); if `mutations` is true, `predict_mutation_table`
    in evcouplings.mutate.calculations and in evcouplings.mutate.protocol, which imports it by name.  `uninstall()`
    restores all of them.
    """
    if model_module is None:
        import evcouplings.couplings.model as model_module
    cls = getattr(model_module, "CouplingsModel", None)
    if model_module not in _ORIGINAL:
        _ORIGINAL[model_module] = (model_module._hamiltonians, model_module._single_mutant_hamiltonians,
                                   getattr(cls, "_CouplingsModel__read_plmc_v2", None))
    model_module._hamiltonians = hamiltonians
    model_module._single_mutant_hamiltonians = single_mutant_hamiltonians
    if reader and cls is not None:
        setattr(cls, "_CouplingsModel__read_plmc_v2", read_plmc_v2)
    if analysis and cls is not None:
        if cls not in _ANALYSIS:
            _ANALYSIS[cls] = {name: cls.__dict__[name] for name in _ANALYSIS_NAMES}
        cls._calculate_ecs = calculate_ecs
        cls.double_mut_mat = double_mut_mat
        cls.to_independent_model = to_independent_model
    if mutations:
        import evcouplings.mutate.calculations as calculations
        import evcouplings.mutate.protocol as mutate_protocol
        for mod in (calculations, mutate_protocol):
            _MUTATE.setdefault(mod, mod.predict_mutation_table)
            mod.predict_mutation_table = predict_mutation_table
    return model_module


def uninstall(model_module=None):
    if model_module is None:
        import evcouplings.couplings.model as model_module
    if model_module in _ORIGINAL:
        ham, smm, rd = _ORIGINAL.pop(model_module)
        model_module._hamiltonians, model_module._single_mutant_hamiltonians = ham, smm
        cls = getattr(model_module, "CouplingsModel", None)
        if cls is not None and rd is not None:
            setattr(cls, "_CouplingsModel__read_plmc_v2", rd)
    cls = getattr(model_module, "CouplingsModel", None)
    if cls in _ANALYSIS:
        for name, attr in _ANALYSIS.pop(cls).items():
            setattr(cls, name, attr)
    while _MUTATE:
        mod, original = _MUTATE.popitem()
        mod.predict_mutation_table = original
