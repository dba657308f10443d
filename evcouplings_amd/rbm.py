"""
Restricted Boltzmann machine of an alignment (Tubiana, Cocco, Monasson 2019; DESIGN_NEXT_ROWS.md section 9.22): Potts
visible units at the L sites, M Bernoulli hidden units,

    I_mu(v) = c_mu + sum_i W_mu,i(v_i),   score(v) = sum_i g_i(v_i) + sum_mu softplus(I_mu(v)) = log P(v) + log Z

    python -m evcouplings_amd.rbm fit IN.a2m -o OUT.npz --hidden M [--focus ID] [--theta T] [--epochs E] [--chains C]
                                      [--steps K] [--lr X] [--lr-decay-after T] [--lambda-g X] [--lambda-w X] [--seed S]
    python -m evcouplings_amd.rbm sample MODEL.npz -n N -o OUT.a2m [--burn-in B] [--no-gaps] [--seed S]
    python -m evcouplings_amd.rbm score MODEL.npz --sequences IN.a2m -o OUT.csv [--features FEATURES.npy]
                                        [--log-z VALUE|ais]
    python -m evcouplings_amd.rbm logz MODEL.npz [-n CHAINS] [-k TEMPS] [--sweeps N] [--seed S]

`score` writes log P(v) + log Z: scores of one model compare, scores of two models do not.  `--log-z` adds the column
log_prob = score - log Z, with the value given or with the estimate of `logz` at its defaults ("ais").  `logz` estimates
log Z by annealed importance sampling (plm.rbm_log_partition, DESIGN_NEXT_ROWS.md section 9.25) and prints it with its
standard error, the effective sample size, log Z_0 and the entropy.  `--features` saves the hidden-unit inputs I [n, M],
the per-sequence feature vector.

The file is an .npz with kind="rbm".  The fit is persistent contrastive divergence by plain gradient ascent (plm.rbm_fit).
The defaults (64 hidden units, 1000 chains, 200 epochs of 2 steps, lr 0.1, lambda_w = 1e-3, the pseudo-count of the
start point) are this project's choice, not taken from a reference implementation.
"""
import argparse
import sys
from types import SimpleNamespace

import numpy as np

from evcouplings_amd import alignment_io, plm

FIELDS = ("g", "c", "W", "alphabet", "index_list", "target_seq", "lambda_g", "lambda_w", "n_eff", "theta")
PSEUDO_COUNT = 1.0      # weight of the uniform pseudo-sequence in the start fields (fit_alignment)


def start_point(msa, weights, q, n_hidden, init_seed=0):
    """
    The start of the fit: g = the centred log of the pseudo-counted frequencies f_i(a) = (sum_s w_s delta(x_si, a) +
    PSEUDO_COUNT / q) / (N_eff + PSEUDO_COUNT) -- one pseudo-sequence of weight PSEUDO_COUNT spread over the q letters --
    so that the start is the independent-site model; c = 0; W ~ N(0, 0.01^2) from numpy.random.Generator(PCG64(init_seed)),
    drawn in the order [M][L][q].  Returns (g, c, W) in float32.
    """
    msa = np.asarray(msa, np.int64)
    w = np.asarray(weights, np.float64)
    L = msa.shape[1]
    f = np.zeros((L, q))
    for a in range(q):
        f[:, a] = (w[:, None] * (msa == a)).sum(axis=0)
    f = (f + PSEUDO_COUNT / q) / (w.sum() + PSEUDO_COUNT)
    g = np.log(f)
    g -= g.mean(axis=1, keepdims=True)
    rng = np.random.Generator(np.random.PCG64(init_seed))
    W = rng.normal(0.0, 0.01, (n_hidden, L, q))
    return g.astype(np.float32), np.zeros(n_hidden, np.float32), W.astype(np.float32)


def fit_alignment(msa, q=21, n_hidden=64, theta_id=0.8, weights=None, n_chains=1000, n_epochs=200, steps_per_epoch=2, lr=0.1,
                  lr_decay_after=0, lambda_g=0.0, lambda_w=1e-3, seed=0, init_seed=0, callback=None, alphabet=None,
                  index_list=None, target_seq=None, device=0):
    """
    Fit the machine to an (N, L) matrix of states.  weights: None (1 / cluster size at identity theta_id, plm.reweight) or
    one weight per sequence.  The start is start_point(...).  Returns the model, a namespace with the FIELDS of the file
    plus `fit`, the dict of plm.rbm_fit without the parameters.
    """
    msa = np.ascontiguousarray(msa, dtype=np.int8)
    if weights is None:
        weights = 1.0 / plm.reweight(msa, theta_id)
    weights = np.asarray(weights, np.float32)
    g0, c0, W0 = start_point(msa, weights, q, n_hidden, init_seed)
    res = plm.rbm_fit(msa, weights, q, g0, c0, W0, n_chains, n_epochs, steps_per_epoch=steps_per_epoch, lr=lr,
                      lr_decay_after=lr_decay_after, lambda_g=lambda_g, lambda_w=lambda_w, seed=seed, callback=callback,
                      device=device)
    L = msa.shape[1]
    alphabet = alignment_io.ALPHABET_PROTEIN[:q] if alphabet is None else alphabet
    return SimpleNamespace(
        g=res.pop("g"), c=res.pop("c"), W=res.pop("W"), alphabet=str(alphabet), L=L, q=int(q), M=int(n_hidden),
        index_list=np.arange(1, L + 1, dtype=np.int32) if index_list is None else np.asarray(index_list, np.int32),
        target_seq="".join(alphabet[k] for k in msa[0]) if target_seq is None else str(target_seq),
        lambda_g=float(lambda_g), lambda_w=float(lambda_w), n_eff=float(np.asarray(weights, np.float64).sum()),
        theta=float(theta_id), fit=res)


def scores(model, seqs, device=0):
    """log P(v) + log Z of (n, L) states"""
    return plm.rbm_score(seqs, model.q, model.g, model.c, model.W, device=device)


def hidden_inputs(model, seqs, device=0):
    """The feature matrix: I [n, M], the inputs of the hidden units for (n, L) states"""
    return plm.rbm_score(seqs, model.q, model.g, model.c, model.W, inputs=True, device=device)[1]


def single_mutant_matrix(model, target, device=0):
    """score(target with site i set to a) - score(target), L x q float64, from one call over the L q single mutants"""
    target = np.asarray(target, np.int8).reshape(-1)
    L, q = model.L, model.q
    if target.shape != (L,):
        raise ValueError("the target has %d sites, the model %d" % (target.size, L))
    rows = np.tile(target, (L * q + 1, 1))
    k = np.arange(L * q)
    rows[k, k // q] = k % q
    s = plm.rbm_score(rows, q, model.g, model.c, model.W, device=device)
    return (s[:L * q] - s[L * q]).reshape(L, q)


def sample_sequences(model, n, burn_in=100, seed=0, exclude="", fix=None, first_chain=0, device=0):
    """
    n states (n, L), one per chain after burn_in block-Gibbs steps from the start rule.  exclude: letters never drawn;
    fix: None or a dict site -> state (every chain starts there and the site is never resampled).
    """
    allowed = None
    if exclude:
        allowed = np.array([ch not in exclude for ch in model.alphabet])
    start = fixed = None
    if fix:
        fixed = np.zeros(model.L, bool)
        # the free sites start from the start rule of a run without steps; the fixed ones are then set
        start = plm.rbm_sample(model.g, model.c, model.W, model.q, n, burn_in=0, seed=seed, allowed=allowed,
                               first_chain=first_chain, device=device)[0]
        for i, a in fix.items():
            fixed[int(i)] = True
            start[:, int(i)] = int(a)
    return plm.rbm_sample(model.g, model.c, model.W, model.q, n, burn_in=burn_in, seed=seed, start=start, fixed=fixed,
                          allowed=allowed, first_chain=first_chain, device=device)[0]


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def log_partition_exact(model):
    """
    log Z in float64 on the host by enumeration of the 2^M hidden states: Z = sum_h exp(sum_mu h_mu c_mu)
    prod_i sum_a exp(g_i(a) + sum_mu h_mu W_mu,i(a)).  For small models and the tests: ValueError above M = 24.
    """
    g, c, W = (np.asarray(a, np.float64) for a in (model.g, model.c, model.W))
    M = c.size
    if M > 24:
        raise ValueError("log_partition_exact enumerates 2^M hidden states: M = %d is above 24" % M)
    terms = np.empty(1 << M)
    block = 1 << min(M, 12)
    for b0 in range(0, 1 << M, block):
        h = ((np.arange(b0, b0 + block)[:, None] >> np.arange(M)[None, :]) & 1).astype(np.float64)      # [B][M]
        U = g[None] + np.tensordot(h, W, axes=(1, 0))                                                   # [B][L][q]
        m = U.max(axis=2)
        terms[b0:b0 + block] = h @ c + (m + np.log(np.exp(U - m[:, :, None]).sum(axis=2))).sum(axis=1)
    t = terms.max()
    return float(t + np.log(np.exp(terms - t).sum()))


def log_partition(model, **kw):
    """
    log Z by annealed importance sampling (plm.rbm_log_partition, whose keyword arguments these are: n_chains, n_temps,
    sweeps_per_temp, betas, seed, ...): its dict, with log_z, log_z_se, ess, log_z0 and, when the anneal ends at beta = 1,
    mean_score and entropy.  For any number of hidden units; log_partition_exact is the check for small ones.
    """
    return plm.rbm_log_partition(model.g, model.c, model.W, model.q, **kw)


def log_probabilities(model, seqs, log_z=None, **kw):
    """
    (log P(v) of (n, L) states, the dict of log_partition): the scores minus log_z.  log_z None: the anneal is run with
    the keyword arguments of log_partition; a given log_z is used as it is, and the dict holds it alone.
    """
    device = kw.get("device", 0)
    res = log_partition(model, **kw) if log_z is None else dict(log_z=float(log_z))
    return scores(model, seqs, device=device) - res["log_z"], res


def mean_log_likelihood(model, msa, weights=None, log_z=None, **kw):
    """the weighted mean of log P over the rows of msa (weights None: every row counts once)"""
    lp, _ = log_probabilities(model, msa, log_z, **kw)
    w = np.ones(len(lp)) if weights is None else np.asarray(weights, np.float64)
    return float((w * lp).sum() / w.sum())


def save(path, model):
    with open(path, "wb") as f:
        np.savez(f, kind="rbm", **{k: getattr(model, k) for k in FIELDS})
    return path


def load(path):
    with np.load(path, allow_pickle=False) as z:
        if "kind" not in z.files or str(z["kind"]) != "rbm":
            raise ValueError("%s is not a restricted Boltzmann machine file (no kind=\"rbm\")" % path)
        missing = [k for k in FIELDS if k not in z.files]
        if missing:
            raise ValueError("%s lacks %s" % (path, ", ".join(missing)))
        d = {k: z[k] for k in FIELDS}
    g = np.asarray(d["g"], np.float32)
    m = SimpleNamespace(g=g, c=np.asarray(d["c"], np.float32), W=np.asarray(d["W"], np.float32), alphabet=str(d["alphabet"]),
                        index_list=np.asarray(d["index_list"], np.int32), target_seq=str(d["target_seq"]), L=g.shape[0],
                        q=g.shape[1])
    m.M = m.c.size
    for k in ("lambda_g", "lambda_w", "n_eff", "theta"):
        setattr(m, k, float(d[k]))
    return m


def _letters(model, states):
    table = np.array(list(model.alphabet))
    return ["".join(row) for row in table[np.asarray(states, np.int64)]]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.rbm", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fit")
    f.add_argument("alignment")
    f.add_argument("-o", required=True)
    f.add_argument("--hidden", type=int, default=64)
    f.add_argument("--focus", default=None, help="focus sequence identifier (default: every column is a model column)")
    f.add_argument("--theta", type=float, default=0.8)
    f.add_argument("--epochs", type=int, default=200)
    f.add_argument("--chains", type=int, default=1000)
    f.add_argument("--steps", type=int, default=2)
    f.add_argument("--lr", type=float, default=0.1)
    f.add_argument("--lr-decay-after", type=int, default=0)
    f.add_argument("--lambda-g", type=float, default=0.0)
    f.add_argument("--lambda-w", type=float, default=1e-3)
    f.add_argument("--seed", type=int, default=0)
    s = sub.add_parser("sample")
    s.add_argument("model")
    s.add_argument("-n", type=int, required=True)
    s.add_argument("-o", required=True)
    s.add_argument("--burn-in", type=int, default=100)
    s.add_argument("--no-gaps", action="store_true")
    s.add_argument("--seed", type=int, default=0)
    c = sub.add_parser("score")
    c.add_argument("model")
    c.add_argument("--sequences", required=True)
    c.add_argument("-o", required=True)
    c.add_argument("--features", default=None, help="save the hidden-unit inputs [n, M] to this .npy file")
    c.add_argument("--log-z", default=None, metavar="VALUE|ais", help="add the column log_prob = score - log Z")
    z = sub.add_parser("logz")
    z.add_argument("model")
    z.add_argument("-n", type=int, default=4096, help="chains")
    z.add_argument("-k", type=int, default=1000, help="temperatures")
    z.add_argument("--sweeps", type=int, default=1)
    z.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "fit":
        enc = alignment_io.encode_alignment(a.alignment, focus_seq=a.focus)
        model = fit_alignment(enc.msa, q=len(enc.alphabet), n_hidden=a.hidden, theta_id=a.theta, n_chains=a.chains,
                              n_epochs=a.epochs, steps_per_epoch=a.steps, lr=a.lr, lr_decay_after=a.lr_decay_after,
                              lambda_g=a.lambda_g, lambda_w=a.lambda_w, seed=a.seed, alphabet=enc.alphabet,
                              index_list=enc.index_list, target_seq=enc.target_seq)
        save(a.o, model)
        row = model.fit["trace"][-1]
        sys.stderr.write("%s after %d epochs: mean score %.6f, max |D - N| = %.3e (g) %.3e (c) %.3e (W), N_eff = %.1f\n"
                         % (model.fit["status"], model.fit["epochs_done"], row[4], row[0], row[1], row[2], model.n_eff))
        return 0
    model = load(a.model)
    if a.cmd == "sample":
        from evcouplings_amd.sample import write_a2m
        x = sample_sequences(model, a.n, burn_in=a.burn_in, seed=a.seed, exclude=model.alphabet[0] if a.no_gaps else "")
        write_a2m(a.o, model, _letters(model, x))
        return 0
    if a.cmd == "logz":
        r = log_partition(model, n_chains=a.n, n_temps=a.k, sweeps_per_temp=a.sweeps, seed=a.seed)
        print("log Z = %.6f +- %.6f (ESS = %.1f of %d chains, %d temperatures x %d sweeps)"
              % (r["log_z"], r["log_z_se"], r["ess"], a.n, a.k, a.sweeps))
        print("log Z_0 = %.6f, entropy = %.6f" % (r["log_z0"], r["entropy"]))
        return 0
    enc = alignment_io.encode_alignment(a.sequences, alphabet=model.alphabet)
    if enc.msa.shape[1] != model.L:
        ap.error("%s has %d columns, the model %d sites" % (a.sequences, enc.msa.shape[1], model.L))
    sc, feats = plm.rbm_score(enc.msa, model.q, model.g, model.c, model.W, inputs=True)
    ids = [h for h, ok in zip(enc.ids, enc.valid) if ok]
    log_z = None
    if a.log_z is not None:
        log_z = log_partition(model)["log_z"] if a.log_z == "ais" else float(a.log_z)
    with open(a.o, "w") as out:
        out.write("id,score,log_prob\n" if log_z is not None else "id,score\n")
        for h, v in zip(ids, sc):
            if log_z is not None:
                out.write("%s,%.17g,%.17g\n" % (h.split()[0], v, v - log_z))
            else:
                out.write("%s,%.17g\n" % (h.split()[0], v))
    if a.features:
        np.save(a.features, feats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
