"""numpy float64 twin of the restricted Boltzmann machine (plm_rbm_*, DESIGN_NEXT_ROWS.md section 9.22):
    I_mu(v) = c_mu + sum_i W_mu,i(v_i),   score(v) = sum_i g_i(v_i) + sum_mu softplus(I_mu(v))
with the parameters g [L][q], c [M], W [M][L][q].  The score, block Gibbs sampling with the margin of every draw, the fit
by persistent contrastive divergence, a float32 mode that makes the contract's adds literally and sequentially in numpy
float32, the near-tie rule of the draw-for-draw tests, and exact enumeration for tiny shapes (P(v), the visible-to-visible
transition matrix of one step).  Not a test module."""
import numpy as np

import sampler_twin as st

F32 = np.float32


def n_params(L, q, M):
    return L * q + M + M * L * q


def pack(g, c, W):
    return np.concatenate([np.asarray(g).ravel(), np.asarray(c).ravel(), np.asarray(W).ravel()])


def unpack(x, L, q, M):
    return x[:L * q].reshape(L, q), x[L * q:L * q + M], x[L * q + M:].reshape(M, L, q)


def random_model(L, q, M, seed=None, sd_g=1.0, sd_c=0.5, sd_w=0.5):
    """g ~ N(0, sd_g), c ~ N(0, sd_c), W ~ N(0, sd_w) from default_rng(9000 + 100 L + M) unless a seed is given, float32"""
    rng = np.random.default_rng(9000 + 100 * L + M if seed is None else seed)
    return (rng.normal(0.0, sd_g, (L, q)).astype(F32), rng.normal(0.0, sd_c, M).astype(F32),
            rng.normal(0.0, sd_w, (M, L, q)).astype(F32))


def sigmoid(I):
    e = np.exp(-np.abs(I))
    return np.where(I >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(I):
    return np.maximum(I, 0.0) + np.log1p(np.exp(-np.abs(I)))


def _rows(W, x):
    """W_mu,i(x_si) as [n][M][L]"""
    L = x.shape[1]
    return np.asarray(W)[:, np.arange(L)[None, :], x].transpose(1, 0, 2)


def inputs(x, c, W):
    """I [n][M] in float64"""
    x = np.asarray(x, np.int64)
    return np.asarray(c, np.float64)[None, :] + _rows(np.asarray(W, np.float64), x).sum(axis=2)


def score(x, g, c, W, with_scale=False):
    """score [n]; with_scale also A [n], the sum of the absolute values of every term that enters a row's sums"""
    x = np.asarray(x, np.int64)
    L = x.shape[1]
    gx = np.asarray(g, np.float64)[np.arange(L)[None, :], x]
    I = inputs(x, c, W)
    s = gx.sum(axis=1) + softplus(I).sum(axis=1)
    if not with_scale:
        return s
    A = (np.abs(gx).sum(axis=1) + np.abs(np.asarray(c, np.float64)).sum()
         + np.abs(_rows(np.asarray(W, np.float64), x)).sum(axis=(1, 2)) + softplus(I).sum(axis=1))
    return s, A


# ---- random numbers -----------------------------------------------------------------------------------------------------

def _word0(seed, chain, kind, step, index):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return st.philox4x32_10(chain, kind, step, index, seed & 0xFFFFFFFF, seed >> 32)[0]


def uniform_hidden(seed, chain, step, mu):
    """u of the counter (chain, 2, step, mu), float64"""
    return ((_word0(seed, chain, 2, step, mu) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def uniform24(word0):
    """the kernels' float32 uniform: ((word0 >> 8) + 0.5) 2^-24 rounded to float32 and kept below 1"""
    u = ((word0 >> np.uint64(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)
    return np.minimum(u, F32(0.99999994))


# ---- block Gibbs --------------------------------------------------------------------------------------------------------

def start_states(g, n_chains, seed, allowed=None, first_chain=0, diagnostics=False):
    """one draw per site of softmax g_i over the allowed states, counter (first_chain + c, 0, 0xFFFFFFFF, i); with
    diagnostics also draw()'s margin and max |U| per (chain, site)"""
    g = np.asarray(g, np.float64)
    L = g.shape[0]
    chains = np.arange(n_chains) + first_chain
    x, margin, maxu = np.zeros((n_chains, L), np.int64), np.ones((n_chains, L)), np.zeros((n_chains, L))
    for i in range(L):
        x[:, i], margin[:, i], maxu[:, i] = st.draw(np.tile(g[i], (n_chains, 1)),
                                                    st.uniform(seed, chains, st.START_SWEEP, i), 1.0, allowed)
    return (x, margin, maxu) if diagnostics else x


def step(x, g, c, W, seed, t, chains, fixed=None, allowed=None, f32=False):
    """One step in place on x (C, L).  Returns (h [C][M], rec) with rec = dict(hm, hs, vm, vu): the margin |u - sigma(I)|
    and the scale S = |c_mu| + sum_i |W_mu,i(v_i)| of every hidden draw, and draw()'s margin and max |U| of every visible
    draw (margin 1 at a fixed site).  f32: the adds of the contract literally, one numpy float32 add at a time."""
    C, L = x.shape
    M, q = len(c), np.asarray(g).shape[1]
    mus = np.arange(M)
    if f32:
        W32, I = np.asarray(W, F32), np.tile(np.asarray(c, F32), (C, 1))
        for i in range(L):
            I = I + W32[:, i, x[:, i]].T
        p = (F32(1.0) / (F32(1.0) + np.exp(-I))).astype(np.float64)
        u = uniform24(_word0(seed, chains[:, None], 2, t, mus[None, :])).astype(np.float64)
    else:
        I = inputs(x, c, W)
        p = sigmoid(I)
        u = uniform_hidden(seed, chains[:, None], t, mus[None, :])
    h = u < p
    rec = dict(hm=np.abs(u - p),
               hs=np.abs(np.asarray(c, np.float64))[None, :] + np.abs(_rows(np.asarray(W, np.float64), x)).sum(axis=2),
               vm=np.ones((C, L)), vu=np.zeros((C, L)))
    if f32:
        U = np.tile(np.asarray(g, F32)[None], (C, 1, 1))
        for mu in range(M):
            U = np.where(h[:, mu][:, None, None], U + W32[mu][None], U)
        U = U.astype(np.float64)
    else:
        U = np.asarray(g, np.float64)[None] + np.tensordot(h.astype(np.float64), np.asarray(W, np.float64), axes=(1, 0))
    for i in range(L):
        if fixed is not None and fixed[i]:
            continue
        x[:, i], rec["vm"][:, i], rec["vu"][:, i] = st.draw(U[:, i], st.uniform(seed, chains, t, i), 1.0, allowed)
    return h, rec


def run(g, c, W, n_chains, n_steps, seed=0, start=None, fixed=None, allowed=None, first_step=0, first_chain=0, f32=False):
    """n_steps steps of every chain, all of them kept: (states [T][C][L], hidden [T][C][M], rec) with every entry of rec
    stacked over the steps."""
    L, M = np.asarray(g).shape[0], len(c)
    chains = np.arange(n_chains) + first_chain
    x = start_states(g, n_chains, seed, allowed, first_chain) if start is None else np.array(start, np.int64).reshape(n_chains, L)
    states, hidden = np.zeros((n_steps, n_chains, L), np.int64), np.zeros((n_steps, n_chains, M), np.int64)
    recs = []
    for t in range(n_steps):
        h, rec = step(x, g, c, W, seed, first_step + t, chains, fixed, allowed, f32)
        states[t], hidden[t] = x, h
        recs.append(rec)
    return states, hidden, {k: np.stack([r[k] for r in recs]) if recs else np.zeros((0,)) for k in ("hm", "hs", "vm", "vu")}


def sample(g, c, W, q, n_chains, burn_in=10, n_snapshots=1, thin=1, seed=0, start=None, fixed=None, allowed=None,
           first_step=0, first_chain=0, hidden=False):
    """Twin of evcouplings_amd.plm.rbm_sample (same arguments, same return value)."""
    T = burn_in + (n_snapshots - 1) * thin
    L, M = np.asarray(g).shape[0], len(c)
    states, hid, _ = run(g, c, W, n_chains, T, seed, start, fixed, allowed, first_step, first_chain)
    x0 = start_states(g, n_chains, seed, allowed, first_chain) if start is None else np.array(start, np.int64).reshape(n_chains, L)
    out, hout = np.zeros((n_snapshots, n_chains, L), np.int8), np.zeros((n_snapshots, n_chains, M), np.int8)
    for k in range(n_snapshots):
        t = burn_in + k * thin
        out[k] = states[t - 1] if t > 0 else x0
        if t > 0:
            hout[k] = hid[t - 1]
    return (out, hout) if hidden else out


def delta_hidden(L, S):
    """L + 1 sequential float32 adds through sigma (slope at most 1/4), plus a few ulps for expf and the division"""
    return 2.0 ** -24 * (L * S / 4.0 + 8.0)


def delta_visible(M, q, maxu):
    """the sampler's delta with M in place of L"""
    return 2.0 ** -24 * (M + 4 * q) * (1.0 + maxu)


def worst_margin(rec, L, q, M):
    """the smallest margin / delta over every draw of a run's rec (above 1: no draw is a near tie)"""
    r = [np.inf]
    if rec["hm"].size:
        r.append((rec["hm"] / delta_hidden(L, rec["hs"])).min())
        r.append((rec["vm"] / delta_visible(M, q, rec["vu"])).min())
    return float(min(r))


def explained(name, states, hidden, tw_states, tw_hidden, rec, q, cap=0.01):
    """The near-tie rule.  states, hidden: [T][C][L] and [T][C][M] after each of T steps, the device's and the twin's.  The
    draws of a chain are ordered (step; hidden units 0 .. M-1; sites 0 .. L-1).  A chain may differ from the twin only if
    at its first differing draw the twin's margin is at most delta (delta_hidden, delta_visible), and at most `cap` of the
    chains may differ at all.  Returns the number of chains that differ."""
    T, C, L = tw_states.shape
    M = tw_hidden.shape[2]
    dh, dv = np.asarray(hidden) != tw_hidden, np.asarray(states) != tw_states
    per_step = dh.any(axis=2) | dv.any(axis=2)                  # [T][C]
    bad = np.nonzero(per_step.any(axis=0))[0]
    unexplained = []
    for ch in bad:
        t = int(np.argmax(per_step[:, ch]))
        if dh[t, ch].any():
            mu = int(np.argmax(dh[t, ch]))
            margin, delta, what = rec["hm"][t, ch, mu], delta_hidden(L, rec["hs"][t, ch, mu]), ("h", mu)
        else:
            i = int(np.argmax(dv[t, ch]))
            margin, delta, what = rec["vm"][t, ch, i], delta_visible(M, q, rec["vu"][t, ch, i]), ("v", i)
        if not margin <= delta:
            unexplained.append((int(ch), t) + what + (float(margin), float(delta)))
    print("%s: %d of %d chains differ from the twin, %d unexplained" % (name, len(bad), C, len(unexplained)))
    assert not unexplained, unexplained[:5]
    assert len(bad) <= cap * C, (len(bad), C)
    return len(bad)


# ---- the fit ------------------------------------------------------------------------------------------------------------

def _one_hot(x, q):
    oh = np.zeros(x.shape + (q,))
    np.put_along_axis(oh, np.asarray(x, np.int64)[:, :, None], 1.0, axis=2)
    return oh


def statistics(x, w, c, W, q, div):
    """(S_g [L][q], S_c [M], S_W [M][L][q]) = sums over the rows of w delta, w p and (w p) delta, over div"""
    oh = _one_hot(x, q)
    wp = np.asarray(w, np.float64)[:, None] * sigmoid(inputs(x, c, W))
    return ((np.asarray(w, np.float64)[:, None, None] * oh).sum(axis=0) / div, wp.sum(axis=0) / div,
            np.einsum("sm,sia->mia", wp, oh) / div)


def fit(msa, weights, q, g, c, W, n_chains, n_epochs, steps_per_epoch=2, lr=0.1, lr_decay_after=0, lambda_g=0.0,
        lambda_w=0.0, seed=0, start=None, first_epoch=0, stop_at=None):
    """Twin of evcouplings_amd.plm.rbm_fit.  stop_at: a global epoch whose callback answers "stop".  The dict also holds
    `worst`, the smallest margin / delta over every draw of the chains, and `x` and `x_start`, the packed parameters."""
    msa = np.asarray(msa, np.int64)
    L, M = msa.shape[1], len(c)
    w = np.asarray(weights, F32).astype(np.float64)
    neff = 0.0
    for v in w:
        neff += v
    x = pack(np.asarray(g, F32), np.asarray(c, F32), np.asarray(W, F32)).astype(F32)
    x_start = x.copy()
    two_lambda = np.concatenate([np.full(L * q, 2.0 * lambda_g), np.zeros(M), np.full(M * L * q, 2.0 * lambda_w)])
    chains = np.arange(n_chains)
    v = None if start is None else np.array(start, np.int64).reshape(n_chains, L)
    trace, worst, done, status = [], np.inf, 0, "maxiter"
    D = Nm = None
    for e in range(n_epochs):
        ge = first_epoch + e
        lr_g = lr if (lr_decay_after == 0 or ge + 1 <= lr_decay_after) else lr * lr_decay_after / (ge + 1)
        gq, cq, Wq = unpack(x, L, q, M)
        D = pack(*statistics(msa, w, cq, Wq, q, neff))
        if v is None:
            v = start_states(gq, n_chains, seed)
        for j in range(steps_per_epoch):
            _, rec = step(v, gq, cq, Wq, seed, ge * steps_per_epoch + j, chains)
            worst = min(worst, worst_margin({k: a[None] for k, a in rec.items()}, L, q, M))
        Nm = pack(*statistics(v, np.ones(n_chains), cq, Wq, q, float(n_chains)))
        d = np.abs(D - Nm)
        trace.append([d[:L * q].max(), d[L * q:L * q + M].max(), d[L * q + M:].max(), lr_g,
                      (w * score(msa, gq, cq, Wq)).sum() / neff])
        if stop_at is not None and ge == stop_at:
            status = "interrupted"
            break
        th = x.astype(np.float64)
        x = (th + lr_g * ((D - Nm) - two_lambda * th)).astype(F32)
        done = e + 1
    go, co, Wo = unpack(x, L, q, M)
    return dict(g=go, c=co, W=Wo, x=x, x_start=x_start, data=unpack(D, L, q, M), model=unpack(Nm, L, q, M),
                chains=v.astype(np.int8), trace=np.array(trace), epochs_done=done, status=status, worst=float(worst))


# ---- exact enumeration (q^L and 2^M small) ------------------------------------------------------------------------------

def all_hidden(M):
    return (np.arange(1 << M)[:, None] >> np.arange(M)[None, :]) & 1


def joint_log_weights(g, c, W):
    """E[v][h] = sum_i g_i(v_i) + sum_mu h_mu I_mu(v) over sampler_twin.all_states(L, q) x all_hidden(M)"""
    L, q = np.asarray(g).shape
    vs = st.all_states(L, q)
    gx = np.asarray(g, np.float64)[np.arange(L)[None, :], vs].sum(axis=1)
    return gx[:, None] + inputs(vs, c, W) @ all_hidden(len(c)).T.astype(np.float64)


def log_z(g, c, W):
    E = joint_log_weights(g, c, W)
    return float(E.max() + np.log(np.exp(E - E.max()).sum()))


def enumerate_p(g, c, W):
    """P(v) of every state of sampler_twin.all_states(L, q), from the score"""
    L, q = np.asarray(g).shape
    s = score(st.all_states(L, q), g, c, W)
    p = np.exp(s - s.max())
    return p / p.sum()


def transition_matrix(g, c, W):
    """T(v -> v') = sum_h P(h | v) P(v' | h) of one step, row-stochastic over all_states(L, q)"""
    L, q = np.asarray(g).shape
    M = len(c)
    vs, hs = st.all_states(L, q), all_hidden(M).astype(np.float64)
    p1 = sigmoid(inputs(vs, c, W))                                                  # [V][M]
    Phv = np.prod(np.where(hs[None] > 0, p1[:, None, :], 1.0 - p1[:, None, :]), axis=2)   # [V][H]
    U = np.asarray(g, np.float64)[None] + np.tensordot(hs, np.asarray(W, np.float64), axes=(1, 0))   # [H][L][q]
    pv = np.exp(U - U.max(axis=2, keepdims=True))
    pv /= pv.sum(axis=2, keepdims=True)
    Pvh = pv[:, np.arange(L)[None, :], vs].prod(axis=2)                              # [H][V]
    return Phv @ Pvh


def mean_log_likelihood(x, w, g, c, W):
    """the exact weighted mean of log P(x_s), by enumeration"""
    w = np.asarray(w, np.float64)
    return float((w * (score(x, g, c, W) - log_z(g, c, W))).sum() / w.sum())
