"""The shapes, seeds and options the restricted-Boltzmann-machine tests share (DESIGN_NEXT_ROWS.md section 9.22):
test_rbm_host.py checks on the CPU, for every case listed here, the conditions the device tests of test_gpu_rbm.py rest
on.  Not a test module."""
import numpy as np

import rbm_twin as tw

# the smallest shapes at which the kernels can still go wrong: one site, state and unit; an enumerable model; q not a
# multiple of 4 and M below one chunk of hidden units; L past one wave, q at the maximum, M no multiple of 4, 8, 32 or 64
SHAPES = [(1, 2, 1), (5, 3, 3), (13, 21, 7), (70, 32, 65)]
ROWS = [1, 5, 257, 1000]


def model(L, q, M):
    """inputs of order one: W ~ N(0, 1 / L)"""
    return tw.random_model(L, q, M, sd_w=1.0 / np.sqrt(L))


# (L, q, M, C, variant, seed, steps): the draw-for-draw cases
DRAW_CASES = [
    (1, 2, 1, 1000, "plain", 11, 3),
    (5, 3, 3, 257, "plain", 12, 3),
    (13, 21, 7, 1000, "plain", 13, 3),
    (13, 21, 7, 257, "fixed", 14, 3),
    (13, 21, 7, 5, "allowed", 15, 3),
    (13, 21, 7, 257, "start", 16, 3),
    (70, 32, 65, 1000, "plain", 17, 2),
    (70, 32, 65, 257, "fixed", 18, 2),
    (70, 32, 65, 257, "allowed", 19, 2),
    (70, 32, 65, 1, "start", 20, 2),
]


def draw_options(L, q, C, variant, seed):
    """the keyword arguments (start, fixed, allowed) of a draw-for-draw case"""
    rng = np.random.default_rng(500 + seed)
    kw = {}
    if variant == "fixed":
        kw["fixed"] = rng.random(L) < 0.3
        kw["fixed"][L // 2] = True
        kw["start"] = rng.integers(0, q, (C, L))
    if variant == "allowed":
        kw["allowed"] = np.ones(q, bool)
        kw["allowed"][[0, q - 1, q // 2]] = False
    if variant == "start":
        kw["start"] = rng.integers(0, q, (C, L))
    return kw


# the distribution after CHI_STEPS steps from the start rule at (5, 3, 3)
CHI_SHAPE, CHI_CHAINS, CHI_STEPS, CHI_SEED = (5, 3, 3), 20000, 3, 77

# (L, q, M, N, C, epochs, steps per epoch, seed): the fits compared with the twin, chains included.  A seed is listed only
# if no draw of the twin's chains is a near tie (test_rbm_host.test_fit_cases_have_no_near_tie).  A visible draw has q - 1
# steps of the running sum to come near, each with probability about 2 delta: at q = 21 and 32 that is 1e-3 per draw, so
# such seeds exist only for a few hundred draws, and the large alphabets go with few chains here (and with many rows of
# data); FIT_STAT_CASES has their many chains.
FIT_CASES = [
    (1, 2, 1, 5, 1, 1, 2, 31),
    (5, 3, 3, 257, 1000, 1, 2, 32),
    (13, 21, 7, 1000, 5, 1, 2, 33),
    (70, 32, 65, 257, 1, 1, 2, 54),
    (5, 3, 3, 4100, 5, 1, 2, 35),            # more than one chunk of sequences in the statistics
    (5, 3, 3, 1000, 257, 3, 2, 38),
    (13, 21, 7, 257, 5, 3, 2, 66),
    (70, 32, 65, 5, 1, 3, 2, 97),
]
# one epoch with many chains at the large alphabets: the model statistics are compared with the twin's statistics of the
# chains the device returns, which needs no condition on the draws
FIT_STAT_CASES = [
    (13, 21, 7, 257, 1000, 1, 2, 71),
    (70, 32, 65, 5, 257, 1, 2, 72),
    (5, 3, 3, 5, 4100, 1, 1, 73),            # more than one chunk of chains
]
FIT_OPTS = dict(lr=0.1, lambda_g=0.01, lambda_w=0.02)


def fit_data(L, q, M, N, seed):
    """(msa, weights, (g, c, W)): random sequences, non-uniform weights with zeros among them (never all), a random start"""
    rng = np.random.default_rng(800 + seed)
    msa = rng.integers(0, q, (N, L)).astype(np.int8)
    w = rng.uniform(0.1, 1.0, N).astype(np.float32)
    w[rng.random(N) < 0.2] = 0.0
    w[0] = 0.75
    return msa, w, model(L, q, M)


# test 8: data planted by an RBM at (5, 3, 3), fitted from the independent-site start
# (rehearsed with the twin: the planted model is 0.094 nats per sequence above the start, 300 epochs at lr = 1 gain 0.085
# of them, 150 epochs only 0.001: the weights first have to grow out of their N(0, 0.01^2) start)
LEARN = dict(shape=(5, 3, 3), N=1000, C=1000, epochs=300, steps=2, lr=1.0, seed=41)


def planted_data():
    L, q, M = LEARN["shape"]
    g, c, W = tw.random_model(L, q, M, seed=4242, sd_g=0.3, sd_c=0.5, sd_w=4.0)
    states, _, _ = tw.run(g, c, W, LEARN["N"], 30, seed=4243)
    return states[-1].astype(np.int8), (g, c, W)
