"""The shapes, seeds and schedules the tests of the RBM's annealed importance sampling share (DESIGN_NEXT_ROWS.md section
9.25): test_rbm_ais_host.py checks on the CPU, for every case listed here, the conditions the device tests of
test_gpu_rbm_ais.py rest on.  Not a test module."""
import functools

import numpy as np

import rbm_ais_twin as at
import rbm_cases
import rbm_twin as tw

SHAPES = rbm_cases.SHAPES            # (1, 2, 1), (5, 3, 3), (13, 21, 7), (70, 32, 65)

# a schedule that is not linear and does not end at 1: read step by step through its prefixes
BETAS = np.array([0.0, 0.4, 0.7, 1.3], np.float32)

# (L, q, M, C, n, seed): the draw-for-draw cases.  Few chains at the two large alphabets: a visible draw has q - 1 steps
# of the running sum to come near (section 9.22), so that many chains would hold near ties between the float32 and the
# float64 argument of the draw.  A seed is listed only if the float32-arg twin and the float64-arg twin differ in at most
# 0.5 % of the chains (test_rbm_ais_host.test_follow_cases_have_few_near_ties).
FOLLOW_CASES = [
    (1, 2, 1, 257, 1, 101), (1, 2, 1, 257, 2, 102),
    (5, 3, 3, 257, 1, 103), (5, 3, 3, 257, 2, 104),
    (13, 21, 7, 5, 1, 105), (13, 21, 7, 5, 2, 106),
    (70, 32, 65, 5, 1, 107), (70, 32, 65, 5, 2, 108),
]


def model(L, q, M):
    return rbm_cases.model(L, q, M)


@functools.lru_cache(maxsize=None)
def follow_twin(L, q, M, C, n, seed, f64_arg=False):
    """the twin of a draw-for-draw case with its trace; computed once, never modified"""
    g, c, W = model(L, q, M)
    return at.ais(g, c, W, C, sweeps_per_temp=n, betas=BETAS, seed=seed, trace=True, f64_arg=f64_arg)


# the two enumerable models: (L, q, M, sd_w), rbm_twin.random_model with its default seed
ENUMERABLE = [(5, 3, 3, 0.7), (13, 21, 7, 0.5)]
ENUMERABLE_K, ENUMERABLE_C, ENUMERABLE_SEEDS = 16, 4096, (0, 1, 2)


def enumerable_model(L, q, M, sd_w):
    return tw.random_model(L, q, M, sd_w=sd_w)


@functools.lru_cache(maxsize=None)
def enumerable_twin(L, q, M, sd_w, seed):
    g, c, W = enumerable_model(L, q, M, sd_w)
    return at.ais(g, c, W, ENUMERABLE_C, ENUMERABLE_K, seed=seed)


# every launch plan gives the same bytes: K steps of n sweeps, C chains against the first C_HEAD of them
PLAN_SHAPES = [(13, 21, 7), (70, 32, 65)]
PLAN_K, PLAN_N, PLAN_C, PLAN_C_HEAD, PLAN_SEED = 7, 2, 300, 101, 211
PLAN_LAUNCHES = (1, 3, 7, 0)

# the fitted model of test_a_fitted_model: rbm_cases.fit_data(13, 21, 7, N, seed), a few tens of epochs
FIT = dict(shape=(13, 21, 7), N=400, seed=61, chains=256, epochs=40, lr=0.1, C=1024, K=(32, 128))
