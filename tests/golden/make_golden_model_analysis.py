#!/usr/bin/env python3
"""
Golden vectors of the numeric analysis the REFERENCE's CouplingsModel runs on a fitted model (run in the build
container only; the reference does not exist on the GPU box).  Input: tests/golden/hip_fit_L24.model (a fit written on
an MI355X, read by the reference's own plmc_v2 reader).  Pinned here, and by which reference code:
  * fn_scores, cn_scores, mi_scores_raw, mi_scores_apc  <- CouplingsModel._calculate_ecs (couplings/model.py:777-827)
                                                           with _zero_sum_gauge (:180-233)
  * ecs (i, j) order and index labels                   <- the same, after sort_values(by="cn", ascending=False)
  * single_mut_mat, double_mut_mat blocks               <- CouplingsModel.single_mut_mat / double_mut_mat (:715-742)
  * to_independent_model().h_i with its lambda_h, N_eff  <- :882-927 (one scipy fmin_bfgs per site)
numba is absent, so the reference's @jit functions run as plain Python under the identity stub of tests/refstubs.py.
No reference source is written into this repo.

Usage:  python tests/golden/make_golden_model_analysis.py      (writes tests/golden/model_analysis_L24.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refstubs  # noqa: E402

N_DMM_PAIRS = 64


def dmm_pairs(L, n=N_DMM_PAIRS, seed=24):
    """a fixed set of i < j pairs: the corners (0,1), (0,L-1), (L-2,L-1) plus seeded random ones"""
    iu, ju = np.triu_indices(L, 1)
    fixed = [(0, 1), (0, L - 1), (L - 2, L - 1)]
    rest = [k for k in range(len(iu)) if (iu[k], ju[k]) not in fixed]
    pick = np.random.default_rng(seed).choice(rest, n - len(fixed), replace=False)
    pairs = fixed + sorted((int(iu[k]), int(ju[k])) for k in pick)
    return np.array(pairs, dtype=np.int32)


def main():
    refstubs.install()
    from evcouplings.couplings.model import CouplingsModel
    m = CouplingsModel(os.path.join(HERE, "hip_fit_L24.model"))
    ecs = m.ecs
    pairs = dmm_pairs(m.L)
    dmm = m.double_mut_mat
    indep = m.to_independent_model()
    out = os.path.join(HERE, "model_analysis_L24.npz")
    np.savez_compressed(
        out,
        fn_scores=m.fn_scores, cn_scores=m.cn_scores, mi_scores_raw=m.mi_scores_raw, mi_scores_apc=m.mi_scores_apc,
        ecs_i=ecs["i"].to_numpy(), ecs_j=ecs["j"].to_numpy(), ecs_index=ecs.index.to_numpy(),
        single_mut_mat=m.single_mut_mat, dmm_pairs=pairs, dmm_blocks=dmm[pairs[:, 0], pairs[:, 1]],
        h_indep=indep.h_i, lambda_h=np.float64(m.lambda_h), n_eff=np.float64(m.N_eff),
    )
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
