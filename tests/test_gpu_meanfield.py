"""
GPU: the mean-field DCA path (csrc/plm_meanfield.hip) stage by stage against the references of tests/meanfield_twin.py.
Every stage is fed with what the stage before it produced on the GPU, so that a failure names its kernel:
  inverse   k_potrf_diag / k_dgemm<0,1> / <0,0> / <1,0>  jij_full against the extended-precision inverse of the
                                                         covariance rebuilt from the call's own f_i / f_ij, within 10x
                                                         what numpy's LU and Cholesky routes miss it by
  extract   k_mf_extract                                 the f32 pair blocks are the rounded dense ones, bit for bit
  fields    k_mf_fields                                  against a longdouble sum over the GPU's couplings, within the
                                                         bound of a length-n float64 sum
  DI        k_mf_di                                      against the oracle's iteration on the GPU's couplings, 1e-10
at every geometry of the 64-wide blocked inverse (one block with and without an identity tail, 2, 3 and 32 block
columns), at q = 2 and q = 32, at condition numbers up to 2e4, and plm_direct_information on models outside the
mean-field gauge.  No pair is excluded from a DI comparison: tests/test_meanfield_twin_host.py shows on the CPU that
none of these inputs has a pair whose iteration count depends on rounding, and each test here asserts it again for
the couplings it actually got.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meanfield_twin as tw  # noqa: E402

from evcouplings_amd._lib import PlmError  # noqa: E402

pytestmark = pytest.mark.gpu
PLM_EINVAL, PLM_EUNSUPPORTED = -1, -4
ARRAYS = ("weights", "fi", "fij", "hi", "jij", "jij_full", "di")


@pytest.fixture(scope="module")
def plm():
    from evcouplings_amd import plm as _plm
    assert _plm.device_count() >= 1, "no gfx950 device: the HIP path has no fallback"
    return _plm


class Run:
    """one plm.mean_field call on a planted alignment and, computed on first use, the references of its stages"""

    def __init__(self, plm, q, L, N, pc):
        self.q, self.L, self.N, self.pc, self.n = q, L, N, pc, L * (q - 1)
        self.out = plm.mean_field(tw.planted_msa(q, L, N), q, theta_id=tw.THETA, pseudo_count=pc)
        self.fi = self.out["fi"].astype(np.float64)
        self.rfi = (1.0 - pc) * self.fi + pc / q
        self._inv = self._di = None

    def inverse(self):
        if self._inv is None:
            C = tw.covariance(self.fi, self.out["fij"].astype(np.float64), self.pc)
            ext = tw.inverse_extended(C)
            self._inv = (ext, tw.inverse_errors(C, ext), float(np.linalg.cond(C)))
        return self._inv

    def di(self):
        if self._di is None:
            with np.errstate(all="ignore"):
                self._di = tw.direct_information_traced(self.out["jij_full"], self.rfi)
        return self._di


def check_inverse(run):
    q, L, n = run.q, run.L, run.n
    J = run.out["jij_full"]
    ext, (err_lu, err_chol), cond = run.inverse()
    got = -J[:, :, :q - 1, :q - 1].transpose(0, 2, 1, 3).reshape(n, n)
    err = float(np.abs(got - ext).max() / np.abs(ext).max())
    yard = max(err_lu, err_chol, 2.0 ** -52)
    print("INVERSE q=%d L=%d N=%d pc=%g n=%d cond=%.3g err_gpu=%.3g err_lu=%.3g err_chol=%.3g ratio=%.3g"
          % (q, L, run.N, run.pc, n, cond, err, err_lu, err_chol, err / yard))
    assert np.isfinite(J).all()
    assert err <= tw.inverse_bound(err_lu, err_chol)
    assert not J[:, :, q - 1, :].any() and not J[:, :, :, q - 1].any()
    assert np.array_equal(J, J.transpose(1, 0, 3, 2))          # X^T X sums (r, c) and (c, r) in the same order


def check_extract(run):
    iu, ju = np.triu_indices(run.L, 1)
    assert run.out["jij"].dtype == np.float32
    assert np.array_equal(run.out["jij"], run.out["jij_full"][iu, ju].astype(np.float32))


def check_fields(run):
    h, B = tw.fields_from(run.out["jij_full"], run.rfi)
    delta = np.abs(run.out["hi"] - h)
    bound = tw.fields_bound(B, run.rfi, run.n)
    share = np.divide(delta, bound, out=np.zeros_like(delta), where=bound > 0)
    print("FIELDS q=%d L=%d N=%d pc=%g max|dh|=%.3g largest share of the bound=%.3g"
          % (run.q, run.L, run.N, run.pc, delta.max(), share.max()))
    assert (delta <= bound).all()
    assert not run.out["hi"][:, run.q - 1].any()


def check_di(run):
    di = run.out["di"]
    want, iters, gap = run.di()
    case = (run.q, run.L, run.N, run.pc)
    assert tw.ambiguous_pairs(gap) == []
    assert iters.max() < tw.DI_UPDATE_CAP                      # the kernel's loop is capped, the oracle's is not
    print("DI q=%d L=%d N=%d pc=%g max|ddi|=%.3g longest loop=%d"
          % (case + (np.nanmax(np.abs(di - want)), iters.max())))
    np.testing.assert_allclose(di, want, rtol=0, atol=1e-10)
    assert np.isfinite(want).all() == (case not in tw.DI_OVERFLOWS)
    assert np.array_equal(di, di.T, equal_nan=True) and not di.diagonal().any()
    assert np.nanargmax(di) == np.nanargmax(want)              # the top pair is the oracle's, in every case
    if case not in tw.ORACLE_COPY_NOT_ON_TOP:                  # see meanfield_twin.ORACLE_COPY_NOT_ON_TOP
        (a, b), _ = tw.planted_pairs(run.L)
        assert di[a, b] == np.nanmax(di)


# ---------------------------------------------------------------- (a) every block geometry of the inverse
@pytest.fixture(scope="module", params=tw.GEOMETRY_CASES, ids=lambda c: "q%d-L%d-N%d" % c)
def geometry(request, plm):
    return Run(plm, *request.param, 0.5)


def test_geometry_inverse(geometry):
    check_inverse(geometry)


def test_geometry_extract(geometry):
    check_extract(geometry)


def test_geometry_fields(geometry):
    check_fields(geometry)


def test_geometry_di(geometry):
    check_di(geometry)


# ---------------------------------------------------------------- (b) conditioning
@pytest.fixture(scope="module", params=tw.CONDITIONING_CASES, ids=lambda c: "q%d-L%d-N%d-pc%g" % c)
def conditioning(request, plm):
    return Run(plm, *request.param)


def test_conditioning_inverse(conditioning):
    check_inverse(conditioning)


def test_conditioning_extract(conditioning):
    check_extract(conditioning)


def test_conditioning_fields(conditioning):
    check_fields(conditioning)


def test_conditioning_di(conditioning):
    check_di(conditioning)


# ---------------------------------------------------------------- (c) plm_direct_information on its own
@pytest.mark.parametrize("q,L", tw.DI_MODEL_CASES)
def test_direct_information_outside_the_gauge(plm, q, L):
    J, rfi, (i, j) = tw.random_di_model(q, L)
    want, iters, gap = tw.direct_information_traced(J, rfi)
    assert tw.ambiguous_pairs(gap) == [] and iters.max() < tw.DI_UPDATE_CAP
    di = plm.direct_information(J, rfi)
    np.testing.assert_allclose(di, want, rtol=0, atol=1e-10)
    assert np.array_equal(di, di.T) and not di.diagonal().any()
    if L > 2:                                                  # with one pair the strong pair is the median
        assert iters[i, j] > np.median(iters[np.triu_indices(L, 1)])


# ---------------------------------------------------------------- (d) optional outputs and determinism
def options_call(plm, **kw):
    q, L, N = tw.OPTIONS_CASE
    return plm.mean_field(tw.planted_msa(q, L, N), q, theta_id=tw.THETA, pseudo_count=0.5, **kw)


def assert_same_bits(got, full, absent=()):
    for name in ARRAYS:
        if name in absent:
            assert name not in got
        else:
            assert got[name].dtype == full[name].dtype and np.array_equal(got[name], full[name]), name
    assert got["n_eff"] == full["n_eff"]


@pytest.fixture(scope="module")
def full_call(plm):
    return options_call(plm)


def test_two_full_calls_are_bit_identical(plm, full_call):
    assert_same_bits(options_call(plm), full_call)


@pytest.mark.parametrize("drop", [("fij",), ("jij_full",), ("di",), ("fij", "jij_full", "di")], ids="+".join)
def test_optional_outputs_do_not_change_the_others(plm, full_call, drop):
    got = options_call(plm, want_fij="fij" not in drop, want_full="jij_full" not in drop, want_di="di" not in drop)
    assert_same_bits(got, full_call, absent=drop)


# ---------------------------------------------------------------- (e) refusals leave the device usable
@pytest.mark.parametrize("q,L,code", [(33, 3, PLM_EUNSUPPORTED), (1, 3, PLM_EUNSUPPORTED), (5, 1, PLM_EINVAL)])
def test_direct_information_refusals(plm, full_call, q, L, code):
    with pytest.raises(PlmError) as e:
        plm.direct_information(np.zeros((L, L, q, q)), np.full((L, q), 1.0 / q))
    assert e.value.code == code
    assert_same_bits(options_call(plm), full_call)


def test_direct_information_with_overflowing_couplings(plm, full_call):
    """exp(800) = inf in one pair's block: that pair's DI is NaN, as the oracle's, through the !(diff > 1e-4) exit of
    the loop; every other pair is untouched"""
    J, rfi, bad = tw.overflowing_di_model()
    with np.errstate(all="ignore"):
        want, iters, gap = tw.direct_information_traced(J, rfi)
    assert np.isnan(want[bad]) and tw.ambiguous_pairs(gap) == []
    di = plm.direct_information(J, rfi)
    np.testing.assert_allclose(di, want, rtol=0, atol=1e-10, equal_nan=True)
    assert np.isnan(di[bad]) and np.isfinite(di).sum() == di.size - 2
    assert_same_bits(options_call(plm), full_call)


def test_singular_alignment_is_refused_or_solved(plm, full_call):
    """50 identical sequences at a pseudo-count of 1e-12: the covariance matrix is positive definite only up to the
    float32 rounding of the frequencies.  Either the factorisation meets a non-positive pivot and the call is refused
    with PLM_EINVAL naming it, or it returns; the next call computes what it always computed."""
    msa = np.tile(np.arange(8, dtype=np.int8) % 21, (50, 1))
    try:
        out = plm.mean_field(msa, 21, theta_id=tw.THETA, pseudo_count=1e-12)
    except PlmError as e:
        assert e.code == PLM_EINVAL and "pivot" in str(e)
    else:
        assert out["jij_full"].shape == (8, 8, 21, 21) and out["n_eff"] == pytest.approx(1.0)
    assert_same_bits(options_call(plm), full_call)
