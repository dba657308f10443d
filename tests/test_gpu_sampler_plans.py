"""Every launch plan of the Gibbs sampler on the MI355X (DESIGN_NEXT_ROWS.md section 9.6): the 24 instantiations
k_gibbs<NV, TILE>, every chunk length, the five k_gibbs_direct<QP>, plans that take the whole LDS of a CU, the hand-over
to the direct form, and the plans the device gets without a hook.  Each case follows the float64 twin
(tests/sampler_twin.py) draw for draw, and the direct form bit for bit.  The plans are forced with PLM_SAMPLE_TILE /
PLM_SAMPLE_JC / PLM_SAMPLE_FORM and read back with plm.sample_plan; tests/sampler_plan_cases.py holds the case matrix and
tests/test_sampler_plan_host.py asserts what it reaches."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_plan_cases as cases  # noqa: E402
import sampler_twin as tw  # noqa: E402
from test_gpu_sampler import _explained, _random_model, _twin_sweeps  # noqa: E402
from evcouplings_amd import _lib, plm  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 0.01                                # of the chains may differ from the float64 twin at all


def _differing(gpu, twin):
    return int((np.asarray(gpu, np.int64) != twin).any(axis=(0, 2)).sum())


def _ran(L, q, Cn, **want):
    """The plan the library makes under the hooks in force, against the one the case is about."""
    p = plm.sample_plan(L, q, Cn)
    assert {k: p[k] for k in want} == want, (L, q, Cn, p)
    return p


@pytest.mark.parametrize("tile", cases.TILES)
def test_every_row_width_on_a_forced_tile(tile):
    """k_gibbs<1 .. 8, tile> and k_gibbs_direct<2 .. 32>, two workgroups, 37 live lanes in the second."""
    L = cases.WIDTH_L
    differ = {"sweeps from start states": 0, "start rule, masks and temperature": 0}
    chains = 0
    for q in cases.WIDTH_QS:
        Cn = tile + 37
        name = "tile %d q=%d" % (tile, q)
        rng = np.random.default_rng(7000 + q + tile)
        h, J = _random_model(rng, L, q)
        x0 = rng.integers(0, q, size=(Cn, L))
        seed = 4242 + q
        W = tw.dense(J, L, q)
        fixed = (np.arange(L) % 5 == 2).astype(np.uint8)
        allowed = ((np.arange(q) != 1) | (q == 2)).astype(np.uint8)        # two states: nothing to forbid
        first = dict(burn_in=1, n_snapshots=2, thin=1, seed=seed, start=x0, energies=False)
        second = dict(burn_in=0, n_snapshots=3, thin=1, seed=seed, beta=1.3, fixed=fixed, allowed=allowed, energies=False)
        with cases.forced(tile=tile):
            _ran(L, q, Cn, direct=False, tile=tile, jc=cases.WIDTH_JC[tile][q], nv=(q + 3) // 4, n_workgroups=2)
            gpu1 = plm.sample(h, J, q, Cn, **first)[0]
            gpu2 = plm.sample(h, J, q, Cn, **second)[0]
        with cases.forced(form="direct"):
            assert Cn % _ran(L, q, Cn, direct=True)["tile"] != 0           # a partial last workgroup
            dir1 = plm.sample(h, J, q, Cn, **first)[0]
            dir2 = plm.sample(h, J, q, Cn, **second)[0]
        # two sweeps from given states
        twin, margin, maxbu = _twin_sweeps(h, W, x0, seed, 2)
        _explained(name, gpu1.astype(np.int64), twin, margin, maxbu, L, q, cap=1.0)
        differ["sweeps from start states"] += _differing(gpu1, twin)
        assert np.array_equal(gpu1, dir1), name
        # the start rule, then two sweeps, with fixed sites, a forbidden state and beta = 1.3
        twin = np.zeros((3, Cn, L), np.int64)
        margin, maxbu = np.ones((3, Cn, L)), np.zeros((3, Cn, L))
        x = tw.start_states(h, Cn, seed, 1.3, allowed, margin=margin[0], maxbu=maxbu[0])
        twin[0] = x
        for s in range(2):
            tw.sweep(x, h, W, seed, s, 1.3, fixed, allowed, margin=margin[s + 1], maxbu=maxbu[s + 1])
            twin[s + 1] = x
        _explained(name + " start rule, masks", gpu2.astype(np.int64), twin, margin, maxbu, L, q, cap=1.0)
        differ["start rule, masks and temperature"] += _differing(gpu2, twin)
        assert np.array_equal(gpu2, dir2), name
        assert (gpu2[:, :, fixed.astype(bool)] == gpu2[0][None][:, :, fixed.astype(bool)]).all()
        assert q == 2 or not (gpu2 == 1).any()
        assert (gpu2[2] != gpu2[0]).any(axis=1).mean() > 0.9
        chains += Cn
    print("tile %d: %s of %d chains differ from the twin" % (tile, differ, chains))
    for what, n in differ.items():
        assert n <= CAP * chains, (what, n, chains)


@pytest.mark.parametrize("q", sorted(cases.CHUNK_QS))
def test_chunk_geometry(q):
    """Tile 64, every chunk length the planner accepts, at lengths below, at and above it: single chunks, chunks longer
    than the model, no group of four sites, more than two rounds of the pipeline depth, chunks that start at multiples
    of 12.  The chunk does not enter the contract: every run equals the direct form bit for bit."""
    Cn = cases.CHUNK_C
    differ = chains = 0
    for L in cases.CHUNK_LS:
        rng = np.random.default_rng(8000 + 100 * q + L)
        h, J = _random_model(rng, L, q)
        x0 = rng.integers(0, q, size=(Cn, L))
        seed = 99 + L
        kw = dict(burn_in=1, n_snapshots=2, thin=1, seed=seed, start=x0, energies=False)
        with cases.forced(form="direct"):
            _ran(L, q, Cn, direct=True)
            direct = plm.sample(h, J, q, Cn, **kw)[0]
        twin, margin, maxbu = _twin_sweeps(h, tw.dense(J, L, q), x0, seed, 2)
        _explained("q=%d L=%d" % (q, L), direct.astype(np.int64), twin, margin, maxbu, L, q, cap=1.0)
        differ += _differing(direct, twin)
        chains += Cn
        for jc in cases.CHUNK_QS[q]:
            with cases.forced(tile=64, jc=jc):
                _ran(L, q, Cn, direct=False, tile=64, jc=jc, n_workgroups=2)
                tiled = plm.sample(h, J, q, Cn, **kw)[0]
            assert np.array_equal(tiled, direct), (q, L, jc, np.argwhere(tiled != direct)[:5])
    print("q=%d: %d of %d chains differ from the twin" % (q, differ, chains))
    assert differ <= CAP * chains, (differ, chains)


@pytest.mark.parametrize("L,tile,Cn", cases.FULL_LDS)
def test_whole_lds_of_a_cu_and_the_hand_over_to_the_direct_form(L, tile, Cn):
    """q = 2: three plans of exactly 163 840 bytes of LDS, and the length one beyond the last of them, which runs on
    the direct form (its chain states take the whole LDS too).  One sweep, draw for draw."""
    q = 2
    rng = np.random.default_rng(9000 + L)
    h, J = _random_model(rng, L, q)
    x0 = rng.integers(0, q, size=(Cn, L))
    with cases.forced(tile=tile):
        if L == 2557:
            _ran(L, q, Cn, direct=True, tile=64, lds_bytes=cases.LDS_OF_A_CU)
        else:
            _ran(L, q, Cn, direct=False, tile=tile or 64, n_workgroups=2, lds_bytes=cases.LDS_OF_A_CU)
        gpu = plm.sample(h, J, q, Cn, burn_in=1, seed=L, start=x0, energies=False)[0]
    twin, margin, maxbu = _twin_sweeps(h, tw.dense(J, L, q), x0, L, 1)
    assert (twin[0] != x0).any(axis=1).all()
    _explained("q=2 L=%d tile %s" % (L, tile), gpu.astype(np.int64), twin, margin, maxbu, L, q, cap=CAP)


def test_a_uniform_that_would_round_to_one():
    """Seed 9, chain 722, sweep 0, site 32: all 24 bits of the word are set, and ((word0 >> 8) + 0.5) 2^-24 rounds to 1
    in float32.  u must stay below 1: with h_i(a_i) = 40 and J = 0 every draw is a_i (the other states weigh e^-40),
    where u = 1 fell through to the last allowed state.  Both forms."""
    L, q, Cn, seed = 33, 21, 1023, 9
    word = tw.philox4x32_10(722, 0, 0, 32, seed, 0)[0]
    assert int(word) >> 8 == 0xFFFFFF
    a = np.random.default_rng(4000 + L).integers(0, q, size=L)
    a[32] = 3                                            # not the last state
    h = np.zeros((L, q), np.float32)
    h[np.arange(L), a] = 40.0
    J = np.zeros((L * (L - 1) // 2, q, q), np.float32)
    x0 = np.random.default_rng(1).integers(0, q, size=(Cn, L))
    for form in ("tiled", "direct"):
        with cases.forced(form=form):
            out = plm.sample(h, J, q, Cn, burn_in=1, seed=seed, start=x0, energies=False)[0]
        assert np.array_equal(out[0], np.tile(a, (Cn, 1))), (form, np.argwhere(out[0] != a)[:5])
    twin, margin, maxbu = _twin_sweeps(h.astype(np.float64), tw.dense(J, L, q), x0, seed, 1)
    assert np.array_equal(twin[0], np.tile(a, (Cn, 1)))


def _compute_units():
    """multiProcessorCount of the current device, asked of the HIP runtime the library has loaded."""
    assert _lib.load().plm_device_count() >= 1
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    dev, n = C.c_int(0), C.c_int(0)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    assert hip.hipDeviceGetAttribute(C.byref(n), 63, dev) == 0        # hipDeviceAttributeMultiprocessorCount
    return n.value


def test_the_plan_the_device_chooses():
    """No hook: the chain counts that take tile 128 and tile 256 on 256 CUs.  The first and the last 300 chains (the
    partial last workgroup among them) follow the twin."""
    n_cu = _compute_units()
    assert 64 <= n_cu <= 512, n_cu
    L, q = cases.NATURAL_L, cases.NATURAL_Q
    rng = np.random.default_rng(77)
    h, J = _random_model(rng, L, q)
    W = tw.dense(J, L, q)
    seen = []
    for Cn in cases.NATURAL_CS:
        with cases.forced():
            p = plm.sample_plan(L, q, Cn)
            assert p == plm.sample_plan(L, q, Cn, n_cu=n_cu)
            tile = 256 if -(-Cn // 256) >= n_cu else 128 if -(-Cn // 128) >= n_cu else 64
            assert (p["direct"], p["tile"], p["n_workgroups"]) == (False, tile, -(-Cn // tile)), (p, n_cu)
            seen.append(tile)
            x0 = rng.integers(0, q, size=(Cn, L))
            gpu = plm.sample(h, J, q, Cn, burn_in=1, seed=Cn, start=x0, energies=False)[0]
        for lo in (0, Cn - 300):
            x = x0[lo:lo + 300].astype(np.int64).copy()
            margin, maxbu = np.ones((1, 300, L)), np.zeros((1, 300, L))
            tw.sweep(x, h, W, Cn, 0, chain0=lo, margin=margin[0], maxbu=maxbu[0])
            _explained("C=%d chains %d.." % (Cn, lo), gpu[:, lo:lo + 300].astype(np.int64), x[None], margin, maxbu, L, q,
                       cap=CAP)
    print("%d CUs: tiles %s" % (n_cu, seen))
    if n_cu == cases.REFERENCE_CUS:
        assert seen == [128, 256]
