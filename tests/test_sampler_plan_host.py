"""The launch planner of the Gibbs sampler (plm_sample_plan / plm.sample_plan, DESIGN_NEXT_ROWS.md section 9.6) on the
host: with a CU count given the call is pure host code, so every plan the library can make is checked here without a
device -- its invariants over a sweep of shapes, the documented plans, the environment hooks, and which instantiations
of k_gibbs and k_gibbs_direct the case matrix of tests/test_gpu_sampler_plans.py reaches."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_plan_cases as cases  # noqa: E402
from evcouplings_amd import _lib, plm  # noqa: E402

QS = range(2, 33)
LS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 31, 32, 33, 37, 64, 300, 604, 605, 620, 636, 637, 1208, 1240, 1276, 1277,
      2416, 2484, 2556, 2557, 2600, 40000)
CS = (1, 63, 64, 65, 16384, 32767, 32768, 65535, 65536, 1 << 18)
CUS = (1, 64, 256, 304)
GS_PF = 8
LDS = cases.LDS_OF_A_CU
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for name in ("PLM_SAMPLE_FORM", "PLM_SAMPLE_TILE", "PLM_SAMPLE_JC"):
        monkeypatch.delenv(name, raising=False)


def _ceil(a, b):
    return -(-a // b)


def _group(L, q):
    """Lanes per chain of the direct form: the smallest power of two >= q whose 256 / group chains fit the LDS (32 if
    none does)."""
    for g in (2, 4, 8, 16, 32):
        if g >= q and (256 // g) * 4 * _ceil(L, 4) <= LDS:
            return g
    return 32


def _tiled_lds(L, q, tile, jc):
    nv = _ceil(q, 4)
    nvp = nv + 1 if nv % 2 == 0 else nv
    return 2 * jc * q * nvp * 16 + _ceil(L, 4) * tile * 4


def _valid(L, q, tile, jc):
    return jc * q * _ceil(q, 4) <= GS_PF * tile and _tiled_lds(L, q, tile, jc) <= LDS


def _plan_before_the_hooks(L, q, C, n_cu):
    """make_plan as it stood before PLM_SAMPLE_TILE / PLM_SAMPLE_JC existed, line for line: (tile, jc) or None."""
    nv = _ceil(q, 4)
    for t, tile in enumerate((256, 128, 64)):
        if t < 2 and _ceil(C, tile) < n_cu:
            continue
        for jc in (16, 12, 8, 4, 2, 1):
            if jc > 1 and jc >= 2 * L:
                continue
            if jc * q * nv > GS_PF * tile:
                continue
            if _tiled_lds(L, q, tile, jc) <= LDS:
                return tile, jc
    for tile in (128, 64):
        for jc in (16, 12, 8, 4, 2, 1):
            if jc * q * nv > GS_PF * tile:
                continue
            if _tiled_lds(L, q, tile, jc) <= LDS:
                return tile, jc
    return None


def _raw(L, q, C, n_cu):
    info = _lib.PlmSamplePlanInfo()
    rc = _lib.load().plm_sample_plan(L, q, C, n_cu, info)
    return rc, info


def test_every_plan_of_the_sweep_is_valid_and_the_one_made_before_the_hooks():
    seen = {"tiled": 0, "direct": 0, "unsupported": 0}
    for q, L, C, n_cu in itertools.product(QS, LS, CS, CUS):
        rc, p = _raw(L, q, C, n_cu)
        where = (L, q, C, n_cu)
        tiled_exists = any(_valid(L, q, tile, jc) for tile in cases.TILES for jc in cases.CHUNKS)
        direct_lds = (256 // _group(L, q)) * 4 * _ceil(L, 4)
        if rc != 0:
            assert rc == EUNSUPPORTED, where
            assert not tiled_exists and direct_lds > LDS, where
            assert _plan_before_the_hooks(L, q, C, n_cu) is None, where
            seen["unsupported"] += 1
            continue
        assert p.nv == _ceil(q, 4), where
        if p.direct:
            assert not tiled_exists, where
            assert _plan_before_the_hooks(L, q, C, n_cu) is None, where
            assert p.lds_bytes == direct_lds <= LDS, where
            assert p.tile == 256 // _group(L, q) and p.jc == 0, where
            seen["direct"] += 1
        else:
            assert p.tile in cases.TILES and p.jc in cases.CHUNKS, where
            assert p.jc * q * p.nv <= GS_PF * p.tile, where
            assert p.lds_bytes == _tiled_lds(L, q, p.tile, p.jc) <= LDS, where
            assert (p.tile, p.jc) == _plan_before_the_hooks(L, q, C, n_cu), where
            seen["tiled"] += 1
        assert p.n_workgroups == _ceil(C, p.tile), where
    print(seen)
    assert min(seen.values()) > 0, seen


def test_every_plan_names_an_instantiated_kernel():
    """The dispatch of plm_sample_internal.h turns (direct, tile, nv) into template arguments and knows k_gibbs / k_ais
    <NV 1..8, TILE 64 | 128 | 256> and k_gibbs_direct / k_ais_direct <QP 2 | 4 | 8 | 16 | 32> only: the planner must not
    return anything else, for any alphabet, on either side of the hand-over from the tiled to the direct form (L = 2484 /
    2485 at q = 21, up to 2556 / 2557 at q = 2) and at a length only the direct form serves."""
    tiled = {(nv, tile) for nv in range(1, 9) for tile in (64, 128, 256)}
    groups = {2, 4, 8, 16, 32}
    seen = set()
    for q, L, (C, n_cu) in itertools.product(QS, (1, 37, 300, 2416, 2484, 2485, 2556, 2557, 20480),
                                             ((300, 256), (40000, 256), (65536, 64))):
        p = plm.sample_plan(L, q, C, n_cu=n_cu)
        where = (L, q, C, n_cu, p)
        if p["direct"]:
            assert 256 % p["tile"] == 0 and 256 // p["tile"] in groups and 256 // p["tile"] >= q, where
        else:
            assert (p["nv"], p["tile"]) in tiled, where
        assert p["nv"] == _ceil(q, 4) and 0 < p["lds_bytes"] <= 163840, where
        seen.add(p["direct"])
        if L == 20480:
            assert p["direct"], where
    assert seen == {False, True}


def test_documented_plans():
    """The plans DESIGN_NEXT_ROWS.md section 9.6 states, on 256 CUs."""
    big = plm.sample_plan(300, 21, 65536, n_cu=256)      # 76.8 KB of states + 75 KB of staging, k_gibbs<6, 256>
    assert big == dict(direct=False, tile=256, jc=16, nv=6, n_workgroups=256, lds_bytes=76800 + 75264)
    assert plm.sample_plan(100, 21, 65536, n_cu=256) == dict(direct=False, tile=256, jc=16, nv=6, n_workgroups=256,
                                                             lds_bytes=25 * 1024 + 75264)
    small = plm.sample_plan(600, 21, 16384, n_cu=256)    # "at C = 16 384 the tile is 64 chains"
    assert small == dict(direct=False, tile=64, jc=4, nv=6, n_workgroups=256, lds_bytes=150 * 256 + 18816)
    # a tile is taken once its workgroups, the partial one included, are as many as the CUs
    for C, tile in ((255 * 128, 64), (255 * 128 + 1, 128), (32768, 128), (255 * 256, 128), (255 * 256 + 1, 256),
                    (65536, 256)):
        assert plm.sample_plan(300, 21, C, n_cu=256)["tile"] == tile, C
    # the tiled form ends where the states of 64 chains no longer fit beside one staged site: L = 2484 at q = 21
    assert plm.sample_plan(2484, 21, 4096, n_cu=256) == dict(direct=False, tile=64, jc=1, nv=6, n_workgroups=64,
                                                             lds_bytes=621 * 256 + 4704)
    assert plm.sample_plan(2485, 21, 4096, n_cu=256) == dict(direct=True, tile=8, jc=0, nv=6, n_workgroups=512,
                                                             lds_bytes=8 * 2488)
    assert plm.sample_plan(2600, 9, 4096, n_cu=256)["direct"]          # test_long_model_runs_on_the_direct_form
    # a length of one site stages that site alone
    assert plm.sample_plan(1, 7, 1000, n_cu=256)["jc"] == 1


def test_whole_lds_plans():
    """q = 2 needs exactly the LDS of a CU at L = 636 / 1276 / 2556 on tile 256 / 128 / 64; one site more does not fit."""
    for (L, tile, C) in cases.FULL_LDS[:3]:
        with cases.forced(tile=tile):
            p = plm.sample_plan(L, 2, C, n_cu=cases.REFERENCE_CUS)
        assert not p["direct"] and p["tile"] == (tile or 64) and p["lds_bytes"] == LDS, (L, p)
        if tile:
            with cases.forced(tile=tile), pytest.raises(_lib.PlmError) as err:
                plm.sample_plan(L + 1, 2, C, n_cu=cases.REFERENCE_CUS)
            assert err.value.code == EINVAL and "PLM_SAMPLE_TILE" in str(err.value)
    L, tile, C = cases.FULL_LDS[3]
    assert tile is None and plm.sample_plan(L, 2, C, n_cu=cases.REFERENCE_CUS) == dict(
        direct=True, tile=64, jc=0, nv=1, n_workgroups=2, lds_bytes=LDS)       # groups of 4 lanes: 128 chains do not fit


def test_hooks_choose_among_the_valid_plans_only():
    L, q, C = 37, 21, 300
    natural = plm.sample_plan(L, q, C, n_cu=256)
    assert (natural["tile"], natural["jc"]) == (64, 4)
    for tile in cases.TILES:
        for jc in cases.CHUNKS:
            with cases.forced(tile=tile, jc=jc):
                if _valid(L, q, tile, jc):
                    p = plm.sample_plan(L, q, C, n_cu=256)
                    assert (p["direct"], p["tile"], p["jc"]) == (False, tile, jc)
                    assert p["lds_bytes"] == _tiled_lds(L, q, tile, jc) and p["n_workgroups"] == _ceil(C, tile)
                else:
                    with pytest.raises(_lib.PlmError) as err:
                        plm.sample_plan(L, q, C, n_cu=256)
                    assert err.value.code == EINVAL
                    assert "PLM_SAMPLE_TILE" in str(err.value) and "PLM_SAMPLE_JC" in str(err.value)
    # one hook alone: the other choice stays the planner's
    with cases.forced(tile=256):
        assert plm.sample_plan(L, q, C, n_cu=256)["jc"] == 16
    with cases.forced(jc=2):
        p = plm.sample_plan(L, q, C, n_cu=256)
        assert (p["tile"], p["jc"]) == (64, 2)
    with cases.forced(jc=8), pytest.raises(_lib.PlmError) as err:       # 8 x 21 x 6 float4 > 8 x 64
        plm.sample_plan(L, q, C, n_cu=256)
    assert err.value.code == EINVAL and "PLM_SAMPLE_JC" in str(err.value) and "PLM_SAMPLE_TILE" not in str(err.value)
    with cases.forced(jc=16):                                            # a forced chunk may be longer than the model
        assert plm.sample_plan(3, 3, C, n_cu=256)["jc"] == 16
    # values outside the sets
    for name, bad in (("PLM_SAMPLE_TILE", "100"), ("PLM_SAMPLE_TILE", "64x"), ("PLM_SAMPLE_TILE", "-64"),
                      ("PLM_SAMPLE_JC", "3"), ("PLM_SAMPLE_JC", "0"), ("PLM_SAMPLE_JC", "sixteen")):
        with cases.forced(**{"tile" if name.endswith("TILE") else "jc": bad}), pytest.raises(_lib.PlmError) as err:
            plm.sample_plan(L, q, C, n_cu=256)
        assert err.value.code == EINVAL and name in str(err.value), (name, bad)
    # the direct form has no tile to force; the tiled form on request does not fall over to the direct one
    with cases.forced(tile=256, jc=16, form="direct"):
        assert plm.sample_plan(L, q, C, n_cu=256) == dict(direct=True, tile=8, jc=0, nv=6, n_workgroups=38, lds_bytes=8 * 40)
    with cases.forced(form="tiled"), pytest.raises(_lib.PlmError) as err:
        plm.sample_plan(2600, 9, C, n_cu=256)
    assert err.value.code == EUNSUPPORTED
    assert plm.sample_plan(L, q, C, n_cu=256) == natural


def test_arguments():
    for args, code in (((0, 21, 8, 256), EINVAL), ((5, 21, 0, 256), EINVAL), ((5, 1, 8, 256), EUNSUPPORTED),
                       ((5, 33, 8, 256), EUNSUPPORTED)):
        assert _raw(*args)[0] == code, args
    assert _lib.load().plm_sample_plan(5, 21, 8, 256, None) == EINVAL


def test_the_gpu_case_matrix_reaches_every_instantiation():
    """tests/test_gpu_sampler_plans.py launches all 24 k_gibbs<NV, TILE>, every chunk length and every k_gibbs_direct<QP>:
    computed from the plans its cases get on the reference device."""
    n_cu = cases.REFERENCE_CUS
    pairs, chunks, groups = set(), set(), set()
    for tile, L, q, C in cases.width_cases():
        with cases.forced(tile=tile):
            p = plm.sample_plan(L, q, C, n_cu=n_cu)
        assert (p["direct"], p["tile"], p["jc"], p["n_workgroups"]) == (False, tile, cases.WIDTH_JC[tile][q], 2), (tile, q, p)
        pairs.add((p["nv"], p["tile"]))
        chunks.add(p["jc"])
        with cases.forced(form="direct"):
            d = plm.sample_plan(L, q, C, n_cu=n_cu)
        assert d["direct"] and C % d["tile"] != 0                       # a partial last workgroup
        groups.add(256 // d["tile"])
    for q, accepted in cases.CHUNK_QS.items():
        assert accepted == tuple(jc for jc in cases.CHUNKS if _valid(max(cases.CHUNK_LS), q, 64, jc)), q
    depth = 3                                                           # GS_DEPTH
    geometry = set()
    for jc, L, q, C in cases.chunk_cases():
        with cases.forced(tile=64, jc=jc):
            p = plm.sample_plan(L, q, C, n_cu=n_cu)
        assert (p["direct"], p["tile"], p["jc"], p["n_workgroups"]) == (False, 64, jc, 2), (jc, L, q, p)
        pairs.add((p["nv"], p["tile"]))
        chunks.add(p["jc"])
        n_chunks = _ceil(L, jc)
        geometry.add(("single chunk", n_chunks == 1))
        geometry.add(("shorter than the chunk", L < jc))
        geometry.add(("no group of four sites", L < 4))
        geometry.add(("fewer chunks than the depth", n_chunks < depth))
        geometry.add(("more than two rounds of the depth", n_chunks > 2 * depth))
        geometry.add(("partial last chunk", L % jc != 0))
        geometry.add(("chunks of 12", jc == 12 and n_chunks > 1))
        geometry.add(("tail of single sites after groups of four", jc >= 4 and L % jc % 4 != 0 and L > 4))
    assert {name for name, hit in geometry if hit} == {name for name, _ in geometry}, sorted(geometry)
    for L, tile, C in cases.FULL_LDS:
        with cases.forced(tile=tile):
            p = plm.sample_plan(L, 2, C, n_cu=n_cu)
        pairs.add((p["nv"], p["tile"])) if not p["direct"] else groups.add(256 // p["tile"])
    assert pairs == {(nv, tile) for nv in range(1, 9) for tile in cases.TILES}, sorted(pairs)
    assert chunks == set(cases.CHUNKS), sorted(chunks)
    assert groups == {2, 4, 8, 16, 32}, sorted(groups)
    # the natural plans of (d) are the two larger tiles on the reference device
    tiles = [plm.sample_plan(cases.NATURAL_L, cases.NATURAL_Q, C, n_cu=n_cu)["tile"] for C in cases.NATURAL_CS]
    assert tiles == [128, 256]
