"""The case matrix of tests/test_gpu_sampler_plans.py: which shapes run under which forced launch plan of the Gibbs sampler
(PLM_SAMPLE_TILE, PLM_SAMPLE_JC, PLM_SAMPLE_FORM; DESIGN_NEXT_ROWS.md section 9.6).  tests/test_sampler_plan_host.py
computes from it, without a device, which instantiations of k_gibbs and k_gibbs_direct the GPU tests reach.  Not a test
module."""
import contextlib
import os

TILES = (64, 128, 256)
CHUNKS = (1, 2, 4, 8, 12, 16)
LDS_OF_A_CU = 163840
REFERENCE_CUS = 256                       # the CU count the documented plans are stated for

# (a) every row width NV = ceil(q / 4) = 1 .. 8 on every tile: two workgroups, the second with 37 live lanes
WIDTH_QS = (2, 3, 7, 11, 16, 17, 21, 28, 32)
WIDTH_L = 37
# the chunk the planner picks there: the largest of CHUNKS with JC q NV <= 8 tile
WIDTH_JC = {64: {2: 16, 3: 16, 7: 16, 11: 12, 16: 8, 17: 4, 21: 4, 28: 2, 32: 2},
            128: {2: 16, 3: 16, 7: 16, 11: 16, 16: 16, 17: 12, 21: 8, 28: 4, 32: 4},
            256: {2: 16, 3: 16, 7: 16, 11: 16, 16: 16, 17: 16, 21: 16, 28: 8, 32: 8}}

# (b) chunk geometry on tile 64: every chunk the planner accepts (JC q NV <= 512) at lengths below, at and above it
CHUNK_QS = {3: (1, 2, 4, 8, 12, 16), 21: (1, 2, 4)}
CHUNK_LS = (1, 2, 3, 5, 16, 17, 37, 49)
CHUNK_C = 101

# (c) q = 2: (L, forced tile or None, chains).  The first three need exactly the LDS of a CU, the fourth one word more
# of chain states than tile 64 holds: the hand-over to the direct form
FULL_LDS = ((636, 256, 261), (1276, 128, 133), (2556, None, 70), (2557, None, 70))

# (d) the natural plan on the device: tile 128 and tile 256 on 256 CUs
NATURAL_L, NATURAL_Q = 9, 21
NATURAL_CS = (32768 + 37, 65536 + 37)


def width_cases():
    """(tile, L, q, C) of (a)."""
    return [(tile, WIDTH_L, q, tile + 37) for tile in TILES for q in WIDTH_QS]


def chunk_cases():
    """(jc, L, q, C) of (b), all on tile 64."""
    return [(jc, L, q, CHUNK_C) for q, jcs in CHUNK_QS.items() for L in CHUNK_LS for jc in jcs]


@contextlib.contextmanager
def forced(tile=None, jc=None, form=None):
    """The planner's environment hooks set (or, for None, unset) inside the block; the environment as it was after it."""
    names = {"PLM_SAMPLE_TILE": tile, "PLM_SAMPLE_JC": jc, "PLM_SAMPLE_FORM": form}
    before = {k: os.environ.get(k) for k in names}
    try:
        for k, v in names.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
