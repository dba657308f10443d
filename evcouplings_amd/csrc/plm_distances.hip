// plm_distances.hip -- minimum atom-atom distances between the residues of one or two chains (plm_residue_distances)
// and the minimum of many such maps laid over one pair of residue axes (plm_distance_maps_aggregate); contract in
// include/plm_hip.h, notes in DESIGN_NEXT_ROWS.md section 9.18.
//
// A workgroup of 256 threads owns a tile of TR x TC residue pairs (TR TC = 256), one pair per thread.  The atoms of the
// tile's TR row residues and TC column residues pass through LDS in chunks of CH atoms per residue, laid out
// [atom][coordinate][residue]: the TC threads of a row read consecutive doubles of the column chunk and one broadcast
// double of the row chunk.  A residue of any number of atoms takes ceil(atoms / CH) chunks; the chunk loops run to the
// longest residue of the tile, and a thread whose own residues are shorter sits the rest out.  Every thread keeps the
// minimum of the squared distances of its pair; the minimum of correctly rounded values does not depend on the order
// they arrive in, so neither the tile shape nor the chunk length can change a bit of the result.
#include "plm_host_util.h"
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>

typedef unsigned long long u64;

namespace {

constexpr int DM_BLOCK = 256;       // threads per workgroup = residue pairs per tile
constexpr int DM_MAX_SIDE = 64;     // longest side of a tile
constexpr int DM_MAX_CHUNK = 32;    // most atoms per residue in one chunk
constexpr double DM_LARGE = 1e6;    // LARGE_DIST of the reference: the cap, and the distance to an empty residue
constexpr u64 DM_NAN_BITS = 0x7FF8000000000000ull;   // above the pattern of every distance as an unsigned integer

struct DistPlan { int tr, tc, tc_shift, ch; };

// d2 = (dx dx + dy dy) + dz dz, every difference, product and sum rounded once (no fused multiply-add)
__device__ __forceinline__ double pair_d2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double s = xx + yy;
    return s + zz;
}

// one chunk of the atoms of `side` residues into LDS: dst[(atom * 3 + k) * side + residue]
__device__ __forceinline__ void stage_chunk(const double *__restrict__ coords, const int2 *__restrict__ res, int side,
                                            int ch, int c0, double *__restrict__ dst) {
    for (int idx = threadIdx.x; idx < side * ch; idx += DM_BLOCK) {
        const int rr = idx / ch, a = idx - rr * ch;
        const int2 g = res[rr];                      // first atom, number of atoms
        if (c0 + a < g.y) {
            const double *__restrict__ p = coords + 3 * ((size_t)g.x + c0 + a);
            dst[(a * 3 + 0) * side + rr] = p[0];
            dst[(a * 3 + 1) * side + rr] = p[1];
            dst[(a * 3 + 2) * side + rr] = p[2];
        }
    }
}

// The distance of the thread's residue pair of the tile at (i0, j0): min(1e6, sqrt(min d2)).  ri / rj: (first atom,
// number of atoms) of every residue, the number 0 for an empty range.  `compute` = false skips the atoms (counts only).
// Called by every thread of the workgroup; *i_out / *j_out are the thread's residues (they may lie past the end).
__device__ __forceinline__ double tile_distance(const double *__restrict__ ci, const int2 *__restrict__ ri, int ni, int i0,
                                                const double *__restrict__ cj, const int2 *__restrict__ rj, int nj, int j0,
                                                const DistPlan &p, bool compute, double *__restrict__ lds,
                                                int2 *__restrict__ s_r, int2 *__restrict__ s_c, int *i_out, int *j_out) {
    const int t = threadIdx.x;
    if (t < p.tr) s_r[t] = i0 + t < ni ? ri[i0 + t] : make_int2(0, 0);
    if (t >= DM_MAX_SIDE && t < DM_MAX_SIDE + p.tc) {
        const int c = t - DM_MAX_SIDE;
        s_c[c] = j0 + c < nj ? rj[j0 + c] : make_int2(0, 0);
    }
    __syncthreads();
    int max_r = 0, max_c = 0;                        // the same in every thread: the barriers below are uniform
    for (int k = 0; k < p.tr; k++) max_r = max(max_r, s_r[k].y);
    for (int k = 0; k < p.tc; k++) max_c = max(max_c, s_c[k].y);
    const int r = t >> p.tc_shift, c = t & (p.tc - 1);
    *i_out = i0 + r;
    *j_out = j0 + c;
    const int len_r = s_r[r].y, len_c = s_c[c].y;
    double *__restrict__ lr = lds, *__restrict__ lc = lds + (size_t)p.ch * 3 * p.tr;
    double m = INFINITY;
    if (compute) {
        for (int ca = 0; ca < max_r; ca += p.ch) {
            for (int cb = 0; cb < max_c; cb += p.ch) {
                __syncthreads();                     // the chunks of the last round are read
                if (cb == 0) stage_chunk(ci, s_r, p.tr, p.ch, ca, lr);
                stage_chunk(cj, s_c, p.tc, p.ch, cb, lc);
                __syncthreads();
                const int na = min(p.ch, len_r - ca), nb = min(p.ch, len_c - cb);
                for (int a = 0; a < na; a++) {
                    const double ax = lr[(a * 3 + 0) * p.tr + r], ay = lr[(a * 3 + 1) * p.tr + r],
                                 az = lr[(a * 3 + 2) * p.tr + r];
                    for (int b = 0; b < nb; b++) {
                        const double d2 = pair_d2(ax, ay, az, lc[(b * 3 + 0) * p.tc + c], lc[(b * 3 + 1) * p.tc + c],
                                                  lc[(b * 3 + 2) * p.tc + c]);
                        m = d2 < m ? d2 : m;
                    }
                }
            }
        }
    }
    const double d = __builtin_sqrt(m);              // correctly rounded; sqrt(inf) = inf for a pair without atoms
    return d < DM_LARGE ? d : DM_LARGE;
}

// One map: grid (tiles of j, tiles of i).  symmetric: the tiles that lie wholly below the diagonal leave at once, and
// a thread with i <= j stores its value at [i][j] and [j][i].
__global__ __launch_bounds__(DM_BLOCK) void k_dist_pair(const double *__restrict__ ci, const int2 *__restrict__ ri, int ni,
                                                       const double *__restrict__ cj, const int2 *__restrict__ rj, int nj,
                                                       int symmetric, DistPlan p, double *__restrict__ out) {
    extern __shared__ __align__(16) double lds[];
    __shared__ int2 s_r[DM_MAX_SIDE], s_c[DM_MAX_SIDE];
    const int i0 = blockIdx.y * p.tr, j0 = blockIdx.x * p.tc;
    if (symmetric && j0 + p.tc - 1 < i0) return;
    int i, j;
    const double d = tile_distance(ci, ri, ni, i0, cj, rj, nj, j0, p, true, lds, s_r, s_c, &i, &j);
    if (i >= ni || j >= nj || (symmetric && i > j)) return;
    out[(size_t)i * nj + j] = d;
    if (symmetric && i < j) out[(size_t)j * nj + i] = d;
}

__global__ __launch_bounds__(DM_BLOCK) void k_dist_fill(u64 *__restrict__ agg, size_t n) {
    const size_t k = (size_t)blockIdx.x * DM_BLOCK + threadIdx.x;
    if (k < n) agg[k] = DM_NAN_BITS;
}

// Many maps over one pair of axes: workgroup b owns tile b - first_tile[s] of the map s whose range holds b.  A cell
// takes the unsigned minimum of the bit patterns that reach it (distances are >= 0: their patterns order as integers,
// all below the NaN the cells start as) and counts the maps: integer atomics, the same result in every order.
// A map of a chain with itself computes the pairs i <= j and sends each to both of its cells.
__global__ __launch_bounds__(DM_BLOCK) void k_dist_agg(const double *__restrict__ coords, const int2 *__restrict__ res,
                                                      const int32_t *__restrict__ chain_off,
                                                      const int32_t *__restrict__ slot_i, const int32_t *__restrict__ slot_j,
                                                      const int32_t *__restrict__ maps, const int32_t *__restrict__ first_tile,
                                                      int n_maps, int m_j, DistPlan p, u64 *__restrict__ agg,
                                                      int32_t *__restrict__ count) {
    extern __shared__ __align__(16) double lds[];
    __shared__ int2 s_r[DM_MAX_SIDE], s_c[DM_MAX_SIDE];
    const int b = blockIdx.x;
    int lo = 0, hi = n_maps - 1;                     // the last map with first_tile[s] <= b (empty maps own no tile)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first_tile[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int ca = maps[2 * lo], cb = maps[2 * lo + 1];
    const int ra = chain_off[ca], rb = chain_off[cb];
    const int ni = chain_off[ca + 1] - ra, nj = chain_off[cb + 1] - rb;
    const int tiles_j = (nj + p.tc - 1) / p.tc;
    const int tile = b - first_tile[lo];
    const int i0 = (tile / tiles_j) * p.tr, j0 = (tile % tiles_j) * p.tc;
    const int same = ca == cb;
    if (same && j0 + p.tc - 1 < i0) return;
    int i, j;
    const double d = tile_distance(coords, res + ra, ni, i0, coords, res + rb, nj, j0, p, agg != nullptr, lds, s_r, s_c,
                                   &i, &j);
    if (i >= ni || j >= nj || (same && i > j)) return;
    const u64 bits = (u64)__double_as_longlong(d);
    for (int pass = 0; pass < (same && i < j ? 2 : 1); pass++) {
        const int si = slot_i[ra + (pass ? j : i)], sj = slot_j[rb + (pass ? i : j)];
        if (si < 0 || sj < 0) continue;
        const size_t cell = (size_t)si * m_j + sj;
        if (agg) atomicMin(agg + cell, bits);
        if (count) atomicAdd(count + cell, 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------

// PLM_DIST_PLAN: comma-separated tokens that force the launch plan (measurements and tests): t<int> the residues on
// the row side of a tile (4, 8, 16, 32 or 64; the column side is 256 / t), c<int> the atoms of a residue per chunk
// (1..32).  Not set, or a token left out: 16 x 16 tiles, 16 atoms.
int dist_plan(DistPlan *p) {
    int tr = 16, ch = 16;
    const char *v = getenv("PLM_DIST_PLAN");
    if (v) {
        const char *s = v;
        bool ok = *s != 0;
        while (ok && *s) {
            const char kind = *s++;
            char *end = nullptr;
            errno = 0;
            const long x = (*s >= '0' && *s <= '9') ? strtol(s, &end, 10) : -1;
            ok = end && end != s && !errno;
            if (ok && kind == 't') ok = x == 4 || x == 8 || x == 16 || x == 32 || x == 64;
            else if (ok && kind == 'c') ok = x >= 1 && x <= DM_MAX_CHUNK;
            else ok = false;
            if (ok) {
                (kind == 't' ? tr : ch) = (int)x;
                s = end;
                if (*s) { ok = *s == ',' && s[1] != 0; s++; }
            }
        }
        if (!ok)
            return plm_fail(PLM_EINVAL, "PLM_DIST_PLAN must be a comma-separated list of t<4|8|16|32|64> and c<int 1..%d> "
                                        "(got '%s')", DM_MAX_CHUNK, v);
    }
    p->tr = tr;
    p->tc = DM_BLOCK / tr;
    p->tc_shift = 0;
    while ((1 << p->tc_shift) < p->tc) p->tc_shift++;
    p->ch = ch;
    return PLM_OK;
}

size_t dist_lds_bytes(const DistPlan &p) { return sizeof(double) * 3 * (size_t)p.ch * (p.tr + p.tc); }

int dist_check_coords(const double *coords, int32_t n_atoms, const char *what) {
    for (size_t k = 0; k < (size_t)n_atoms * 3; k++)
        if (!std::isfinite(coords[k]))
            return plm_fail(PLM_EINVAL, "%s[%zu][%zu] is not finite", what, k / 3, k % 3);
    return PLM_OK;
}

// (first, last) inclusive -> (first, number of atoms); an empty range (last < first) becomes (0, 0) whatever it names
int dist_ranges(const int32_t *ranges, size_t n_res, int32_t n_atoms, const char *what, std::vector<int2> *out) {
    out->resize(n_res);
    for (size_t r = 0; r < n_res; r++) {
        const int32_t first = ranges[2 * r], last = ranges[2 * r + 1];
        if (last < first) { (*out)[r] = make_int2(0, 0); continue; }
        if (first < 0 || last >= n_atoms)
            return plm_fail(PLM_EINVAL, "%s[%zu] = (%d, %d) reaches outside the %d atoms", what, r, first, last, n_atoms);
        (*out)[r] = make_int2(first, last - first + 1);
    }
    return PLM_OK;
}

}  // namespace

int plm_residue_distances(const double *coords_i, int32_t n_atoms_i, const int32_t *ranges_i, int32_t n_res_i,
                          const double *coords_j, int32_t n_atoms_j, const int32_t *ranges_j, int32_t n_res_j,
                          double *dist_out, int device, void *stream) {
    if (!coords_i || !ranges_i || !dist_out) return plm_fail(PLM_EINVAL, "NULL coordinates, ranges or output");
    if ((coords_j == nullptr) != (ranges_j == nullptr))
        return plm_fail(PLM_EINVAL, "axis j needs both coordinates and ranges, or neither (the symmetric call)");
    const bool symmetric = coords_j == nullptr;
    if (symmetric) { n_atoms_j = n_atoms_i; n_res_j = n_res_i; }
    if (n_atoms_i < 1 || n_res_i < 1 || n_atoms_j < 1 || n_res_j < 1)
        return plm_fail(PLM_EINVAL, "sizes below 1 (atoms %d and %d, residues %d and %d)", n_atoms_i, n_atoms_j, n_res_i,
                        n_res_j);
    DistPlan plan;
    PLM_TRY(dist_plan(&plan));
    if (((long long)n_res_i + plan.tr - 1) / plan.tr > 65535)
        return plm_fail(PLM_EINVAL, "%d residues on axis i are more than 65535 tiles of %d", n_res_i, plan.tr);
    std::vector<int2> res_i, res_j;
    PLM_TRY(dist_ranges(ranges_i, (size_t)n_res_i, n_atoms_i, "ranges_i", &res_i));
    PLM_TRY(dist_check_coords(coords_i, n_atoms_i, "coords_i"));
    if (!symmetric) {
        PLM_TRY(dist_ranges(ranges_j, (size_t)n_res_j, n_atoms_j, "ranges_j", &res_j));
        PLM_TRY(dist_check_coords(coords_j, n_atoms_j, "coords_j"));
    }
    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n_out = (size_t)n_res_i * n_res_j;
    PLM_TRY(plm_check_free(8.0 * (3.0 * n_atoms_i + n_res_i + (symmetric ? 0.0 : 3.0 * n_atoms_j + n_res_j) + (double)n_out),
                           "plm_residue_distances"));
    double *dci = nullptr, *dcj = nullptr, *dout = nullptr;
    int2 *dri = nullptr, *drj = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&dci, (size_t)n_atoms_i * 3));
    PLM_TRY(mem.alloc(&dri, (size_t)n_res_i));
    PLM_TRY(mem.alloc(&dout, n_out));
    PLM_HIP(hipMemcpyAsync(dci, coords_i, sizeof(double) * 3 * n_atoms_i, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dri, res_i.data(), sizeof(int2) * n_res_i, hipMemcpyHostToDevice, st));
    if (symmetric) {
        dcj = dci;
        drj = dri;
    } else {
        PLM_TRY(mem.alloc(&dcj, (size_t)n_atoms_j * 3));
        PLM_TRY(mem.alloc(&drj, (size_t)n_res_j));
        PLM_HIP(hipMemcpyAsync(dcj, coords_j, sizeof(double) * 3 * n_atoms_j, hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(drj, res_j.data(), sizeof(int2) * n_res_j, hipMemcpyHostToDevice, st));
    }
    const dim3 grid((n_res_j + plan.tc - 1) / plan.tc, (n_res_i + plan.tr - 1) / plan.tr);
    hipLaunchKernelGGL(k_dist_pair, grid, dim3(DM_BLOCK), dist_lds_bytes(plan), st, dci, dri, n_res_i, dcj, drj, n_res_j,
                       symmetric ? 1 : 0, plan, dout);
    PLM_HIP(hipGetLastError());
    PLM_HIP(hipMemcpyAsync(dist_out, dout, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_distance_maps_aggregate(const double *coords, int32_t n_atoms, const int32_t *ranges, const int32_t *chain_offsets,
                                int32_t n_chains, const int32_t *slots_i, const int32_t *slots_j, int32_t m_i, int32_t m_j,
                                const int32_t *maps, int32_t n_maps, double *agg, int32_t *count, int device,
                                void *stream) {
    if (!coords || !ranges || !chain_offsets || !slots_i || !maps)
        return plm_fail(PLM_EINVAL, "NULL coordinates, ranges, chain offsets, slots or maps");
    if (n_atoms < 1 || n_chains < 1 || m_i < 1 || m_j < 1 || n_maps < 1)
        return plm_fail(PLM_EINVAL, "sizes below 1 (atoms %d, chains %d, map %d x %d, maps %d)", n_atoms, n_chains, m_i, m_j,
                        n_maps);
    if (chain_offsets[0] != 0) return plm_fail(PLM_EINVAL, "chain_offsets[0] = %d, not 0", chain_offsets[0]);
    for (int c = 0; c < n_chains; c++)
        if (chain_offsets[c + 1] < chain_offsets[c])
            return plm_fail(PLM_EINVAL, "chain_offsets[%d] = %d lies below chain_offsets[%d] = %d", c + 1,
                            chain_offsets[c + 1], c, chain_offsets[c]);
    const int32_t n_res = chain_offsets[n_chains];
    if (n_res < 1) return plm_fail(PLM_EINVAL, "the chains hold no residue");
    if (!slots_j) slots_j = slots_i;
    DistPlan plan;
    PLM_TRY(dist_plan(&plan));
    // slots: -1..M-1, and no two residues of one chain at one slot of an axis
    const int32_t *const slots[2] = {slots_i, slots_j};
    const int32_t m_axis[2] = {m_i, m_j};
    for (int axis = 0; axis < (slots_j == slots_i && m_i == m_j ? 1 : 2); axis++) {
        std::vector<int32_t> owner((size_t)m_axis[axis], -1);     // the chain that last took the slot
        for (int c = 0; c < n_chains; c++)
            for (int32_t r = chain_offsets[c]; r < chain_offsets[c + 1]; r++) {
                const int32_t s = slots[axis][r];
                if (s < -1 || s >= m_axis[axis])
                    return plm_fail(PLM_EINVAL, "slots_%c[%d] = %d outside -1..%d", "ij"[axis], r, s, m_axis[axis] - 1);
                if (s < 0) continue;
                if (owner[s] == c)
                    return plm_fail(PLM_EINVAL, "two residues of chain %d share slot %d of axis %c", c, s, "ij"[axis]);
                owner[s] = c;
            }
    }
    std::vector<int32_t> first_tile((size_t)n_maps + 1, 0);
    long long tiles = 0;
    for (int s = 0; s < n_maps; s++) {
        const int32_t a = maps[2 * s], b = maps[2 * s + 1];
        if (a < 0 || a >= n_chains || b < 0 || b >= n_chains)
            return plm_fail(PLM_EINVAL, "maps[%d] = (%d, %d) names a chain outside 0..%d", s, a, b, n_chains - 1);
        const long long ni = chain_offsets[a + 1] - chain_offsets[a], nj = chain_offsets[b + 1] - chain_offsets[b];
        first_tile[s] = (int32_t)tiles;
        tiles += ((ni + plan.tr - 1) / plan.tr) * ((nj + plan.tc - 1) / plan.tc);
        if (tiles > INT_MAX) return plm_fail(PLM_EINVAL, "the maps take more than 2^31 - 1 tiles");
    }
    first_tile[n_maps] = (int32_t)tiles;
    std::vector<int2> res;
    PLM_TRY(dist_ranges(ranges, (size_t)n_res, n_atoms, "ranges", &res));
    PLM_TRY(dist_check_coords(coords, n_atoms, "coords"));
    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n_out = (size_t)m_i * m_j;
    PLM_TRY(plm_check_free(24.0 * n_atoms + 16.0 * n_res + 4.0 * (n_chains + 1) + 12.0 * n_maps + 4.0 +
                               (agg ? 8.0 : 0.0) * (double)n_out + (count ? 4.0 : 0.0) * (double)n_out,
                           "plm_distance_maps_aggregate"));
    double *dc = nullptr;
    int2 *dr = nullptr;
    int32_t *doff = nullptr, *dsi = nullptr, *dsj = nullptr, *dmaps = nullptr, *dfirst = nullptr, *dcount = nullptr;
    u64 *dagg = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&dc, (size_t)n_atoms * 3));
    PLM_TRY(mem.alloc(&dr, (size_t)n_res));
    PLM_TRY(mem.alloc(&doff, (size_t)n_chains + 1));
    PLM_TRY(mem.alloc(&dsi, (size_t)n_res));
    PLM_TRY(mem.alloc(&dmaps, (size_t)n_maps * 2));
    PLM_TRY(mem.alloc(&dfirst, (size_t)n_maps + 1));
    PLM_HIP(hipMemcpyAsync(dc, coords, sizeof(double) * 3 * n_atoms, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dr, res.data(), sizeof(int2) * n_res, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(doff, chain_offsets, sizeof(int32_t) * ((size_t)n_chains + 1), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dsi, slots_i, sizeof(int32_t) * n_res, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dmaps, maps, sizeof(int32_t) * 2 * n_maps, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dfirst, first_tile.data(), sizeof(int32_t) * ((size_t)n_maps + 1), hipMemcpyHostToDevice, st));
    dsj = dsi;
    if (slots_j != slots_i) {
        PLM_TRY(mem.alloc(&dsj, (size_t)n_res));
        PLM_HIP(hipMemcpyAsync(dsj, slots_j, sizeof(int32_t) * n_res, hipMemcpyHostToDevice, st));
    }
    if (agg) {
        PLM_TRY(mem.alloc(&dagg, n_out));
        hipLaunchKernelGGL(k_dist_fill, dim3((unsigned)((n_out + DM_BLOCK - 1) / DM_BLOCK)), dim3(DM_BLOCK), 0, st, dagg, n_out);
        PLM_HIP(hipGetLastError());
    }
    if (count) {
        PLM_TRY(mem.alloc(&dcount, n_out));
        PLM_HIP(hipMemsetAsync(dcount, 0, sizeof(int32_t) * n_out, st));
    }
    if (tiles > 0 && (agg || count)) {
        hipLaunchKernelGGL(k_dist_agg, dim3((unsigned)tiles), dim3(DM_BLOCK), dist_lds_bytes(plan), st, dc, dr, doff, dsi, dsj,
                           dmaps, dfirst, n_maps, m_j, plan, dagg, dcount);
        PLM_HIP(hipGetLastError());
    }
    if (agg) PLM_HIP(hipMemcpyAsync(agg, dagg, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
    if (count) PLM_HIP(hipMemcpyAsync(count, dcount, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}
