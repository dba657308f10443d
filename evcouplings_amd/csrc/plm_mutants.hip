// plm_mutants.hip -- energy differences of mutants relative to a target sequence, on gfx950 (DESIGN_NEXT_ROWS.md 9.16).
//
// Replaces the per-row numba loop `_delta_hamiltonian` (evcouplings/couplings/model.py:112-176) behind the reference's
// predict_mutation_table, and enumerates all letter combinations at a few sites with the same arithmetic:
//   k_single_tables   S_J, S_h of every (site, letter) from the float32 canonical parameters       -- both entry points
//   k_effects_thread  one thread per variant of at most MU_SHORT substitutions                      -- plm_mutant_effects
//   k_effects_wave    one 64-lane wave per longer variant                                           -- plm_mutant_effects
//   k_scan_gather     the single entries and E tables of the scanned sites, compact                 -- plm_mutant_scan
//   k_scan            one thread per combination: energies, histogram, extremes, compaction         -- plm_mutant_scan
// Everything is float64 on float32 parameters, summed in a fixed order; the only atomics are integer ones (histogram
// counts, the slot counter of the compaction).
#include "plm_host_util.h"
#include <math.h>
#include <limits>

namespace {

#define MU_Q 32                // largest alphabet
#ifndef MU_SHORT
#define MU_SHORT 8             // substitutions a single thread takes; longer variants get a wave each
#endif
#define MU_PAIRS (PLM_SCAN_MAX_SITES * (PLM_SCAN_MAX_SITES - 1) / 2)
#define MU_SCAN_THREADS 256
#define MU_SCAN_ITEMS 16       // combinations per thread the scan grid is sized for

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// number of the block of pair i < j in the canonical order
__device__ __forceinline__ int64_t pair_index(int i, int j, int L) {
    return (int64_t)i * (2 * L - i - 1) / 2 + (j - i - 1);
}

// J_ij(a, b) for i != j in either order: the i > j blocks are the transposes of the stored ones
__device__ __forceinline__ double coupling(const float *__restrict__ J, int L, int q, int i, int j, int a, int b) {
    return i < j ? (double)J[pair_index(i, j, L) * q * q + a * q + b] : (double)J[pair_index(j, i, L) * q * q + b * q + a];
}

// E_ij(a, b) = J_ij(a,b) - J_ij(a,t_j) - J_ij(t_i,b) + J_ij(t_i,t_j)
__device__ __forceinline__ double epistasis(const float *__restrict__ J, int L, int q, int i, int j, int a, int b, int ti,
                                            int tj) {
    return ((coupling(J, L, q, i, j, a, b) - coupling(J, L, q, i, j, a, tj)) - coupling(J, L, q, i, j, ti, b)) +
           coupling(J, L, q, i, j, ti, tj);
}

// One wave per site i, lane a < q: tab[i][a] = (S_J, S_h).  For j < i the stored block (j, i) is read along its row t_j
// (consecutive lanes on consecutive floats), for j > i the block (i, j) along its column t_j.
__global__ __launch_bounds__(64) void k_single_tables(const float *__restrict__ x, const int8_t *__restrict__ target, int L,
                                                     int q, double *__restrict__ tab) {
    const int i = blockIdx.x, a = threadIdx.x;
    if (a >= q) return;
    const float *J = x + (size_t)L * q;
    const int ti = target[i], qq = q * q;
    double sj = 0.0;
    for (int j = 0; j < i; j++) {
        const float *row = J + pair_index(j, i, L) * qq + target[j] * q;
        sj += (double)row[a] - (double)row[ti];
    }
    for (int j = i + 1; j < L; j++) {
        const float *blk = J + pair_index(i, j, L) * qq;
        const int tj = target[j];
        sj += (double)blk[a * q + tj] - (double)blk[ti * q + tj];
    }
    double *o = tab + ((size_t)i * q + a) * 2;
    o[0] = sj;
    o[1] = (double)x[(size_t)i * q + a] - (double)x[(size_t)i * q + ti];
}

__device__ __forceinline__ void write_variant(double *__restrict__ out, uint8_t *__restrict__ status, int64_t v, int code,
                                              double dj, double dh) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    out[v * 3 + 0] = code ? nan : dj + dh;
    out[v * 3 + 1] = code ? nan : dj;
    out[v * 3 + 2] = code ? nan : dh;
    status[v] = (uint8_t)code;
}

// One thread per variant.  A variant of more than L entries is refused here, whatever its length; one of more than
// MU_SHORT valid ones is left to k_effects_wave.  Positions and states are checked before anything is indexed by them.
__global__ __launch_bounds__(256) void k_effects_thread(const float *__restrict__ x, const double *__restrict__ tab,
                                                       const int8_t *__restrict__ target, int L, int q, int64_t n,
                                                       const int64_t *__restrict__ off, const int32_t *__restrict__ pos,
                                                       const int8_t *__restrict__ st, double *__restrict__ out,
                                                       uint8_t *__restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int64_t b = off[v], Ml = off[v + 1] - b;
    if (Ml > L) {
        write_variant(out, status, v, PLM_MUT_ETOOMANY, 0.0, 0.0);
        return;
    }
    if (Ml > MU_SHORT) return;
    const int M = (int)Ml;
    int p[MU_SHORT], s[MU_SHORT], t[MU_SHORT] = {0};
    bool bad_pos = false, bad_st = false, rep = false;
#pragma unroll
    for (int m = 0; m < MU_SHORT; m++) {
        p[m] = m < M ? pos[b + m] : 0;
        s[m] = m < M ? (int)st[b + m] : 0;
        bad_pos |= p[m] < 0 || p[m] >= L;
        bad_st |= s[m] < 0 || s[m] >= q;
    }
#pragma unroll
    for (int m = 1; m < MU_SHORT; m++)
#pragma unroll
        for (int k = 0; k < m; k++) rep |= m < M && p[m] == p[k];
    const int code = bad_pos ? PLM_MUT_EPOSITION : bad_st ? PLM_MUT_ESTATE : rep ? PLM_MUT_EREPEAT : PLM_MUT_OK;
    if (code) {
        write_variant(out, status, v, code, 0.0, 0.0);
        return;
    }
    const float *J = x + (size_t)L * q;
    double dj = 0.0, dh = 0.0;
#pragma unroll
    for (int m = 0; m < MU_SHORT; m++)
        if (m < M) {
            const double *e = tab + ((size_t)p[m] * q + s[m]) * 2;
            dj += e[0];
            dh += e[1];
            t[m] = target[p[m]];
        }
#pragma unroll
    for (int m = 0; m < MU_SHORT - 1; m++)
#pragma unroll
        for (int k = m + 1; k < MU_SHORT; k++)
            if (k < M) dj += epistasis(J, L, q, p[m], p[k], s[m], s[k], t[m], t[k]);
    write_variant(out, status, v, PLM_MUT_OK, dj, dh);
}

// One wave per variant of MU_SHORT < M <= L entries (the host lists them).  Lanes stride over the entries for the checks
// and the single terms, and over the partner n > m of every m for the pair terms; butterfly sums, so every lane holds
// the same total.
__global__ __launch_bounds__(64) void k_effects_wave(const float *__restrict__ x, const double *__restrict__ tab,
                                                    const int8_t *__restrict__ target, int L, int q,
                                                    const int64_t *__restrict__ list, const int64_t *__restrict__ off,
                                                    const int32_t *__restrict__ pos, const int8_t *__restrict__ st,
                                                    double *__restrict__ out, uint8_t *__restrict__ status) {
    const int lane = threadIdx.x;
    const int64_t v = list[blockIdx.x];
    const int64_t b = off[v];
    const int M = (int)(off[v + 1] - b);           // MU_SHORT < M <= L: the host's filter
    int bad_pos = 0, bad_st = 0, rep = 0;
    for (int m = lane; m < M; m += 64) {
        const int pp = pos[b + m], ss = st[b + m];
        bad_pos |= pp < 0 || pp >= L;
        bad_st |= ss < 0 || ss >= q;
    }
    bad_pos = __any(bad_pos);
    bad_st = __any(bad_st);
    if (!bad_pos && !bad_st) {
        for (int m = lane; m < M; m += 64) {
            const int pp = pos[b + m];
            for (int k = 0; k < m; k++) rep |= pos[b + k] == pp;
        }
        rep = __any(rep);
    }
    const int code = bad_pos ? PLM_MUT_EPOSITION : bad_st ? PLM_MUT_ESTATE : rep ? PLM_MUT_EREPEAT : PLM_MUT_OK;
    if (code) {
        if (lane == 0) write_variant(out, status, v, code, 0.0, 0.0);
        return;
    }
    const float *J = x + (size_t)L * q;
    double dj = 0.0, dh = 0.0, de = 0.0;
    for (int m = lane; m < M; m += 64) {
        const double *e = tab + ((size_t)pos[b + m] * q + st[b + m]) * 2;
        dj += e[0];
        dh += e[1];
    }
    for (int m = 0; m < M - 1; m++) {
        const int i = pos[b + m], a = st[b + m], ti = target[i];
        for (int k = m + 1 + lane; k < M; k += 64) {
            const int j = pos[b + k];
            de += epistasis(J, L, q, i, j, a, st[b + k], ti, target[j]);
        }
    }
    dj = wave_sum(dj) + wave_sum(de);
    dh = wave_sum(dh);
    if (lane == 0) write_variant(out, status, v, PLM_MUT_OK, dj, dh);
}

// ---- the scan ---------------------------------------------------------------------------------------------------
// Compact tables of one call, n_tab doubles: the single entries (S_J, S_h) of letter l of site s at 2 (lo[s] + l), then
// for every site pair s < u, in row-major order, a table [nl[s]][nl[u]] of E at poff[scan_pair(s, u)].
struct ScanMeta {
    int k, n_tab;
    int site[PLM_SCAN_MAX_SITES], nl[PLM_SCAN_MAX_SITES], lo[PLM_SCAN_MAX_SITES];
    int poff[MU_PAIRS];
};

// s < u, numbered as among PLM_SCAN_MAX_SITES sites whatever k is (a constant once the loops are unrolled)
__device__ __host__ inline int scan_pair(int s, int u) { return s * (2 * PLM_SCAN_MAX_SITES - s - 1) / 2 + (u - s - 1); }

__global__ __launch_bounds__(256) void k_scan_gather(const float *__restrict__ x, const double *__restrict__ tab,
                                                    const int8_t *__restrict__ target, const int8_t *__restrict__ letters,
                                                    int L, int q, ScanMeta mt, double *__restrict__ T) {
    const float *J = x + (size_t)L * q;
    const int n_single = mt.lo[mt.k - 1] + mt.nl[mt.k - 1];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < mt.n_tab; e += gridDim.x * 256) {
        if (e < 2 * n_single) {
            const int l = e >> 1;
            int s = 0;
            while (s + 1 < mt.k && l >= mt.lo[s + 1]) s++;
            T[e] = tab[((size_t)mt.site[s] * q + letters[l]) * 2 + (e & 1)];
            continue;
        }
        int s = 0, u = 1, base = 2 * n_single;
        for (int a = 0; a < mt.k - 1; a++)
            for (int c = a + 1; c < mt.k; c++)
                if (e >= mt.poff[scan_pair(a, c)]) { s = a; u = c; base = mt.poff[scan_pair(a, c)]; }
        const int r = e - base, ls = r / mt.nl[u], lu = r - ls * mt.nl[u];
        const int i = mt.site[s], j = mt.site[u];
        T[e] = epistasis(J, L, q, i, j, letters[mt.lo[s] + ls], letters[mt.lo[u] + lu], target[i], target[j]);
    }
}

// Every block takes a contiguous run of `per_block` combinations, its threads striding through it.  The tables stay in
// global memory (they are read through the caches; staging them in the LDS was measured and did not pay, section 9.16).
// Dynamic LDS, one array: [n_edges edges][n_edges + 1 counts][8 doubles of the block's extremes].
__global__ __launch_bounds__(MU_SCAN_THREADS) void k_scan(const double *__restrict__ T, ScanMeta mt, int64_t first,
                                                         int64_t count, int64_t per_block, double *__restrict__ en,
                                                         const double *__restrict__ edges_g, int n_edges,
                                                         unsigned long long *__restrict__ hist,
                                                         double *__restrict__ block_min, double *__restrict__ block_max,
                                                         int use_thr, double thr, int64_t capacity,
                                                         unsigned long long *__restrict__ n_kept,
                                                         int64_t *__restrict__ kept_idx, double *__restrict__ kept_en) {
    extern __shared__ double smem[];
    const int tid = threadIdx.x;
    double *edges = smem;
    unsigned int *cnt = (unsigned int *)(edges + n_edges);
    double *red = smem + n_edges + (n_edges + 2) / 2;                    // past the n_edges + 1 counts, 8-byte aligned
    for (int e = tid; e < n_edges; e += MU_SCAN_THREADS) edges[e] = edges_g[e];
    if (hist)
        for (int e = tid; e <= n_edges; e += MU_SCAN_THREADS) cnt[e] = 0u;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per_block;
    const int64_t hi = lo + per_block < count ? lo + per_block : count;
    double vmin = INFINITY, vmax = -INFINITY;
    for (int64_t r = lo + tid; r < hi; r += MU_SCAN_THREADS) {
        // digits of the mixed-radix index, the last site fastest; 32-bit division once the rest fits
        uint64_t rest = (uint64_t)(first + r);
        int d[PLM_SCAN_MAX_SITES];
#pragma unroll
        for (int s = PLM_SCAN_MAX_SITES - 1; s >= 0; s--) {
            d[s] = 0;
            if (s < mt.k) {
                const unsigned int nl = (unsigned int)mt.nl[s];
                if (rest >> 32) {
                    const uint64_t qt = rest / nl;
                    d[s] = (int)(rest - qt * nl);
                    rest = qt;
                } else {
                    const unsigned int r32 = (unsigned int)rest, qt = r32 / nl;
                    d[s] = (int)(r32 - qt * nl);
                    rest = qt;
                }
            }
        }
        double dj = 0.0, dh = 0.0;
#pragma unroll
        for (int s = 0; s < PLM_SCAN_MAX_SITES; s++)
            if (s < mt.k) {
                dj += T[2 * (mt.lo[s] + d[s])];
                dh += T[2 * (mt.lo[s] + d[s]) + 1];
            }
#pragma unroll
        for (int s = 0; s < PLM_SCAN_MAX_SITES - 1; s++)
#pragma unroll
            for (int u = s + 1; u < PLM_SCAN_MAX_SITES; u++)
                if (u < mt.k) dj += T[mt.poff[scan_pair(s, u)] + d[s] * mt.nl[u] + d[u]];
        const double dH = dj + dh;
        if (en) {
            en[r * 3 + 0] = dH;
            en[r * 3 + 1] = dj;
            en[r * 3 + 2] = dh;
        }
        vmin = fmin(vmin, dH);
        vmax = fmax(vmax, dH);
        if (hist) {
            int a = 0, b = n_edges;                   // the number of edges <= dH, by comparison only
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (edges[mid] <= dH) a = mid + 1; else b = mid;
            }
            atomicAdd(&cnt[a], 1u);
        }
        if (use_thr && dH >= thr) {
            const unsigned long long slot = atomicAdd(n_kept, 1ull);
            if (slot < (unsigned long long)capacity) {
                kept_idx[slot] = first + r;
                kept_en[slot * 3 + 0] = dH;
                kept_en[slot * 3 + 1] = dj;
                kept_en[slot * 3 + 2] = dh;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        vmin = fmin(vmin, __shfl_xor(vmin, o, 64));
        vmax = fmax(vmax, __shfl_xor(vmax, o, 64));
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = vmin;
        red[4 + (tid >> 6)] = vmax;
    }
    __syncthreads();
    if (tid == 0) {
        block_min[blockIdx.x] = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
        block_max[blockIdx.x] = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
    }
    if (hist)
        for (int e = tid; e <= n_edges; e += MU_SCAN_THREADS)
            if (cnt[e]) atomicAdd(&hist[e], (unsigned long long)cnt[e]);
}

int check_model(const float *x, int L, int q, const int8_t *target) {
    if (!x || !target) return plm_fail(PLM_EINVAL, "NULL argument");
    if (L < 2) return plm_fail(PLM_EINVAL, "need at least 2 sites (got %d)", L);
    if (q < 2 || q > MU_Q) return plm_fail(PLM_EUNSUPPORTED, "mutant effects support 2..32 states (got %d)", q);
    for (int k = 0; k < L; k++)
        if (target[k] < 0 || target[k] >= q)
            return plm_fail(PLM_EINVAL, "target[%d] = %d outside 0..%d", k, (int)target[k], q - 1);
    return PLM_OK;
}

// the model, the target and the single tables on the device
int upload_model(DeviceBuffers &mem, const float *x, int L, int q, const int8_t *target, hipStream_t st, float **xd,
                 int8_t **td, double **tab) {
    const size_t nx = (size_t)plm_n_canon(L, q);
    PLM_TRY(mem.alloc(xd, nx));
    PLM_TRY(mem.alloc(td, (size_t)L));
    PLM_TRY(mem.alloc(tab, (size_t)L * q * 2));
    PLM_HIP(hipMemcpyAsync(*xd, x, sizeof(float) * nx, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(*td, target, (size_t)L, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_single_tables, dim3(L), dim3(64), 0, st, *xd, *td, L, q, *tab);
    PLM_HIP(hipGetLastError());
    return PLM_OK;
}

}  // namespace

int plm_mutant_effects(const float *x_canonical, int32_t n_sites, int32_t n_states, const int8_t *target,
                       int64_t n_variants, const int64_t *offsets, int64_t n_entries, const int32_t *positions,
                       const int8_t *states, int device, void *stream, double *out, uint8_t *status,
                       double *tables_out) {
    PLM_TRY(check_model(x_canonical, n_sites, n_states, target));
    if (n_variants < 0 || n_entries < 0) return plm_fail(PLM_EINVAL, "negative count");
    if (!offsets) return plm_fail(PLM_EINVAL, "NULL offsets");
    if (n_variants > 0 && (!out || !status)) return plm_fail(PLM_EINVAL, "NULL output");
    if (n_entries > 0 && (!positions || !states)) return plm_fail(PLM_EINVAL, "NULL positions or states");
    if (offsets[0] != 0) return plm_fail(PLM_EINVAL, "offsets[0] = %lld, expected 0", (long long)offsets[0]);
    for (int64_t v = 0; v < n_variants; v++)
        if (offsets[v + 1] < offsets[v])
            return plm_fail(PLM_EINVAL, "offsets decrease at variant %lld", (long long)v);
    if (offsets[n_variants] != n_entries)
        return plm_fail(PLM_EINVAL, "offsets end at %lld, positions hold %lld entries", (long long)offsets[n_variants],
                        (long long)n_entries);
    const int L = n_sites, q = n_states;
    // the variants that get a wave each (those beyond L entries are refused by the thread kernel)
    std::vector<int64_t> longs;
    for (int64_t v = 0; v < n_variants; v++) {
        const int64_t M = offsets[v + 1] - offsets[v];
        if (M > MU_SHORT && M <= L) longs.push_back(v);
    }
    if (n_variants > (int64_t)0x7fffffff * 256) return plm_fail(PLM_EUNSUPPORTED, "too many variants for one call");
    PLM_TRY(plm_check_device(device));
    const double need = 4.0 * plm_n_canon(L, q) + L + 16.0 * L * q + 8.0 * (n_variants + 1) + 5.0 * n_entries +
                        25.0 * n_variants + 8.0 * longs.size();
    PLM_TRY(plm_check_free(need, "mutant effects"));
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    float *xd = nullptr;
    int8_t *td = nullptr, *sd = nullptr;
    double *tab = nullptr, *od = nullptr;
    int64_t *offd = nullptr, *ld = nullptr;
    int32_t *pd = nullptr;
    uint8_t *std_ = nullptr;
    PLM_TRY(upload_model(mem, x_canonical, L, q, target, st, &xd, &td, &tab));
    if (n_variants > 0) {
        PLM_TRY(mem.alloc(&offd, (size_t)n_variants + 1));
        PLM_TRY(mem.alloc(&pd, (size_t)n_entries));
        PLM_TRY(mem.alloc(&sd, (size_t)n_entries));
        PLM_TRY(mem.alloc(&od, (size_t)n_variants * 3));
        PLM_TRY(mem.alloc(&std_, (size_t)n_variants));
        PLM_HIP(hipMemcpyAsync(offd, offsets, sizeof(int64_t) * (n_variants + 1), hipMemcpyHostToDevice, st));
        if (n_entries > 0) {
            PLM_HIP(hipMemcpyAsync(pd, positions, sizeof(int32_t) * n_entries, hipMemcpyHostToDevice, st));
            PLM_HIP(hipMemcpyAsync(sd, states, (size_t)n_entries, hipMemcpyHostToDevice, st));
        }
        hipLaunchKernelGGL(k_effects_thread, dim3((unsigned)((n_variants + 255) / 256)), dim3(256), 0, st, xd, tab, td, L, q,
                           n_variants, offd, pd, sd, od, std_);
        PLM_HIP(hipGetLastError());
        if (!longs.empty()) {
            PLM_TRY(mem.alloc(&ld, longs.size()));
            PLM_HIP(hipMemcpyAsync(ld, longs.data(), sizeof(int64_t) * longs.size(), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_effects_wave, dim3((unsigned)longs.size()), dim3(64), 0, st, xd, tab, td, L, q, ld, offd, pd,
                               sd, od, std_);
            PLM_HIP(hipGetLastError());
        }
        PLM_HIP(hipMemcpyAsync(out, od, sizeof(double) * 3 * n_variants, hipMemcpyDeviceToHost, st));
        PLM_HIP(hipMemcpyAsync(status, std_, (size_t)n_variants, hipMemcpyDeviceToHost, st));
    }
    if (tables_out)
        PLM_HIP(hipMemcpyAsync(tables_out, tab, sizeof(double) * 2 * L * q, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_mutant_scan(const float *x_canonical, int32_t n_sites, int32_t n_states, const int8_t *target,
                    const plm_scan_opts *opts, int device, void *stream, plm_scan_result *result) {
    if (!opts || !result) return plm_fail(PLM_EINVAL, "NULL opts or result");
    PLM_TRY(check_model(x_canonical, n_sites, n_states, target));
    const int L = n_sites, q = n_states, k = opts->n_scan_sites;
    if (opts->flags) return plm_fail(PLM_EINVAL, "unknown flags 0x%x", opts->flags);
    if (k < 1) return plm_fail(PLM_EINVAL, "need at least one site to scan");
    if (k > PLM_SCAN_MAX_SITES) return plm_fail(PLM_EUNSUPPORTED, "a scan takes at most %d sites (got %d)", PLM_SCAN_MAX_SITES, k);
    if (!opts->sites) return plm_fail(PLM_EINVAL, "NULL sites");
    if (opts->letters && !opts->letter_offsets) return plm_fail(PLM_EINVAL, "letters without letter_offsets");
    ScanMeta mt;
    memset(&mt, 0, sizeof mt);
    mt.k = k;
    std::vector<int8_t> letters;
    for (int s = 0; s < k; s++) {
        const int site = opts->sites[s];
        if (site < 0 || site >= L) return plm_fail(PLM_EINVAL, "site %d outside 0..%d", site, L - 1);
        for (int u = 0; u < s; u++)
            if (opts->sites[u] == site) return plm_fail(PLM_EINVAL, "site %d named twice", site);
        mt.site[s] = site;
        mt.lo[s] = (int)letters.size();
        if (opts->letters) {
            const int64_t a = opts->letter_offsets[s], b = opts->letter_offsets[s + 1];
            if ((s == 0 && a != 0) || b <= a || b - a > q)
                return plm_fail(PLM_EINVAL, "site %d needs between 1 and %d distinct letters", site, q);
            uint32_t seen = 0;
            for (int64_t e = a; e < b; e++) {
                const int c = opts->letters[e];
                if (c < 0 || c >= q) return plm_fail(PLM_EINVAL, "letter %d of site %d outside 0..%d", c, site, q - 1);
                if (seen >> c & 1u) return plm_fail(PLM_EINVAL, "letter %d of site %d named twice", c, site);
                seen |= 1u << c;
                letters.push_back((int8_t)c);
            }
        } else {
            for (int c = 0; c < q; c++) letters.push_back((int8_t)c);
        }
        mt.nl[s] = (int)letters.size() - mt.lo[s];
    }
    int64_t total = 1;
    for (int s = 0; s < k; s++) {
        if (total > ((int64_t)1 << 62) / mt.nl[s]) return plm_fail(PLM_EUNSUPPORTED, "2^62 combinations or more");
        total *= mt.nl[s];
    }
    if (total >= (int64_t)1 << 62) return plm_fail(PLM_EUNSUPPORTED, "2^62 combinations or more");
    const int64_t first = opts->first, count = opts->count;
    if (first < 0 || count < 0 || first > total || count > total - first)
        return plm_fail(PLM_EINVAL, "range [%lld, %lld + %lld) outside the %lld combinations", (long long)first,
                        (long long)first, (long long)count, (long long)total);
    const int n_edges = opts->n_edges;
    if (n_edges < 0 || n_edges > PLM_SCAN_MAX_EDGES)
        return plm_fail(PLM_EINVAL, "a histogram takes at most %d edges (got %d)", PLM_SCAN_MAX_EDGES, n_edges);
    const bool want_hist = result->histogram != nullptr;
    if (want_hist != (opts->edges != nullptr) || (!want_hist && n_edges != 0))
        return plm_fail(PLM_EINVAL, "edges and histogram go together");
    for (int e = 0; e < n_edges; e++)
        if (opts->edges[e] != opts->edges[e] || (e > 0 && opts->edges[e] < opts->edges[e - 1]))
            return plm_fail(PLM_EINVAL, "edges must be ascending numbers (edge %d)", e);
    const bool use_thr = opts->use_threshold != 0;
    const int64_t capacity = use_thr ? opts->capacity : 0;
    if (use_thr && opts->threshold != opts->threshold) return plm_fail(PLM_EINVAL, "threshold is NaN");
    if (capacity < 0) return plm_fail(PLM_EINVAL, "negative capacity");
    if (capacity > 0 && (!result->kept_index || !result->kept_energies))
        return plm_fail(PLM_EINVAL, "capacity without kept_index and kept_energies");
    const int n_single = (int)letters.size();
    int at = 2 * n_single;
    for (int s = 0; s < k - 1; s++)
        for (int u = s + 1; u < k; u++) {
            mt.poff[scan_pair(s, u)] = at;
            at += mt.nl[s] * mt.nl[u];
        }
    mt.n_tab = at;
    result->n_combinations = total;
    result->n_kept = 0;
    result->dh_min = std::numeric_limits<double>::infinity();
    result->dh_max = -std::numeric_limits<double>::infinity();
    PLM_TRY(plm_check_device(device));
    // the grid: MU_SCAN_ITEMS combinations per thread, at most 8 blocks per CU, a block's run below 2^31 (its counts
    // are 32-bit)
    hipDeviceProp_t prop;
    PLM_HIP(hipGetDeviceProperties(&prop, device));
    const int64_t max_blocks = (int64_t)prop.multiProcessorCount * 8;
    int64_t grid = (count + (int64_t)MU_SCAN_THREADS * MU_SCAN_ITEMS - 1) / ((int64_t)MU_SCAN_THREADS * MU_SCAN_ITEMS);
    grid = std::max<int64_t>(1, std::min(grid, max_blocks));
    grid = std::max(grid, (count >> 31) + 1);
    if (grid > 0x7fffffff) return plm_fail(PLM_EUNSUPPORTED, "range too long for one call");
    int64_t per_block = (count + grid - 1) / grid;
    per_block = std::max<int64_t>(MU_SCAN_THREADS, (per_block + MU_SCAN_THREADS - 1) / MU_SCAN_THREADS * MU_SCAN_THREADS);
    const size_t lds = sizeof(double) * ((size_t)n_edges + (n_edges + 2) / 2 + 8);
    const double need = 4.0 * plm_n_canon(L, q) + L + 16.0 * L * q + 8.0 * mt.n_tab + 16.0 * grid + 8.0 * (n_edges + 1) * 2 +
                        (result->energies ? 24.0 * count : 0.0) + 32.0 * capacity + 64;
    PLM_TRY(plm_check_free(need, "the mutant scan"));
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    float *xd = nullptr;
    int8_t *td = nullptr, *letd = nullptr;
    double *tab = nullptr, *T = nullptr, *en = nullptr, *ed = nullptr, *bmin = nullptr, *bmax = nullptr, *ken = nullptr;
    unsigned long long *hist = nullptr, *nk = nullptr;
    int64_t *kidx = nullptr;
    PLM_TRY(upload_model(mem, x_canonical, L, q, target, st, &xd, &td, &tab));
    PLM_TRY(mem.alloc(&letd, letters.size()));
    PLM_TRY(mem.alloc(&T, (size_t)mt.n_tab));
    PLM_TRY(mem.alloc(&bmin, (size_t)grid));
    PLM_TRY(mem.alloc(&bmax, (size_t)grid));
    PLM_TRY(mem.alloc(&nk, 1));
    PLM_HIP(hipMemcpyAsync(letd, letters.data(), letters.size(), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemsetAsync(nk, 0, sizeof(unsigned long long), st));
    if (result->energies && count > 0) PLM_TRY(mem.alloc(&en, (size_t)count * 3));
    if (want_hist) {
        PLM_TRY(mem.alloc(&ed, (size_t)n_edges));
        PLM_TRY(mem.alloc(&hist, (size_t)n_edges + 1));
        if (n_edges > 0) PLM_HIP(hipMemcpyAsync(ed, opts->edges, sizeof(double) * n_edges, hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * (n_edges + 1), st));
    }
    if (capacity > 0) {
        PLM_TRY(mem.alloc(&kidx, (size_t)capacity));
        PLM_TRY(mem.alloc(&ken, (size_t)capacity * 3));
    }
    hipLaunchKernelGGL(k_scan_gather, dim3((unsigned)std::min(64, (mt.n_tab + 255) / 256)), dim3(256), 0, st, xd, tab, td, letd,
                       L, q, mt, T);
    PLM_HIP(hipGetLastError());
    if (count > 0) {
        hipLaunchKernelGGL(k_scan, dim3((unsigned)grid), dim3(MU_SCAN_THREADS), lds, st, T, mt, first, count, per_block, en, ed,
                           n_edges, hist, bmin, bmax, use_thr ? 1 : 0, opts->threshold, capacity, nk, kidx, ken);
        PLM_HIP(hipGetLastError());
    }
    std::vector<double> hmin((size_t)grid), hmax((size_t)grid);
    unsigned long long n_kept = 0;
    if (count > 0) {
        PLM_HIP(hipMemcpyAsync(hmin.data(), bmin, sizeof(double) * grid, hipMemcpyDeviceToHost, st));
        PLM_HIP(hipMemcpyAsync(hmax.data(), bmax, sizeof(double) * grid, hipMemcpyDeviceToHost, st));
        if (en) PLM_HIP(hipMemcpyAsync(result->energies, en, sizeof(double) * 3 * count, hipMemcpyDeviceToHost, st));
    }
    if (want_hist)
        PLM_HIP(hipMemcpyAsync(result->histogram, hist, sizeof(uint64_t) * (n_edges + 1), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipMemcpyAsync(&n_kept, nk, sizeof n_kept, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    if (count > 0) {
        for (int64_t b = 0; b < grid; b++) {
            result->dh_min = std::min(result->dh_min, hmin[(size_t)b]);
            result->dh_max = std::max(result->dh_max, hmax[(size_t)b]);
        }
    }
    result->n_kept = (int64_t)n_kept;
    if (n_kept > 0 && (int64_t)n_kept <= capacity) {
        // the slots were handed out in the order of arrival: put the entries into index order
        std::vector<int64_t> idx((size_t)n_kept);
        std::vector<double> ke((size_t)n_kept * 3);
        PLM_HIP(hipMemcpy(idx.data(), kidx, sizeof(int64_t) * n_kept, hipMemcpyDeviceToHost));
        PLM_HIP(hipMemcpy(ke.data(), ken, sizeof(double) * 3 * n_kept, hipMemcpyDeviceToHost));
        std::vector<size_t> order((size_t)n_kept);
        for (size_t e = 0; e < order.size(); e++) order[e] = e;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return idx[a] < idx[b]; });
        for (size_t e = 0; e < order.size(); e++) {
            result->kept_index[e] = idx[order[e]];
            memcpy(result->kept_energies + 3 * e, &ke[3 * order[e]], sizeof(double) * 3);
        }
    }
    return PLM_OK;
}
