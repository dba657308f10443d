// plm_cross.hip -- inter-protein coupling energies of two sequence sets, on gfx950 (DESIGN_NEXT_ROWS.md 9.23).
//
//   E(s,t) = sum_{i in A} sum_{j in B} J_ij(a_si, b_tj)          for every row s of A and row t of B of one group
//
// in two stages, both float64 sums of float32 values in the order include/plm_hip.h fixes:
//   k_cross_v       V[t][i][a] = sum_j jab[i][j][a][b_tj]: one wave per (tile of 64 b-rows, i, a), a lane per b-row; the
//                   64 lanes read inside one row of q floats of jab
//   k_cross_pairs   E[s][t] = sum_i V[t][i][a_si]: a workgroup owns 64 b-rows (a lane each) and a range of a-rows; a
//                   chunk of sites of V sits in the LDS as [i][a][lane], the state a_si is the same for the whole wave, so a
//                   read hits 64 consecutive doubles; a wave keeps CR_BATCH a-rows in registers across the site chunks
//   k_cross_rows / k_cross_cols   merge the best-partner partials of the workgroups (max with an index tie-break)
// A tile of 64 b-rows may span many groups: the a-rows of those groups are one contiguous range, which the workgroup walks,
// and a lane takes part only for the a-rows of its own group.  Small groups therefore share workgroups.
// Every E(s,t) is summed by one lane in one order: no output bit depends on the split (PLM_CROSS_TILE: a-rows per
// workgroup) or on the V chunk (PLM_CROSS_VCHUNK: tiles of b-rows per V buffer).  No floating-point atomics.
#include "plm_host_util.h"
#include <errno.h>
#include <limits.h>
#include <stdlib.h>
#include <limits>

namespace {

#define CR_Q 32                      // largest alphabet
#define CR_BATCH 16                  // a-rows a wave holds in registers
#define CR_WAVES 8                   // waves of a pair workgroup
#define CR_ROWS (CR_BATCH * CR_WAVES)   // a-rows per pass of a workgroup
#define CR_THREADS (64 * CR_WAVES)
#define CR_LDS_V 49152               // bytes of V a workgroup stages at a time
#define CR_SITES 16                  // ... and at most this many sites of it
#define CR_PRE (CR_LDS_V / 8 / CR_THREADS)          // doubles of a chunk a thread carries
#define CR_PRE_S (CR_ROWS * CR_SITES / CR_THREADS)   // ... and states
#define CR_SPLIT 512                 // a-rows per workgroup unless PLM_CROSS_TILE says otherwise
#define CR_V_BYTES (1ull << 30)      // largest V buffer; more b-rows than fit are taken in chunks of tiles
#define CR_NONE INT64_MAX            // "no partner" while merging: loses every index tie

struct CrossItem {                   // one pair workgroup: a-rows s0 .. s1-1 against the 64 b-rows of `tile`
    int64_t tile, s0, s1, rp;        // rp: where its row partials start
};

struct Best {                        // plm_cross_best with CR_NONE for "no partner" until the last merge
    int64_t index;
    double best, second;
};

// (b, i, s) <- the two best of the union; ties to the smaller index
__device__ __forceinline__ void merge_best(double &b, int64_t &i, double &s, double ob, int64_t oi, double os) {
    if (b > ob || (b == ob && i <= oi)) {
        s = fmax(s, ob);
    } else {
        s = fmax(os, b);
        b = ob;
        i = oi;
    }
}

// sbt: the b-rows by tiles with four sites to a word, [tile][ceil(LB / 4)][64] words (state 0 wherever no row or site
// is).  V: [tile of the chunk][i][a][64].  A skipped term adds +0.0 instead of nothing: a sum that starts from +0.0 never
// becomes -0.0, so the bits are those of the sum without the term.
__global__ __launch_bounds__(256) void k_cross_v(const float *__restrict__ jab, const uint32_t *__restrict__ sbt, int LA,
                                                 int LB, int q, int skip, int64_t tile0, int64_t n_waves,
                                                 double *__restrict__ V) {
    const int lane = threadIdx.x & 63;
    const int64_t W = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (W >= n_waves) return;
    const int a = (int)(W % q);
    const int64_t r = W / q;
    const int i = (int)(r % LA);
    const int64_t tl = r / LA;
    const int LB4 = (LB + 3) / 4;
    const uint32_t *sb = sbt + (size_t)(tile0 + tl) * LB4 * 64 + lane;
    const float *row = jab + ((size_t)i * LB * q + a) * q;
    const size_t qq = (size_t)q * q;
    double acc = 0.0;
#pragma unroll 4
    for (int j4 = 0; j4 < LB4; j4++) {
        const uint32_t w = sb[(size_t)j4 * 64];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j4 * 4 + u;
            if (j < LB) {                                            // the same for the whole wave
                const int b = (int)((w >> (8 * u)) & 255u);
                const float v = row[j * qq + b];
                acc += b != skip ? (double)v : 0.0;
            }
        }
    }
    V[(((size_t)tl * LA + i) * q + a) * 64 + lane] = acc;
}

// Dynamic LDS: [ic_max q 64 doubles of V][CR_WAVES 64 Best of the column merge][wave][ic_max][CR_BATCH states of the a-rows].
// lo / hi / mbase / mnb [tiles 64]: the a-rows of a b-row's group, and where E(s, t) goes: matrix[mbase + s mnb].
__global__ __launch_bounds__(CR_THREADS) void k_cross_pairs(const double *__restrict__ V, int64_t tile0,
                                                           const CrossItem *__restrict__ items,
                                                           const int8_t *__restrict__ sa, int LA, int q, int ic_max,
                                                           int skip, const int64_t *__restrict__ lo_g,
                                                           const int64_t *__restrict__ hi_g,
                                                           const int64_t *__restrict__ mbase_g,
                                                           const int64_t *__restrict__ mnb_g, double *__restrict__ matrix,
                                                           Best *__restrict__ rowpart, Best *__restrict__ colpart) {
    extern __shared__ double smem[];
    double *Vs = smem;
    Best *mc = (Best *)(smem + (size_t)ic_max * q * 64);
    uint8_t *ss = (uint8_t *)(mc + CR_WAVES * 64);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const CrossItem it = items[blockIdx.x];
    const int64_t t = it.tile * 64 + lane;
    const int64_t lo = lo_g[t], hi = hi_g[t];
    const int64_t mbase = matrix ? mbase_g[t] : 0, mnb = matrix ? mnb_g[t] : 0;
    const double *Vt = V + (size_t)(it.tile - tile0) * LA * q * 64;
    const double ninf = -INFINITY;
    double cb = ninf, cs = ninf;
    int64_t ci = CR_NONE;
    // The next chunk of sites (and the states of the pass's a-rows at them) is fetched into registers while the current
    // one is summed from the LDS.  The row of a skipped state is stored as +0.0 (see k_cross_v).
    double pre[CR_PRE];
    uint8_t pres[CR_PRE_S];
    auto fetch = [&](int64_t sb, int i0) {
        const int ic = min(ic_max, LA - i0), n = ic * q * 64;
        const double *src = Vt + (size_t)i0 * q * 64;
#pragma unroll
        for (int u = 0; u < CR_PRE; u++) {
            const int e = tid + u * CR_THREADS;
            pre[u] = e < n ? src[e] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CR_PRE_S; u++) {
            const int e = tid + u * CR_THREADS;
            uint8_t v = 0;
            if (e < CR_ROWS * ic) {
                const int r = e / ic, ii = e - r * ic;
                const int64_t s = sb + r;
                if (s < it.s1) v = (uint8_t)sa[(size_t)s * LA + i0 + ii];
            }
            pres[u] = v;
        }
    };
    auto store = [&](int i0) {
        const int ic = min(ic_max, LA - i0), n = ic * q * 64;
#pragma unroll
        for (int u = 0; u < CR_PRE; u++) {
            const int e = tid + u * CR_THREADS;
            if (e < n) Vs[e] = (e >> 6) % q == skip ? 0.0 : pre[u];
        }
#pragma unroll
        for (int u = 0; u < CR_PRE_S; u++) {
            const int e = tid + u * CR_THREADS;
            if (e < CR_ROWS * ic) {
                const int r = e / ic, ii = e - r * ic;
                ss[((r / CR_BATCH) * ic_max + ii) * CR_BATCH + r % CR_BATCH] = pres[u];
            }
        }
    };
    fetch(it.s0, 0);
    for (int64_t sb = it.s0; sb < it.s1; sb += CR_ROWS) {
        double acc[CR_BATCH];
#pragma unroll
        for (int k = 0; k < CR_BATCH; k++) acc[k] = 0.0;
        for (int i0 = 0; i0 < LA; i0 += ic_max) {
            const int ic = min(ic_max, LA - i0);
            __syncthreads();                                          // the previous chunk is consumed
            store(i0);
            __syncthreads();
            const bool last = i0 + ic_max >= LA;
            if (!last || sb + CR_ROWS < it.s1) fetch(last ? sb + CR_ROWS : sb, last ? 0 : i0 + ic_max);
            for (int ii = 0; ii < ic; ii++) {
                const double *col = Vs + (size_t)ii * q * 64 + lane;
                const uint4 pk = *(const uint4 *)(ss + (w * ic_max + ii) * CR_BATCH);   // the wave's 16 states at this site
                const uint32_t wd[4] = {pk.x, pk.y, pk.z, pk.w};
#pragma unroll
                for (int k = 0; k < CR_BATCH; k++) acc[k] += col[((wd[k >> 2] >> ((k & 3) * 8)) & 255u) * 64];
            }
        }
#pragma unroll
        for (int k = 0; k < CR_BATCH; k++) {
            const int64_t s = sb + w * CR_BATCH + k;
            if (s >= it.s1) break;                                   // the same for the whole wave
            const bool active = s >= lo && s < hi;
            if (matrix && active) matrix[mbase + s * mnb] = acc[k];
            if (rowpart || colpart) {
                if (active) merge_best(cb, ci, cs, acc[k], s, ninf);
                double rb = active ? acc[k] : ninf, rs = ninf;
                int ri = active ? lane : 64;
                for (int o = 32; o > 0; o >>= 1) {
                    const double ob = __shfl_xor(rb, o, 64), os = __shfl_xor(rs, o, 64);
                    const int oi = __shfl_xor(ri, o, 64);
                    if (rb > ob || (rb == ob && ri <= oi)) {
                        rs = fmax(rs, ob);
                    } else {
                        rs = fmax(os, rb);
                        rb = ob;
                        ri = oi;
                    }
                }
                if (rowpart && lane == 0) {
                    Best o;
                    o.index = ri < 64 ? it.tile * 64 + ri : CR_NONE;
                    o.best = rb;
                    o.second = rs;
                    rowpart[it.rp + (s - it.s0)] = o;
                }
            }
        }
    }
    if (colpart) {
        Best mine;
        mine.index = ci;
        mine.best = cb;
        mine.second = cs;
        mc[w * 64 + lane] = mine;
        __syncthreads();
        if (w == 0) {
            for (int k = 1; k < CR_WAVES; k++) {
                const Best o = mc[k * 64 + lane];
                merge_best(cb, ci, cs, o.best, o.index, o.second);
            }
            Best o;
            o.index = ci;
            o.best = cb;
            o.second = cs;
            colpart[(size_t)blockIdx.x * 64 + lane] = o;
        }
    }
}

// One thread per a-row s of the chunk's range: the tiles T0 .. T1-1 whose a-rows alo[T] .. ahi[T]-1 hold s are
// consecutive (both arrays ascend); their partials are merged into rows[s].
__global__ __launch_bounds__(256) void k_cross_rows(const Best *__restrict__ rowpart, const int64_t *__restrict__ alo,
                                                    const int64_t *__restrict__ ahi, const int64_t *__restrict__ tile_rp,
                                                    int64_t T0, int64_t T1, int64_t s_first, int64_t s_end,
                                                    Best *__restrict__ rows) {
    const int64_t s = s_first + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= s_end) return;
    int64_t a = T0, b = T1;                       // the first tile with ahi > s
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (ahi[mid] > s) b = mid; else a = mid + 1;
    }
    Best r = rows[s];
    for (int64_t T = a; T < T1 && alo[T] <= s; T++) {
        const Best o = rowpart[tile_rp[T] + (s - alo[T])];
        merge_best(r.best, r.index, r.second, o.best, o.index, o.second);
    }
    rows[s] = r;
}

// One thread per b-row of the chunk's tiles: the partials of the tile's workgroups
__global__ __launch_bounds__(256) void k_cross_cols(const Best *__restrict__ colpart, const int64_t *__restrict__ item_first,
                                                    int64_t T0, int64_t T1, int64_t item0, int64_t n_b,
                                                    Best *__restrict__ cols) {
    const int64_t t = T0 * 64 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T1 * 64 || t >= n_b) return;
    const int64_t T = t >> 6;
    const int lane = (int)(t & 63);
    Best r = cols[t];
    for (int64_t k = item_first[T]; k < item_first[T + 1]; k++) {
        const Best o = colpart[(size_t)(k - item0) * 64 + lane];
        merge_best(r.best, r.index, r.second, o.best, o.index, o.second);
    }
    cols[t] = r;
}

// an environment variable that must be a positive integer when it is set; 0 when it is not
int cross_env(const char *name, int64_t *out) {
    *out = 0;
    const char *v = getenv(name);
    if (!v) return PLM_OK;
    char *end = nullptr;
    errno = 0;
    const long long x = strtoll(v, &end, 10);
    if (errno || end == v || *end || x < 1 || x > INT_MAX)
        return plm_fail(PLM_EINVAL, "%s must be a positive integer (got '%s')", name, v);
    *out = x;
    return PLM_OK;
}

int check_offsets(const int64_t *off, int64_t n_groups, int64_t n, const char *what) {
    if (off[0] != 0) return plm_fail(PLM_EINVAL, "%s[0] = %lld, expected 0", what, (long long)off[0]);
    for (int64_t g = 0; g < n_groups; g++)
        if (off[g + 1] < off[g]) return plm_fail(PLM_EINVAL, "%s decrease at group %lld", what, (long long)g);
    if (off[n_groups] != n)
        return plm_fail(PLM_EINVAL, "%s end at %lld, the set holds %lld rows", what, (long long)off[n_groups], (long long)n);
    return PLM_OK;
}

int check_states(const int8_t *x, int64_t n, int L, int q, const char *what) {
    for (int64_t s = 0; s < n; s++)
        for (int k = 0; k < L; k++) {
            const int v = x[(size_t)s * L + k];
            if (v < 0 || v >= q)
                return plm_fail(PLM_EINVAL, "%s[%lld][%d] = %d outside 0..%d", what, (long long)s, k, v, q - 1);
        }
    return PLM_OK;
}

void fill_best(plm_cross_best *out, int64_t n) {
    const double ninf = -std::numeric_limits<double>::infinity();
    for (int64_t k = 0; k < n; k++) {
        out[k].index = -1;
        out[k].best = ninf;
        out[k].second = ninf;
    }
}

int launch_check(int64_t blocks, const char *what) {
    if (blocks > 0x7fffffff) return plm_fail(PLM_EUNSUPPORTED, "%s: too many workgroups for one launch", what);
    return PLM_OK;
}

}  // namespace

int plm_cross_energies(const float *jab, int32_t n_sites_a, int32_t n_sites_b, int32_t n_states, const int8_t *seqs_a,
                       int64_t n_a, const int8_t *seqs_b, int64_t n_b, int64_t n_groups, const int64_t *a_offsets,
                       const int64_t *b_offsets, const plm_cross_opts *opts, int device, void *stream, double *matrix_out,
                       plm_cross_best *rows_best, plm_cross_best *cols_best) {
    static_assert(sizeof(Best) == sizeof(plm_cross_best), "the device partials are copied out as plm_cross_best");
    static_assert(CR_PRE * CR_THREADS * 8 == CR_LDS_V && CR_PRE_S * CR_THREADS == CR_ROWS * CR_SITES,
                  "a thread's registers hold its share of a chunk");
    if (!jab || !seqs_a || !seqs_b || !a_offsets || !b_offsets || !opts) return plm_fail(PLM_EINVAL, "NULL argument");
    if (!opts->want_best) rows_best = cols_best = nullptr;
    if (!matrix_out && !rows_best && !cols_best) return plm_fail(PLM_EINVAL, "no output asked for");
    const int LA = n_sites_a, LB = n_sites_b, q = n_states;
    if (LA < 1 || LB < 1) return plm_fail(PLM_EINVAL, "need at least one site on each side (got %d and %d)", LA, LB);
    if (n_a < 0 || n_b < 0 || n_groups < 0) return plm_fail(PLM_EINVAL, "negative count");
    if (q < 2 || q > CR_Q) return plm_fail(PLM_EUNSUPPORTED, "cross energies support 2..32 states (got %d)", q);
    const int skip = opts->skip_state;
    if (skip < -1 || skip >= q) return plm_fail(PLM_EINVAL, "skip_state = %d outside -1..%d", skip, q - 1);
    PLM_TRY(check_offsets(a_offsets, n_groups, n_a, "a_offsets"));
    PLM_TRY(check_offsets(b_offsets, n_groups, n_b, "b_offsets"));
    PLM_TRY(check_states(seqs_a, n_a, LA, q, "seqs_a"));
    PLM_TRY(check_states(seqs_b, n_b, LB, q, "seqs_b"));
    int64_t split = 0, vchunk = 0;
    PLM_TRY(cross_env("PLM_CROSS_TILE", &split));
    PLM_TRY(cross_env("PLM_CROSS_VCHUNK", &vchunk));
    if (!split) split = CR_SPLIT;
    if ((double)LA * LB * q * q >= 4.6e18 || (double)n_a * LA >= 4.6e18 || (double)n_b * LB >= 4.6e18)
        return plm_fail(PLM_EUNSUPPORTED, "sizes beyond 2^62");

    // ---- the plan: per b-row the a-rows of its group and its place in the matrix; per tile its a-rows and workgroups
    const int64_t n_tiles = (n_b + 63) / 64;
    const size_t padded = (size_t)n_tiles * 64;
    std::vector<int64_t> lo(padded, 0), hi(padded, 0), mbase(padded, 0), mnb(padded, 0);
    double n_matrix = 0.0;
    int64_t block = 0;
    {
        for (int64_t g = 0; g < n_groups; g++) {
            const int64_t na = a_offsets[g + 1] - a_offsets[g], nb = b_offsets[g + 1] - b_offsets[g];
            n_matrix += (double)na * (double)nb;
            if (n_matrix >= 1.1e18) return plm_fail(PLM_EUNSUPPORTED, "2^60 pairs or more");
            for (int64_t t = b_offsets[g]; t < b_offsets[g + 1]; t++) {
                lo[(size_t)t] = a_offsets[g];
                hi[(size_t)t] = a_offsets[g + 1];
                mbase[(size_t)t] = block - a_offsets[g] * nb + (t - b_offsets[g]);
                mnb[(size_t)t] = nb;
            }
            block += na * nb;
        }
    }
    const int64_t total_pairs = block;
    std::vector<int64_t> alo((size_t)n_tiles + 1, 0), ahi((size_t)n_tiles + 1, 0), tile_rp((size_t)n_tiles + 1, 0),
        item_first((size_t)n_tiles + 1, 0);
    std::vector<CrossItem> items;
    for (int64_t T = 0; T < n_tiles; T++) {
        const int64_t last = std::min(n_b, (T + 1) * 64) - 1;
        alo[(size_t)T] = lo[(size_t)T * 64];
        ahi[(size_t)T] = hi[(size_t)last];
        item_first[(size_t)T] = (int64_t)items.size();
        for (int64_t s0 = alo[(size_t)T]; s0 < ahi[(size_t)T]; s0 += split) {
            CrossItem it;
            it.tile = T;
            it.s0 = s0;
            it.s1 = std::min(ahi[(size_t)T], s0 + split);
            it.rp = 0;
            items.push_back(it);
            if (items.size() > ((size_t)1 << 28))
                return plm_fail(PLM_EUNSUPPORTED, "more than 2^28 workgroups (PLM_CROSS_TILE = %lld?)", (long long)split);
        }
    }
    item_first[(size_t)n_tiles] = (int64_t)items.size();
    // the V chunks: tiles T0 .. T1-1 at a time; row partials are numbered inside a chunk
    const double v_tile = 8.0 * LA * q * 64;
    int64_t tiles_per = vchunk ? vchunk : std::max<int64_t>(1, (int64_t)((double)CR_V_BYTES / v_tile));
    tiles_per = std::max<int64_t>(1, std::min(tiles_per, std::max<int64_t>(n_tiles, 1)));
    int64_t max_rp = 0, max_items = 0;
    for (int64_t T0 = 0; T0 < n_tiles; T0 += tiles_per) {
        const int64_t T1 = std::min(n_tiles, T0 + tiles_per);
        int64_t rp = 0;
        for (int64_t T = T0; T < T1; T++) {
            tile_rp[(size_t)T] = rp;
            for (int64_t k = item_first[(size_t)T]; k < item_first[(size_t)T + 1]; k++)
                items[(size_t)k].rp = rp + (items[(size_t)k].s0 - alo[(size_t)T]);
            rp += ahi[(size_t)T] - alo[(size_t)T];
        }
        max_rp = std::max(max_rp, rp);
        max_items = std::max(max_items, item_first[(size_t)T1] - item_first[(size_t)T0]);
    }
    const bool want_rows = rows_best != nullptr, want_cols = cols_best != nullptr, want_best = want_rows || want_cols;
    const int ic_max = std::max(1, std::min(std::min(LA, CR_SITES), CR_LDS_V / (q * 64 * 8)));
    const size_t lds = (size_t)ic_max * q * 64 * 8 + sizeof(Best) * CR_WAVES * 64 + (size_t)CR_ROWS * ic_max;
    PLM_TRY(launch_check(max_items, "cross energies"));
    PLM_TRY(launch_check((int64_t)(((double)tiles_per * LA * q + 3) / 4), "cross energies, stage 1"));

    PLM_TRY(plm_check_device(device));
    const double need = 4.0 * LA * LB * q * q + (double)n_a * LA + (double)padded * (LB + 3) + 32.0 * padded + 32.0 * (n_tiles + 1) +
                        32.0 * items.size() + v_tile * tiles_per + (matrix_out ? 8.0 * n_matrix : 0.0) +
                        (want_best ? 24.0 * ((double)n_a + padded + max_rp + 64.0 * max_items) : 0.0) + 4096.0;
    PLM_TRY(plm_check_free(need, "cross energies"));
    if (n_a == 0 || n_b == 0 || items.empty()) {              // nothing to pair: every row is without partners
        if (want_rows) fill_best(rows_best, n_a);
        if (want_cols) fill_best(cols_best, n_b);
        return PLM_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    float *jd = nullptr;
    int8_t *sad = nullptr;
    uint32_t *sbd = nullptr;
    int64_t *lod = nullptr, *hid = nullptr, *mbd = nullptr, *mnd = nullptr, *alod = nullptr, *ahid = nullptr, *rpd = nullptr,
            *ifd = nullptr;
    CrossItem *itd = nullptr;
    double *Vd = nullptr, *md = nullptr;
    Best *rowsd = nullptr, *colsd = nullptr, *rowpart = nullptr, *colpart = nullptr;
    const size_t n_jab = (size_t)LA * LB * q * q;
    // the b-rows by tiles, four sites to a word
    const int LB4 = (LB + 3) / 4;
    std::vector<uint32_t> sbt((size_t)n_tiles * LB4 * 64, 0u);
    for (int64_t t = 0; t < n_b; t++)
        for (int j = 0; j < LB; j++)
            sbt[((size_t)(t >> 6) * LB4 + j / 4) * 64 + (t & 63)] |= (uint32_t)(uint8_t)seqs_b[(size_t)t * LB + j] << (8 * (j & 3));
    PLM_TRY(mem.alloc(&jd, n_jab));
    PLM_TRY(mem.alloc(&sad, (size_t)n_a * LA));
    PLM_TRY(mem.alloc(&sbd, sbt.size()));
    PLM_TRY(mem.alloc(&lod, padded));
    PLM_TRY(mem.alloc(&hid, padded));
    PLM_TRY(mem.alloc(&itd, items.size()));
    PLM_TRY(mem.alloc(&Vd, (size_t)tiles_per * LA * q * 64));
    PLM_HIP(hipMemcpyAsync(jd, jab, sizeof(float) * n_jab, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(sad, seqs_a, (size_t)n_a * LA, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(sbd, sbt.data(), sizeof(uint32_t) * sbt.size(), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(lod, lo.data(), sizeof(int64_t) * padded, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(hid, hi.data(), sizeof(int64_t) * padded, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(itd, items.data(), sizeof(CrossItem) * items.size(), hipMemcpyHostToDevice, st));
    if (matrix_out) {
        PLM_TRY(mem.alloc(&mbd, padded));
        PLM_TRY(mem.alloc(&mnd, padded));
        PLM_TRY(mem.alloc(&md, (size_t)total_pairs));
        PLM_HIP(hipMemcpyAsync(mbd, mbase.data(), sizeof(int64_t) * padded, hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(mnd, mnb.data(), sizeof(int64_t) * padded, hipMemcpyHostToDevice, st));
    }
    std::vector<Best> none;
    if (want_best) {
        // the running results start as "no partner"
        none.resize((size_t)std::max<int64_t>(n_a, (int64_t)padded));
        for (Best &b : none) {
            b.index = CR_NONE;
            b.best = b.second = -std::numeric_limits<double>::infinity();
        }
        PLM_TRY(mem.alloc(&rowsd, (size_t)n_a));
        PLM_TRY(mem.alloc(&colsd, padded));
        PLM_TRY(mem.alloc(&rowpart, (size_t)max_rp));
        PLM_TRY(mem.alloc(&colpart, (size_t)max_items * 64));
        PLM_TRY(mem.alloc(&alod, (size_t)n_tiles + 1));
        PLM_TRY(mem.alloc(&ahid, (size_t)n_tiles + 1));
        PLM_TRY(mem.alloc(&rpd, (size_t)n_tiles + 1));
        PLM_TRY(mem.alloc(&ifd, (size_t)n_tiles + 1));
        PLM_HIP(hipMemcpyAsync(rowsd, none.data(), sizeof(Best) * n_a, hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(colsd, none.data(), sizeof(Best) * padded, hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(alod, alo.data(), sizeof(int64_t) * (n_tiles + 1), hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(ahid, ahi.data(), sizeof(int64_t) * (n_tiles + 1), hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(rpd, tile_rp.data(), sizeof(int64_t) * (n_tiles + 1), hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(ifd, item_first.data(), sizeof(int64_t) * (n_tiles + 1), hipMemcpyHostToDevice, st));
    }
    for (int64_t T0 = 0; T0 < n_tiles; T0 += tiles_per) {
        const int64_t T1 = std::min(n_tiles, T0 + tiles_per);
        const int64_t n_waves = (T1 - T0) * LA * q;
        hipLaunchKernelGGL(k_cross_v, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, st, jd, sbd, LA, LB, q, skip, T0,
                           n_waves, Vd);
        PLM_HIP(hipGetLastError());
        const int64_t item0 = item_first[(size_t)T0], n_items = item_first[(size_t)T1] - item0;
        if (n_items == 0) continue;
        hipLaunchKernelGGL(k_cross_pairs, dim3((unsigned)n_items), dim3(CR_THREADS), lds, st, Vd, T0, itd + item0, sad, LA, q,
                           ic_max, skip, lod, hid, mbd, mnd, md, want_best ? rowpart : nullptr,
                           want_best ? colpart : nullptr);
        PLM_HIP(hipGetLastError());
        if (want_best) {
            const int64_t s_first = alo[(size_t)T0], s_end = ahi[(size_t)T1 - 1];
            if (s_end > s_first) {
                hipLaunchKernelGGL(k_cross_rows, dim3((unsigned)((s_end - s_first + 255) / 256)), dim3(256), 0, st, rowpart,
                                   alod, ahid, rpd, T0, T1, s_first, s_end, rowsd);
                PLM_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(k_cross_cols, dim3((unsigned)(((T1 - T0) * 64 + 255) / 256)), dim3(256), 0, st, colpart, ifd,
                               T0, T1, item0, n_b, colsd);
            PLM_HIP(hipGetLastError());
        }
    }
    if (matrix_out && total_pairs > 0)
        PLM_HIP(hipMemcpyAsync(matrix_out, md, sizeof(double) * total_pairs, hipMemcpyDeviceToHost, st));
    if (want_rows) PLM_HIP(hipMemcpyAsync(rows_best, rowsd, sizeof(Best) * n_a, hipMemcpyDeviceToHost, st));
    if (want_cols) PLM_HIP(hipMemcpyAsync(cols_best, colsd, sizeof(Best) * n_b, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; want_rows && k < n_a; k++)
        if (rows_best[k].index == CR_NONE) rows_best[k].index = -1;
    for (int64_t k = 0; want_cols && k < n_b; k++)
        if (cols_best[k].index == CR_NONE) cols_best[k].index = -1;
    return PLM_OK;
}
