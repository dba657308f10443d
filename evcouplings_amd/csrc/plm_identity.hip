// plm_identity.hip -- pairwise identities between two sets of sequences (plm_cross_identities) and the greedy
// redundancy filter built on them (plm_redundancy_filter); contract in include/plm_hip.h, notes in DESIGN_NEXT_ROWS.md
// section 9.11.  The compare is the one of the reweighting kernel K1 (plm_kernels.hip): one lane per row of A, the row
// of B wave-uniform through the scalar cache, 4 sites per VALU triple (xor+add, and, popcount-accumulate).
//
// Device image of a set (ident_image): rows of Lw dwords, Lw a multiple of 16.  With a gap state the host swaps it
// with state 0, so the gap is byte 0 on the device, and the padding behind the row is gap as well; the lane's own
// gaps become 0x7f (no state: states are 0..126), so neither a gap nor the padding ever matches, and the padding is in
// no "both ungapped" count.  Without a gap state every value 0..126 is a state, none is free for two paddings that
// differ: both sides pad with 127, the padding always matches, and the matches are L - mismatches, not 4 Lw - mismatches.
#include "plm_host_util.h"
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>

typedef uint32_t u32;

namespace {

constexpr int ID_CW = 16;        // dwords (64 sites) per chunk of a row
constexpr int ID_TT = 32;        // rows of B per register tile of the column-chunked form
constexpr int ID_BLK = 256;      // rows per workgroup; the block of the greedy filter
constexpr int ID_BW = ID_BLK / 32;
constexpr int ID_REG_MAX = 192;  // longest row (dwords) the register-resident form holds
constexpr int ID_MAX_ROWS = 1 << 30;  // the kernels add a split's rows to a row index in 32 bits
constexpr int ID_FILTER_WGS = 1024;   // workgroups of one cross pass of the greedy filter (one block of rows of A)

// 0x80 in every zero byte of v, exactly (all bytes < 0x80; see plm_kernels.hip for why the shorter form is not exact)
__device__ __forceinline__ u32 zero_bytes(u32 v) { return ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u; }
__device__ __forceinline__ u32 gaps_to_sentinel(u32 v) { return v + (zero_bytes(v) >> 7) * 0x7fu; }

template <int DENOM>
__device__ __forceinline__ bool similar(int m, int d, int thresh, const int32_t *__restrict__ thr) {
    if constexpr (DENOM == PLM_IDENT_DENOM_COLUMNS) return m >= thresh;
    else return m >= thr[d];     // thr[d] = ceil(theta d - 1e-9) from the host, thr[0] = INT_MAX: d = 0 is never similar
}

struct Best { int cnt, bi, bm, bd; };

// is (m, d) nearer than (bm, bd)?  exact: m / max(d, 1) > bm / max(bd, 1) in 64-bit integers
__device__ __forceinline__ bool nearer(int m, int d, int bm, int bd) {
    return (long long)m * max(bd, 1) > (long long)bm * max(d, 1);
}

// partners arrive in ascending t: "strictly nearer" keeps the smallest index of a tie
template <int DENOM>
__device__ __forceinline__ void take_pair(Best &r, int t, int m, int d, int thresh, const int32_t *__restrict__ thr) {
    r.cnt += similar<DENOM>(m, d, thresh, thr) ? 1 : 0;
    bool better;
    if constexpr (DENOM == PLM_IDENT_DENOM_COLUMNS) better = m > r.bm;
    else better = nearer(m, d, r.bm, r.bd);
    if (r.bi < 0 || better) { r.bi = t; r.bm = m; r.bd = d; }
}

// part: [4][splits][n_a] -- n_within, best index, best match, best denominator of every split of the B range
__device__ __forceinline__ void store_part(int32_t *__restrict__ part, int n_a, int s, const Best &r) {
    const size_t plane = (size_t)gridDim.y * n_a, o = (size_t)blockIdx.y * n_a + s;
    part[o] = r.cnt;
    part[o + plane] = r.bi;
    part[o + 2 * plane] = r.bm;
    part[o + 3 * plane] = r.bd;
}

// Register-resident form (rows up to 768 sites, denominators COLUMNS and SHORTER): the lane's row stays in LW VGPRs,
// the rows of B stream through the scalar cache in 16-dword chunks, the next chunk in flight while this one is compared.
// n_b_dev != nullptr: the number of rows of B is read from the device (the kept rows of the greedy filter); the grid
// then covers an upper bound and the workgroups past the end store empty results.
template <int LW, int DENOM>
__global__ __launch_bounds__(256) void k_ident_reg(const u32 *__restrict__ a32, int n_a, const u32 *__restrict__ b32,
                                                  int n_b_arg, const int32_t *__restrict__ n_b_dev, int Lw, int Lm, int L,
                                                  const int32_t *__restrict__ res_a, const int32_t *__restrict__ res_b,
                                                  const int32_t *__restrict__ thr, int thresh, int gap_mode,
                                                  int exclude_self, int tper, int32_t *__restrict__ part) {
    const int n_b = n_b_dev ? *n_b_dev : n_b_arg;
    const int s = blockIdx.x * ID_BLK + threadIdx.x;
    const int sr = min(s, n_a - 1);                 // the lanes past the end compare the last row and store nothing
    const int tb0 = blockIdx.y * tper, tb1 = min(n_b, tb0 + tper);
    const u32 *__restrict__ myrow = a32 + (size_t)sr * Lw;
    u32 mine[LW];
#pragma unroll
    for (int k = 0; k < LW; k += 4) {
        if (k < Lw) {   // Lw is a multiple of 16: whole uint4 loads
            const uint4 v = *(const uint4 *)(myrow + k);
            mine[k] = v.x; mine[k + 1] = v.y; mine[k + 2] = v.z; mine[k + 3] = v.w;
            if (gap_mode) {
#pragma unroll
                for (int e = 0; e < 4; e++) mine[k + e] = gaps_to_sentinel(mine[k + e]);
            }
        } else {
            mine[k] = mine[k + 1] = mine[k + 2] = mine[k + 3] = 0;   // never compared (c < nch below)
        }
    }
    struct Chunk { u32 v[ID_CW]; };
    u32 c7f = 0x7f7f7f7fu;
    asm volatile("" : "+v"(c7f));   // keep the constant in a VGPR (VOP3 takes one SGPR, no literal)
    const int nch = Lw / ID_CW;
    const int my_res = DENOM == PLM_IDENT_DENOM_SHORTER ? res_a[sr] : 0;
    Best r = {0, -1, 0, 0};
    for (int t = tb0; t < tb1; ++t) {
        const Chunk *__restrict__ trow = (const Chunk *)(b32 + (size_t)t * Lw);
        int mism = 0;
        Chunk cur = trow[0];
#pragma unroll
        for (int c = 0; c < LW / ID_CW; c++) {
            if (c < nch) {
                Chunk nxt = cur;
                if (c + 1 < nch) nxt = trow[c + 1];
#pragma unroll
                for (int k = 0; k < ID_CW; k++) {
                    u32 y;   // (mine ^ partner) + 0x7f7f7f7f in one VALU op: bit 7 of a byte set <=> sites differ
                    asm("v_xad_u32 %0, %1, %2, %3" : "=v"(y) : "v"(mine[ID_CW * c + k]), "s"(cur.v[k]), "v"(c7f));
                    mism += __builtin_popcount(y & 0x80808080u);
                }
                cur = nxt;
            }
        }
        const int d = DENOM == PLM_IDENT_DENOM_SHORTER ? min(my_res, res_b[t]) : L;
        if (!(exclude_self && t == s)) take_pair<DENOM>(r, t, Lm - mism, d, thresh, thr);
    }
    if (s < n_a) store_part(part, n_a, s, r);
}

// One register tile of the column-chunked form: the lane's row against the ID_TT rows t0 .. t0 + ID_TT - 1 of B (row
// indices past t_last are clamped to it: the caller ignores their results), 16 dwords of the lane's row at a time.
// mism[tt]: sites that differ; ngap[tt] (BOTH): sites of the padded row where either side has the gap.
template <bool BOTH>
__device__ __forceinline__ void tile_compare(const u32 *__restrict__ myrow, const u32 *__restrict__ b32, int Lw, int t0,
                                             int t_last, int gap_mode, int (&mism)[ID_TT], int (&ngap)[BOTH ? ID_TT : 1]) {
#pragma unroll
    for (int k = 0; k < ID_TT; k++) mism[k] = 0;
    if constexpr (BOTH) {
#pragma unroll
        for (int k = 0; k < ID_TT; k++) ngap[k] = 0;
    }
    for (int c0 = 0; c0 < Lw; c0 += ID_CW) {   // Lw is a multiple of ID_CW
        u32 mine[ID_CW], mgap[BOTH ? ID_CW : 1];
#pragma unroll
        for (int k = 0; k < ID_CW; k++) {
            mine[k] = myrow[c0 + k];
            if constexpr (BOTH) mgap[k] = zero_bytes(mine[k]);
            if (gap_mode) mine[k] = gaps_to_sentinel(mine[k]);
        }
#pragma unroll
        for (int tt = 0; tt < ID_TT; tt++) {
            const u32 *__restrict__ trow = b32 + (size_t)min(t0 + tt, t_last) * Lw + c0;
            int acc = mism[tt];
#pragma unroll
            for (int k = 0; k < ID_CW; k++) {
                const u32 other = trow[k];
                const u32 y = (mine[k] ^ other) + 0x7f7f7f7fu;      // bit 7 set <=> sites differ
                acc += __builtin_popcount(y & 0x80808080u);
                if constexpr (BOTH) ngap[tt] += __builtin_popcount(mgap[k] | zero_bytes(other));
            }
            mism[tt] = acc;
        }
    }
}

template <int DENOM>
__device__ __forceinline__ int pair_denominator(int L, int Lw, int ngap, int my_res, int other_res) {
    if constexpr (DENOM == PLM_IDENT_DENOM_BOTH) return 4 * Lw - ngap;     // the padding is gap on both sides
    else if constexpr (DENOM == PLM_IDENT_DENOM_SHORTER) return min(my_res, other_res);
    else return L;
}

// Column-chunked form: any row length, every denominator.
template <int DENOM>
__global__ __launch_bounds__(256) void k_ident_chunk(const u32 *__restrict__ a32, int n_a, const u32 *__restrict__ b32,
                                                    int n_b_arg, const int32_t *__restrict__ n_b_dev, int Lw, int Lm, int L,
                                                    const int32_t *__restrict__ res_a, const int32_t *__restrict__ res_b,
                                                    const int32_t *__restrict__ thr, int thresh, int gap_mode,
                                                    int exclude_self, int tper, int32_t *__restrict__ part) {
    constexpr bool BOTH = DENOM == PLM_IDENT_DENOM_BOTH;
    const int n_b = n_b_dev ? *n_b_dev : n_b_arg;
    const int s = blockIdx.x * ID_BLK + threadIdx.x;
    const int sr = min(s, n_a - 1);
    const int tb0 = blockIdx.y * tper, tb1 = min(n_b, tb0 + tper);
    const u32 *__restrict__ myrow = a32 + (size_t)sr * Lw;
    const int my_res = DENOM == PLM_IDENT_DENOM_SHORTER ? res_a[sr] : 0;
    Best r = {0, -1, 0, 0};
    for (int t0 = tb0; t0 < tb1; t0 += ID_TT) {
        int mism[ID_TT], ngap[BOTH ? ID_TT : 1];
        tile_compare<BOTH>(myrow, b32, Lw, t0, tb1 - 1, gap_mode, mism, ngap);
#pragma unroll
        for (int tt = 0; tt < ID_TT; tt++) {
            const int t = t0 + tt;
            if (t < tb1 && !(exclude_self && t == s)) {
                const int other_res = DENOM == PLM_IDENT_DENOM_SHORTER ? res_b[t] : 0;
                const int d = pair_denominator<DENOM>(L, Lw, ngap[BOTH ? tt : 0], my_res, other_res);
                take_pair<DENOM>(r, t, Lm - mism[tt], d, thresh, thr);
            }
        }
    }
    if (s < n_a) store_part(part, n_a, s, r);
}

// the splits in ascending order of their B ranges, with the rule of take_pair: the smallest index of a tie survives
__global__ __launch_bounds__(256) void k_ident_merge(const int32_t *__restrict__ part, int splits, int n_a,
                                                    int32_t *__restrict__ n_within, int32_t *__restrict__ best_index,
                                                    int32_t *__restrict__ best_match, int32_t *__restrict__ best_denom) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_a) return;
    const size_t plane = (size_t)splits * n_a;
    Best r = {0, -1, 0, 0};
    for (int k = 0; k < splits; k++) {
        const size_t o = (size_t)k * n_a + s;
        r.cnt += part[o];
        const int bi = part[o + plane], bm = part[o + 2 * plane], bd = part[o + 3 * plane];
        if (bi >= 0 && (r.bi < 0 || nearer(bm, bd, r.bm, r.bd))) { r.bi = bi; r.bm = bm; r.bd = bd; }
    }
    if (n_within) n_within[s] = r.cnt;
    if (best_index) best_index[s] = r.bi;
    if (best_match) best_match[s] = r.bm;
    if (best_denom) best_denom[s] = r.bd;
}

// Greedy filter, step 2: the similarity bits of the block r0 .. r0 + 255 with itself.  Workgroup y compares every row
// of the block with the rows r0 + 32 y .. r0 + 32 y + 31: bits[row in block][y], bit tt <=> similar to row r0 + 32 y + tt.
template <int DENOM>
__global__ __launch_bounds__(256) void k_ident_bits(const u32 *__restrict__ msa32, int N, int r0, int Lw, int Lm, int L,
                                                   const int32_t *__restrict__ res, const int32_t *__restrict__ thr,
                                                   int thresh, int gap_mode, u32 *__restrict__ bits) {
    constexpr bool BOTH = DENOM == PLM_IDENT_DENOM_BOTH;
    const int s = min(r0 + (int)threadIdx.x, N - 1);
    const int t0 = r0 + ID_TT * blockIdx.y;
    const int my_res = DENOM == PLM_IDENT_DENOM_SHORTER ? res[s] : 0;
    int mism[ID_TT], ngap[BOTH ? ID_TT : 1];
    tile_compare<BOTH>(msa32 + (size_t)s * Lw, msa32, Lw, t0, N - 1, gap_mode, mism, ngap);
    u32 w = 0;
#pragma unroll
    for (int tt = 0; tt < ID_TT; tt++) {
        const int t = min(t0 + tt, N - 1);
        const int other_res = DENOM == PLM_IDENT_DENOM_SHORTER ? res[t] : 0;
        const int d = pair_denominator<DENOM>(L, Lw, ngap[BOTH ? tt : 0], my_res, other_res);
        if (t0 + tt < N && similar<DENOM>(Lm - mism[tt], d, thresh, thr)) w |= 1u << tt;
    }
    bits[threadIdx.x * ID_BW + blockIdx.y] = w;
}

// Greedy filter, step 3 (one workgroup): a row of the block falls to a kept row of an earlier block (the counts of the
// cross pass, part[split][row]) or to a kept earlier row of its own block (bits); wave 0 walks the block in order, lane
// w < 8 holding word w of the kept mask.  The kept rows are then appended to the compact image the next cross passes
// read, and the number of kept rows moves on.
__global__ __launch_bounds__(256) void k_ident_resolve(const int32_t *__restrict__ part, int splits, int n_rows, int r0,
                                                      const u32 *__restrict__ bits, const u32 *__restrict__ msa32, int Lw,
                                                      const int32_t *__restrict__ res, u32 *__restrict__ kept32,
                                                      int32_t *__restrict__ kept_res, int32_t *__restrict__ n_kept,
                                                      uint8_t *__restrict__ keep_out) {
    __shared__ u32 sim[ID_BLK][ID_BW + 1];
    __shared__ int dropped[ID_BLK];
    __shared__ u32 keptw[ID_BW];
    const int s = threadIdx.x;
    const int base = *n_kept;
    int hits = 0;
    if (s < n_rows)
        for (int k = 0; k < splits; k++) hits += part[(size_t)k * n_rows + s];
    dropped[s] = (s >= n_rows || hits > 0) ? 1 : 0;
#pragma unroll
    for (int w = 0; w < ID_BW; w++) sim[s][w] = bits[s * ID_BW + w];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        u32 kw = 0;
        for (int row = 0; row < n_rows; row++) {
            const u32 v = lane < ID_BW ? (sim[row][lane] & kw) : 0u;
            const bool keep = !__any(v != 0) && !dropped[row];
            if (keep && lane == (row >> 5)) kw |= 1u << (row & 31);
        }
        if (lane < ID_BW) keptw[lane] = kw;
    }
    __syncthreads();     // every thread has read *n_kept by now
    const bool keep = (keptw[s >> 5] >> (s & 31)) & 1u;
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < ID_BW; w++) {
        const int c = __builtin_popcount(keptw[w]);
        total += c;
        if (w < (s >> 5)) before += c;
    }
    before += __builtin_popcount(keptw[s >> 5] & ((1u << (s & 31)) - 1u));
    if (s < n_rows) {
        keep_out[r0 + s] = keep ? 1 : 0;
        if (keep) {
            const u32 *__restrict__ src = msa32 + (size_t)(r0 + s) * Lw;
            u32 *__restrict__ dst = kept32 + (size_t)(base + before) * Lw;
            for (int k = 0; k < Lw; k += 4) *(uint4 *)(dst + k) = *(const uint4 *)(src + k);
            kept_res[base + before] = res[r0 + s];
        }
    }
    if (s == 0) *n_kept = base + total;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct IdentRule {     // what the kernels need of plm_ident_opts and the row length
    int L, Lw, Lm, denom, gap_mode, thresh;
    std::vector<int32_t> thr;      // [L + 1], BOTH / SHORTER
};

int ident_rule(const plm_ident_opts *o, int L, IdentRule *r) {
    if (!o) return plm_fail(PLM_EINVAL, "NULL opts");
    if (L <= 0) return plm_fail(PLM_EINVAL, "n_sites must be positive (got %d)", L);
    if (o->gap_state < -1 || o->gap_state > 126) return plm_fail(PLM_EINVAL, "gap state %d outside -1..126", o->gap_state);
    if (o->denominator != PLM_IDENT_DENOM_COLUMNS && o->denominator != PLM_IDENT_DENOM_BOTH &&
        o->denominator != PLM_IDENT_DENOM_SHORTER)
        return plm_fail(PLM_EINVAL, "unknown denominator %d", o->denominator);
    if (o->denominator != PLM_IDENT_DENOM_COLUMNS && o->gap_state < 0)
        return plm_fail(PLM_EINVAL, "the denominators BOTH and SHORTER need a gap state");
    if (!std::isfinite(o->threshold)) return plm_fail(PLM_EINVAL, "the threshold is not finite");
    if ((long long)L + 4 * ID_CW > INT_MAX / 4) return plm_fail(PLM_EINVAL, "n_sites %d is too large", L);
    r->L = L;
    r->Lw = ((L + 4 * ID_CW - 1) / (4 * ID_CW)) * ID_CW;
    r->denom = o->denominator;
    r->gap_mode = o->gap_state >= 0 ? 1 : 0;
    r->Lm = r->gap_mode ? 4 * r->Lw : L;     // matches = Lm - mismatches (file header)
    const double theta = o->threshold;
    // clamped: beyond +-(L + 1) every value decides alike, and the cast stays defined
    auto rule = [&](int d) { return (int)std::min(std::max(std::ceil(theta * (double)d - 1e-9), -1.0), (double)L + 1.0); };
    r->thresh = rule(L);                     // the expression of the reweighting (cluster_threshold, plm_host.cpp)
    r->thr.assign((size_t)L + 1, INT_MAX);
    for (int d = 1; d <= L; d++) r->thr[d] = rule(d);
    return PLM_OK;
}

// PLM_IDENT_TPER: rows of B per workgroup, or 0 when it is not set
int ident_forced_tper(int *out) {
    *out = 0;
    const char *v = getenv("PLM_IDENT_TPER");
    if (!v) return PLM_OK;
    char *end = nullptr;
    errno = 0;
    const long x = strtol(v, &end, 10);
    if (errno || end == v || *end || x < 1 || x > INT_MAX)
        return plm_fail(PLM_EINVAL, "PLM_IDENT_TPER must be a positive integer (got '%s')", v);
    *out = (int)x;
    return PLM_OK;
}

// The device image of a set (file header) and, with a gap state, the residues of every row.
int ident_image(const int8_t *x, int n, const IdentRule &r, int gap_state, const char *what, std::vector<int8_t> *rows,
                std::vector<int32_t> *res) {
    const size_t row_len = (size_t)r.Lw * 4;
    rows->assign((size_t)n * row_len, r.gap_mode ? (int8_t)0 : (int8_t)127);
    res->assign((size_t)n, r.L);
    for (int s = 0; s < n; s++) {
        const int8_t *src = x + (size_t)s * r.L;
        int8_t *dst = rows->data() + (size_t)s * row_len;
        int gaps = 0;
        for (int i = 0; i < r.L; i++) {
            const int8_t v = src[i];
            if (v < 0 || v > 126) return plm_fail(PLM_EINVAL, "%s[%d][%d] = %d outside 0..126", what, s, i, (int)v);
            if (r.gap_mode) {      // the gap state and state 0 change places: the gap is byte 0 on the device
                dst[i] = v == gap_state ? (int8_t)0 : v == 0 ? (int8_t)gap_state : v;
                gaps += v == gap_state;
            } else {
                dst[i] = v;
            }
        }
        (*res)[s] = r.L - gaps;
    }
    return PLM_OK;
}

struct CrossArgs {
    const u32 *a, *b;
    int n_a, n_b;
    const int32_t *n_b_dev, *res_a, *res_b, *thr;
    int exclude_self, tper, splits;
    int32_t *part;
};

template <int DENOM> hipError_t launch_cross_denom(const IdentRule &r, const CrossArgs &x, hipStream_t st) {
    const dim3 grid((x.n_a + ID_BLK - 1) / ID_BLK, x.splits), block(ID_BLK);
#define IDENT_ARGS x.a, x.n_a, x.b, x.n_b, x.n_b_dev, r.Lw, r.Lm, r.L, x.res_a, x.res_b, x.thr, r.thresh, r.gap_mode, \
                   x.exclude_self, x.tper, x.part
    if constexpr (DENOM != PLM_IDENT_DENOM_BOTH) {     // BOTH counts per pair and column: the chunked form only
        if (r.Lw <= 32) hipLaunchKernelGGL((k_ident_reg<32, DENOM>), grid, block, 0, st, IDENT_ARGS);
        else if (r.Lw <= 64) hipLaunchKernelGGL((k_ident_reg<64, DENOM>), grid, block, 0, st, IDENT_ARGS);
        else if (r.Lw <= 96) hipLaunchKernelGGL((k_ident_reg<96, DENOM>), grid, block, 0, st, IDENT_ARGS);
        else if (r.Lw <= 128) hipLaunchKernelGGL((k_ident_reg<128, DENOM>), grid, block, 0, st, IDENT_ARGS);
        else if (r.Lw <= ID_REG_MAX) hipLaunchKernelGGL((k_ident_reg<ID_REG_MAX, DENOM>), grid, block, 0, st, IDENT_ARGS);
        else hipLaunchKernelGGL((k_ident_chunk<DENOM>), grid, block, 0, st, IDENT_ARGS);
    } else {
        hipLaunchKernelGGL((k_ident_chunk<DENOM>), grid, block, 0, st, IDENT_ARGS);
    }
#undef IDENT_ARGS
    return hipGetLastError();
}

hipError_t launch_cross(const IdentRule &r, const CrossArgs &x, hipStream_t st) {
    if (r.denom == PLM_IDENT_DENOM_BOTH) return launch_cross_denom<PLM_IDENT_DENOM_BOTH>(r, x, st);
    if (r.denom == PLM_IDENT_DENOM_SHORTER) return launch_cross_denom<PLM_IDENT_DENOM_SHORTER>(r, x, st);
    return launch_cross_denom<PLM_IDENT_DENOM_COLUMNS>(r, x, st);
}

// rows of B per workgroup and the number of splits: about `want_blocks` workgroups in all, whole register tiles
void ident_split(int n_a, int n_b, int forced_tper, int want_blocks, int *tper, int *splits) {
    const int xblocks = (n_a + ID_BLK - 1) / ID_BLK;
    int t = forced_tper;
    if (!t) {
        const int want = std::max(1, (want_blocks + xblocks - 1) / xblocks);
        t = (n_b + want - 1) / want;
        t = ((t + ID_TT - 1) / ID_TT) * ID_TT;
    }
    *tper = std::min(t, std::max(n_b, 1));
    *splits = std::max(1, (n_b + *tper - 1) / *tper);
}

}  // namespace

int plm_cross_identities(const int8_t *a, int32_t n_a, const int8_t *b, int32_t n_b, int32_t n_sites,
                         const plm_ident_opts *opts, int32_t *best_index, int32_t *best_match, int32_t *best_denom,
                         int32_t *n_within, int device, void *stream) {
    if (!a || !b) return plm_fail(PLM_EINVAL, "NULL sequences");
    if (n_a <= 0 || n_b <= 0) return plm_fail(PLM_EINVAL, "empty set (n_a = %d, n_b = %d)", n_a, n_b);
    if (n_a > ID_MAX_ROWS || n_b > ID_MAX_ROWS) return plm_fail(PLM_EINVAL, "more than 2^30 rows (n_a = %d, n_b = %d)", n_a, n_b);
    IdentRule r;
    PLM_TRY(ident_rule(opts, n_sites, &r));
    int forced = 0, tper = 0, splits = 0;
    PLM_TRY(ident_forced_tper(&forced));
    ident_split(n_a, n_b, forced, 2048, &tper, &splits);
    if (splits > 65535) return plm_fail(PLM_EINVAL, "PLM_IDENT_TPER = %d splits %d rows into more than 65535 ranges", forced, n_b);
    std::vector<int8_t> img_a, img_b;
    std::vector<int32_t> res_a, res_b;
    PLM_TRY(ident_image(a, n_a, r, opts->gap_state, "a", &img_a, &res_a));
    PLM_TRY(ident_image(b, n_b, r, opts->gap_state, "b", &img_b, &res_b));
    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n_part = (size_t)4 * splits * n_a;
    PLM_TRY(plm_check_free((double)img_a.size() + (double)img_b.size() +
                           sizeof(int32_t) * ((double)n_part + 5.0 * n_a + n_b + r.thr.size()), "plm_cross_identities"));
    u32 *da = nullptr, *db = nullptr;
    int32_t *dra = nullptr, *drb = nullptr, *dthr = nullptr, *part = nullptr, *out = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&da, img_a.size() / 4));
    PLM_TRY(mem.alloc(&db, img_b.size() / 4));
    PLM_TRY(mem.alloc(&dra, (size_t)n_a));
    PLM_TRY(mem.alloc(&drb, (size_t)n_b));
    PLM_TRY(mem.alloc(&dthr, r.thr.size()));
    PLM_TRY(mem.alloc(&part, n_part));
    PLM_TRY(mem.alloc(&out, (size_t)4 * n_a));
    PLM_HIP(hipMemcpyAsync(da, img_a.data(), img_a.size(), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(db, img_b.data(), img_b.size(), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dra, res_a.data(), sizeof(int32_t) * n_a, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(drb, res_b.data(), sizeof(int32_t) * n_b, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dthr, r.thr.data(), sizeof(int32_t) * r.thr.size(), hipMemcpyHostToDevice, st));
    const CrossArgs x = {da, db, n_a, n_b, nullptr, dra, drb, dthr, opts->exclude_self ? 1 : 0, tper, splits, part};
    PLM_HIP(launch_cross(r, x, st));
    hipLaunchKernelGGL(k_ident_merge, dim3((n_a + 255) / 256), dim3(256), 0, st, part, splits, n_a, out, out + n_a,
                       out + 2 * (size_t)n_a, out + 3 * (size_t)n_a);
    PLM_HIP(hipGetLastError());
    int32_t *const host[4] = {n_within, best_index, best_match, best_denom};
    for (int k = 0; k < 4; k++)
        if (host[k])
            PLM_HIP(hipMemcpyAsync(host[k], out + (size_t)k * n_a, sizeof(int32_t) * n_a, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_redundancy_filter(const int8_t *msa, int32_t n_seqs, int32_t n_sites, const plm_ident_opts *opts,
                          uint8_t *keep_out, int32_t *n_kept, int device, void *stream) {
    if (!msa || !keep_out) return plm_fail(PLM_EINVAL, "NULL alignment or keep_out");
    if (n_seqs <= 0) return plm_fail(PLM_EINVAL, "empty alignment (n_seqs = %d)", n_seqs);
    if (n_seqs > ID_MAX_ROWS) return plm_fail(PLM_EINVAL, "more than 2^30 rows (n_seqs = %d)", n_seqs);
    IdentRule r;
    PLM_TRY(ident_rule(opts, n_sites, &r));
    int forced = 0;
    PLM_TRY(ident_forced_tper(&forced));       // validated like everywhere; the passes below split on their own
    std::vector<int8_t> img;
    std::vector<int32_t> res;
    PLM_TRY(ident_image(msa, n_seqs, r, opts->gap_state, "msa", &img, &res));
    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    const int N = n_seqs;
    const size_t n_part = (size_t)4 * ID_FILTER_WGS * ID_BLK;     // ident_split makes at most ID_FILTER_WGS splits
    PLM_TRY(plm_check_free(2.0 * (double)img.size() + sizeof(int32_t) * ((double)n_part + 2.0 * N + r.thr.size()) + N,
                           "plm_redundancy_filter"));
    u32 *dm = nullptr, *dk = nullptr, *bits = nullptr;
    int32_t *dres = nullptr, *dkres = nullptr, *dthr = nullptr, *part = nullptr, *dn = nullptr;
    uint8_t *dkeep = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&dm, img.size() / 4));
    PLM_TRY(mem.alloc(&dk, img.size() / 4));
    PLM_TRY(mem.alloc(&dres, (size_t)N));
    PLM_TRY(mem.alloc(&dkres, (size_t)N));
    PLM_TRY(mem.alloc(&dthr, r.thr.size()));
    PLM_TRY(mem.alloc(&part, n_part));
    PLM_TRY(mem.alloc(&bits, (size_t)ID_BLK * ID_BW));
    PLM_TRY(mem.alloc(&dn, (size_t)1));
    PLM_TRY(mem.alloc(&dkeep, (size_t)N));
    PLM_HIP(hipMemcpyAsync(dm, img.data(), img.size(), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dres, res.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(dthr, r.thr.data(), sizeof(int32_t) * r.thr.size(), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemsetAsync(dn, 0, sizeof(int32_t), st));
    for (int r0 = 0; r0 < N; r0 += ID_BLK) {
        const int rows = std::min(ID_BLK, N - r0);
        int tper = 0, splits = 0;
        if (r0 > 0) {     // step 1: the block against the kept rows of the earlier blocks (at most r0 of them)
            ident_split(rows, r0, 0, ID_FILTER_WGS, &tper, &splits);
            const CrossArgs x = {dm + (size_t)r0 * r.Lw, dk, rows, r0, dn, dres + r0, dkres, dthr, 0, tper, splits, part};
            PLM_HIP(launch_cross(r, x, st));
        }
#define IDENT_BITS(D) hipLaunchKernelGGL((k_ident_bits<D>), dim3(1, ID_BW), dim3(ID_BLK), 0, st, dm, N, r0, r.Lw, r.Lm, \
                                         r.L, dres, dthr, r.thresh, r.gap_mode, bits)
        if (r.denom == PLM_IDENT_DENOM_BOTH) IDENT_BITS(PLM_IDENT_DENOM_BOTH);
        else if (r.denom == PLM_IDENT_DENOM_SHORTER) IDENT_BITS(PLM_IDENT_DENOM_SHORTER);
        else IDENT_BITS(PLM_IDENT_DENOM_COLUMNS);
#undef IDENT_BITS
        PLM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ident_resolve, dim3(1), dim3(ID_BLK), 0, st, part, splits, rows, r0, bits, dm, r.Lw, dres, dk,
                           dkres, dn, dkeep);
        PLM_HIP(hipGetLastError());
    }
    int32_t kept = 0;
    PLM_HIP(hipMemcpyAsync(keep_out, dkeep, (size_t)N, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipMemcpyAsync(&kept, dn, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    if (n_kept) *n_kept = kept;
    return PLM_OK;
}
