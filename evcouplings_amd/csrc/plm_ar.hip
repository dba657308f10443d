// plm_ar.hip -- the autoregressive Potts model (DESIGN_NEXT_ROWS.md section 9.19):
//     P(x) = prod_i P(x_i | x_<i),   P(x_i = b | x_<i) = softmax_b( h_i(b) + sum_{j<i} J_ji(x_j, b) )
// exact log-probabilities (plm_ar_logprob), ancestral sampling (plm_ar_sample), the regularised negative log-likelihood
// with its gradient (plm_ar_eval) and the L-BFGS fit (plm_ar_fit).  The parameters are the canonical vector of
// plm_hamiltonians: block (j, i), j < i, entry [a][b] couples state a of the EARLIER site j with state b of the LATER
// site i and enters the conditional of site i only.
//
// Every kernel reads the couplings "by later site": for site i one contiguous table [j < i][a][QP] (QP = q rounded up
// to 4), table i behind table i - 1, so pair (j, i) is row block i (i - 1) / 2 + j.  A conditional gathers one padded
// row per earlier site; the chunks of a table go through LDS, a workgroup owning (site, tile of sequences or chains).
// The float64 paths make every sum in an order the shape alone fixes: no floating-point atomics anywhere.
#include "plm_gibbs_device.h"
#include "plm_host_util.h"
#include "plm_internal.h"
#include "plm_lbfgs_driver.h"

#include <math.h>
#include <stdlib.h>
#include <cmath>
#include <type_traits>

namespace {

#define AR_STAGE_BYTES 32768          // LDS of one staged chunk of a table
#define AR_SUM_BLOCKS 256             // workgroups of the first stage of k_ar_sums

__host__ __device__ inline int64_t ar_tri(int64_t i) { return i * (i - 1) / 2; }      // pairs (j, k) with j < k < i

// pair t of the by-later-site order -> (j, i); exact for every t below 2^52
__device__ __forceinline__ void ar_pair_of(int64_t t, int *j, int *i) {
    int64_t k = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
    while (ar_tri(k) > t) k--;
    while (ar_tri(k + 1) <= t) k++;
    *i = (int)k;
    *j = (int)(t - ar_tri(k));
}
// index of block (j, i), j < i, in the canonical order (row-major over the upper triangle)
__device__ __forceinline__ int64_t ar_canon_pair(int j, int i, int L) {
    return (int64_t)j * L - (int64_t)j * (j + 1) / 2 + (i - j - 1);
}

// ---- repack: canonical -> by later site, rows padded to QP floats ---------------------------------------------------
__global__ __launch_bounds__(256) void k_ar_repack(const float *__restrict__ canon, int L, int q, int QP,
                                                   float *__restrict__ T) {
    int j, i;
    ar_pair_of(blockIdx.x, &j, &i);
    const float *src = canon + (int64_t)L * q + ar_canon_pair(j, i, L) * q * q;
    float *dst = T + (int64_t)blockIdx.x * q * QP;
    for (int k = threadIdx.x; k < q * QP; k += 256) {
        const int a = k / QP, b = k - a * QP;
        dst[k] = b < q ? src[a * q + b] : 0.f;
    }
}

// sequences [n][L] -> columns [L][n]: the lanes of a conditional are sequences and read one site at a time
__global__ __launch_bounds__(256) void k_ar_columns(const int8_t *__restrict__ x, int n, int L, int8_t *__restrict__ xT) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)n * L) return;
    const int j = (int)(k / n), s = (int)(k - (int64_t)j * n);
    xT[k] = x[(int64_t)s * L + j];
}

// one chunk of table i, sites [j0, j1), from global memory into LDS rows of NVP float4 (NVP odd: rows of different
// states start in different banks)
template <int NV, int NVP>
__device__ __forceinline__ void ar_stage(const float4 *__restrict__ Ti, int j0, int j1, int q, float4 *stage) {
    const int n4 = (j1 - j0) * q * NV;
    const float4 *src = Ti + (int64_t)j0 * q * NV;
    for (int k = threadIdx.x; k < n4; k += blockDim.x) stage[(k / NV) * NVP + (k % NV)] = src[k];
}

// ---- the conditionals in float64 (plm_ar_logprob, plm_ar_eval) ------------------------------------------------------
// A workgroup owns (site i, 256 sequences); a lane carries the q logits of its sequence in registers.  logit_b starts as
// (double) h_i(b) and takes one float64 add per j = 0 .. i-1 in that order; the log-softmax is max, then the sum of exp
// in state order.  Sites are launched last first: site i costs i rows.
//   site_lp [n][L]: log P(x_si | x_s,<i);  RES: R [L][n][q] = w_s (delta(x_si, b) - p_sib)
template <int NV, bool RES>
__global__ __launch_bounds__(256) void k_ar_cond(const float *__restrict__ T, const float *__restrict__ h,
                                                 const int8_t *__restrict__ xT, const double *__restrict__ w, int L, int q,
                                                 int n, int JC, double *__restrict__ site_lp, double *__restrict__ R) {
    constexpr int NVP = (NV % 2 == 0) ? NV + 1 : NV;
    extern __shared__ float4 lds4[];
    const int i = L - 1 - (int)blockIdx.y;
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int sc = min(s, n - 1);
    double U[NV * 4];
#pragma unroll
    for (int b = 0; b < NV * 4; b++) U[b] = b < q ? (double)h[i * q + b] : 0.0;
    const float4 *Ti = (const float4 *)T + ar_tri(i) * q * NV;
    for (int j0 = 0; j0 < i; j0 += JC) {
        const int j1 = min(i, j0 + JC);
        __syncthreads();
        ar_stage<NV, NVP>(Ti, j0, j1, q, lds4);
        __syncthreads();
        for (int j = j0; j < j1; j++) {
            const int x = xT[(int64_t)j * n + sc];
            const float4 *row = lds4 + ((j - j0) * q + x) * NVP;
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const float4 r = row[v];
                U[4 * v + 0] += (double)r.x;
                U[4 * v + 1] += (double)r.y;
                U[4 * v + 2] += (double)r.z;
                U[4 * v + 3] += (double)r.w;
            }
        }
    }
    if (s >= n) return;
    const int xi = xT[(int64_t)i * n + s];
    double m = -INFINITY, ux = 0.0;
#pragma unroll
    for (int b = 0; b < NV * 4; b++) {
        if (b < q) m = fmax(m, U[b]);
        ux = b == xi ? U[b] : ux;
    }
    double S = 0.0;
#pragma unroll
    for (int b = 0; b < NV * 4; b++) {
        U[b] = b < q ? exp(U[b] - m) : 0.0;
        S += U[b];
    }
    site_lp[(int64_t)s * L + i] = (ux - m) - log(S);
    if (RES) {
        const double ws = w[s];
        double *r = R + ((int64_t)i * n + s) * q;
#pragma unroll
        for (int b = 0; b < NV * 4; b++)
            if (b < q) r[b] = ws * ((b == xi ? 1.0 : 0.0) - U[b] / S);
    }
}

// log P of a sequence: its site terms in site order
__global__ __launch_bounds__(256) void k_ar_logp(const double *__restrict__ site_lp, int n, int L, double *__restrict__ logp) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    double t = 0.0;
    for (int i = 0; i < L; i++) t += site_lp[(int64_t)s * L + i];
    logp[s] = t;
}

// the sum of 256 lanes' values by a fixed tree; every lane gets it
__device__ __forceinline__ double ar_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}

// out[0] = sum_s w_s log P(x_s): one workgroup, lane t takes s = t, t + 256, ..., then the tree
__global__ __launch_bounds__(256) void k_ar_wsum(const double *__restrict__ w, const double *__restrict__ logp, int n,
                                                 double *out) {
    __shared__ double red[256];
    double t = 0.0;
    for (int s = threadIdx.x; s < n; s += 256) t += w[s] * logp[s];
    t = ar_block_sum(t, red);
    if (threadIdx.x == 0) out[0] = t;
}

// ---- the gradient ---------------------------------------------------------------------------------------------------
// fields: a workgroup per site; lane (slice, b) sums R over s = slice, slice + 256 / q, ..., state b then sums the slices
__global__ __launch_bounds__(256) void k_ar_grad_h(const double *__restrict__ R, const float *__restrict__ x, int q, int n,
                                                   double neff, double lambda_h, double *__restrict__ g) {
    __shared__ double part[256];
    const int i = blockIdx.x, nsl = 256 / q, b = threadIdx.x % q, sl = threadIdx.x / q;
    double acc = 0.0;
    if (sl < nsl)
        for (int s = sl; s < n; s += nsl) acc += R[((int64_t)i * n + s) * q + b];
    part[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < q) {
        double t = 0.0;
        for (int k = 0; k < nsl; k++) t += part[k * q + threadIdx.x];
        g[i * q + threadIdx.x] = -(t / neff) + 2.0 * lambda_h * (double)x[i * q + threadIdx.x];
    }
}

// couplings, the one-hot^T x residual product over sequences: a workgroup owns (site i, 256 / q earlier sites from j0,
// slice blockIdx.y of the sequences).  Lane (j, b) owns the LDS column acc[j][.][b] and adds r_sib at row x_sj: no two
// lanes touch the same word, so there is neither a barrier nor an atomic, and the order is the sequence loop's.
//   P [slices][pairs by later site][q][q]
__global__ __launch_bounds__(256) void k_ar_grad_pair(const double *__restrict__ R, const int8_t *__restrict__ xT,
                                                      const int2 *__restrict__ tiles, int q, int n, int per_slice,
                                                      int64_t n_pairs, double *__restrict__ P) {
    extern __shared__ double acc[];
    const int i = tiles[blockIdx.x].x, j0 = tiles[blockIdx.x].y;
    const int JT = 256 / q, jl = threadIdx.x / q, b = threadIdx.x % q, j = j0 + jl;
    if (jl >= JT || j >= i) return;
    double *col = acc + (int64_t)jl * q * q + b;
    for (int a = 0; a < q; a++) col[a * q] = 0.0;
    const int s0 = blockIdx.y * per_slice, s1 = min(n, s0 + per_slice);
    const int8_t *xj = xT + (int64_t)j * n;
    const double *Ri = R + (int64_t)i * n * q + b;
#pragma unroll 4
    for (int s = s0; s < s1; s++) col[(int)xj[s] * q] += Ri[(int64_t)s * q];
    double *dst = P + ((int64_t)blockIdx.y * n_pairs + ar_tri(i) + j) * q * q + b;
    for (int a = 0; a < q; a++) dst[a * q] = col[a * q];
}

// the slices in slice order, the division by N_eff after the sum, the regulariser, and the scatter back to the
// canonical order: a workgroup per pair
__global__ __launch_bounds__(256) void k_ar_pair_finish(const double *__restrict__ P, const float *__restrict__ x, int L,
                                                        int q, int n_slices, int64_t n_pairs, double neff, double lambda_j,
                                                        double *__restrict__ g) {
    int j, i;
    ar_pair_of(blockIdx.x, &j, &i);
    const int64_t dst = (int64_t)L * q + ar_canon_pair(j, i, L) * q * q;
    for (int k = threadIdx.x; k < q * q; k += 256) {
        double t = 0.0;
        for (int y = 0; y < n_slices; y++) t += P[((int64_t)y * n_pairs + blockIdx.x) * q * q + k];
        g[dst + k] = -(t / neff) + 2.0 * lambda_j * (double)x[dst + k];
    }
}

// sum h^2, sum J^2, g.g and g.d over the canonical vector in float64: AR_SUM_BLOCKS workgroups with a grid stride,
// then one workgroup over their partials.  g and d may be null.
__global__ __launch_bounds__(256) void k_ar_sums(const float *__restrict__ x, const double *__restrict__ g,
                                                 const float *__restrict__ d, int64_t nh, int64_t n, double *__restrict__ part) {
    __shared__ double red[256];
    double t[4] = {0, 0, 0, 0};      // every index below is a constant: the sums stay in registers
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)AR_SUM_BLOCKS * 256) {
        const double xv = (double)x[k], gv = g ? g[k] : 0.0;
        t[0] += k < nh ? xv * xv : 0.0;
        t[1] += k < nh ? 0.0 : xv * xv;
        t[2] += gv * gv;
        if (d) t[3] += gv * (double)d[k];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const double r = ar_block_sum(t[e], red);
        if (threadIdx.x == 0) part[e * AR_SUM_BLOCKS + blockIdx.x] = r;
    }
}
__global__ __launch_bounds__(256) void k_ar_sums_final(const double *__restrict__ part, double *out) {
    __shared__ double red[256];
    for (int e = 0; e < 4; e++) {
        const double r = ar_block_sum(part[e * AR_SUM_BLOCKS + threadIdx.x], red);
        if (threadIdx.x == 0) out[e] = r;
    }
}

// the gradient as the pair history takes it: rounded to float32 once, zeros behind the last parameter
__global__ __launch_bounds__(256) void k_ar_round(const double *__restrict__ g, int64_t n, int64_t n4, float *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n4) out[k] = k < n ? (float)g[k] : 0.f;
}

// ---- the sampler ----------------------------------------------------------------------------------------------------
// byte of site i of the tile's chain `lane`: four consecutive sites of a chain share a word (the xs layout of the
// tiled sweep kernels)
#define AR_XS(i, lane, tile) ((((i) >> 2) * (tile) + (lane)) * 4 + ((i) & 3))

// Tiled form: lanes are chains, the site loop is inside.  U_b starts as h_i(b) in float32 and takes one float32 add per
// j = 0 .. i-1 in that order; the draw is draw_state with the Philox counter (first_chain + c, 0, 0, i).
template <int NV>
__global__ __launch_bounds__(256) void k_ar_sample(const float *__restrict__ T, const float *__restrict__ h, int L, int q,
                                                   int C, int JC, uint32_t first_chain, uint32_t allowed, float beta,
                                                   uint32_t seed_lo, uint32_t seed_hi, int8_t *__restrict__ out) {
    constexpr int NVP = (NV % 2 == 0) ? NV + 1 : NV;
    extern __shared__ float4 lds4[];
    const int TILE = blockDim.x, tid = threadIdx.x;
    uint8_t *xs = (uint8_t *)(lds4 + JC * q * NVP);
    const int c0 = blockIdx.x * TILE;
    const int n_here = min(TILE, C - c0);
    for (int i = 0; i < L; i++) {
        float4 U[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) {
            U[v].x = 4 * v + 0 < q ? h[i * q + 4 * v + 0] : 0.f;
            U[v].y = 4 * v + 1 < q ? h[i * q + 4 * v + 1] : 0.f;
            U[v].z = 4 * v + 2 < q ? h[i * q + 4 * v + 2] : 0.f;
            U[v].w = 4 * v + 3 < q ? h[i * q + 4 * v + 3] : 0.f;
        }
        const float4 *Ti = (const float4 *)T + ar_tri(i) * q * NV;
        for (int j0 = 0; j0 < i; j0 += JC) {
            const int j1 = min(i, j0 + JC);
            __syncthreads();
            ar_stage<NV, NVP>(Ti, j0, j1, q, lds4);
            __syncthreads();
            for (int j = j0; j < j1; j++) {
                const int x = xs[AR_XS(j, tid, TILE)];
                const float4 *row = lds4 + ((j - j0) * q + x) * NVP;
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float4 r = row[v];
                    U[v].x += r.x; U[v].y += r.y; U[v].z += r.z; U[v].w += r.w;
                }
            }
        }
        const int a = draw_state<NV>(U, q, allowed, beta,
                                     philox_word0(first_chain + (uint32_t)(c0 + tid), 0u, 0u, (uint32_t)i, seed_lo, seed_hi));
        xs[AR_XS(i, tid, TILE)] = (uint8_t)a;
    }
    __syncthreads();
    for (int k = tid; k < n_here * L; k += TILE) {
        const int c = k / L, j = k - c * L;
        out[(int64_t)c0 * L + k] = (int8_t)xs[AR_XS(j, c, TILE)];
    }
}

// Direct form, for models whose chain states leave no room for a staged chunk: lanes = (chain, state) in groups of QG
// lanes (a power of two >= q), the rows read from global memory.  The same additions in the same order and draw_group:
// the same states as the tiled form, bit for bit.
template <int QG>
__global__ __launch_bounds__(256) void k_ar_sample_direct(const float *__restrict__ T, const float *__restrict__ h, int L,
                                                          int q, int QP, int C, uint32_t first_chain, uint32_t allowed,
                                                          float beta, uint32_t seed_lo, uint32_t seed_hi,
                                                          int8_t *__restrict__ out) {
    constexpr int CPW = 256 / QG;
    extern __shared__ float4 lds4[];
    uint8_t *xs = (uint8_t *)lds4;
    const int tid = threadIdx.x, a = tid % QG, cl = tid / QG;
    const int Lp = (L + 3) & ~3;
    const int c0 = blockIdx.x * CPW;
    const int n_here = min(CPW, C - c0);
    uint8_t *xc = xs + cl * Lp;
    for (int i = 0; i < L; i++) {
        const float *Ti = T + ar_tri(i) * q * QP;
        float U = a < q ? h[i * q + a] : 0.f;
        for (int j = 0; j < i; j++) {
            const int x = xc[j];
            if (a < q) U += Ti[((int64_t)j * q + x) * QP + a];
        }
        const int x = draw_group<QG>(U, a, q, allowed, beta,
                                     philox_word0(first_chain + (uint32_t)(c0 + cl), 0u, 0u, (uint32_t)i, seed_lo, seed_hi));
        if (a == 0) xc[i] = (uint8_t)x;
        __syncthreads();
    }
    for (int k = tid; k < n_here * L; k += 256) {
        const int c = k / L, j = k - c * L;
        out[(int64_t)c0 * L + k] = (int8_t)xs[c * Lp + j];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline int ar_nv(int q) { return (q + 3) / 4; }
inline int ar_nvp(int q) { return ar_nv(q) % 2 == 0 ? ar_nv(q) + 1 : ar_nv(q); }
// sites per staged chunk
inline int ar_jc(int q) { return std::max(1, AR_STAGE_BYTES / (q * ar_nvp(q) * 16)); }
inline double ar_table_bytes(int L, int q) { return 16.0 * ((double)L * (L - 1) / 2 * q * ar_nv(q)); }

// f(std::integral_constant<int, NV>) for the NV = ceil(q / 4) float4 of a row
template <class F> void ar_for_nv(int q, F f) {
    switch (ar_nv(q)) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    }
}

int ar_check_shape(int L, int q, const char *who) {
    if (L < 1) return plm_fail(PLM_EINVAL, "%s: need n_sites >= 1 (got %d)", who, L);
    if (q < 2 || q > GS_Q) return plm_fail(PLM_EUNSUPPORTED, "%s supports 2..32 states (got %d)", who, q);
    return PLM_OK;
}
int ar_check_states(const int8_t *x, int n, int L, int q, const char *what) {
    for (size_t k = 0; k < (size_t)n * L; k++)
        if (x[k] < 0 || x[k] >= q)
            return plm_fail(PLM_EINVAL, "%s[%zu][%zu] = %d outside 0..%d", what, k / L, k % L, (int)x[k], q - 1);
    return PLM_OK;
}

// The model on the device: the canonical vector is the caller's, the table is built from it.
hipError_t ar_repack(hipStream_t st, const float *canon, int L, int q, float *T) {
    if (L < 2) return hipSuccess;
    hipLaunchKernelGGL(k_ar_repack, dim3((unsigned)ar_tri(L)), dim3(256), 0, st, canon, L, q, ar_nv(q) * 4, T);
    return hipGetLastError();
}

// Everything an evaluation of n sequences needs on the device, and the launches of one evaluation.
struct ArEval {
    int L, q, n;
    bool grad;                // plm_ar_logprob: conditionals only
    int64_t n_can, n_pairs;
    int n_slices = 1, per_slice = 1;
    double neff = 1.0, lambda_h = 0, lambda_j = 0;
    std::vector<int2> h_tiles;
    int8_t *x = nullptr, *xT = nullptr;
    double *w = nullptr, *site = nullptr, *logp = nullptr, *R = nullptr, *P = nullptr, *part = nullptr;
    float *T = nullptr;
    int2 *tiles = nullptr;

    ArEval(int L_, int q_, int n_, bool grad_) : L(L_), q(q_), n(n_), grad(grad_) {
        n_can = (int64_t)plm_n_canon(L, q);
        n_pairs = ar_tri(L);
        if (!grad) return;
        // (site i, 256 / q earlier sites) tiles, the later sites first; the sequences are cut into slices only where
        // the tiles alone would leave most of the device idle
        const int JT = 256 / q;
        for (int i = L - 1; i >= 1; i--)
            for (int j0 = 0; j0 < i; j0 += JT) h_tiles.push_back(make_int2(i, j0));
        const int want = h_tiles.empty() ? 1 : (int)((1024 + h_tiles.size() - 1) / h_tiles.size());
        n_slices = std::max(1, std::min(std::min(16, want), (n + 255) / 256));
        per_slice = (n + n_slices - 1) / n_slices;
    }
    double bytes() const {
        double b = 2.0 * n * L + 8.0 * n * L + 16.0 * n + ar_table_bytes(L, q);
        if (grad) b += 8.0 * n * L * q + 8.0 * n_slices * n_pairs * q * q + 8.0 * h_tiles.size() + 8.0 * 4 * AR_SUM_BLOCKS;
        return b;
    }
    int alloc(DeviceBuffers &mem) {
        PLM_TRY(mem.alloc(&x, (size_t)n * L));
        PLM_TRY(mem.alloc(&xT, (size_t)n * L));
        PLM_TRY(mem.alloc(&site, (size_t)n * L));
        PLM_TRY(mem.alloc(&logp, (size_t)n));
        PLM_TRY(mem.alloc(&w, (size_t)n));
        PLM_TRY(mem.alloc(&T, (size_t)n_pairs * q * ar_nv(q) * 4));
        if (!grad) return PLM_OK;
        PLM_TRY(mem.alloc(&R, (size_t)n * L * q));
        PLM_TRY(mem.alloc(&P, (size_t)n_slices * n_pairs * q * q));
        PLM_TRY(mem.alloc(&tiles, h_tiles.size()));
        PLM_TRY(mem.alloc(&part, (size_t)4 * AR_SUM_BLOCKS));
        return PLM_OK;
    }
    // the sequences (and with a gradient the weights and the tile list); h_w may be null
    int upload(hipStream_t st, const int8_t *seqs, const double *h_w) {
        PLM_HIP(hipMemcpyAsync(x, seqs, (size_t)n * L, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ar_columns, dim3((unsigned)(((int64_t)n * L + 255) / 256)), dim3(256), 0, st, x, n, L, xT);
        PLM_HIP(hipGetLastError());
        if (h_w) PLM_HIP(hipMemcpyAsync(w, h_w, sizeof(double) * n, hipMemcpyHostToDevice, st));
        if (!h_tiles.empty())
            PLM_HIP(hipMemcpyAsync(tiles, h_tiles.data(), sizeof(int2) * h_tiles.size(), hipMemcpyHostToDevice, st));
        return PLM_OK;
    }
    // site terms and log P of the canonical vector xc (device); with a gradient also the residuals
    int conditionals(hipStream_t st, const float *xc) {
        PLM_HIP(ar_repack(st, xc, L, q, T));
        const int JC = ar_jc(q);
        const size_t lds = (size_t)JC * q * ar_nvp(q) * 16;
        const dim3 grid((unsigned)((n + 255) / 256), (unsigned)L);
        ar_for_nv(q, [&](auto nv) {
            constexpr int NV = decltype(nv)::value;
            if (grad) hipLaunchKernelGGL((k_ar_cond<NV, true>), grid, dim3(256), lds, st, T, xc, xT, w, L, q, n, JC, site, R);
            else hipLaunchKernelGGL((k_ar_cond<NV, false>), grid, dim3(256), lds, st, T, xc, xT, w, L, q, n, JC, site, R);
        });
        PLM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ar_logp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, site, n, L, logp);
        PLM_HIP(hipGetLastError());
        return PLM_OK;
    }
    // One evaluation at xc: g (device, canonical, double) and scal[0..4] = sum_s w_s log P(x_s), sum h^2, sum J^2, g.g
    // and, with a direction, g.d.  Nothing here waits for the device.
    int enqueue(hipStream_t st, const float *xc, double *g, double *scal, const float *dir) {
        PLM_TRY(conditionals(st, xc));
        hipLaunchKernelGGL(k_ar_wsum, dim3(1), dim3(256), 0, st, w, logp, n, scal);
        hipLaunchKernelGGL(k_ar_grad_h, dim3((unsigned)L), dim3(256), 0, st, R, xc, q, n, neff, lambda_h, g);
        PLM_HIP(hipGetLastError());
        if (!h_tiles.empty()) {
            const int JT = 256 / q;
            hipLaunchKernelGGL(k_ar_grad_pair, dim3((unsigned)h_tiles.size(), (unsigned)n_slices), dim3(256),
                               sizeof(double) * JT * q * q, st, R, xT, tiles, q, n, per_slice, n_pairs, P);
            hipLaunchKernelGGL(k_ar_pair_finish, dim3((unsigned)n_pairs), dim3(256), 0, st, P, xc, L, q, n_slices, n_pairs,
                               neff, lambda_j, g);
            PLM_HIP(hipGetLastError());
        }
        PLM_HIP(sums(st, xc, g, dir, scal + 1));
        return PLM_OK;
    }
    hipError_t sums(hipStream_t st, const float *xc, const double *g, const float *dir, double *out) {
        hipLaunchKernelGGL(k_ar_sums, dim3(AR_SUM_BLOCKS), dim3(256), 0, st, xc, g, dir, (int64_t)L * q, n_can, part);
        hipLaunchKernelGGL(k_ar_sums_final, dim3(1), dim3(256), 0, st, part, out);
        return hipGetLastError();
    }
    // F and its first term from the scalars of enqueue
    void objective(const double *scal, double *fx, double *nll) const {
        *nll = -(scal[0] / neff);
        *fx = *nll + lambda_h * scal[1] + lambda_j * scal[2];
    }
};

// the checks plm_ar_eval and plm_ar_fit share; *neff = sum_s w_s in sequence order
int ar_check_data(const int8_t *msa, const float *weights, int n, int L, int q, double lambda_h, double lambda_j,
                  const char *who, std::vector<double> *w, double *neff) {
    if (!msa || !weights) return plm_fail(PLM_EINVAL, "%s: NULL alignment or weights", who);
    if (n < 1) return plm_fail(PLM_EINVAL, "%s: need n_seqs >= 1 (got %d)", who, n);
    PLM_TRY(ar_check_shape(L, q, who));
    if ((double)n * L >= 2147483647.0) return plm_fail(PLM_EINVAL, "%s: n_seqs x n_sites must stay below 2^31", who);
    if (!(lambda_h >= 0) || !(lambda_j >= 0) || !std::isfinite(lambda_h) || !std::isfinite(lambda_j))
        return plm_fail(PLM_EINVAL, "%s: lambda_h and lambda_j must be finite and >= 0 (got %g, %g)", who, lambda_h, lambda_j);
    w->resize(n);
    double t = 0.0;
    for (int s = 0; s < n; s++) {
        if (!(weights[s] >= 0.f) || !std::isfinite(weights[s]))
            return plm_fail(PLM_EINVAL, "%s: weight %d is negative or not finite (%g)", who, s, (double)weights[s]);
        (*w)[s] = (double)weights[s];
        t += (*w)[s];
    }
    if (!(t > 0)) return plm_fail(PLM_EINVAL, "%s: the weights sum to zero", who);
    PLM_TRY(ar_check_states(msa, n, L, q, "msa"));
    *neff = t;
    return PLM_OK;
}

// ArEval as lbfgs_minimize (plm_lbfgs_driver.h) sees it: L-BFGS over float32 parameters with the float64 evaluation
// above, in one arithmetic -- no variable projection, no straddled pairs, no H0 diagonal, no debug output.  The gradient
// is rounded to float32 once, where it enters the history; f, g.d of a trial and of the start of a search, and the norms
// of the stop rule are the float64 sums of k_ar_sums.  One host synchronisation per evaluation.
struct ArProblem {
    enum { SL_EVAL = 0, SL_DG0 = 8, SL_EX = 12, SL_MD = 16, SL_COUNT = 16 + 3 * PLM_MAX_BASIS + 1 };
    static constexpr bool vp = false, debug = false;
    ArEval &ev;
    const hipStream_t st;
    const int m;
    const double eps;
    const int64_t nc = ev.n_can, n4 = (nc + 3) / 4 * 4;
    float *x = nullptr, *xp = nullptr, *g = nullptr, *gp = nullptr, *xa = nullptr, *ga = nullptr, *dir = nullptr, *S = nullptr;
    double *g64 = nullptr, *g64p = nullptr, *scal = nullptr, *scratch = nullptr, *h_scal = nullptr;
    int n_evals = 0;
    double gg = 0, hh = 0, xx = 0;      // float64 g.g, x.x over the fields, x.x at the last accepted point

    // F, its gradient (g64 and, rounded, g) at x; with a direction also g.d
    int evaluate(const float *direction) {
        PLM_TRY(ev.enqueue(st, x, g64, scal + SL_EVAL, direction));
        hipLaunchKernelGGL(k_ar_round, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, g64, nc, n4, g);
        PLM_HIP(hipGetLastError());
        n_evals++;
        return PLM_OK;
    }
    int fetch() {
        PLM_HIP(hipMemcpyAsync(h_scal, scal, sizeof(double) * SL_COUNT, hipMemcpyDeviceToHost, st));
        PLM_HIP(hipStreamSynchronize(st));
        return PLM_OK;
    }
    int start(LbfgsHistory &hist, LbfgsOutcome *out) {
        PLM_TRY(evaluate(nullptr));
        PLM_TRY(fetch());
        ev.objective(h_scal + SL_EVAL, &out->fx, &out->nll);
        if (!std::isfinite(out->fx)) return plm_fail(PLM_ENUMERIC, "plm_ar_fit: the objective is not finite at the start point");
        out->cond = read_norms();
        first_step(hist);
        return PLM_OK;
    }
    double read_norms() {      // of the evaluation just fetched; returns |g| / max(1, |x|)
        gg = h_scal[SL_EVAL + 3], hh = h_scal[SL_EVAL + 1], xx = hh + h_scal[SL_EVAL + 2];
        return std::sqrt(gg) / std::max(1.0, std::sqrt(xx));
    }
    LbfgsVectors vectors() const {
        return {x, g, xp, gp, xa, ga, dir, S, S + (size_t)m * n4, n4, 0, nullptr, scratch, scal + SL_MD, scal + SL_EX,
                h_scal + SL_MD, st};
    }
    // the history's g.g is the float32 gradient's: a steepest-descent step starts from the float64 one
    double first_step(LbfgsHistory &hist) const {
        hist.gDg = hist.gg = gg;
        return 1.0 / std::sqrt(gg);
    }
    void swap_points() {
        std::swap(x, xp);
        std::swap(g, gp);
        std::swap(g64, g64p);
    }
    // g.d at the point the search starts from, from its float64 gradient; it comes back with the first trial
    int begin_search() {
        PLM_HIP(ev.sums(st, xp, g64p, dir, scal + SL_DG0));
        return PLM_OK;
    }
    template <class Pass> int evaluate_trial(int, Pass &&gram_pass) {
        PLM_TRY(evaluate(dir));
        PLM_HIP(gram_pass());
        return fetch();
    }
    double search_dg0(double) const { return h_scal[SL_DG0 + 3]; }
    void trial_values(double *fx, double *nll, double *dg) const {
        ev.objective(h_scal + SL_EVAL, fx, nll);
        *dg = h_scal[SL_EVAL + 4];
    }
    template <class P> int after_search(int, const MtSearch &, double, double, int, P &&, LbfgsOutcome *, bool *) { return PLM_OK; }
    void accepted_norms(const LbfgsHistory &, double *cond, double *xx_out, double *hh_out) {
        *cond = read_norms();
        *xx_out = xx, *hh_out = hh;
    }
    int converged(double *cond, bool *done) const { *done = *cond <= eps; return PLM_OK; }
    int anchor_buffers() const { return PLM_OK; }      // allocated with the rest
};

}  // namespace

int plm_ar_logprob(const int8_t *seqs, int32_t n_seqs, int32_t n_sites, int32_t n_states, const float *x_canonical,
                   int device, void *stream, double *logp_out, double *site_logp_out) {
    const int n = n_seqs, L = n_sites, q = n_states;
    if (!seqs || !x_canonical || !logp_out) return plm_fail(PLM_EINVAL, "plm_ar_logprob: NULL argument");
    if (n < 1) return plm_fail(PLM_EINVAL, "plm_ar_logprob: need n_seqs >= 1 (got %d)", n);
    PLM_TRY(ar_check_shape(L, q, "plm_ar_logprob"));
    if ((double)n * L >= 2147483647.0) return plm_fail(PLM_EINVAL, "plm_ar_logprob: n_seqs x n_sites must stay below 2^31");
    PLM_TRY(ar_check_states(seqs, n, L, q, "seqs"));
    PLM_TRY(plm_check_device(device));
    ArEval ev(L, q, n, false);
    PLM_TRY(plm_check_free(ev.bytes() + 4.0 * plm_n_canon(L, q), "plm_ar_logprob", ar_table_bytes(L, q)));
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    float *xc = nullptr;
    PLM_TRY(mem.alloc(&xc, (size_t)ev.n_can));
    PLM_TRY(ev.alloc(mem));
    PLM_HIP(hipMemcpyAsync(xc, x_canonical, sizeof(float) * ev.n_can, hipMemcpyHostToDevice, st));
    PLM_TRY(ev.upload(st, seqs, nullptr));
    PLM_TRY(ev.conditionals(st, xc));
    PLM_HIP(hipMemcpyAsync(logp_out, ev.logp, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (site_logp_out)
        PLM_HIP(hipMemcpyAsync(site_logp_out, ev.site, sizeof(double) * (size_t)n * L, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_ar_sample(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_ar_sample_opts *opts, int device,
                  void *stream, int8_t *states_out) {
    if (!opts) return plm_fail(PLM_EINVAL, "plm_ar_sample: NULL options");
    const int L = n_sites, q = n_states, C = opts->n_samples;
    if (C < 1) return plm_fail(PLM_EINVAL, "plm_ar_sample: need n_samples >= 1 (got %d)", C);
    if (!x_canonical || !states_out) return plm_fail(PLM_EINVAL, "plm_ar_sample: NULL argument");
    PLM_TRY(ar_check_shape(L, q, "plm_ar_sample"));
    if (!(opts->beta > 0.f) || !std::isfinite(opts->beta))
        return plm_fail(PLM_EINVAL, "plm_ar_sample: beta must be finite and > 0 (got %g)", (double)opts->beta);
    if ((double)C * L >= 2147483647.0) return plm_fail(PLM_EINVAL, "plm_ar_sample: n_samples x n_sites must stay below 2^31");
    uint32_t allowed = plm_state_mask(q);
    if (opts->allowed) {
        allowed = 0;
        for (int a = 0; a < q; a++)
            if (opts->allowed[a]) allowed |= 1u << a;
        if (!allowed) return plm_fail(PLM_EINVAL, "plm_ar_sample: no state is allowed");
    }
    // the form: tiled wherever a tile's chain states and one staged chunk fit the LDS, with the largest tile that still
    // gives every CU a workgroup; PLM_AR_FORM=direct | tiled forces one (measurements and tests only: same states)
    const char *form = getenv("PLM_AR_FORM");
    if (form && *form && strcmp(form, "direct") && strcmp(form, "tiled"))
        return plm_fail(PLM_EINVAL, "PLM_AR_FORM must be direct or tiled (got '%s')", form);
    PLM_TRY(plm_check_device(device));
    const int64_t n_can = (int64_t)plm_n_canon(L, q);
    PLM_TRY(plm_check_free(ar_table_bytes(L, q) + 4.0 * n_can + (double)C * L, "plm_ar_sample", ar_table_bytes(L, q)));
    hipDeviceProp_t prop;
    PLM_HIP(hipGetDeviceProperties(&prop, device));
    const int JC = ar_jc(q), L4 = (L + 3) / 4;
    const size_t stage_b = (size_t)JC * q * ar_nvp(q) * 16;
    int tile = 256;
    while (tile > 64 && (stage_b + (size_t)L4 * tile * 4 > GS_LDS_BYTES || (C + tile - 1) / tile < prop.multiProcessorCount))
        tile /= 2;
    const bool fits = stage_b + (size_t)L4 * tile * 4 <= GS_LDS_BYTES;
    const bool direct = form && *form ? !strcmp(form, "direct") : !fits;
    if (!direct && !fits)
        return plm_fail(PLM_EUNSUPPORTED, "plm_ar_sample: %d sites do not fit the LDS of a CU in the tiled form", L);
    int QG = 2;
    while (QG < q) QG *= 2;
    const size_t direct_b = (size_t)(256 / QG) * L4 * 4;
    if (direct && direct_b > GS_LDS_BYTES)
        return plm_fail(PLM_EUNSUPPORTED, "plm_ar_sample: %d sites with %d states: the chain states of a workgroup do not fit the LDS of a CU", L, q);
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    float *xc = nullptr, *T = nullptr;
    int8_t *states = nullptr;
    PLM_TRY(mem.alloc(&xc, (size_t)n_can));
    PLM_TRY(mem.alloc(&T, (size_t)ar_tri(L) * q * ar_nv(q) * 4));
    PLM_TRY(mem.alloc(&states, (size_t)C * L));
    PLM_HIP(hipMemcpyAsync(xc, x_canonical, sizeof(float) * n_can, hipMemcpyHostToDevice, st));
    PLM_HIP(ar_repack(st, xc, L, q, T));
    const uint32_t lo = (uint32_t)(opts->seed & 0xFFFFFFFFu), hi = (uint32_t)(opts->seed >> 32);
    if (!direct) {
        const dim3 grid((unsigned)((C + tile - 1) / tile));
        const size_t lds = stage_b + (size_t)L4 * tile * 4;
        hipError_t e = hipSuccess;
        ar_for_nv(q, [&](auto nv) {
            constexpr int NV = decltype(nv)::value;
            e = hipFuncSetAttribute((const void *)k_ar_sample<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return;
            hipLaunchKernelGGL(k_ar_sample<NV>, grid, dim3(tile), lds, st, T, xc, L, q, C, JC, opts->first_chain, allowed,
                               opts->beta, lo, hi, states);
        });
        PLM_HIP(e);
    } else {
        const int cpw = 256 / QG;
        const dim3 grid((unsigned)((C + cpw - 1) / cpw));
#define AR_DIRECT_LAUNCH(QG_)                                                                                          \
        case QG_:                                                                                                      \
            PLM_HIP(hipFuncSetAttribute((const void *)k_ar_sample_direct<QG_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        (int)direct_b));                                                               \
            hipLaunchKernelGGL(k_ar_sample_direct<QG_>, grid, dim3(256), direct_b, st, T, xc, L, q, ar_nv(q) * 4, C,    \
                               opts->first_chain, allowed, opts->beta, lo, hi, states);                                \
            break;
        switch (QG) { AR_DIRECT_LAUNCH(2) AR_DIRECT_LAUNCH(4) AR_DIRECT_LAUNCH(8) AR_DIRECT_LAUNCH(16) AR_DIRECT_LAUNCH(32) }
#undef AR_DIRECT_LAUNCH
    }
    PLM_HIP(hipGetLastError());
    PLM_HIP(hipMemcpyAsync(states_out, states, (size_t)C * L, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_ar_eval(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states, double lambda_h,
                double lambda_j, const float *x_canonical, int device, void *stream, double *fx_out, double *nll_out,
                double *g_out) {
    const int n = n_seqs, L = n_sites, q = n_states;
    std::vector<double> w;
    double neff = 0;
    PLM_TRY(ar_check_data(msa, weights, n, L, q, lambda_h, lambda_j, "plm_ar_eval", &w, &neff));
    if (!x_canonical || !fx_out) return plm_fail(PLM_EINVAL, "plm_ar_eval: NULL argument");
    PLM_TRY(plm_check_device(device));
    ArEval ev(L, q, n, true);
    ev.neff = neff, ev.lambda_h = lambda_h, ev.lambda_j = lambda_j;
    PLM_TRY(plm_check_free(ev.bytes() + 12.0 * plm_n_canon(L, q), "plm_ar_eval", ar_table_bytes(L, q)));
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    float *xc = nullptr;
    double *g = nullptr, *scal = nullptr, *h_scal = nullptr;
    PLM_TRY(mem.alloc(&xc, (size_t)ev.n_can));
    PLM_TRY(mem.alloc(&g, (size_t)ev.n_can));
    PLM_TRY(mem.alloc(&scal, (size_t)8));
    PLM_TRY(mem.alloc_pinned(&h_scal, (size_t)8));
    PLM_TRY(ev.alloc(mem));
    PLM_HIP(hipMemcpyAsync(xc, x_canonical, sizeof(float) * ev.n_can, hipMemcpyHostToDevice, st));
    PLM_TRY(ev.upload(st, msa, w.data()));
    PLM_TRY(ev.enqueue(st, xc, g, scal, nullptr));
    PLM_HIP(hipMemcpyAsync(h_scal, scal, sizeof(double) * 5, hipMemcpyDeviceToHost, st));
    if (g_out) PLM_HIP(hipMemcpyAsync(g_out, g, sizeof(double) * ev.n_can, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    double nll;
    ev.objective(h_scal, fx_out, &nll);
    if (nll_out) *nll_out = nll;
    return PLM_OK;
}

// The L-BFGS fit: the checks and the buffers of an ArProblem, then lbfgs_minimize (plm_lbfgs_driver.h) -- the iteration
// that plm_ctx_optimize runs as well.
int plm_ar_fit(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
               const plm_ar_fit_opts *opts, const float *x_start, plm_iter_cb cb, void *user, int device, void *stream,
               float *x_out, plm_ar_fit_result *result) {
    if (!opts || !x_out || !result) return plm_fail(PLM_EINVAL, "plm_ar_fit: NULL argument");
    const int n = n_seqs, L = n_sites, q = n_states;
    std::vector<double> w;
    double neff = 0;
    PLM_TRY(ar_check_data(msa, weights, n, L, q, opts->lambda_h, opts->lambda_j, "plm_ar_fit", &w, &neff));
    if (opts->max_iter < 0) return plm_fail(PLM_EINVAL, "plm_ar_fit: max_iter must be >= 0 (0: no limit; got %d)", opts->max_iter);
    if (!(opts->epsilon > 0) || !std::isfinite(opts->epsilon))
        return plm_fail(PLM_EINVAL, "plm_ar_fit: epsilon must be finite and > 0 (got %g)", opts->epsilon);
    if (opts->lbfgs_m < 1 || opts->lbfgs_m > 20) return plm_fail(PLM_EINVAL, "plm_ar_fit: lbfgs_m must be 1..20 (got %d)", opts->lbfgs_m);
    PLM_TRY(plm_check_device(device));
    const double t0 = lbfgs_now();
    const int m = opts->lbfgs_m;
    ArEval ev(L, q, n, true);
    ev.neff = neff, ev.lambda_h = opts->lambda_h, ev.lambda_j = opts->lambda_j;
    ArProblem p{ev, (hipStream_t)stream, m, opts->epsilon};
    const int64_t nc = p.nc, n4 = p.n4;
    const size_t scratch_n = (size_t)(3 * PLM_MAX_BASIS + 4) * PLM_DOT_BLOCKS;
    PLM_TRY(plm_check_free(ev.bytes() + 4.0 * n4 * (7 + 2 * m) + 16.0 * nc + 8.0 * scratch_n, "plm_ar_fit",
                           ar_table_bytes(L, q)));
    DeviceBuffers mem;
    for (float **v : {&p.x, &p.xp, &p.g, &p.gp, &p.xa, &p.ga, &p.dir}) PLM_TRY(mem.alloc(v, (size_t)n4));
    PLM_TRY(mem.alloc(&p.S, (size_t)2 * m * n4));
    PLM_TRY(mem.alloc(&p.g64, (size_t)nc));
    PLM_TRY(mem.alloc(&p.g64p, (size_t)nc));
    PLM_TRY(mem.alloc(&p.scal, (size_t)ArProblem::SL_COUNT));
    PLM_TRY(mem.alloc(&p.scratch, scratch_n));
    PLM_TRY(mem.alloc_pinned(&p.h_scal, (size_t)ArProblem::SL_COUNT));
    PLM_TRY(ev.alloc(mem));
    for (float *v : {p.x, p.xp, p.dir}) PLM_HIP(hipMemsetAsync(v, 0, sizeof(float) * n4, p.st));
    if (x_start) PLM_HIP(hipMemcpyAsync(p.x, x_start, sizeof(float) * nc, hipMemcpyHostToDevice, p.st));
    PLM_TRY(ev.upload(p.st, msa, w.data()));
    LbfgsOutcome o;
    PLM_TRY(lbfgs_minimize(p, LbfgsLimits{m, opts->epsilon, opts->max_iter, cb, user, t0}, &o));
    PLM_HIP(hipMemcpyAsync(x_out, p.x, sizeof(float) * nc, hipMemcpyDeviceToHost, p.st));
    PLM_HIP(hipStreamSynchronize(p.st));
    result->status = o.status;
    result->iterations = o.k;
    result->evaluations = p.n_evals;
    result->ls_reason = o.ls_reason;
    result->fx = o.fx;
    result->nll = o.nll;
    result->gnorm = std::sqrt(p.gg);
    result->xnorm = std::sqrt(p.xx);
    return PLM_OK;
}
