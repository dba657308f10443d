// plm_rbm.hip -- a restricted Boltzmann machine with Potts visible units and Bernoulli hidden units (DESIGN_NEXT_ROWS.md
// section 9.22; Tubiana, Cocco, Monasson 2019):
//     I_mu(v) = c_mu + sum_i W_mu,i(v_i),   P(v, h) ~ exp( sum_i g_i(v_i) + sum_mu h_mu I_mu(v) )
// the score with the hidden-unit inputs (plm_rbm_score), block Gibbs sampling (plm_rbm_sample), persistent
// contrastive divergence (plm_rbm_fit) and log Z by annealed importance sampling (plm_rbm_ais, section 9.25).  The
// parameters are one float32 vector, g [L][q], c [M], W [M][L][q].
//
// W is expanded once per call or epoch (k_rbm_expand) into the two layouts the kernels read:
//   Wt [L q][Mp]      one (i, v_i) is one row of M floats (Mp = M rounded up to 8): the gather of the hidden inputs
//   Wv [M][L][4 NV]   one (mu, i) is one row of q floats (NV = ceil(q / 4) float4): the visible logits
// and the fields into Gp [L][4 NV].  In the block-Gibbs kernel the lanes are chains: a lane gathers its own row of Wt for
// the hidden inputs, and every lane of a wave reads the same row of Wv for the visible logits (one address per wave) and
// adds it under its own hidden bit.  The float64 sums of the fit are made in an order the shape alone fixes: no
// floating-point atomics anywhere.
#include "plm_gibbs_device.h"
#include "plm_sample_internal.h"

#include <math.h>
#include <stdlib.h>
#include <cmath>

namespace {

#define RBM_HB 8               // hidden units a lane accumulates at a time in k_rbm_steps (two float4 of a Wt row)
#define RBM_CHUNK 4096         // sequences (or chains) per partial sum of k_rbm_accum: a constant, so the order is the shape's

// the byte of site i of the tile's chain `lane`: four consecutive sites of a chain share a word
#define RBM_XS(i, lane) ((((i) >> 2) * TILE + (lane)) * 4 + ((i) & 3))

inline int rbm_nv(int q) { return (q + 3) / 4; }
inline int rbm_mp(int M) { return (M + RBM_HB - 1) / RBM_HB * RBM_HB; }
inline int64_t rbm_n_par(int L, int q, int M) { return (int64_t)L * q + M + (int64_t)M * L * q; }

// ---- the layouts ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rbm_expand(const float *__restrict__ x, int L, int q, int M, int Mp, int NV4,
                                                    float *__restrict__ Gp, float *__restrict__ Wt,
                                                    float *__restrict__ Wv) {
    const float *W = x + (int64_t)L * q + M;
    const int64_t stride = (int64_t)gridDim.x * 256, k0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t k = k0; k < (int64_t)L * q * Mp; k += stride) {
        const int64_t r = k / Mp;                     // i q + a
        const int mu = (int)(k - r * Mp);
        Wt[k] = mu < M ? W[(int64_t)mu * L * q + r] : 0.f;
    }
    for (int64_t k = k0; k < (int64_t)M * L * NV4; k += stride) {
        const int64_t r = k / NV4;                    // mu L + i
        const int a = (int)(k - r * NV4);
        Wv[k] = a < q ? W[r * q + a] : 0.f;
    }
    for (int64_t k = k0; k < (int64_t)L * NV4; k += stride) {
        const int64_t i = k / NV4;
        const int a = (int)(k - i * NV4);
        Gp[k] = a < q ? x[i * q + a] : 0.f;
    }
}

// ---- the float64 paths ----------------------------------------------------------------------------------------------
__device__ __forceinline__ double rbm_sigmoid(double I) {
    if (I >= 0.0) return 1.0 / (1.0 + exp(-I));
    const double e = exp(I);
    return e / (1.0 + e);
}

// I [n][M] = (double) c_mu, then one add per site i = 0 .. L-1; P [n][M] = sigma(I) (or null).  A workgroup is 64 hidden
// units x 4 sequences: the 64 lanes of a wave read one row of Wt.
__global__ __launch_bounds__(256) void k_rbm_inputs(const float *__restrict__ Wt, const float *__restrict__ c,
                                                    const int8_t *__restrict__ x, int n, int L, int q, int M, int Mp,
                                                    double *__restrict__ I_out, double *__restrict__ P_out) {
    const int s = blockIdx.x * 4 + threadIdx.y, mu = blockIdx.y * 64 + threadIdx.x;
    if (s >= n || mu >= M) return;
    const int8_t *xs = x + (int64_t)s * L;
    double I = (double)c[mu];
    for (int i = 0; i < L; i++) I += (double)Wt[((int64_t)i * q + xs[i]) * Mp + mu];
    I_out[(int64_t)s * M + mu] = I;
    if (P_out) P_out[(int64_t)s * M + mu] = rbm_sigmoid(I);
}

// score = the fields in site order, then softplus(I_mu) = max(I, 0) + log1p(exp(-|I|)) in mu order: one running sum
__global__ __launch_bounds__(256) void k_rbm_score(const float *__restrict__ g, const int8_t *__restrict__ x,
                                                   const double *__restrict__ I, int n, int L, int q, int M,
                                                   double *__restrict__ score) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    double t = 0.0;
    for (int i = 0; i < L; i++) t += (double)g[i * q + x[(int64_t)s * L + i]];
    for (int mu = 0; mu < M; mu++) {
        const double v = I[(int64_t)s * M + mu];
        t += fmax(v, 0.0) + log1p(exp(-fabs(v)));
    }
    score[s] = t;
}

// out [L][q] = sum_s w_s delta(x_si, a) / div: a workgroup per site, lane (slice, a) takes s = slice, slice + 8, ...,
// then state a adds the 8 slices in slice order.  w null: every weight is 1 (exact counts).
__global__ __launch_bounds__(256) void k_rbm_site_freq(const int8_t *__restrict__ x, const double *__restrict__ w, int n,
                                                       int L, int q, double div, double *__restrict__ out) {
    __shared__ double red[256];
    const int i = blockIdx.x, a = threadIdx.x & 31, sl = threadIdx.x >> 5;
    double acc = 0.0;
    for (int s = sl; s < n; s += 8)
        if (x[(int64_t)s * L + i] == a) acc += w ? w[s] : 1.0;
    red[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < q) {
        double t = 0.0;
        for (int k = 0; k < 8; k++) t += red[k * 32 + threadIdx.x];
        out[i * q + threadIdx.x] = t / div;
    }
}

// The one-hot product [L q x n] x [n x M] over one chunk of RBM_CHUNK sequences: a workgroup owns (site i, 64 hidden
// units, chunk); wave `sl` takes the chunk's sequences sl, sl + 4, ...; lane mu owns the LDS column acc[sl][.][mu] and
// adds w_s p_s,mu at row x_si (one row per wave: no two lanes touch the same word, so neither a barrier nor an atomic).
// The four waves are then added in wave order.  part [chunk][M][L][q], part_c [chunk][M] (written by site 0).
__global__ __launch_bounds__(256) void k_rbm_accum(const int8_t *__restrict__ x, const double *__restrict__ w,
                                                   const double *__restrict__ P, int n, int L, int q, int M,
                                                   double *__restrict__ part, double *__restrict__ part_c) {
    extern __shared__ double acc[];                   // [4][q][64]
    __shared__ double cs[256];
    const int i = blockIdx.x, l = threadIdx.x & 63, sl = threadIdx.x >> 6, mu = blockIdx.y * 64 + l;
    const bool live = mu < M;
    double *col = acc + (int64_t)sl * q * 64 + l;
    for (int a = 0; a < q; a++) col[a * 64] = 0.0;
    const int s0 = blockIdx.z * RBM_CHUNK, s1 = min(n, s0 + RBM_CHUNK);
    double csum = 0.0;
    for (int s = s0 + sl; s < s1; s += 4) {
        const double p = live ? __dmul_rn(w ? w[s] : 1.0, P[(int64_t)s * M + mu]) : 0.0;
        col[(int)x[(int64_t)s * L + i] * 64] += p;
        csum += p;
    }
    cs[threadIdx.x] = csum;
    __syncthreads();
    if (sl != 0 || !live) return;
    double *dst = part + (((int64_t)blockIdx.z * M + mu) * L + i) * q;
    for (int a = 0; a < q; a++)
        dst[a] = ((acc[a * 64 + l] + acc[(q + a) * 64 + l]) + acc[(2 * q + a) * 64 + l]) + acc[(3 * q + a) * 64 + l];
    if (i == 0) part_c[(int64_t)blockIdx.z * M + mu] = ((cs[l] + cs[64 + l]) + cs[128 + l]) + cs[192 + l];
}

// stat [c | W] = (the chunks in chunk order) / div; stat is a vector in the layout of the parameters
__global__ __launch_bounds__(256) void k_rbm_finish(const double *__restrict__ part, const double *__restrict__ part_c,
                                                    int n_chunks, int M, int64_t n_w, int64_t n_g, double div,
                                                    double *__restrict__ stat) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= M + n_w) return;
    double t = 0.0;
    if (k < M)
        for (int z = 0; z < n_chunks; z++) t += part_c[(int64_t)z * M + k];
    else
        for (int z = 0; z < n_chunks; z++) t += part[(int64_t)z * n_w + (k - M)];
    stat[n_g + k] = t / div;
}

// the sum of 256 lanes' values by a fixed tree (or their maximum); every lane gets it
template <bool MAX> __device__ __forceinline__ double rbm_block_reduce(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            red[threadIdx.x] = MAX ? fmax(red[threadIdx.x], red[threadIdx.x + o]) : red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}

// one workgroup: row = (max |D - N| over g, over c, over W, lr, sum_s w_s score_s / N_eff); lane t takes the entries
// t, t + 256, ..., then the tree
__global__ __launch_bounds__(256) void k_rbm_trace(const double *__restrict__ D, const double *__restrict__ Nm,
                                                   int64_t n_g, int M, int64_t n_par, const double *__restrict__ w,
                                                   const double *__restrict__ score, int n, double neff, double lr,
                                                   double *__restrict__ row) {
    __shared__ double red[256];
    double m[3] = {0.0, 0.0, 0.0};
    for (int64_t t = threadIdx.x; t < n_par; t += 256) {
        const double d = fabs(D[t] - Nm[t]);
        if (t < n_g) m[0] = fmax(m[0], d);
        else if (t < n_g + M) m[1] = fmax(m[1], d);
        else m[2] = fmax(m[2], d);
    }
    double sc = 0.0;
    for (int s = threadIdx.x; s < n; s += 256) sc += w[s] * score[s];
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const double r = rbm_block_reduce<true>(m[e], red);
        if (threadIdx.x == 0) row[e] = r;
    }
    sc = rbm_block_reduce<false>(sc, red);
    if (threadIdx.x == 0) {
        row[3] = lr;
        row[4] = sc / neff;
    }
}

// theta <- (float)( theta + lr ((D - N) - (2 lambda) theta) ), every operation in float64 and rounded on its own
__global__ __launch_bounds__(256) void k_rbm_update(float *__restrict__ x, const double *__restrict__ D,
                                                    const double *__restrict__ Nm, int64_t n_g, int M, int64_t n_par,
                                                    double lr, double two_lambda_g, double two_lambda_w) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_par) return;
    const double th = (double)x[t];
    const double l2 = t < n_g ? two_lambda_g : (t < n_g + M ? 0.0 : two_lambda_w);
    const double grad = __dsub_rn(__dsub_rn(D[t], Nm[t]), __dmul_rn(l2, th));
    x[t] = (float)__dadd_rn(th, __dmul_rn(lr, grad));
}

// ---- block Gibbs ----------------------------------------------------------------------------------------------------
// Lanes are chains: a workgroup is a tile of TILE = 64 of them and NW = blockDim.x / 64 waves that share the tile's work,
// the states in LDS as xs[L/4][64][4] bytes and the hidden units as hb[M/32][64][4] bytes of 8 bits each.  Given the sites
// the hidden units are independent, and given the hidden units the sites are: wave w takes the chunks of RBM_HB hidden
// units w, w + NW, ... and then the sites w, w + NW, ..., with a barrier between the two halves of a step.  A draw
// depends on (chain, step, unit or site) only, so NW changes nothing but the time.  Step t (index t0 + t):
//   (a) RBM_HB hidden units at a time: I_mu = c_mu in float32, then one float32 add per site i = 0 .. L-1 of the lane's
//       row (i, x_i) of Wt; p = 1 / (1 + expf(-I)); h_mu = u < p with the counter (chain, 2, step, mu)
//   (b) every site that is not fixed: U_a = g_i(a), then for mu = 0 .. M-1 the row (mu, i) of Wv -- the same row for every
//       lane -- added where the lane's h_mu is set; draw_state with the counter (chain, 0, step, i)
// src null: the start rule on g.  hid (or null) [C][M]: the hidden units of the last step (zeros when n_steps == 0).
template <int NV>
__global__ __launch_bounds__(512) void k_rbm_steps(const float4 *__restrict__ G4, const float *__restrict__ c,
                                                   const float *__restrict__ Wt, const float4 *__restrict__ Wv4, int L,
                                                   int q, int M, int Mp, int C, const int8_t *src,
                                                   const uint8_t *__restrict__ fixed, uint32_t allowed,
                                                   uint32_t first_chain, uint32_t t0, int n_steps, uint32_t seed_lo,
                                                   uint32_t seed_hi, int8_t *dst, int8_t *__restrict__ hid) {
    extern __shared__ uint32_t rbm_lds[];
    constexpr int TILE = 64;
    const int tid = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6, n_thr = blockDim.x;
    const int L4 = (L + 3) >> 2, MB = (M + RBM_HB - 1) / RBM_HB, MW = (MB + 3) >> 2;
    uint32_t *xw = rbm_lds, *hw = rbm_lds + L4 * TILE;
    uint8_t *xs = (uint8_t *)xw, *hb = (uint8_t *)hw;
    const int c0 = blockIdx.x * TILE;
    const int n_here = min(TILE, C - c0);
    const uint32_t chain = first_chain + (uint32_t)(c0 + tid);
    for (int k = threadIdx.x; k < (L4 + MW) * TILE; k += n_thr) rbm_lds[k] = 0u;
    __syncthreads();
    if (src) {
        for (int k = threadIdx.x; k < n_here * L; k += n_thr) {
            const int cl = k / L, j = k - cl * L;
            xs[RBM_XS(j, cl)] = (uint8_t)src[(int64_t)c0 * L + k];
        }
    } else {
        for (int i = wave; i < L; i += NW) {
            float4 U[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) U[v] = G4[i * NV + v];
            xs[RBM_XS(i, tid)] = (uint8_t)draw_state<NV>(U, q, allowed, 1.0f,
                                                          philox_word0(chain, 0u, GS_START_SWEEP, (uint32_t)i, seed_lo, seed_hi));
        }
    }
    __syncthreads();
    for (int t = 0; t < n_steps; t++) {
        const uint32_t step = t0 + (uint32_t)t;
        for (int ch = wave; ch < MB; ch += NW) {
            uint32_t bits = 0u;
            {
                const int m0 = ch * RBM_HB;
                float I[RBM_HB];
#pragma unroll
                for (int k = 0; k < RBM_HB; k++) I[k] = m0 + k < M ? c[m0 + k] : 0.f;
                const float *base = Wt + m0;
                for (int i4 = 0; i4 < L4; i4++) {
                    const uint32_t word = xw[i4 * TILE + tid];
#pragma unroll
                    for (int k4 = 0; k4 < 4; k4++) {
                        const int i = 4 * i4 + k4;
                        if (i < L) {
                            const int xi = (word >> (8 * k4)) & 0xff;
                            const float4 *row = (const float4 *)(base + ((int64_t)i * q + xi) * Mp);
                            const float4 r0 = row[0], r1 = row[1];
                            I[0] += r0.x; I[1] += r0.y; I[2] += r0.z; I[3] += r0.w;
                            I[4] += r1.x; I[5] += r1.y; I[6] += r1.z; I[7] += r1.w;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < RBM_HB; k++) {
                    if (m0 + k < M) {
                        const float p = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-I[k])));
                        const float u = uniform24(philox_word0(chain, 2u, step, (uint32_t)(m0 + k), seed_lo, seed_hi));
                        if (u < p) bits |= 1u << k;
                    }
                }
            }
            hb[RBM_XS(ch, tid)] = (uint8_t)bits;      // byte ch & 3 of word ch / 4: bit mu - 32 (mu / 32) of that word
        }
        __syncthreads();
        for (int i = wave; i < L; i += NW) {
            if (fixed && fixed[i]) continue;
            float4 U[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) U[v] = G4[i * NV + v];
            for (int w = 0; w < MW; w++) {
                const uint32_t bits = hw[w * TILE + tid];
                const int kmax = min(32, M - 32 * w);
                for (int k = 0; k < kmax; k++) {
                    const bool on = (bits >> k) & 1u;
                    const float4 *row = Wv4 + ((int64_t)(32 * w + k) * L + i) * NV;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        const float4 r = row[v];
                        U[v].x = on ? U[v].x + r.x : U[v].x;
                        U[v].y = on ? U[v].y + r.y : U[v].y;
                        U[v].z = on ? U[v].z + r.z : U[v].z;
                        U[v].w = on ? U[v].w + r.w : U[v].w;
                    }
                }
            }
            xs[RBM_XS(i, tid)] = (uint8_t)draw_state<NV>(U, q, allowed, 1.0f,
                                                          philox_word0(chain, 0u, step, (uint32_t)i, seed_lo, seed_hi));
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < n_here * L; k += n_thr) {
        const int cl = k / L, j = k - cl * L;
        dst[(int64_t)c0 * L + k] = (int8_t)xs[RBM_XS(j, cl)];
    }
    if (hid)
        for (int k = threadIdx.x; k < n_here * M; k += n_thr) {
            const int cl = k / M, mu = k - cl * M;
            hid[(int64_t)c0 * M + k] = (int8_t)((hw[(mu >> 5) * TILE + cl] >> (mu & 31)) & 1u);
        }
}

// ---- annealed importance sampling (section 9.25) ----------------------------------------------------------------------
// The products and sums the contract states with one rounding each: the pragma keeps the compiler from fusing them into
// one multiply-add (see field_plus_scaled of plm_tempered_device.h).
__device__ __forceinline__ double rbm_scaled_input(float beta, double I) {
#pragma clang fp contract(off)
    return (double)beta * I;
}
__device__ __forceinline__ float rbm_tempered_arg(float g, float beta, float S) {
#pragma clang fp contract(off)
    const float p = beta * S;
    return g + p;
}
// sum + (sp(x1) - sp(x0)), sp(x) = fmax(x, 0) + log1p(e) with e = exp(-|x|) from the caller
__device__ __forceinline__ double rbm_weight_add(double sum, double x1, double e1, double x0, double e0) {
#pragma clang fp contract(off)
    const double s1 = fmax(x1, 0.0) + log1p(e1);
    const double s0 = fmax(x0, 0.0) + log1p(e0);
    const double term = s1 - s0;
    return sum + term;
}
// rbm_sigmoid(x) from e = exp(-|x|): on either of its branches that is the exponential rbm_sigmoid takes, of the same
// argument, so the value is the same
__device__ __forceinline__ double rbm_sigmoid_from(double x, double e) {
    return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// The steps [k0, k1) of the anneal on the tile of k_rbm_steps (lanes are chains, NW waves share the hidden chunks and then
// the sites), with the inverse temperature betas[k + 1] on the hidden layer: the inputs of a chunk of RBM_HB hidden units
// in float64, x = beta I, the draw on sigma(x), and on the first sweep of a step the chunk's sum of
// softplus(beta_k I) - softplus(beta_{k-1} I) into ws[chunk][lane] (LDS, behind the hidden bits).  After the barrier
// between the halves wave 0 adds the chunk sums in chunk order into log w, which it holds in a register: the order is
// the shape's, whatever NW.  first != 0: the start rule and log w = 0; otherwise states and log w are read, and both are
// written back.  hid (or null) [C][M]: the hidden units of the launch's last sweep.
template <int NV>
__global__ __launch_bounds__(512) void k_rbm_ais(const float4 *__restrict__ G4, const float *__restrict__ c,
                                                 const float *__restrict__ Wt, const float4 *__restrict__ Wv4, int L, int q,
                                                 int M, int Mp, int C, const float *__restrict__ betas /* [K + 1] */,
                                                 int k0, int k1, int n_per, int first, uint32_t allowed, uint32_t seed_lo,
                                                 uint32_t seed_hi, int8_t *states /* [C][L] */,
                                                 double *logw_io /* [C] */, int8_t *__restrict__ hid) {
    extern __shared__ uint32_t rbm_lds[];
    constexpr int TILE = 64;
    const int tid = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6, n_thr = blockDim.x;
    const int L4 = (L + 3) >> 2, MB = (M + RBM_HB - 1) / RBM_HB, MW = (MB + 3) >> 2;
    uint32_t *xw = rbm_lds, *hw = rbm_lds + L4 * TILE;
    uint8_t *xs = (uint8_t *)xw, *hb = (uint8_t *)hw;
    double *ws = (double *)(rbm_lds + (L4 + MW) * TILE);      // [MB][TILE]; (L4 + MW) 256 bytes in: aligned
    const int c0 = blockIdx.x * TILE;
    const int n_here = min(TILE, C - c0);
    const uint32_t chain = (uint32_t)(c0 + tid);
    for (int k = threadIdx.x; k < (L4 + MW) * TILE; k += n_thr) rbm_lds[k] = 0u;
    __syncthreads();
    if (first) {
        for (int i = wave; i < L; i += NW) {
            float4 U[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) U[v] = G4[i * NV + v];
            xs[RBM_XS(i, tid)] = (uint8_t)draw_state<NV>(U, q, allowed, 1.0f,
                                                          philox_word0(chain, 0u, GS_START_SWEEP, (uint32_t)i, seed_lo, seed_hi));
        }
    } else {
        for (int k = threadIdx.x; k < n_here * L; k += n_thr) {
            const int cl = k / L, j = k - cl * L;
            xs[RBM_XS(j, cl)] = (uint8_t)states[(int64_t)c0 * L + k];
        }
    }
    const bool keeps_w = wave == 0 && tid < n_here;
    double logw = (!first && keeps_w) ? logw_io[c0 + tid] : 0.0;
    __syncthreads();
    for (int k = k0; k < k1; k++) {
        const float beta = betas[k + 1], beta_prev = betas[k];
        for (int s = 0; s < n_per; s++) {
            const uint32_t sweep = (uint32_t)k * (uint32_t)n_per + (uint32_t)s;
            const bool weigh = s == 0;
            for (int ch = wave; ch < MB; ch += NW) {
                const int m0 = ch * RBM_HB;
                double I[RBM_HB];
#pragma unroll
                for (int k8 = 0; k8 < RBM_HB; k8++) I[k8] = m0 + k8 < M ? (double)c[m0 + k8] : 0.0;
                const float *base = Wt + m0;
                for (int i4 = 0; i4 < L4; i4++) {
                    const uint32_t word = xw[i4 * TILE + tid];
#pragma unroll
                    for (int k4 = 0; k4 < 4; k4++) {
                        const int i = 4 * i4 + k4;
                        if (i < L) {
                            const int xi = (word >> (8 * k4)) & 0xff;
                            const float4 *row = (const float4 *)(base + ((int64_t)i * q + xi) * Mp);
                            const float4 r0 = row[0], r1 = row[1];
                            I[0] += (double)r0.x; I[1] += (double)r0.y; I[2] += (double)r0.z; I[3] += (double)r0.w;
                            I[4] += (double)r1.x; I[5] += (double)r1.y; I[6] += (double)r1.z; I[7] += (double)r1.w;
                        }
                    }
                }
                uint32_t bits = 0u;
                double wsum = 0.0;
#pragma unroll
                for (int k8 = 0; k8 < RBM_HB; k8++) {
                    if (m0 + k8 < M) {
                        const double x = rbm_scaled_input(beta, I[k8]);
                        const double e = exp(-fabs(x));
                        if (weigh) {
                            const double x0 = rbm_scaled_input(beta_prev, I[k8]);
                            wsum = rbm_weight_add(wsum, x, e, x0, exp(-fabs(x0)));
                        }
                        const double p = rbm_sigmoid_from(x, e);
                        const float u = uniform24(philox_word0(chain, 2u, sweep, (uint32_t)(m0 + k8), seed_lo, seed_hi));
                        if ((double)u < p) bits |= 1u << k8;
                    }
                }
                hb[RBM_XS(ch, tid)] = (uint8_t)bits;
                if (weigh) ws[ch * TILE + tid] = wsum;
            }
            __syncthreads();
            if (weigh && wave == 0) {                 // ws is next written behind the barrier that ends this sweep
                double t = 0.0;
                for (int ch = 0; ch < MB; ch++) t += ws[ch * TILE + tid];
                logw += t;
            }
            for (int i = wave; i < L; i += NW) {
                float4 S[NV];
#pragma unroll
                for (int v = 0; v < NV; v++) S[v] = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int w = 0; w < MW; w++) {
                    const uint32_t bits = hw[w * TILE + tid];
                    const int kmax = min(32, M - 32 * w);
                    for (int kb = 0; kb < kmax; kb++) {
                        const bool on = (bits >> kb) & 1u;
                        const float4 *row = Wv4 + ((int64_t)(32 * w + kb) * L + i) * NV;
#pragma unroll
                        for (int v = 0; v < NV; v++) {
                            const float4 r = row[v];
                            S[v].x = on ? S[v].x + r.x : S[v].x;
                            S[v].y = on ? S[v].y + r.y : S[v].y;
                            S[v].z = on ? S[v].z + r.z : S[v].z;
                            S[v].w = on ? S[v].w + r.w : S[v].w;
                        }
                    }
                }
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float4 gv = G4[i * NV + v];
                    S[v].x = rbm_tempered_arg(gv.x, beta, S[v].x);
                    S[v].y = rbm_tempered_arg(gv.y, beta, S[v].y);
                    S[v].z = rbm_tempered_arg(gv.z, beta, S[v].z);
                    S[v].w = rbm_tempered_arg(gv.w, beta, S[v].w);
                }
                xs[RBM_XS(i, tid)] = (uint8_t)draw_state<NV>(S, q, allowed, 1.0f,
                                                              philox_word0(chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
            }
            __syncthreads();
        }
    }
    for (int k = threadIdx.x; k < n_here * L; k += n_thr) {
        const int cl = k / L, j = k - cl * L;
        states[(int64_t)c0 * L + k] = (int8_t)xs[RBM_XS(j, cl)];
    }
    if (keeps_w) logw_io[c0 + tid] = logw;
    if (hid)
        for (int k = threadIdx.x; k < n_here * M; k += n_thr) {
            const int cl = k / M, mu = k - cl * M;
            hid[(int64_t)c0 * M + k] = (int8_t)((hw[(mu >> 5) * TILE + cl] >> (mu & 31)) & 1u);
        }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int rbm_check_shape(int L, int q, int M, const char *who) {
    if (L < 1 || M < 1) return plm_fail(PLM_EINVAL, "%s: need n_sites >= 1 and n_hidden >= 1 (got %d, %d)", who, L, M);
    PLM_TRY(gibbs::check_states(q, who));
    if ((double)M * L * q >= 2147483647.0) return plm_fail(PLM_EINVAL, "%s: n_hidden x n_sites x n_states must stay below 2^31", who);
    // the tiles of 64 hidden units are one dimension of a grid
    if (M > 64 * 65535) return plm_fail(PLM_EUNSUPPORTED, "%s: more than %d hidden units (got %d)", who, 64 * 65535, M);
    return PLM_OK;
}
int rbm_check_rows(const int8_t *x, int n, int L, int q, const char *who, const char *what) {
    if ((double)n * L >= 2147483647.0) return plm_fail(PLM_EINVAL, "%s: the rows of %s x n_sites must stay below 2^31", who, what);
    for (size_t k = 0; k < (size_t)n * L; k++)
        if (x[k] < 0 || x[k] >= q)
            return plm_fail(PLM_EINVAL, "%s: %s[%zu][%zu] = %d outside 0..%d", who, what, k / L, k % L, (int)x[k], q - 1);
    return PLM_OK;
}

// The model on the device: the parameters and the tables expanded from them.
struct RbmModel {
    const int L, q, M, NV, Mp;
    const int64_t n_g, n_w, n_par;
    float *x = nullptr, *Gp = nullptr, *Wt = nullptr, *Wv = nullptr;
    RbmModel(int L_, int q_, int M_)
        : L(L_), q(q_), M(M_), NV(rbm_nv(q_)), Mp(rbm_mp(M_)), n_g((int64_t)L_ * q_), n_w((int64_t)M_ * L_ * q_),
          n_par(rbm_n_par(L_, q_, M_)) {}
    const float *c() const { return x + n_g; }
    double bytes() const { return 4.0 * ((double)n_par + (double)L * NV * 4 + (double)L * q * Mp + (double)M * L * NV * 4); }
    int alloc(DeviceBuffers &mem) {
        PLM_TRY(mem.alloc(&x, (size_t)n_par));
        PLM_TRY(mem.alloc(&Gp, (size_t)L * NV * 4));
        PLM_TRY(mem.alloc(&Wt, (size_t)L * q * Mp));
        PLM_TRY(mem.alloc(&Wv, (size_t)M * L * NV * 4));
        return PLM_OK;
    }
    hipError_t expand(hipStream_t st) const {
        const int64_t most = std::max((int64_t)L * q * Mp, (int64_t)M * L * NV * 4);
        const unsigned grid = (unsigned)std::min<int64_t>(4096, (most + 255) / 256);
        hipLaunchKernelGGL(k_rbm_expand, dim3(grid), dim3(256), 0, st, x, L, q, M, Mp, NV * 4, Gp, Wt, Wv);
        return hipGetLastError();
    }
    // I [n][M] and (P non-null) sigma(I) of n rows of states on the device
    hipError_t inputs(hipStream_t st, const int8_t *rows, int n, double *I, double *P) const {
        hipLaunchKernelGGL(k_rbm_inputs, dim3((unsigned)((n + 3) / 4), (unsigned)((M + 63) / 64)), dim3(64, 4), 0, st, Wt,
                           c(), rows, n, L, q, M, Mp, I, P);
        return hipGetLastError();
    }
    hipError_t score(hipStream_t st, const int8_t *rows, const double *I, int n, double *out) const {
        hipLaunchKernelGGL(k_rbm_score, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, rows, I, n, L, q, M, out);
        return hipGetLastError();
    }
};

// The launch plan of the steps: the waves that share a tile of 64 chains -- the fewest (a power of two, 8 at most) with
// which the tiles bring 16 waves to every CU, since a wave alone waits for every row it reads.  PLM_RBM_WAVES=1|2|4|8
// forces the number (measurements and tests only: the same chains).
struct RbmPlan {
    int waves = 0;
    size_t lds = 0;
};
size_t rbm_lds_bytes(int L, int M) { return (size_t)((L + 3) / 4 + (M + 31) / 32) * 64 * 4; }
// with the chunk sums ws[M / 8][64] of k_rbm_ais behind them
size_t rbm_ais_lds_bytes(int L, int M) { return rbm_lds_bytes(L, M) + (size_t)((M + RBM_HB - 1) / RBM_HB) * 64 * sizeof(double); }
int rbm_check_lds(int L, int M, size_t lds) {
    if (lds > GS_LDS_BYTES)
        return plm_fail(PLM_EUNSUPPORTED, "%d sites and %d hidden units: the states of 64 chains do not fit the LDS of a CU", L, M);
    return PLM_OK;
}
// lds: the bytes of a tile (0: those of k_rbm_steps)
int rbm_plan(int L, int M, int C, int device, RbmPlan *out, size_t lds = 0) {
    if (lds == 0) lds = rbm_lds_bytes(L, M);
    PLM_TRY(rbm_check_lds(L, M, lds));
    const char *forced = getenv("PLM_RBM_WAVES");
    int waves = 1;
    if (forced && *forced) {
        waves = atoi(forced);
        if (waves != 1 && waves != 2 && waves != 4 && waves != 8)
            return plm_fail(PLM_EINVAL, "PLM_RBM_WAVES must be 1, 2, 4 or 8 (got '%s')", forced);
    } else {
        hipDeviceProp_t prop;
        PLM_HIP(hipGetDeviceProperties(&prop, device));
        const int64_t tiles = (C + 63) / 64;
        while (waves < 8 && tiles * waves < 16 * (int64_t)prop.multiProcessorCount) waves *= 2;
    }
    out->waves = waves;
    out->lds = lds;
    return PLM_OK;
}

// n_steps steps with the indices t0 .. from src (null: the start rule) into dst, both [C][L] (they may be one buffer: a
// workgroup reads its tile before it writes it); hid: null or [C][M]
hipError_t rbm_steps(const RbmModel &m, const RbmPlan &p, hipStream_t st, int C, const int8_t *src, const uint8_t *fixed,
                     uint32_t allowed, uint32_t first_chain, uint64_t seed, uint32_t t0, int n_steps, int8_t *dst,
                     int8_t *hid) {
    const gibbs::Seed sd(seed);
    const dim3 grid((unsigned)((C + 63) / 64));
    hipError_t e = hipSuccess;
#define RBM_STEPS_CASE(NV_)                                                                                            \
    case NV_:                                                                                                          \
        e = hipFuncSetAttribute((const void *)k_rbm_steps<NV_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds); \
        if (e != hipSuccess) return e;                                                                                 \
        hipLaunchKernelGGL(k_rbm_steps<NV_>, grid, dim3(64 * p.waves), p.lds, st, (const float4 *)m.Gp, m.c(), m.Wt,          \
                           (const float4 *)m.Wv, m.L, m.q, m.M, m.Mp, C, src, fixed, allowed, first_chain, t0, n_steps, \
                           sd.lo, sd.hi, dst, hid);                                                                    \
        break;
    switch (m.NV) {
        RBM_STEPS_CASE(1) RBM_STEPS_CASE(2) RBM_STEPS_CASE(3) RBM_STEPS_CASE(4)
        RBM_STEPS_CASE(5) RBM_STEPS_CASE(6) RBM_STEPS_CASE(7) RBM_STEPS_CASE(8)
    default: return hipErrorInvalidValue;
    }
#undef RBM_STEPS_CASE
    return hipGetLastError();
}

// the steps [k0, k1) of the anneal in one launch of k_rbm_ais, under a plan made with rbm_ais_lds_bytes
hipError_t rbm_ais_steps(const RbmModel &m, const RbmPlan &p, hipStream_t st, int C, const float *betas, int k0, int k1,
                         int n_per, uint64_t seed, int8_t *states, double *logw, int8_t *hid) {
    const gibbs::Seed sd(seed);
    const dim3 grid((unsigned)((C + 63) / 64));
    const uint32_t allowed = plm_state_mask(m.q);
    hipError_t e = hipSuccess;
#define RBM_AIS_CASE(NV_)                                                                                              \
    case NV_:                                                                                                          \
        e = hipFuncSetAttribute((const void *)k_rbm_ais<NV_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds); \
        if (e != hipSuccess) return e;                                                                                 \
        hipLaunchKernelGGL(k_rbm_ais<NV_>, grid, dim3(64 * p.waves), p.lds, st, (const float4 *)m.Gp, m.c(), m.Wt,     \
                           (const float4 *)m.Wv, m.L, m.q, m.M, m.Mp, C, betas, k0, k1, n_per, k0 == 0 ? 1 : 0, allowed, \
                           sd.lo, sd.hi, states, logw, hid);                                                           \
        break;
    switch (m.NV) {
        RBM_AIS_CASE(1) RBM_AIS_CASE(2) RBM_AIS_CASE(3) RBM_AIS_CASE(4)
        RBM_AIS_CASE(5) RBM_AIS_CASE(6) RBM_AIS_CASE(7) RBM_AIS_CASE(8)
    default: return hipErrorInvalidValue;
    }
#undef RBM_AIS_CASE
    return hipGetLastError();
}

// Steps of n_per sweeps per launch, out of K, that keep a launch of plm_rbm_ais near a second.  An estimate, not a
// measurement of this kernel: the 10.2 ms block-Gibbs step of section 9.22 (65 536 chains, L = 300, M = 128, NV = 6, four
// tiles per CU) scaled in proportion to M L NV and the tiles per CU.
int rbm_ais_steps_per_launch(const RbmModel &m, int C, int n_per, int K, int n_cu) {
    const double rounds = std::ceil((double)((C + 63) / 64) / std::max(n_cu, 1));
    const double per_step = (double)n_per * 10.2e-3 * ((double)m.M * m.L * m.NV) / (128.0 * 300.0 * 6.0) * rounds / 4.0;
    const double steps = 1.0 / std::max(per_step, 1e-9);
    return steps >= (double)K ? K : std::max(1, (int)steps);
}

// The statistics of n rows (data or chains) at the expanded model: stat [g | c | W] in float64.
struct RbmStats {
    const RbmModel &m;
    double *part = nullptr, *part_c = nullptr;
    static int chunks(int n) { return (n + RBM_CHUNK - 1) / RBM_CHUNK; }
    static double bytes(const RbmModel &m, int n_most) { return 8.0 * chunks(n_most) * ((double)m.n_w + m.M); }
    int alloc(DeviceBuffers &mem, int n_most) {
        PLM_TRY(mem.alloc(&part, (size_t)chunks(n_most) * m.n_w));
        PLM_TRY(mem.alloc(&part_c, (size_t)chunks(n_most) * m.M));
        return PLM_OK;
    }
    hipError_t fields(hipStream_t st, const int8_t *rows, const double *w, int n, double div, double *stat) const {
        hipLaunchKernelGGL(k_rbm_site_freq, dim3((unsigned)m.L), dim3(256), 0, st, rows, w, n, m.L, m.q, div, stat);
        return hipGetLastError();
    }
    hipError_t hidden(hipStream_t st, const int8_t *rows, const double *w, const double *P, int n, double div,
                      double *stat) const {
        const int nz = chunks(n);
        const hipError_t e = hipFuncSetAttribute((const void *)k_rbm_accum, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(sizeof(double) * 4 * m.q * 64));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rbm_accum, dim3((unsigned)m.L, (unsigned)((m.M + 63) / 64), (unsigned)nz), dim3(256),
                           sizeof(double) * 4 * m.q * 64, st, rows, w, P, n, m.L, m.q, m.M, part, part_c);
        hipLaunchKernelGGL(k_rbm_finish, dim3((unsigned)((m.M + m.n_w + 255) / 256)), dim3(256), 0, st, part, part_c, nz, m.M,
                           m.n_w, m.n_g, div, stat);
        return hipGetLastError();
    }
};

bool rbm_bad(double v) { return !(v >= 0.0) || !std::isfinite(v); }

// the five device events around the four phases of an epoch (plm_rbm_fit_result.phase_ms)
struct RbmEvents {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    RbmEvents() = default;
    RbmEvents(const RbmEvents &) = delete;
    RbmEvents &operator=(const RbmEvents &) = delete;
    ~RbmEvents() {
        for (hipEvent_t v : e)
            if (v) (void)hipEventDestroy(v);
    }
    hipError_t create() {
        on = true;
        for (hipEvent_t &v : e) {
            const hipError_t rc = hipEventCreate(&v);
            if (rc != hipSuccess) return rc;
        }
        return hipSuccess;
    }
    hipError_t mark(int k, hipStream_t st) const { return on ? hipEventRecord(e[k], st) : hipSuccess; }
};

}  // namespace

int plm_rbm_score(const int8_t *seqs, int32_t n_seqs, int32_t n_sites, int32_t n_states, int32_t n_hidden,
                  const float *params, int device, void *stream, double *score_out, double *inputs_out) {
    const int n = n_seqs, L = n_sites, q = n_states, M = n_hidden;
    if (!seqs || !params || !score_out) return plm_fail(PLM_EINVAL, "plm_rbm_score: NULL argument");
    if (n < 1) return plm_fail(PLM_EINVAL, "plm_rbm_score: need n_seqs >= 1 (got %d)", n);
    PLM_TRY(rbm_check_shape(L, q, M, "plm_rbm_score"));
    PLM_TRY(rbm_check_rows(seqs, n, L, q, "plm_rbm_score", "seqs"));
    PLM_TRY(plm_check_device(device));
    RbmModel m(L, q, M);
    PLM_TRY(plm_check_free(m.bytes() + (double)n * L + 8.0 * n * M + 8.0 * n, "plm_rbm_score"));
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    int8_t *x = nullptr;
    double *I = nullptr, *sc = nullptr;
    PLM_TRY(m.alloc(mem));
    PLM_TRY(mem.alloc(&x, (size_t)n * L));
    PLM_TRY(mem.alloc(&I, (size_t)n * M));
    PLM_TRY(mem.alloc(&sc, (size_t)n));
    PLM_HIP(hipMemcpyAsync(m.x, params, sizeof(float) * m.n_par, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(x, seqs, (size_t)n * L, hipMemcpyHostToDevice, st));
    PLM_HIP(m.expand(st));
    PLM_HIP(m.inputs(st, x, n, I, nullptr));
    PLM_HIP(m.score(st, x, I, n, sc));
    PLM_HIP(hipMemcpyAsync(score_out, sc, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (inputs_out) PLM_HIP(hipMemcpyAsync(inputs_out, I, sizeof(double) * (size_t)n * M, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_rbm_sample(int32_t n_sites, int32_t n_states, int32_t n_hidden, const float *params, const plm_rbm_sample_opts *opts,
                   int device, void *stream, int8_t *states_out, int8_t *hidden_out) {
    if (!opts) return plm_fail(PLM_EINVAL, "plm_rbm_sample: NULL options");
    if (!params || !states_out) return plm_fail(PLM_EINVAL, "plm_rbm_sample: NULL argument");
    const int L = n_sites, q = n_states, M = n_hidden, C = opts->n_chains, K = opts->n_snapshots;
    if (C < 1 || K < 1 || opts->burn_in < 0 || opts->thin < 1)
        return plm_fail(PLM_EINVAL, "plm_rbm_sample: need n_chains >= 1, n_snapshots >= 1, burn_in >= 0, thin >= 1 (got %d, %d, %d, %d)",
                        C, K, opts->burn_in, opts->thin);
    PLM_TRY(rbm_check_shape(L, q, M, "plm_rbm_sample"));
    if ((double)C * L >= 2147483647.0 || (double)C * M >= 2147483647.0)
        return plm_fail(PLM_EINVAL, "plm_rbm_sample: n_chains x n_sites and n_chains x n_hidden must stay below 2^31");
    if ((double)opts->first_chain + C > 4294967296.0)
        return plm_fail(PLM_EINVAL, "plm_rbm_sample: first_chain + n_chains must stay within 2^32");
    if ((double)opts->first_step + opts->burn_in + (double)(K - 1) * opts->thin >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "plm_rbm_sample: the step indices must stay below 2^32 - 1");
    uint32_t allowed = 0;
    PLM_TRY(gibbs::allowed_mask(q, opts->allowed, &allowed));
    if (opts->start) PLM_TRY(gibbs::check_start(opts->start, C, L, q, allowed, opts->fixed));
    PLM_TRY(plm_check_device(device));
    RbmModel m(L, q, M);
    const size_t CL = (size_t)C * L, CM = (size_t)C * M;
    PLM_TRY(plm_check_free(m.bytes() + (double)CL * (K + 1) + (hidden_out ? (double)CM * K : 0.0) + L, "plm_rbm_sample"));
    RbmPlan plan;
    PLM_TRY(rbm_plan(L, M, C, device, &plan));
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    int8_t *snaps = nullptr, *hid = nullptr, *start = nullptr;
    uint8_t *fixed = nullptr;
    PLM_TRY(m.alloc(mem));
    PLM_TRY(mem.alloc(&snaps, CL * K));
    if (hidden_out) PLM_TRY(mem.alloc(&hid, CM * K));
    if (opts->start) PLM_TRY(mem.alloc(&start, CL));
    if (opts->fixed) PLM_TRY(mem.alloc(&fixed, (size_t)L));
    PLM_HIP(hipMemcpyAsync(m.x, params, sizeof(float) * m.n_par, hipMemcpyHostToDevice, st));
    if (start) PLM_HIP(hipMemcpyAsync(start, opts->start, CL, hipMemcpyHostToDevice, st));
    if (fixed) PLM_HIP(hipMemcpyAsync(fixed, opts->fixed, (size_t)L, hipMemcpyHostToDevice, st));
    PLM_HIP(m.expand(st));
    uint32_t t = opts->first_step;
    for (int k = 0; k < K; k++) {
        const int n_steps = k == 0 ? opts->burn_in : opts->thin;
        const int8_t *src = k == 0 ? start : snaps + (size_t)(k - 1) * CL;
        PLM_HIP(rbm_steps(m, plan, st, C, src, fixed, allowed, opts->first_chain, opts->seed, t, n_steps, snaps + (size_t)k * CL,
                          hid ? hid + (size_t)k * CM : nullptr));
        t += (uint32_t)n_steps;
    }
    PLM_HIP(hipMemcpyAsync(states_out, snaps, CL * K, hipMemcpyDeviceToHost, st));
    if (hid) PLM_HIP(hipMemcpyAsync(hidden_out, hid, CM * K, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_rbm_fit(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states, int32_t n_hidden,
                const float *x_start, const plm_rbm_fit_opts *opts, int device, void *stream, plm_rbm_epoch_cb cb, void *user,
                plm_rbm_fit_result *result) {
    if (!opts || !result) return plm_fail(PLM_EINVAL, "plm_rbm_fit: NULL options or result");
    if (!msa || !weights || !x_start) return plm_fail(PLM_EINVAL, "plm_rbm_fit: NULL alignment, weights or x_start");
    const int N = n_seqs, L = n_sites, q = n_states, M = n_hidden;
    const int C = opts->n_chains, E = opts->n_epochs, K = opts->steps_per_epoch, e0 = opts->first_epoch, T = opts->lr_decay_after;
    if (N < 1 || C < 1 || E < 1 || K < 1 || e0 < 0 || T < 0)
        return plm_fail(PLM_EINVAL, "plm_rbm_fit: need n_seqs >= 1, n_chains >= 1, n_epochs >= 1, steps_per_epoch >= 1, first_epoch >= 0, "
                                    "lr_decay_after >= 0 (got %d, %d, %d, %d, %d, %d)", N, C, E, K, e0, T);
    PLM_TRY(rbm_check_shape(L, q, M, "plm_rbm_fit"));
    if (rbm_bad(opts->lr) || rbm_bad(opts->lambda_g) || rbm_bad(opts->lambda_w))
        return plm_fail(PLM_EINVAL, "plm_rbm_fit: lr, lambda_g and lambda_w must be finite and >= 0 (got %g, %g, %g)", opts->lr,
                        opts->lambda_g, opts->lambda_w);
    if (((double)e0 + (double)E) * (double)K >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "plm_rbm_fit: (first_epoch + n_epochs) steps_per_epoch must stay below 2^32 - 1 steps");
    if ((double)C * L >= 2147483647.0 || (double)C * M >= 2147483647.0)
        return plm_fail(PLM_EINVAL, "plm_rbm_fit: n_chains x n_sites and n_chains x n_hidden must stay below 2^31");
    if (std::max(N, C) > RBM_CHUNK * 65535)      // the chunks are one dimension of a grid
        return plm_fail(PLM_EUNSUPPORTED, "plm_rbm_fit: more than %d sequences or chains", RBM_CHUNK * 65535);
    std::vector<double> w((size_t)N);
    double neff = 0.0;
    for (int s = 0; s < N; s++) {
        if (!(weights[s] >= 0.f) || !std::isfinite(weights[s]))
            return plm_fail(PLM_EINVAL, "plm_rbm_fit: weight %d is negative or not finite (%g)", s, (double)weights[s]);
        w[s] = (double)weights[s];
        neff += w[s];
    }
    if (!(neff > 0.0)) return plm_fail(PLM_EINVAL, "plm_rbm_fit: the weights sum to zero");
    PLM_TRY(rbm_check_rows(msa, N, L, q, "plm_rbm_fit", "msa"));
    const uint32_t allowed = plm_state_mask(q);
    if (opts->start) PLM_TRY(gibbs::check_start(opts->start, C, L, q, allowed, nullptr));
    PLM_TRY(plm_check_device(device));
    RbmModel m(L, q, M);
    RbmStats stats{m};
    const int n_most = std::max(N, C);
    const size_t NL = (size_t)N * L, CL = (size_t)C * L;
    PLM_TRY(plm_check_free(m.bytes() + (double)NL + (double)CL + 8.0 * N * (2.0 * M + 2.0) + 16.0 * C * M + 16.0 * m.n_par +
                               RbmStats::bytes(m, n_most) + 40.0 * E, "plm_rbm_fit"));
    RbmPlan plan;
    PLM_TRY(rbm_plan(L, M, C, device, &plan));
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    int8_t *x = nullptr, *ch = nullptr;
    double *wd = nullptr, *Id = nullptr, *Pd = nullptr, *sc = nullptr, *Ic = nullptr, *Pc = nullptr, *D = nullptr, *Nm = nullptr;
    double *trace = nullptr, *row_host = nullptr;
    PLM_TRY(m.alloc(mem));
    PLM_TRY(mem.alloc(&x, NL));
    PLM_TRY(mem.alloc(&ch, CL));
    PLM_TRY(mem.alloc(&wd, (size_t)N));
    PLM_TRY(mem.alloc(&Id, (size_t)N * M));
    PLM_TRY(mem.alloc(&Pd, (size_t)N * M));
    PLM_TRY(mem.alloc(&sc, (size_t)N));
    PLM_TRY(mem.alloc(&Ic, (size_t)C * M));
    PLM_TRY(mem.alloc(&Pc, (size_t)C * M));
    PLM_TRY(mem.alloc(&D, (size_t)m.n_par));
    PLM_TRY(mem.alloc(&Nm, (size_t)m.n_par));
    PLM_TRY(mem.alloc(&trace, (size_t)5 * E));
    PLM_TRY(stats.alloc(mem, n_most));
    PLM_TRY(mem.alloc_pinned(&row_host, 5));
    PLM_HIP(hipMemcpyAsync(m.x, x_start, sizeof(float) * m.n_par, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(x, msa, NL, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(wd, w.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    if (opts->start) PLM_HIP(hipMemcpyAsync(ch, opts->start, CL, hipMemcpyHostToDevice, st));
    PLM_HIP(stats.fields(st, x, wd, N, neff, D));                 // D_g does not depend on the parameters
    RbmEvents ev;
    if (result->phase_ms) {
        PLM_HIP(ev.create());
        for (int k = 0; k < 4; k++) result->phase_ms[k] = 0.0;
    }

    int done_epochs = 0, rows = 0, status = PLM_STATUS_MAXITER;
    for (int ep = 0; ep < E; ep++) {
        const int64_t g = (int64_t)e0 + ep;
        double lr_g = opts->lr;
        if (T > 0 && g + 1 > T) lr_g = opts->lr * (double)T / (double)(g + 1);
        PLM_HIP(ev.mark(0, st));
        PLM_HIP(m.expand(st));
        PLM_HIP(m.inputs(st, x, N, Id, Pd));
        PLM_HIP(m.score(st, x, Id, N, sc));
        PLM_HIP(stats.hidden(st, x, wd, Pd, N, neff, D));
        PLM_HIP(ev.mark(1, st));
        const int8_t *src = (ep == 0 && !opts->start) ? nullptr : ch;
        PLM_HIP(rbm_steps(m, plan, st, C, src, nullptr, allowed, 0u, opts->seed, (uint32_t)(g * K), K, ch, nullptr));
        PLM_HIP(ev.mark(2, st));
        PLM_HIP(m.inputs(st, ch, C, Ic, Pc));
        PLM_HIP(stats.fields(st, ch, nullptr, C, (double)C, Nm));
        PLM_HIP(stats.hidden(st, ch, nullptr, Pc, C, (double)C, Nm));
        hipLaunchKernelGGL(k_rbm_trace, dim3(1), dim3(256), 0, st, D, Nm, m.n_g, M, m.n_par, wd, sc, N, neff, lr_g,
                           trace + (size_t)5 * ep);
        PLM_HIP(hipGetLastError());
        PLM_HIP(ev.mark(3, st));
        rows = ep + 1;
        if (cb) {
            PLM_HIP(hipMemcpyAsync(row_host, trace + (size_t)5 * ep, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
            PLM_HIP(hipStreamSynchronize(st));
            if (cb((int32_t)g, row_host[0], row_host[1], row_host[2], row_host[3], row_host[4], user)) {
                status = PLM_STATUS_INTERRUPTED;
                break;
            }
        }
        hipLaunchKernelGGL(k_rbm_update, dim3((unsigned)((m.n_par + 255) / 256)), dim3(256), 0, st, m.x, D, Nm, m.n_g, M, m.n_par,
                           lr_g, 2.0 * opts->lambda_g, 2.0 * opts->lambda_w);
        PLM_HIP(hipGetLastError());
        if (ev.on) {                                  // a timed fit waits for every epoch
            PLM_HIP(ev.mark(4, st));
            PLM_HIP(hipEventSynchronize(ev.e[4]));
            for (int k = 0; k < 4; k++) {
                float ms = 0.f;
                PLM_HIP(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
                result->phase_ms[k] += (double)ms;
            }
        }
        done_epochs = ep + 1;
    }
    if (result->x_out) PLM_HIP(hipMemcpyAsync(result->x_out, m.x, sizeof(float) * m.n_par, hipMemcpyDeviceToHost, st));
    if (result->data_out) PLM_HIP(hipMemcpyAsync(result->data_out, D, sizeof(double) * m.n_par, hipMemcpyDeviceToHost, st));
    if (result->model_out) PLM_HIP(hipMemcpyAsync(result->model_out, Nm, sizeof(double) * m.n_par, hipMemcpyDeviceToHost, st));
    if (result->chains_out) PLM_HIP(hipMemcpyAsync(result->chains_out, ch, CL, hipMemcpyDeviceToHost, st));
    if (result->trace) PLM_HIP(hipMemcpyAsync(result->trace, trace, (size_t)5 * rows * sizeof(double), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    result->epochs_done = done_epochs;
    result->status = status;
    return PLM_OK;
}

int plm_rbm_ais(int32_t n_sites, int32_t n_states, int32_t n_hidden, const float *params, const plm_ais_opts *opts,
                int device, void *stream, plm_ais_cb cb, void *user, plm_rbm_ais_result *result) {
    if (!opts || !result) return plm_fail(PLM_EINVAL, "plm_rbm_ais: NULL options or result");
    if (!params) return plm_fail(PLM_EINVAL, "plm_rbm_ais: NULL model");
    const int L = n_sites, q = n_states, M = n_hidden, C = opts->n_chains, K = opts->n_temps, n = opts->sweeps_per_temp;
    PLM_TRY(rbm_check_shape(L, q, M, "plm_rbm_ais"));
    if (C < 1 || K < 1 || n < 1 || opts->steps_per_launch < 0)
        return plm_fail(PLM_EINVAL, "plm_rbm_ais: need n_chains >= 1, n_temps >= 1, sweeps_per_temp >= 1, steps_per_launch >= 0 "
                                    "(got %d, %d, %d, %d)", C, K, n, opts->steps_per_launch);
    if ((double)K * (double)n >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "plm_rbm_ais: n_temps x sweeps_per_temp must stay below 2^32 - 1 sweeps");
    if ((double)C * L >= 2147483647.0 || (double)C * M >= 2147483647.0)
        return plm_fail(PLM_EINVAL, "plm_rbm_ais: n_chains x n_sites and n_chains x n_hidden must stay below 2^31");
    if (opts->betas) {
        if (opts->betas[0] != 0.f) return plm_fail(PLM_EINVAL, "plm_rbm_ais: betas[0] must be 0 (got %g)", (double)opts->betas[0]);
        for (int k = 1; k <= K; k++)
            if (!std::isfinite(opts->betas[k]) || !(opts->betas[k] >= opts->betas[k - 1]))
                return plm_fail(PLM_EINVAL, "plm_rbm_ais: betas must be finite and non-decreasing (betas[%d] = %g after %g)", k,
                                (double)opts->betas[k], (double)opts->betas[k - 1]);
    }
    PLM_TRY(rbm_check_lds(L, M, rbm_ais_lds_bytes(L, M)));
    PLM_TRY(plm_check_device(device));
    RbmModel m(L, q, M);
    const size_t CL = (size_t)C * L, CM = (size_t)C * M;
    PLM_TRY(plm_check_free(m.bytes() + (double)CL + 8.0 * C + (result->hidden ? (double)CM : 0.0) + 4.0 * ((double)K + 1.0),
                           "plm_rbm_ais"));
    RbmPlan plan;
    PLM_TRY(rbm_plan(L, M, C, device, &plan, rbm_ais_lds_bytes(L, M)));
    int n_cu = 0;
    PLM_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    const int per_launch = opts->steps_per_launch > 0 ? std::min(opts->steps_per_launch, K)
                                                      : rbm_ais_steps_per_launch(m, C, n, K, n_cu);

    // log Z_0 = M log 2 + sum_i log sum_a exp g_i(a) in float64
    double log_z0 = (double)M * log(2.0);
    for (int i = 0; i < L; i++) {
        const float *g = params + (size_t)i * q;
        double mx = g[0], s = 0.0;
        for (int a = 1; a < q; a++) mx = std::max(mx, (double)g[a]);
        for (int a = 0; a < q; a++) s += exp((double)g[a] - mx);
        log_z0 += mx + log(s);
    }
    std::vector<float> betas((size_t)K + 1);
    for (int k = 0; k <= K; k++) betas[k] = opts->betas ? opts->betas[k] : (float)((double)k / (double)K);

    hipStream_t st = (hipStream_t)stream;
    DeviceBuffers mem;
    float *d_betas = nullptr;
    int8_t *states = nullptr, *hid = nullptr;
    double *d_logw = nullptr;
    PLM_TRY(m.alloc(mem));
    PLM_TRY(mem.alloc(&d_betas, betas.size()));
    PLM_TRY(mem.alloc(&states, CL));
    PLM_TRY(mem.alloc(&d_logw, (size_t)C));
    if (result->hidden) PLM_TRY(mem.alloc(&hid, CM));
    PLM_HIP(hipMemcpyAsync(m.x, params, sizeof(float) * m.n_par, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(d_betas, betas.data(), betas.size() * sizeof(float), hipMemcpyHostToDevice, st));
    PLM_HIP(m.expand(st));
    int steps_done = 0, status = PLM_STATUS_CONVERGED;
    while (steps_done < K) {
        const int k1 = std::min(K, steps_done + per_launch);
        PLM_HIP(rbm_ais_steps(m, plan, st, C, d_betas, steps_done, k1, n, opts->seed, states, d_logw, hid));
        steps_done = k1;
        if (cb && steps_done < K) {
            PLM_HIP(hipStreamSynchronize(st));
            if (cb((int32_t)steps_done, (int32_t)K, user)) {
                status = PLM_STATUS_INTERRUPTED;
                break;
            }
        }
    }
    std::vector<double> logw((size_t)C);
    PLM_HIP(hipMemcpyAsync(logw.data(), d_logw, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (result->states) PLM_HIP(hipMemcpyAsync(result->states, states, CL, hipMemcpyDeviceToHost, st));
    if (result->hidden) PLM_HIP(hipMemcpyAsync(result->hidden, hid, CM, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    if (result->log_w) std::copy(logw.begin(), logw.end(), result->log_w);
    result->log_z0 = log_z0;
    result->steps_done = steps_done;
    result->status = status;
    if (status == PLM_STATUS_INTERRUPTED) {
        result->log_z = result->log_z_se = result->ess = NAN;
        return PLM_OK;
    }
    plm_ais_summary(logw.data(), C, log_z0, &result->log_z, &result->log_z_se, &result->ess);
    return PLM_OK;
}
