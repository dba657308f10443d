// plm_gibbs_device.h -- the device code every sweep kernel shares: the Philox block, the uniform, the draw of the
// contract in its two forms, the staging pipeline of the tiled form (DESIGN_NEXT_ROWS.md section 9.6) and the frame of
// either form around the site loop (section 9.14).  Included by plm_sample.hip (k_gibbs*), plm_anneal.hip (k_anneal*)
// and, through plm_tempered_device.h, by plm_ais.hip and plm_pt.hip; everything here has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

#define GS_Q 32                 // largest alphabet
#define GS_PF 8                 // float4 of a W chunk one thread carries from global memory to LDS
#define GS_DEPTH 3              // chunks in flight per thread (the three register sets of k_gibbs)
#define GS_LDS_BYTES 163840     // LDS of a CU
#define GS_START_SWEEP 0xFFFFFFFFu

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11); only word 0 of the block is used
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// u = ((word0 >> 8) + 0.5) 2^-24 in float32, kept below 1: above 2^23 the sum rounds to an integer (ties to even), and
// for the one word in 2^24 with all 24 bits set it rounds to 2^24, u = 1, where no running sum exceeds u S_last and the
// draw would fall through to the last allowed state whatever its weight.  That word takes the largest float32 below 1;
// u S < S then holds for every S, so the first state with S_a > u S_last always exists.
__device__ __forceinline__ float uniform24(uint32_t word0) {
    return fminf(__fmul_rn((float)(word0 >> 8) + 0.5f, 5.9604644775390625e-08f), 0.99999994f);
}

// One draw of the contract: e_a = exp(beta U_a - max) over the allowed states in state order, running sum S_a, the new
// state is the first allowed a with S_a > u S_last (the last allowed state if none).  U holds NV float4 (states a >= q
// are padding).  u = ((word0 >> 8) + 0.5) 2^-24.
template <int NV>
__device__ __forceinline__ int draw_state(const float4 *U, int q, uint32_t allowed, float beta, uint32_t word0) {
    float e[NV * 4];
    float m = -INFINITY;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        e[4 * v + 0] = __fmul_rn(beta, U[v].x);
        e[4 * v + 1] = __fmul_rn(beta, U[v].y);
        e[4 * v + 2] = __fmul_rn(beta, U[v].z);
        e[4 * v + 3] = __fmul_rn(beta, U[v].w);
    }
#pragma unroll
    for (int a = 0; a < NV * 4; a++)
        if (a < q && ((allowed >> a) & 1u)) m = fmaxf(m, e[a]);
    float S = 0.f;
#pragma unroll
    for (int a = 0; a < NV * 4; a++) {
        const bool on = a < q && ((allowed >> a) & 1u);
        S += on ? expf(__fsub_rn(e[a], m)) : 0.f;
        e[a] = S;                                   // the running sum; flat across states that are not allowed
    }
    const float u = uniform24(word0);
    const float t = __fmul_rn(u, S);
    int pick = -1, last = 0;
#pragma unroll
    for (int a = 0; a < NV * 4; a++) {
        const bool on = a < q && ((allowed >> a) & 1u);
        if (on) last = a;
        if (on && pick < 0 && e[a] > t) pick = a;
    }
    return pick < 0 ? last : pick;
}

// The two steps of the pipeline as macros over register sets with named members.  The members are native vectors: a
// float4 (a struct) is assigned between address spaces by memcpy, which kept the sets in scratch memory, with a wait
// after every load.
typedef float gs_f4 __attribute__((ext_vector_type(4)));
struct PreSet { gs_f4 a0, a1, a2, a3, a4, a5, a6, a7; };    // GS_PF float4
#define GS_FOR_P(X, pr) X(0, pr) X(1, pr) X(2, pr) X(3, pr) X(4, pr) X(5, pr) X(6, pr) X(7, pr)
#define GS_LOAD_P(p, pr) pr.a##p = ((const gs_f4 *)src4)[min(tid + p * TILE, n4 - 1)];   /* past the chunk: a copy that is not stored */
#define GS_STORE_P(p, pr) { const int k = tid + p * TILE; if (k < n4) ((gs_f4 *)buf)[(k / NV) * NVP + (k % NV)] = pr.a##p; }
#define GS_FETCH(ch_, pr) do { \
                if ((ch_) < n_chunks) { \
                    const int n4 = (min(L, ((ch_) + 1) * JC) - (ch_) * JC) * row4; \
                    const float4 *src4 = Wi + (int64_t)(ch_) * JC * row4; \
                    GS_FOR_P(GS_LOAD_P, pr) \
                } \
    } while (0)
#define GS_STEP(ch_, pr) do { \
                    if ((ch_) < n_chunks) { \
                        const int j0 = (ch_) * JC, j1 = min(L, j0 + JC); \
                        float4 *buf = stage + (g & 1u) * buf_f4; \
                        g++; \
                        const int n4 = (j1 - j0) * row4; \
                        GS_FOR_P(GS_STORE_P, pr) \
                        GS_FETCH((ch_) + GS_DEPTH, pr); \
                        __syncthreads(); \
                        int j = j0; \
                        while (j < j1) { \
                            const uint32_t word = xw[(j >> 2) * TILE + tid]; \
                            if ((j & 3) == 0 && j + 4 <= j1) { \
                                const float4 *r0 = buf + ((j - j0) * q + (word & 0xff)) * NVP; \
                                const float4 *r1 = buf + ((j + 1 - j0) * q + ((word >> 8) & 0xff)) * NVP; \
                                const float4 *r2 = buf + ((j + 2 - j0) * q + ((word >> 16) & 0xff)) * NVP; \
                                const float4 *r3 = buf + ((j + 3 - j0) * q + (word >> 24)) * NVP; \
                                float4 w0[NV], w1[NV], w2[NV], w3[NV]; \
_Pragma("unroll") \
                                for (int v = 0; v < NV; v++) { w0[v] = r0[v]; w1[v] = r1[v]; w2[v] = r2[v]; w3[v] = r3[v]; } \
_Pragma("unroll") \
                                for (int v = 0; v < NV; v++) { \
                                    U[v].x += w0[v].x; U[v].y += w0[v].y; U[v].z += w0[v].z; U[v].w += w0[v].w; \
                                    U[v].x += w1[v].x; U[v].y += w1[v].y; U[v].z += w1[v].z; U[v].w += w1[v].w; \
                                    U[v].x += w2[v].x; U[v].y += w2[v].y; U[v].z += w2[v].z; U[v].w += w2[v].w; \
                                    U[v].x += w3[v].x; U[v].y += w3[v].y; U[v].z += w3[v].z; U[v].w += w3[v].w; \
                                } \
                                j += 4; \
                            } else { \
                                if (j != i) { \
                                    const int x = (word >> (8 * (j & 3))) & 0xff; \
                                    const float4 *row = buf + ((j - j0) * q + x) * NVP; \
_Pragma("unroll") \
                                    for (int v = 0; v < NV; v++) { \
                                        const float4 w = row[v]; \
                                        U[v].x += w.x; U[v].y += w.y; U[v].z += w.z; U[v].w += w.w; \
                                    } \
                                } \
                                j++; \
                            } \
                        } \
                    } \
    } while (0)

// The pipeline of site i: U[a] = init + sum_{j != i} J_ij(a, x_j) of the lane's chain in float32, j = 0 .. L-1, with
// init a float4 expression in v (the fields for k_gibbs, zero for the tempered sweeps).  GS_DEPTH chunks are in flight
// in registers (one LDS round trip per chunk would leave the sweep bound by the latency of the loads: measured,
// section 9.6).  Declares Wi and U; the rest are the locals of the tiled kernels by name.
#define GS_SITE_U(init)                                                                 \
    const float4 *Wi = W + (int64_t)i * L * row4;                                       \
    float4 U[NV];                                                                       \
    _Pragma("unroll") for (int v = 0; v < NV; v++) U[v] = (init);                       \
    PreSet pre0, pre1, pre2;                                                            \
    GS_FETCH(0, pre0);                                                                  \
    GS_FETCH(1, pre1);                                                                  \
    GS_FETCH(2, pre2);                                                                  \
    for (int base = 0; base < n_chunks; base += GS_DEPTH) {                             \
        GS_STEP(base, pre0);                                                            \
        GS_STEP(base + 1, pre1);                                                        \
        GS_STEP(base + 2, pre2);                                                        \
    }

// U_a of a state known only at run time, as a chain of selects over the NV 4 registers (an indexed array would live in
// scratch memory)
template <int NV>
__device__ __forceinline__ float pick_state(const float4 *U, int a) {
    float r = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        r = a == 4 * v + 0 ? U[v].x : r;
        r = a == 4 * v + 1 ? U[v].y : r;
        r = a == 4 * v + 2 ? U[v].z : r;
        r = a == 4 * v + 3 ? U[v].w : r;
    }
    return r;
}

// The frame of the tiled form, once for k_gibbs, tempered_tile and k_anneal: everything around their site loops, as
// text over the kernel's names (NV, TILE, W, L, q, C, JC, and allowed, seed_lo, seed_hi for the start rule).  The site
// loops and the order in which a kernel opens are its own (sections 9.10, 9.13, 9.14).
// GS_TILE_FRAME and GS_TILE_PIPE declare the locals GS_SITE_U / GS_STEP use by name, in two parts because the place of
// the second changes the code: the tempered body declares it at the top, k_gibbs and k_anneal before their sweeps.
// The chain states of the tile live in LDS behind the two staging buffers as xs[L/4][TILE][4] bytes: a lane reads four
// consecutive sites of its chain with one ds_read_b32, the 64 lanes of a wave 256 consecutive bytes.
#define GS_TILE_FRAME()                                                                                        \
    constexpr int NVP = (NV % 2 == 0) ? NV + 1 : NV;                                                           \
    extern __shared__ float4 lds4[];                                                                           \
    const int tid = threadIdx.x;                                                                               \
    const int L4 = (L + 3) >> 2;                                                                               \
    const int c0 = blockIdx.x * TILE;                                                                          \
    const int chain = c0 + tid;                                                                                \
    const int n_here = min(TILE, C - c0);                                                                      \
    const int buf_f4 = JC * q * NVP;                         /* one staging buffer, in float4 */               \
    float4 *stage = lds4;                                                                                      \
    uint8_t *xs = (uint8_t *)(lds4 + 2 * buf_f4);                                                              \
    uint32_t *xw = (uint32_t *)xs;                                                                             \
    const float4 *H = W + (int64_t)L * L * q * NV;
#define GS_TILE_PIPE()                                                                                         \
    const int n_chunks = (L + JC - 1) / JC;                                                                    \
    const int row4 = q * NV;                                 /* float4 of one block W[i][j] */                 \
    uint32_t g = 0;                                          /* chunks staged so far: the LDS buffer alternates with it */
// the byte of site i of the tile's chain `lane` in xs
#define GS_XS(i, lane) ((((i) >> 2) * TILE + (lane)) * 4 + ((i) & 3))
#define GS_ZERO_STATES() for (int k = tid; k < L4 * TILE; k += TILE) xw[k] = 0u;
// the start rule: one draw per site of softmax beta h_i
#define GS_DRAW_START(beta_)                                                                                   \
    for (int i = 0; i < L; i++) {                                                                              \
        float4 Hi[NV];                                                                                         \
        _Pragma("unroll") for (int v = 0; v < NV; v++) Hi[v] = H[i * NV + v];                                  \
        const int a = draw_state<NV>(Hi, q, allowed, (beta_), philox_word0((uint32_t)chain, 0u, GS_START_SWEEP, \
                                                                           (uint32_t)i, seed_lo, seed_hi));    \
        xs[GS_XS(i, tid)] = (uint8_t)a;                                                                        \
    }
// the states of the tile's chains from and to global memory, [C][L]
#define GS_LOAD_STATES(src_)                                                                                   \
    for (int k = tid; k < n_here * L; k += TILE) {                                                             \
        const int c = k / L, j = k - c * L;                                                                    \
        xs[GS_XS(j, c)] = (uint8_t)(src_)[(int64_t)c0 * L + k];                                                \
    }
#define GS_STORE_STATES(dst_)                                                                                  \
    for (int k = tid; k < n_here * L; k += TILE) {                                                             \
        const int c = k / L, j = k - c * L;                                                                    \
        (dst_)[(int64_t)c0 * L + k] = (int8_t)xs[GS_XS(j, c)];                                                 \
    }

// The frame of the direct form, once for k_gibbs_direct, tempered_direct and k_anneal_direct, over the kernel's names
// (QP, Wf, L, q, QS, C, and allowed, seed_lo, seed_hi for the start rule): lanes = (chain, state), 256 / QP chains per
// workgroup, the chain states in LDS as xs[chain][Lp] bytes.  xc, the states of the lane's chain, is GS_DIRECT_XC() at
// the place each kernel declared it: the place changes the code the compiler makes (section 9.14).
#define GS_DIRECT_FRAME()                                                                                      \
    constexpr int CPW = 256 / QP;                                                                              \
    extern __shared__ float4 lds4[];                                                                           \
    uint8_t *xs = (uint8_t *)lds4;                                                                             \
    const int tid = threadIdx.x, a = tid % QP, cl = tid / QP;                                                  \
    const int lane0 = (tid & 63) & ~(QP - 1);                /* the group's first lane within the wave */      \
    (void)lane0;                                                                                               \
    const int Lp = (L + 3) & ~3;                                                                               \
    const int c0 = blockIdx.x * CPW;                                                                           \
    const int chain = c0 + cl;                                                                                 \
    const int n_here = min(CPW, C - c0);                                                                       \
    const float *Hf = Wf + (int64_t)L * L * q * QS;
#define GS_DIRECT_XC() uint8_t *xc = xs + cl * Lp;
// U_a = init + sum_{j != i} J_ij(a, x_j) of the group's chain in float32, j = 0 .. L-1, for site i; init (the field or
// zero) is read after Wi.  Declares Wi and U, as GS_SITE_U does.
#define GS_DIRECT_SITE_U(init)                                                                                 \
    const float *Wi = Wf + (int64_t)i * L * q * QS;                                                            \
    float U = (init);                                                                                          \
    for (int j = 0; j < L; j++) {                                                                              \
        if (j == i) continue;                                                                                  \
        const int x = xc[j];                                                                                   \
        if (a < q) U += Wi[((int64_t)j * q + x) * QS + a];                                                     \
    }
#define GS_DIRECT_ZERO() for (int k = tid; k < CPW * Lp; k += 256) xs[k] = 0;
#define GS_DIRECT_DRAW_START(beta_)                                                                            \
    for (int i = 0; i < L; i++) {                                                                              \
        const float Hi = a < q ? Hf[i * QS + a] : 0.f;                                                         \
        const int x = draw_group<QP>(Hi, a, q, allowed, (beta_), philox_word0((uint32_t)chain, 0u, GS_START_SWEEP, \
                                                                              (uint32_t)i, seed_lo, seed_hi)); \
        if (a == 0) xs[cl * Lp + i] = (uint8_t)x;                                                              \
    }
#define GS_DIRECT_LOAD(src_)                                                                                   \
    for (int k = tid; k < n_here * L; k += 256) {                                                              \
        const int c = k / L, j = k - c * L;                                                                    \
        xs[c * Lp + j] = (uint8_t)(src_)[(int64_t)c0 * L + k];                                                 \
    }
#define GS_DIRECT_STORE(dst_)                                                                                  \
    for (int k = tid; k < n_here * L; k += 256) {                                                              \
        const int c = k / L, j = k - c * L;                                                                    \
        (dst_)[(int64_t)c0 * L + k] = (int8_t)xs[c * Lp + j];                                                  \
    }

// The same draw with one lane per state (groups of QP lanes, QP a power of two >= q): the maximum by a butterfly, the
// running sum by every lane of the group in state order -- the same additions in the same order as draw_state, so the
// two forms of the sweep give the same states bit for bit.
template <int QP>
__device__ __forceinline__ int draw_group(float U, int a, int q, uint32_t allowed, float beta, uint32_t word0) {
    const bool on = a < q && ((allowed >> a) & 1u);
    const float bu = __fmul_rn(beta, U);
    float m = on ? bu : -INFINITY;
#pragma unroll
    for (int o = QP / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const float e = on ? expf(__fsub_rn(bu, m)) : 0.f;
    const int base = (threadIdx.x & 63) & ~(QP - 1);
    float S = 0.f;
    for (int b = 0; b < q; b++) S += __shfl(e, base + b, 64);
    const float u = uniform24(word0);
    const float t = __fmul_rn(u, S);
    int pick = -1, last = 0;
    S = 0.f;
    for (int b = 0; b < q; b++) {
        S += __shfl(e, base + b, 64);
        const bool okb = (allowed >> b) & 1u;
        if (okb) last = b;
        if (okb && pick < 0 && S > t) pick = b;
    }
    return pick < 0 ? last : pick;
}
}  // namespace
