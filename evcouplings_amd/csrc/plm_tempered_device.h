// plm_tempered_device.h -- the Gibbs sweep at an inverse temperature on the couplings only, with the coupling energy E
// of every chain followed in float64: the one body, in the tiled and in the direct form, of the sweep kernels of
// plm_ais.hip (k_ais, k_ais_direct) and plm_pt.hip (k_pt, k_pt_direct); DESIGN_NEXT_ROWS.md sections 9.8 - 9.10.
// A kernel builds a policy from its own arguments and calls the body.  The policy answers only where annealed
// importance sampling and parallel tempering differ:
//
//   bool three_start_modes             a constant: the launch may measure E on given states (PT_MEASURE)
//   int start_mode()                   one of the PT_* values below
//   void begin(chain, C)               once, before anything else; the chain exists if chain < C
//   void read(chain, E)                PT_CONTINUE: the chain's scalars from global memory (chain < C)
//   int first_step(), end_step()       the steps [first, end) of the launch; n_sweeps() sweeps in each
//   float beta(step)                   the inverse temperature of the lane's chain in that step
//   void before_sweeps(step, beta, E)  what E is used for before the step's sweeps
//   uint32_t sweep_index(step, s)      the Philox sweep index of sweep s of the step
//   void write(chain, E)               the chain's scalars back to global memory (chain < C)
//
// The bodies are whole kernels on purpose: cut into one function per site update, with U passed as an array, the
// tiled form took up to 82 registers more (the table in section 9.10).  The pipeline stays the macro over named locals.
// The kernels run at the limit of the scalar registers (106, with up to 480 spilled to lanes), so what a policy does
// not need must not be computed for it: begin takes C and not the comparison, which would stay live in a register
// pair to the last line for a policy that ignores it, and the tiled form opens in the statement order each kernel had
// before the bodies were shared (with two modes the measuring pass belongs to the start rule's branch, and a
// continuation reads its scalars before the barrier).  Either costs k_ais up to 50 more spilled registers.
#pragma once
#include "plm_gibbs_device.h"

namespace {

// how a launch of the sweep kernels comes by its states and E
enum { PT_CONTINUE = 0,      // states and E from global memory
       PT_START_RULE = 1,    // the sampler's start rule at beta = 1, E from a measuring pass
       PT_MEASURE = 2 };     // states from global memory, E from a measuring pass

// The product and the sum the contract states with one rounding each.  The _rn intrinsics of HIP are plain operators,
// which the compiler fuses into one multiply-add with a single rounding; the pragma keeps the two roundings.
__device__ __forceinline__ float field_plus_scaled(float h, float beta, float u) {
#pragma clang fp contract(off)
    const float p = beta * u;
    return h + p;
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

// The three passes a launch of the tiled form may open with, over the locals of tempered_tile by name: the start rule
// (one draw per site of softmax h_i), the states of the tile from global memory, and the measuring pass (no draws;
// every pair is met from both of its sites)
#define TS_DRAW_START()                                                                                        \
    for (int i = 0; i < L; i++) {                                                                              \
        float4 Hi[NV];                                                                                         \
        _Pragma("unroll") for (int v = 0; v < NV; v++) Hi[v] = H[i * NV + v];                                  \
        const int a = draw_state<NV>(Hi, q, allowed, 1.0f, philox_word0((uint32_t)chain, 0u, GS_START_SWEEP,   \
                                                                        (uint32_t)i, seed_lo, seed_hi));       \
        xs[((i >> 2) * TILE + tid) * 4 + (i & 3)] = (uint8_t)a;                                                \
    }
#define TS_LOAD_STATES()                                                                                       \
    for (int k = tid; k < n_here * L; k += TILE) {                                                             \
        const int c = k / L, j = k - c * L;                                                                    \
        xs[((j >> 2) * TILE + c) * 4 + (j & 3)] = (uint8_t)states[(int64_t)c0 * L + k];                        \
    }
#define TS_MEASURE()                                                                                           \
    for (int i = 0; i < L; i++) {                                                                              \
        GS_SITE_U(make_float4(0.f, 0.f, 0.f, 0.f))                                                             \
        E += (double)pick_state<NV>(U, xs[((i >> 2) * TILE + tid) * 4 + (i & 3)]);                             \
    }                                                                                                          \
    E *= 0.5;

// The tiled form.  The LDS layout, the staging and the site order are those of k_gibbs; U starts at zero, the field is
// added after the loop, and E follows through U[a_new] - U[a_old], which the lane holds when it draws.  C counts chains
// (walkers).  A lane beyond C in the last tile reads and writes nothing of its own.
template <int NV, int TILE, typename Policy>
__device__ __forceinline__ void tempered_tile(const float4 *__restrict__ W, int L, int q, int C, int JC, uint32_t allowed,
                                              uint32_t seed_lo, uint32_t seed_hi, int8_t *__restrict__ states /* [C][L] */,
                                              Policy P) {
    constexpr int NVP = (NV % 2 == 0) ? NV + 1 : NV;
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x;
    const int L4 = (L + 3) >> 2;
    const int c0 = blockIdx.x * TILE;
    const int chain = c0 + tid;
    const int n_here = min(TILE, C - c0);
    const int buf_f4 = JC * q * NVP;
    float4 *stage = lds4;
    uint8_t *xs = (uint8_t *)(lds4 + 2 * buf_f4);
    uint32_t *xw = (uint32_t *)xs;
    const float4 *H = W + (int64_t)L * L * q * NV;
    const int n_chunks = (L + JC - 1) / JC;
    const int row4 = q * NV;
    uint32_t g = 0;
    const int mode = P.start_mode();
    P.begin(chain, C);

    for (int k = tid; k < L4 * TILE; k += TILE) xw[k] = 0u;
    __syncthreads();
    double E = 0.0;
    if constexpr (Policy::three_start_modes) {             // states, barrier, E
        if (mode == PT_START_RULE) {
            TS_DRAW_START()
        } else {
            TS_LOAD_STATES()
        }
        __syncthreads();
        if (mode == PT_CONTINUE) {
            if (chain < C) P.read(chain, E);
        } else {
            TS_MEASURE()
        }
    } else if (mode == PT_START_RULE) {                    // two modes: the start with its E, or the continuation
        TS_DRAW_START()
        __syncthreads();
        TS_MEASURE()
    } else {
        TS_LOAD_STATES()
        if (chain < C) P.read(chain, E);
        __syncthreads();
    }

    for (int k = P.first_step(); k < P.end_step(); k++) {
        const float beta = P.beta(k);
        P.before_sweeps(k, beta, E);
        for (int s = 0; s < P.n_sweeps(); s++) {
            const uint32_t sweep = P.sweep_index(k, s);
            for (int i = 0; i < L; i++) {
                GS_SITE_U(make_float4(0.f, 0.f, 0.f, 0.f))
                float4 arg[NV];
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float4 hv = H[i * NV + v];
                    arg[v].x = field_plus_scaled(hv.x, beta, U[v].x);
                    arg[v].y = field_plus_scaled(hv.y, beta, U[v].y);
                    arg[v].z = field_plus_scaled(hv.z, beta, U[v].z);
                    arg[v].w = field_plus_scaled(hv.w, beta, U[v].w);
                }
                const int at = ((i >> 2) * TILE + tid) * 4 + (i & 3);
                const int a_old = xs[at];
                const int a = draw_state<NV>(arg, q, allowed, 1.0f,
                                             philox_word0((uint32_t)chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
                E += (double)pick_state<NV>(U, a) - (double)pick_state<NV>(U, a_old);
                xs[at] = (uint8_t)a;                       // a lane reads only its own chain: no barrier
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < n_here * L; k += TILE) {
        const int c = k / L, j = k - c * L;
        states[(int64_t)c0 * L + k] = (int8_t)xs[((j >> 2) * TILE + c) * 4 + (j & 3)];
    }
    if (chain < C) P.write(chain, E);
}

// The direct form.  Lanes = (chain, state) as in k_gibbs_direct: lane a holds U_a, the two U of the energy step come
// from the lanes a_new and a_old of the group -- the same additions in the same order as the tiled form.  Every lane of
// a group carries the same policy and E; lane 0 writes them.
template <int QP, typename Policy>
__device__ __forceinline__ void tempered_direct(const float *__restrict__ Wf, int L, int q, int QS, int C,
                                                uint32_t allowed, uint32_t seed_lo, uint32_t seed_hi,
                                                int8_t *__restrict__ states, Policy P) {
    constexpr int CPW = 256 / QP;
    extern __shared__ float4 lds4[];
    uint8_t *xs = (uint8_t *)lds4;
    const int tid = threadIdx.x, a = tid % QP, cl = tid / QP;
    const int lane0 = (tid & 63) & ~(QP - 1);              // the group's first lane within the wave
    const int Lp = (L + 3) & ~3;
    const int c0 = blockIdx.x * CPW;
    const int chain = c0 + cl;
    const int n_here = min(CPW, C - c0);
    const float *Hf = Wf + (int64_t)L * L * q * QS;
    uint8_t *xc = xs + cl * Lp;
    // U_a = sum_{j != i} J_ij(a, x_j) of the group's chain in float32, j = 0 .. L-1, from zero
    const auto site_u = [&](int i) {
        const float *Wi = Wf + (int64_t)i * L * q * QS;
        float U = 0.f;
        for (int j = 0; j < L; j++) {
            if (j == i) continue;
            const int x = xc[j];
            if (a < q) U += Wi[((int64_t)j * q + x) * QS + a];
        }
        return U;
    };
    const int mode = P.start_mode();
    P.begin(chain, C);
    for (int k = tid; k < CPW * Lp; k += 256) xs[k] = 0;
    __syncthreads();
    if (mode == PT_START_RULE) {
        for (int i = 0; i < L; i++) {
            const float Hi = a < q ? Hf[i * QS + a] : 0.f;
            const int x = draw_group<QP>(Hi, a, q, allowed, 1.0f,
                                         philox_word0((uint32_t)chain, 0u, GS_START_SWEEP, (uint32_t)i, seed_lo, seed_hi));
            if (a == 0) xc[i] = (uint8_t)x;
        }
    } else {
        for (int k = tid; k < n_here * L; k += 256) {
            const int c = k / L, j = k - c * L;
            xs[c * Lp + j] = (uint8_t)states[(int64_t)c0 * L + k];
        }
    }
    __syncthreads();
    double E = 0.0;
    if (mode == PT_CONTINUE) {
        if (chain < C) P.read(chain, E);
    } else {
        for (int i = 0; i < L; i++) E += (double)__shfl(site_u(i), lane0 + xc[i], 64);   // the measuring pass
        E *= 0.5;
    }
    for (int k = P.first_step(); k < P.end_step(); k++) {
        const float beta = P.beta(k);
        P.before_sweeps(k, beta, E);
        for (int s = 0; s < P.n_sweeps(); s++) {
            const uint32_t sweep = P.sweep_index(k, s);
            for (int i = 0; i < L; i++) {
                const float U = site_u(i);
                const float arg = a < q ? field_plus_scaled(Hf[i * QS + a], beta, U) : 0.f;
                const int x_old = xc[i];
                const int x = draw_group<QP>(arg, a, q, allowed, 1.0f,
                                             philox_word0((uint32_t)chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
                E += (double)__shfl(U, lane0 + x, 64) - (double)__shfl(U, lane0 + x_old, 64);
                if (a == 0) xc[i] = (uint8_t)x;            // the group is inside one wave: its lanes have read x_old
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < n_here * L; k += 256) {
        const int c = k / L, j = k - c * L;
        states[(int64_t)c0 * L + k] = (int8_t)xs[c * Lp + j];
    }
    if (a == 0 && chain < C) P.write(chain, E);
}

}  // namespace
