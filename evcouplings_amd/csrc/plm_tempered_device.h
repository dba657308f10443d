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
// tiled form took up to 82 registers more (the table in section 9.10).  The pipeline stays the macro over named locals,
// and so is the frame around the site loop, which the bodies share with k_gibbs* and k_anneal* (plm_gibbs_device.h).
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

// The measuring pass a launch of the tiled form may open with, over the locals of the frame by name (no draws; every
// pair is met from both of its sites)
#define TS_MEASURE()                                                                                           \
    for (int i = 0; i < L; i++) {                                                                              \
        GS_SITE_U(make_float4(0.f, 0.f, 0.f, 0.f))                                                             \
        E += (double)pick_state<NV>(U, xs[GS_XS(i, tid)]);                                                     \
    }                                                                                                          \
    E *= 0.5;

// The tiled form.  The LDS layout, the staging and the site order are those of k_gibbs; U starts at zero, the field is
// added after the loop, and E follows through U[a_new] - U[a_old], which the lane holds when it draws.  C counts chains
// (walkers).  A lane beyond C in the last tile reads and writes nothing of its own.
template <int NV, int TILE, typename Policy>
__device__ __forceinline__ void tempered_tile(const float4 *__restrict__ W, int L, int q, int C, int JC, uint32_t allowed,
                                              uint32_t seed_lo, uint32_t seed_hi, int8_t *__restrict__ states /* [C][L] */,
                                              Policy P) {
    GS_TILE_FRAME()
    GS_TILE_PIPE()
    const int mode = P.start_mode();
    P.begin(chain, C);

    GS_ZERO_STATES()
    __syncthreads();
    double E = 0.0;
    if constexpr (Policy::three_start_modes) {             // states, barrier, E
        if (mode == PT_START_RULE) {
            GS_DRAW_START(1.0f)
        } else {
            GS_LOAD_STATES(states)
        }
        __syncthreads();
        if (mode == PT_CONTINUE) {
            if (chain < C) P.read(chain, E);
        } else {
            TS_MEASURE()
        }
    } else if (mode == PT_START_RULE) {                    // two modes: the start with its E, or the continuation
        GS_DRAW_START(1.0f)
        __syncthreads();
        TS_MEASURE()
    } else {
        GS_LOAD_STATES(states)
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
                const int at = GS_XS(i, tid);
                const int a_old = xs[at];
                const int a = draw_state<NV>(arg, q, allowed, 1.0f,
                                             philox_word0((uint32_t)chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
                E += (double)pick_state<NV>(U, a) - (double)pick_state<NV>(U, a_old);
                xs[at] = (uint8_t)a;                       // a lane reads only its own chain: no barrier
            }
        }
    }
    __syncthreads();
    GS_STORE_STATES(states)
    if (chain < C) P.write(chain, E);
}

// The direct form.  Lanes = (chain, state) as in k_gibbs_direct: lane a holds U_a, the two U of the energy step come
// from the lanes a_new and a_old of the group -- the same additions in the same order as the tiled form.  Every lane of
// a group carries the same policy and E; lane 0 writes them.
template <int QP, typename Policy>
__device__ __forceinline__ void tempered_direct(const float *__restrict__ Wf, int L, int q, int QS, int C,
                                                uint32_t allowed, uint32_t seed_lo, uint32_t seed_hi,
                                                int8_t *__restrict__ states, Policy P) {
    GS_DIRECT_FRAME()
    GS_DIRECT_XC()
    const auto site_u = [&](int i) {                       // from zero; a lambda, as the kernels had it (section 9.14)
        GS_DIRECT_SITE_U(0.f)
        return U;
    };
    const int mode = P.start_mode();
    P.begin(chain, C);
    GS_DIRECT_ZERO()
    __syncthreads();
    if (mode == PT_START_RULE) {
        GS_DIRECT_DRAW_START(1.0f)
    } else {
        GS_DIRECT_LOAD(states)
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
    GS_DIRECT_STORE(states)
    if (a == 0 && chain < C) P.write(chain, E);
}

}  // namespace
