// plm_anneal.hip -- simulated annealing and greedy ascent on a Potts model on gfx950 (DESIGN_NEXT_ROWS.md section 9.13):
// the search for sequences of high statistical energy H(x) = sum_i h_i(x_i) + sum_{i<j} J_ij(x_i, x_j).  Every chain
// makes Gibbs sweeps of plm_sample's contract at the inverse temperatures of a schedule (the temperature acts on fields
// and couplings alike, so a step is bit for bit a sweep of plm_sample at that beta), then deterministic greedy sweeps up
// to a local optimum, and keeps the best state it met at the checkpoints after every step.
//
//   k_anneal          the tiled form: one lane per chain, the LDS layout and the staging pipeline of k_gibbs
//   k_anneal_direct   the direct form: lanes = (chain, state), as k_gibbs_direct
// A launch runs the annealing steps [k0, k1) of the schedule, or a run of greedy sweeps; between launches the chain
// lives in global memory (states, gain, best, best_gain, best_at, last_move, converged).
//
// The body is not the tempered one (plm_tempered_device.h): there U starts at zero and the temperature scales the
// couplings only; here U starts at the field as in k_gibbs, sites can be fixed, and the greedy step draws nothing.
// What surrounds the site loop is the frame of plm_gibbs_device.h, which all the sweep kernels share.
#include "plm_sample_internal.h"
#include "plm_gibbs_device.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace {

// what a launch does, the same for both forms
struct AnnealArgs {
    const float *betas;          // [K] on the device, NULL when K == 0
    const uint8_t *fixed;        // [L] or NULL
    int8_t *states, *best;       // [C][L]
    double *gain, *best_gain;    // [C]
    int32_t *best_at, *last_move;
    uint8_t *converged;
    int k0, k1, n_per;           // the annealing steps [k0, k1) of this launch, n_per sweeps in each
    int n_greedy, greedy_done;   // then at most n_greedy greedy sweeps, numbered from greedy_done + 1
    int final_at;                // != 0: the number of the checkpoint that follows the greedy sweeps (K + 1)
    int start_rule;              // != 0: the states come from the start rule and are checkpoint 0
    uint32_t first_sweep, allowed, seed_lo, seed_hi;
};

// a* = the first allowed state in state order with the largest U, and that U; -1 when no comparison succeeded
template <int NV>
__device__ __forceinline__ int greedy_state(const float4 *U, int q, uint32_t allowed, float &u_best) {
    float m = -INFINITY;
    int best = -1;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const float u[4] = {U[v].x, U[v].y, U[v].z, U[v].w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int a = 4 * v + k;
            const bool up = a < q && ((allowed >> a) & 1u) && u[k] > m;
            m = up ? u[k] : m;
            best = up ? a : best;
        }
    }
    u_best = m;
    return best;
}

// The tiled form.  Everything up to the sweeps is k_gibbs; a lane beyond C in the last tile walks a chain of zeros,
// counts as converged and writes nothing.
template <int NV, int TILE>
__global__ __launch_bounds__(TILE) void k_anneal(const float4 *__restrict__ W, int L, int q, int C, int JC, AnnealArgs A) {
    GS_TILE_FRAME()
    const uint32_t allowed = A.allowed, seed_lo = A.seed_lo, seed_hi = A.seed_hi;

    GS_ZERO_STATES()
    __syncthreads();
    if (A.start_rule) {
        GS_DRAW_START(1.0f)
    } else {
        GS_LOAD_STATES(A.states)
    }
    __syncthreads();
    if (A.start_rule) {                                       // checkpoint 0
        GS_STORE_STATES(A.best)
    }
    double gain = 0.0, best_gain = 0.0;
    int best_at = 0, last_move = 0;
    bool conv = true;
    if (chain < C) {
        gain = A.gain[chain];
        best_gain = A.best_gain[chain];
        best_at = A.best_at[chain];
        last_move = A.last_move[chain];
        conv = A.converged[chain] != 0;
    }

    GS_TILE_PIPE()
    const int k_end = A.k1 + (A.n_greedy > 0 ? 1 : 0);       // the greedy sweeps run as one more step
    for (int k = A.k0; k < k_end; k++) {
        const bool greedy = k >= A.k1;
        const float beta = greedy ? 1.0f : A.betas[k];
        const int n_sweeps = greedy ? A.n_greedy : A.n_per;
        for (int s = 0; s < n_sweeps; s++) {
            const uint32_t sweep = A.first_sweep + (uint32_t)k * (uint32_t)A.n_per + (uint32_t)s;
            bool moved = false;
            for (int i = 0; i < L; i++) {
                if (A.fixed && A.fixed[i]) continue;          // uniform over the workgroup
                GS_SITE_U(H[i * NV + v])
                const int at = GS_XS(i, tid);
                const int a_old = xs[at];
                const float u_old = pick_state<NV>(U, a_old);
                int a;
                float u_new;
                if (greedy) {
                    a = greedy_state<NV>(U, q, allowed, u_new);
                    if (!(u_new > u_old)) {                   // a tie never moves
                        a = a_old;
                        u_new = u_old;
                    }
                } else {
                    a = draw_state<NV>(U, q, allowed, beta,
                                       philox_word0((uint32_t)chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
                    u_new = pick_state<NV>(U, a);
                }
                gain += (double)u_new - (double)u_old;
                moved = moved || a != a_old;
                xs[at] = (uint8_t)a;                          // a lane reads only its own chain: no barrier
            }
            if (greedy) {
                if (moved) last_move = A.greedy_done + s + 1;
                else conv = true;
                if (__syncthreads_and(conv)) break;           // every live chain of the tile is a fixed point
            }
        }
        const int at_no = greedy ? A.final_at : k + 1;
        if (at_no && chain < C && gain > best_gain) {         // the checkpoint: the lane copies its own chain
            best_gain = gain;
            best_at = at_no;
            for (int j = 0; j < L; j++) A.best[(int64_t)chain * L + j] = (int8_t)xs[GS_XS(j, tid)];
        }
    }
    __syncthreads();
    GS_STORE_STATES(A.states)
    if (chain < C) {
        A.gain[chain] = gain;
        A.best_gain[chain] = best_gain;
        A.best_at[chain] = best_at;
        A.last_move[chain] = last_move;
        A.converged[chain] = conv ? 1 : 0;
    }
}

// The direct form.  Lane a of a group holds U_a; the greedy maximum is a butterfly over (U, state) that prefers the
// lower state on equal U, so every lane of the group ends with the a* of the tiled form.  Every lane of a group carries
// the chain's scalars; lane 0 writes them.
template <int QP>
__global__ __launch_bounds__(256) void k_anneal_direct(const float *__restrict__ Wf, int L, int q, int QS, int C,
                                                       AnnealArgs A) {
    GS_DIRECT_FRAME()
    GS_DIRECT_XC()
    const uint32_t allowed = A.allowed, seed_lo = A.seed_lo, seed_hi = A.seed_hi;
    const bool on = a < q && ((allowed >> a) & 1u);
    GS_DIRECT_ZERO()
    __syncthreads();
    if (A.start_rule) {
        GS_DIRECT_DRAW_START(1.0f)
    } else {
        GS_DIRECT_LOAD(A.states)
    }
    __syncthreads();
    if (A.start_rule) {                                       // checkpoint 0
        GS_DIRECT_STORE(A.best)
    }
    double gain = 0.0, best_gain = 0.0;
    int best_at = 0, last_move = 0;
    bool conv = true;
    if (chain < C) {
        gain = A.gain[chain];
        best_gain = A.best_gain[chain];
        best_at = A.best_at[chain];
        last_move = A.last_move[chain];
        conv = A.converged[chain] != 0;
    }
    const int k_end = A.k1 + (A.n_greedy > 0 ? 1 : 0);
    for (int k = A.k0; k < k_end; k++) {
        const bool greedy = k >= A.k1;
        const float beta = greedy ? 1.0f : A.betas[k];
        const int n_sweeps = greedy ? A.n_greedy : A.n_per;
        for (int s = 0; s < n_sweeps; s++) {
            const uint32_t sweep = A.first_sweep + (uint32_t)k * (uint32_t)A.n_per + (uint32_t)s;
            bool moved = false;
            for (int i = 0; i < L; i++) {
                if (A.fixed && A.fixed[i]) continue;
                GS_DIRECT_SITE_U(a < q ? Hf[i * QS + a] : 0.f)
                const int x_old = xc[i];
                const float u_old = __shfl(U, lane0 + x_old, 64);
                int x;
                float u_new;
                if (greedy) {
                    float m = on ? U : -INFINITY;
                    int am = on ? a : QP;
#pragma unroll
                    for (int o = QP / 2; o > 0; o >>= 1) {
                        const float m2 = __shfl_xor(m, o, 64);
                        const int a2 = __shfl_xor(am, o, 64);
                        const bool take = m2 > m || (m2 == m && a2 < am);
                        m = take ? m2 : m;
                        am = take ? a2 : am;
                    }
                    const bool go = m > u_old;                // a tie never moves
                    x = go ? am : x_old;
                    u_new = go ? m : u_old;
                } else {
                    x = draw_group<QP>(U, a, q, allowed, beta,
                                       philox_word0((uint32_t)chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
                    u_new = __shfl(U, lane0 + x, 64);
                }
                gain += (double)u_new - (double)u_old;
                moved = moved || x != x_old;
                if (a == 0) xc[i] = (uint8_t)x;               // the group is inside one wave: its lanes have read x_old
                __syncthreads();
            }
            if (greedy) {
                if (moved) last_move = A.greedy_done + s + 1;
                else conv = true;
                if (__syncthreads_and(conv)) break;
            }
        }
        const int at_no = greedy ? A.final_at : k + 1;
        if (at_no && chain < C && gain > best_gain) {         // the lanes of the group share the copy
            best_gain = gain;
            best_at = at_no;
            for (int j = a; j < L; j += QP) A.best[(int64_t)chain * L + j] = (int8_t)xc[j];
        }
    }
    __syncthreads();
    GS_DIRECT_STORE(A.states)
    if (a == 0 && chain < C) {
        A.gain[chain] = gain;
        A.best_gain[chain] = best_gain;
        A.best_at[chain] = best_at;
        A.last_move[chain] = last_move;
        A.converged[chain] = conv ? 1 : 0;
    }
}

// one launch under the plan gibbs::plan_sweeps made
hipError_t launch_anneal(const gibbs::SweepPlan &p, hipStream_t st, const float4 *W, int L, int q, int C,
                         const AnnealArgs &a) {
    return gibbs::dispatch(
        p,
        [&](auto nv, auto tile) {
            return gibbs::launch_tiled(k_anneal<nv(), tile()>, tile(), C, p, st, W, L, q, C, p.JC, a);
        },
        [&](auto qp) {
            return gibbs::launch_direct(k_anneal_direct<qp()>, qp(), C, p, st, (const float *)W, L, q, p.NV * 4, C, a);
        });
}

}  // namespace

int plm_anneal(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_anneal_opts *opts, int device,
               void *stream, plm_anneal_cb cb, void *user, plm_anneal_result *result) {
    if (!opts || !result) return plm_fail(PLM_EINVAL, "NULL options or result");
    const int L = n_sites, q = n_states, C = opts->n_chains, K = opts->n_steps, n = opts->sweeps_per_step;
    const int G = opts->max_greedy;
    if (L < 1 || C < 1 || K < 0 || n < 1 || G < 0 || opts->steps_per_launch < 0)
        return plm_fail(PLM_EINVAL, "need n_sites >= 1, n_chains >= 1, n_steps >= 0, sweeps_per_step >= 1, max_greedy >= 0, "
                                    "steps_per_launch >= 0 (got %d, %d, %d, %d, %d, %d)", L, C, K, n, G, opts->steps_per_launch);
    if (K == 0 && G == 0) return plm_fail(PLM_EINVAL, "n_steps and max_greedy are both 0: nothing to do");
    PLM_TRY(gibbs::check_states(q, "annealing"));
    if ((K > 0) != (opts->betas != nullptr))
        return plm_fail(PLM_EINVAL, "betas must hold n_steps values, and be NULL when n_steps is 0");
    for (int k = 0; k < K; k++)
        if (!isfinite(opts->betas[k]) || !(opts->betas[k] > 0.f))
            return plm_fail(PLM_EINVAL, "betas must be finite and > 0 (betas[%d] = %g)", k, (double)opts->betas[k]);
    if ((double)opts->first_sweep + (double)K * (double)n >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "first_sweep + n_steps x sweeps_per_step must stay below 2^32 - 1 sweeps");
    uint32_t allowed = 0;
    PLM_TRY(gibbs::allowed_mask(q, opts->allowed, &allowed));
    PLM_TRY(plm_check_device(device));
    // sizes first: nothing below this point is dereferenced before the device is known to hold the call
    const double table_b = gibbs::table_bytes(L, q);
    const double chain_b = 2.0 * C * L + 28.0 * C + 4.0 * K + L;
    PLM_TRY(plm_check_free(table_b + gibbs::canon_bytes(L, q) + chain_b, "annealing", table_b));
    PLM_TRY(gibbs::check_chain_sites(C, L));
    if (!x_canonical) return plm_fail(PLM_EINVAL, "NULL model");
    if (opts->start) PLM_TRY(gibbs::check_start(opts->start, C, L, q, allowed, opts->fixed));
    gibbs::SweepPlan plan;
    PLM_TRY(gibbs::plan_sweeps(L, q, C, device, &plan));
    int n_cu = 0;
    PLM_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    // annealing steps per launch, and greedy sweeps per launch: the sweeps of as many steps
    const int per_launch = K == 0 ? 1
                           : opts->steps_per_launch > 0 ? std::min(opts->steps_per_launch, K)
                                                        : gibbs::default_steps_per_launch(plan, L, C, n, K, n_cu);
    const int greedy_per_launch =
        G == 0 ? 1
        : opts->steps_per_launch > 0 ? (int)std::min<int64_t>((int64_t)opts->steps_per_launch * n, G)
                                     : gibbs::default_steps_per_launch(plan, L, C, 1, G, n_cu);

    hipStream_t st = (hipStream_t)stream;
    const size_t CL = (size_t)C * L;
    gibbs::DeviceModel model(L, q);
    float *d_betas = nullptr;
    AnnealArgs a = {};
    uint8_t *fixed = nullptr;
    DeviceBuffers mem;
    PLM_TRY(model.alloc_canon(mem));
    PLM_TRY(model.alloc_table(mem));
    PLM_TRY(mem.alloc(&a.states, CL));
    PLM_TRY(mem.alloc(&a.best, CL));
    PLM_TRY(mem.alloc(&a.gain, (size_t)C));
    PLM_TRY(mem.alloc(&a.best_gain, (size_t)C));
    PLM_TRY(mem.alloc(&a.best_at, (size_t)C));
    PLM_TRY(mem.alloc(&a.last_move, (size_t)C));
    PLM_TRY(mem.alloc(&a.converged, (size_t)C));
    if (K > 0) PLM_TRY(mem.alloc(&d_betas, (size_t)K));
    if (opts->fixed) PLM_TRY(mem.alloc(&fixed, (size_t)L));
    PLM_HIP(model.upload(st, x_canonical));
    if (K > 0) PLM_HIP(hipMemcpyAsync(d_betas, opts->betas, (size_t)K * sizeof(float), hipMemcpyHostToDevice, st));
    if (fixed) PLM_HIP(hipMemcpyAsync(fixed, opts->fixed, (size_t)L, hipMemcpyHostToDevice, st));
    if (opts->start) {                                        // checkpoint 0 of given states
        PLM_HIP(hipMemcpyAsync(a.states, opts->start, CL, hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(a.best, opts->start, CL, hipMemcpyHostToDevice, st));
    }
    PLM_HIP(hipMemsetAsync(a.gain, 0, (size_t)C * sizeof(double), st));
    PLM_HIP(hipMemsetAsync(a.best_gain, 0, (size_t)C * sizeof(double), st));
    PLM_HIP(hipMemsetAsync(a.best_at, 0, (size_t)C * sizeof(int32_t), st));
    PLM_HIP(hipMemsetAsync(a.last_move, 0, (size_t)C * sizeof(int32_t), st));
    PLM_HIP(hipMemsetAsync(a.converged, 0, (size_t)C, st));
    PLM_HIP(model.expand(st));
    a.betas = d_betas;
    a.fixed = fixed;
    a.n_per = n;
    a.start_rule = opts->start ? 0 : 1;
    a.first_sweep = opts->first_sweep;
    a.allowed = allowed;
    const gibbs::Seed seed(opts->seed);
    a.seed_lo = seed.lo;
    a.seed_hi = seed.hi;

    int steps_done = 0, status = PLM_STATUS_CONVERGED;
    while (steps_done < K) {
        a.k0 = steps_done;
        a.k1 = std::min(K, steps_done + per_launch);
        PLM_HIP(launch_anneal(plan, st, model.W, L, q, C, a));
        a.start_rule = 0;
        steps_done = a.k1;
        if (cb && (steps_done < K || G > 0)) {
            PLM_HIP(hipStreamSynchronize(st));
            if (cb((int32_t)steps_done, (int32_t)K, user)) {
                status = PLM_STATUS_INTERRUPTED;
                break;
            }
        }
    }
    if (status == PLM_STATUS_CONVERGED) {
        a.k0 = a.k1 = K;
        for (int done = 0; done < G; done += greedy_per_launch) {
            a.n_greedy = std::min(greedy_per_launch, G - done);
            a.greedy_done = done;
            a.final_at = done + a.n_greedy == G ? K + 1 : 0;
            PLM_HIP(launch_anneal(plan, st, model.W, L, q, C, a));
            a.start_rule = 0;
        }
    }

    const bool want_en = result->energies != nullptr, want_best_en = result->best_energies != nullptr;
    std::vector<int8_t> states_h, best_h;                     // the rows the energies are taken of, when not returned
    int8_t *states_out = result->states, *best_out = result->best;
    if (want_en && !states_out) {
        states_h.resize(CL);
        states_out = states_h.data();
    }
    if (want_best_en && !best_out) {
        best_h.resize(CL);
        best_out = best_h.data();
    }
    if (states_out) PLM_HIP(hipMemcpyAsync(states_out, a.states, CL, hipMemcpyDeviceToHost, st));
    if (best_out) PLM_HIP(hipMemcpyAsync(best_out, a.best, CL, hipMemcpyDeviceToHost, st));
    if (result->gain) PLM_HIP(hipMemcpyAsync(result->gain, a.gain, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (result->best_gain)
        PLM_HIP(hipMemcpyAsync(result->best_gain, a.best_gain, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (result->best_at)
        PLM_HIP(hipMemcpyAsync(result->best_at, a.best_at, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (result->last_move)
        PLM_HIP(hipMemcpyAsync(result->last_move, a.last_move, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (result->converged) PLM_HIP(hipMemcpyAsync(result->converged, a.converged, (size_t)C, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    mem.free_all();                          // before plm_hamiltonians allocates its own
    result->steps_done = steps_done;
    result->status = status;
    if (want_en) PLM_TRY(gibbs::state_energies(states_out, (size_t)C, L, q, x_canonical, device, stream, result->energies));
    if (want_best_en)
        PLM_TRY(gibbs::state_energies(best_out, (size_t)C, L, q, x_canonical, device, stream, result->best_energies));
    return PLM_OK;
}
