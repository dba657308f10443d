// plm_pt.hip -- parallel tempering (replica exchange) of a Potts model on gfx950 (DESIGN_NEXT_ROWS.md section 9.9).
// C independent ladders of R walkers each sample the family p_beta(x) ~ exp(sum_i h_i(x_i) + beta sum_{i<j} J_ij(x_i, x_j))
// of plm_ais at the R inverse temperatures of the ladder.  Walker w = l R + s is slot s of ladder l and chain w of the
// random numbers; it carries its states, its coupling energy E in float64 and its rung.  A round is n Gibbs sweeps of
// every walker at the beta of its rung, then one exchange pass between neighbouring rungs of the round's parity; an
// exchange swaps rungs, never states.
//
//   k_pt           the tiled form of the tempered sweep (plm_tempered_device.h), the body of k_ais, under the policy of
//                  this file: the lane's own beta, read through the walker's rung, and no log weight
//   k_pt_direct    the direct form: lanes = (walker, state), the same additions in the same order
//   k_pt_swap      one thread per (ladder, pair) of the round's parity; the pairs of one pass are disjoint
//   k_pt_snapshot  states and E in rung order into the output of one snapshot
// The loop over the rounds is enqueued without a host wait unless there is a callback, and allocates nothing.
#include "plm_sample_internal.h"
#include "plm_tempered_device.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace {

// The differences and the product the contract states with one rounding each: the pragma keeps the compiler from
// fusing them (see field_plus_scaled).
__device__ __forceinline__ double exchange_delta(double beta_hi, double beta_lo, double e_a, double e_b) {
#pragma clang fp contract(off)
    const double db = beta_hi - beta_lo;
    const double de = e_a - e_b;
    return db * de;
}

// The policy of the tempered body: one step of n_sweeps sweeps with the indices sweep0 .. (none: a launch that only
// starts the walkers), every lane at the beta of its own walker's rung (a vector register), E the only scalar of a
// walker.  A lane beyond C in the last tile reads no rung.
struct PtPolicy {
    const float *ladder;         // [R]
    const int *rung_of_slot;     // [C]
    uint32_t sweep0;
    int n, mode;
    double *e_io;                // [C]
    float lane_beta;
    static constexpr bool three_start_modes = true;
    __device__ __forceinline__ int start_mode() const { return mode; }
    __device__ __forceinline__ void begin(int chain, int C) { lane_beta = chain < C ? ladder[rung_of_slot[chain]] : 0.f; }
    __device__ __forceinline__ void read(int chain, double &E) const { E = e_io[chain]; }
    __device__ __forceinline__ int first_step() const { return 0; }
    __device__ __forceinline__ int end_step() const { return 1; }
    __device__ __forceinline__ int n_sweeps() const { return n; }
    __device__ __forceinline__ float beta(int) const { return lane_beta; }
    __device__ __forceinline__ void before_sweeps(int, float, double) const {}
    __device__ __forceinline__ uint32_t sweep_index(int, int s) const { return sweep0 + (uint32_t)s; }
    __device__ __forceinline__ void write(int chain, double E) const { e_io[chain] = E; }
};

// C counts walkers (ladders x rungs)
template <int NV, int TILE>
__global__ __launch_bounds__(TILE) void k_pt(const float4 *__restrict__ W, int L, int q, int C, int JC,
                                             const float *__restrict__ ladder /* [R] */,
                                             const int *__restrict__ rung_of_slot /* [C] */, uint32_t sweep0, int n_sweeps,
                                             int mode, uint32_t allowed, uint32_t seed_lo, uint32_t seed_hi,
                                             int8_t *__restrict__ states /* [C][L] */, double *__restrict__ e_io /* [C] */) {
    tempered_tile<NV, TILE>(W, L, q, C, JC, allowed, seed_lo, seed_hi, states,
                            PtPolicy{ladder, rung_of_slot, sweep0, n_sweeps, mode, e_io, 0.f});
}

template <int QP>
__global__ __launch_bounds__(256) void k_pt_direct(const float *__restrict__ Wf, int L, int q, int QS, int C,
                                                   const float *__restrict__ ladder, const int *__restrict__ rung_of_slot,
                                                   uint32_t sweep0, int n_sweeps, int mode, uint32_t allowed,
                                                   uint32_t seed_lo, uint32_t seed_hi, int8_t *__restrict__ states,
                                                   double *__restrict__ e_io) {
    tempered_direct<QP>(Wf, L, q, QS, C, allowed, seed_lo, seed_hi, states,
                        PtPolicy{ladder, rung_of_slot, sweep0, n_sweeps, mode, e_io, 0.f});
}

// The exchange pass of global round g: blockIdx.y (and its stride) counts the pairs of the round's parity, between the
// rungs r = parity + 2 k and r + 1; a thread is one ladder.  It reads the E of the two walkers at those rungs and, on
// acceptance, writes the two entries of either map that belong to its pair: no two threads of a pass touch the same entry.
// The lanes of a wave share r, so a wave adds its count of acceptances to accepts[r] in one atomic.
__global__ __launch_bounds__(256) void k_pt_swap(int n_ladders, int R, int parity, int n_pairs, uint32_t g,
                                                 const float *__restrict__ ladder, const double *__restrict__ e,
                                                 int *__restrict__ rung_of_slot, int *__restrict__ slot_of_rung,
                                                 uint32_t seed_lo, uint32_t seed_hi,
                                                 unsigned long long *__restrict__ accepts /* [R - 1] */) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    for (int k = blockIdx.y; k < n_pairs; k += gridDim.y) {
        const int r = parity + 2 * k;
        bool accept = false;
        if (l < n_ladders) {
            const int64_t w0 = (int64_t)l * R;
            const int a = slot_of_rung[w0 + r], b = slot_of_rung[w0 + r + 1];
            const double delta = exchange_delta((double)ladder[r + 1], (double)ladder[r], e[w0 + a], e[w0 + b]);
            const double u = (double)uniform24(philox_word0((uint32_t)l, 1u, g, (uint32_t)r, seed_lo, seed_hi));
            accept = delta >= 0.0 || u < exp(delta);
            if (accept) {
                slot_of_rung[w0 + r] = b;
                slot_of_rung[w0 + r + 1] = a;
                rung_of_slot[w0 + a] = r + 1;
                rung_of_slot[w0 + b] = r;
            }
        }
        const unsigned long long votes = __ballot(accept);
        if (votes && (threadIdx.x & 63) == 0) atomicAdd(&accepts[r], (unsigned long long)__popcll(votes));
    }
}

// One snapshot: row (l, r) of the output takes the states and E of the walker at rung r of ladder l; with all_rungs == 0
// the only row of a ladder is rung R - 1.  One thread per state.
__global__ __launch_bounds__(256) void k_pt_snapshot(const int8_t *__restrict__ states, const double *__restrict__ e,
                                                     const int *__restrict__ slot_of_rung, int n_ladders, int R, int L,
                                                     int all_rungs, int8_t *__restrict__ out_states,
                                                     double *__restrict__ out_e) {
    const int RO = all_rungs ? R : 1;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_ladders * RO * L) return;
    const int64_t row = t / L;
    const int i = (int)(t - row * L);
    const int l = (int)(row / RO), r = all_rungs ? (int)(row % RO) : R - 1;
    const int64_t w = (int64_t)l * R + slot_of_rung[(int64_t)l * R + r];
    out_states[t] = states[w * L + i];
    if (i == 0) out_e[row] = e[w];
}

struct PtArgs {
    const float4 *W;
    int L, q, C;                 // C: walkers
    const float *ladder;
    const int *rung_of_slot;
    uint32_t sweep0;
    int n_sweeps, mode;
    uint32_t allowed;
    gibbs::Seed seed;
    int8_t *states;
    double *e;
};

// n_sweeps sweeps of every walker under the plan gibbs::plan_sweeps made
hipError_t launch_sweeps(const gibbs::SweepPlan &p, hipStream_t st, const PtArgs &a) {
    return gibbs::dispatch(
        p,
        [&](auto nv, auto tile) {
            return gibbs::launch_tiled(k_pt<nv(), tile()>, tile(), a.C, p, st, a.W, a.L, a.q, a.C, p.JC, a.ladder,
                                       a.rung_of_slot, a.sweep0, a.n_sweeps, a.mode, a.allowed, a.seed.lo, a.seed.hi,
                                       a.states, a.e);
        },
        [&](auto qp) {
            return gibbs::launch_direct(k_pt_direct<qp()>, qp(), a.C, p, st, (const float *)a.W, a.L, a.q, p.NV * 4, a.C,
                                        a.ladder, a.rung_of_slot, a.sweep0, a.n_sweeps, a.mode, a.allowed, a.seed.lo,
                                        a.seed.hi, a.states, a.e);
        });
}

}  // namespace

int plm_pt(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_pt_opts *opts, int device, void *stream,
           plm_pt_cb cb, void *user, plm_pt_result *result) {
    if (!opts || !result) return plm_fail(PLM_EINVAL, "NULL options or result");
    const int L = n_sites, q = n_states, C = opts->n_ladders, R = opts->n_rungs, K = opts->n_snapshots;
    const int n = opts->sweeps_per_round, burn = opts->burn_in, thin = opts->thin, first = opts->first_round;
    if (L < 1 || C < 1 || R < 1 || K < 1 || n < 1 || burn < 0 || thin < 1 || first < 0)
        return plm_fail(PLM_EINVAL, "need n_sites >= 1, n_ladders >= 1, n_rungs >= 1, n_snapshots >= 1, sweeps_per_round >= 1, "
                                    "burn_in >= 0, thin >= 1, first_round >= 0 (got %d, %d, %d, %d, %d, %d, %d, %d)", L, C, R,
                        K, n, burn, thin, first);
    PLM_TRY(gibbs::check_states(q, "parallel tempering"));
    if (!opts->betas) return plm_fail(PLM_EINVAL, "NULL ladder");
    for (int r = 0; r < R; r++)
        if (!isfinite(opts->betas[r]) || !(opts->betas[r] >= (r ? opts->betas[r - 1] : 0.f)))
            return plm_fail(PLM_EINVAL, "the ladder must be finite, non-negative and non-decreasing (betas[%d] = %g)", r,
                            (double)opts->betas[r]);
    const double rounds_d = (double)burn + ((double)K - 1.0) * (double)thin;
    if (((double)first + rounds_d + 1.0) * (double)n >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "(first_round + rounds + 1) x sweeps_per_round must stay below 2^32 - 1 sweeps");
    if (opts->start_rungs && !opts->start) return plm_fail(PLM_EINVAL, "start_rungs without start");
    if (opts->start_e && !(opts->start && opts->start_rungs))
        return plm_fail(PLM_EINVAL, "start_e without start and start_rungs");
    if ((double)C * R * L >= 2147483647.0)
        return plm_fail(PLM_EINVAL, "n_ladders x n_rungs x n_sites must stay below 2^31");
    PLM_TRY(plm_check_device(device));
    // sizes first: nothing below this point is dereferenced before the device is known to hold the call
    const int CR = C * R, RO = opts->all_rungs ? R : 1, rounds = (int)rounds_d;
    const double table_b = gibbs::table_bytes(L, q);
    const double walker_b = (double)CR * L + 16.0 * CR + 12.0 * R;
    const double snap_b = (double)K * C * RO * ((double)L + 8.0);
    PLM_TRY(plm_check_free(table_b + gibbs::canon_bytes(L, q) + walker_b + snap_b, "parallel tempering", table_b));
    if (!x_canonical) return plm_fail(PLM_EINVAL, "NULL model");
    const uint32_t allowed = plm_state_mask(q);
    std::vector<int> ros((size_t)CR), sor((size_t)CR);
    if (opts->start) {
        PLM_TRY(gibbs::check_start(opts->start, CR, L, q, allowed, nullptr));
        for (int l = 0; l < C; l++) {
            int *so = &sor[(size_t)l * R];
            std::fill(so, so + R, -1);
            for (int s = 0; s < R; s++) {
                const int r = opts->start_rungs ? opts->start_rungs[(size_t)l * R + s] : s;
                if (r < 0 || r >= R || so[r] >= 0)
                    return plm_fail(PLM_EINVAL, "start_rungs of ladder %d is not a permutation of 0..%d", l, R - 1);
                so[r] = s;
                ros[(size_t)l * R + s] = r;
            }
        }
    } else {
        for (int w = 0; w < CR; w++) ros[w] = sor[w] = w % R;
    }
    gibbs::SweepPlan plan;
    PLM_TRY(gibbs::plan_sweeps(L, q, CR, device, &plan));

    hipStream_t st = (hipStream_t)stream;
    const size_t WL = (size_t)CR * L, snap_rows = (size_t)C * RO;
    gibbs::DeviceModel model(L, q);
    float *d_ladder = nullptr;
    int8_t *states = nullptr, *snap_x = nullptr;
    double *d_e = nullptr, *snap_e = nullptr;
    int *d_ros = nullptr, *d_sor = nullptr;
    unsigned long long *d_acc = nullptr;
    DeviceBuffers mem;
    PLM_TRY(model.alloc_canon(mem));
    PLM_TRY(mem.alloc(&d_ladder, (size_t)R));
    PLM_TRY(model.alloc_table(mem));
    PLM_TRY(mem.alloc(&states, WL));
    PLM_TRY(mem.alloc(&d_e, (size_t)CR));
    PLM_TRY(mem.alloc(&d_ros, (size_t)CR));
    PLM_TRY(mem.alloc(&d_sor, (size_t)CR));
    PLM_TRY(mem.alloc(&d_acc, (size_t)R));
    PLM_TRY(mem.alloc(&snap_x, (size_t)K * snap_rows * L));
    PLM_TRY(mem.alloc(&snap_e, (size_t)K * snap_rows));
    PLM_HIP(model.upload(st, x_canonical));
    PLM_HIP(hipMemcpyAsync(d_ladder, opts->betas, (size_t)R * sizeof(float), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(d_ros, ros.data(), (size_t)CR * sizeof(int), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(d_sor, sor.data(), (size_t)CR * sizeof(int), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemsetAsync(d_acc, 0, (size_t)R * sizeof(unsigned long long), st));
    PLM_HIP(hipMemsetAsync(snap_x, 0, (size_t)K * snap_rows * L, st));
    PLM_HIP(hipMemsetAsync(snap_e, 0, (size_t)K * snap_rows * sizeof(double), st));
    if (opts->start) PLM_HIP(hipMemcpyAsync(states, opts->start, WL, hipMemcpyHostToDevice, st));
    if (opts->start_e) PLM_HIP(hipMemcpyAsync(d_e, opts->start_e, (size_t)CR * sizeof(double), hipMemcpyHostToDevice, st));
    PLM_HIP(model.expand(st));

    const gibbs::Seed seed(opts->seed);
    PtArgs args = {model.W, L, q, CR, d_ladder, d_ros, 0u, 0, opts->start ? PT_MEASURE : PT_START_RULE, allowed, seed,
                   states, d_e};
    if (!opts->start_e) PLM_HIP(launch_sweeps(plan, st, args));      // the walkers' start: no sweeps
    args.mode = PT_CONTINUE;
    args.n_sweeps = n;
    const unsigned snap_blocks = (unsigned)((snap_rows * L + 255) / 256);
    int done = 0, next_snap = 0, status = PLM_STATUS_CONVERGED;
    for (;;) {
        if (next_snap < K && (int64_t)done == (int64_t)burn + (int64_t)next_snap * thin) {
            hipLaunchKernelGGL(k_pt_snapshot, dim3(snap_blocks), dim3(256), 0, st, states, d_e, d_sor, C, R, L,
                               opts->all_rungs ? 1 : 0, snap_x + (size_t)next_snap * snap_rows * L,
                               snap_e + (size_t)next_snap * snap_rows);
            PLM_HIP(hipGetLastError());
            next_snap++;
        }
        if (done == rounds) break;
        const uint32_t g = (uint32_t)first + (uint32_t)done;
        args.sweep0 = g * (uint32_t)n;
        PLM_HIP(launch_sweeps(plan, st, args));
        const int parity = (int)(g & 1u), n_pairs = (R - parity) / 2;
        if (n_pairs > 0) {
            const dim3 grid((unsigned)((C + 255) / 256), (unsigned)std::min(n_pairs, 65535));
            hipLaunchKernelGGL(k_pt_swap, grid, dim3(256), 0, st, C, R, parity, n_pairs, g, d_ladder, d_e, d_ros, d_sor,
                               seed.lo, seed.hi, d_acc);
            PLM_HIP(hipGetLastError());
        }
        done++;
        if (cb && done < rounds) {
            PLM_HIP(hipStreamSynchronize(st));
            if (cb((int32_t)done, (int32_t)rounds, user)) {
                status = PLM_STATUS_INTERRUPTED;
                break;
            }
        }
    }
    std::vector<unsigned long long> acc((size_t)R, 0ull);
    PLM_HIP(hipMemcpyAsync(acc.data(), d_acc, (size_t)R * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (result->samples)
        PLM_HIP(hipMemcpyAsync(result->samples, snap_x, (size_t)K * snap_rows * L, hipMemcpyDeviceToHost, st));
    if (result->e_j)
        PLM_HIP(hipMemcpyAsync(result->e_j, snap_e, (size_t)K * snap_rows * sizeof(double), hipMemcpyDeviceToHost, st));
    if (result->walkers) PLM_HIP(hipMemcpyAsync(result->walkers, states, WL, hipMemcpyDeviceToHost, st));
    if (result->rungs)
        PLM_HIP(hipMemcpyAsync(result->rungs, d_ros, (size_t)CR * sizeof(int), hipMemcpyDeviceToHost, st));
    if (result->walker_e)
        PLM_HIP(hipMemcpyAsync(result->walker_e, d_e, (size_t)CR * sizeof(double), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    int64_t of_parity[2] = {0, 0};
    for (int d = 0; d < done; d++) of_parity[((uint32_t)first + (uint32_t)d) & 1u]++;
    for (int r = 0; r + 1 < R; r++) {
        if (result->accepts) result->accepts[r] = (int64_t)acc[r];
        if (result->attempts) result->attempts[r] = (int64_t)C * of_parity[r & 1];
    }
    result->rounds_done = done;
    result->status = status;
    return PLM_OK;
}
