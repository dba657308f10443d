// plm_ais.hip -- log Z of a Potts model by annealed importance sampling on gfx950 (DESIGN_NEXT_ROWS.md section 9.8).
// The path p_beta(x) ~ exp(sum_i h_i(x_i) + beta sum_{i<j} J_ij(x_i, x_j)) runs from the independent-site model of the
// fields (beta = 0, sampled exactly, log Z_0 in closed form) to the couplings scaled by the last beta.  Every chain makes
// Gibbs sweeps of plm_sample's contract with the temperature on the couplings only, and carries its coupling energy E
// and its log weight in float64: log w += (beta_k - beta_{k-1}) E before the sweeps at beta_k.
//
//   k_ais          the tiled form of the tempered sweep (plm_tempered_device.h) under the policy of this file
//   k_ais_direct   the direct form: lanes = (chain, state), the two U by shuffles inside the group
// A launch runs the steps [k0, k1) of the schedule; the first one draws the start states and measures E there.
#include "plm_sample_internal.h"
#include "plm_tempered_device.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace {

// The product and the sum the contract states with one rounding each (see field_plus_scaled): the pragma keeps the
// compiler from fusing them into one multiply-add.
__device__ __forceinline__ double weight_step(double logw, double dbeta, double e) {
#pragma clang fp contract(off)
    const double p = dbeta * e;
    return logw + p;
}

// The policy of the tempered body: the steps [k0, k1) of the schedule, n_per sweeps at betas[k + 1] after the weight
// step of log w, one beta for the whole launch (a scalar register).  first != 0: the start rule, log w = 0 and E from
// the measuring pass; otherwise states, E and log w are read, and all are written back.
struct AisPolicy {
    const float *betas;          // [K + 1]
    int k0, k1, n_per, first;
    double *e_io, *logw_io;      // [C]
    double logw;
    static constexpr bool three_start_modes = false;
    __device__ __forceinline__ int start_mode() const { return first ? PT_START_RULE : PT_CONTINUE; }
    __device__ __forceinline__ void begin(int, int) {}
    __device__ __forceinline__ void read(int chain, double &E) {
        E = e_io[chain];
        logw = logw_io[chain];
    }
    __device__ __forceinline__ int first_step() const { return k0; }
    __device__ __forceinline__ int end_step() const { return k1; }
    __device__ __forceinline__ int n_sweeps() const { return n_per; }
    __device__ __forceinline__ float beta(int k) const { return betas[k + 1]; }
    __device__ __forceinline__ void before_sweeps(int k, float beta, double E) {
        logw = weight_step(logw, (double)beta - (double)betas[k], E);
    }
    __device__ __forceinline__ uint32_t sweep_index(int k, int s) const {
        return (uint32_t)k * (uint32_t)n_per + (uint32_t)s;
    }
    __device__ __forceinline__ void write(int chain, double E) const {
        e_io[chain] = E;
        logw_io[chain] = logw;
    }
};

template <int NV, int TILE>
__global__ __launch_bounds__(TILE) void k_ais(const float4 *__restrict__ W, int L, int q, int C, int JC,
                                              const float *__restrict__ betas /* [K + 1] */, int k0, int k1, int n_per,
                                              int first, uint32_t allowed, uint32_t seed_lo, uint32_t seed_hi,
                                              int8_t *__restrict__ states /* [C][L] */, double *__restrict__ e_io /* [C] */,
                                              double *__restrict__ logw_io /* [C] */) {
    tempered_tile<NV, TILE>(W, L, q, C, JC, allowed, seed_lo, seed_hi, states,
                            AisPolicy{betas, k0, k1, n_per, first, e_io, logw_io, 0.0});
}

template <int QP>
__global__ __launch_bounds__(256) void k_ais_direct(const float *__restrict__ Wf, int L, int q, int QS, int C,
                                                    const float *__restrict__ betas, int k0, int k1, int n_per, int first,
                                                    uint32_t allowed, uint32_t seed_lo, uint32_t seed_hi,
                                                    int8_t *__restrict__ states, double *__restrict__ e_io,
                                                    double *__restrict__ logw_io) {
    tempered_direct<QP>(Wf, L, q, QS, C, allowed, seed_lo, seed_hi, states,
                        AisPolicy{betas, k0, k1, n_per, first, e_io, logw_io, 0.0});
}

struct AisArgs {
    const float4 *W;
    int L, q, C;
    const float *betas;
    int k0, k1, n_per, first;
    uint32_t allowed;
    uint64_t seed;
    int8_t *states;
    double *e, *logw;
};

// the steps [k0, k1) under the plan gibbs::plan_sweeps made
hipError_t launch_steps(const gibbs::SweepPlan &p, hipStream_t st, const AisArgs &a) {
    const gibbs::Seed sd(a.seed);
    return gibbs::dispatch(
        p,
        [&](auto nv, auto tile) {
            return gibbs::launch_tiled(k_ais<nv(), tile()>, tile(), a.C, p, st, a.W, a.L, a.q, a.C, p.JC, a.betas, a.k0, a.k1,
                                       a.n_per, a.first, a.allowed, sd.lo, sd.hi, a.states, a.e, a.logw);
        },
        [&](auto qp) {
            return gibbs::launch_direct(k_ais_direct<qp()>, qp(), a.C, p, st, (const float *)a.W, a.L, a.q, p.NV * 4, a.C,
                                        a.betas, a.k0, a.k1, a.n_per, a.first, a.allowed, sd.lo, sd.hi, a.states, a.e,
                                        a.logw);
        });
}

}  // namespace

int plm_ais(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_ais_opts *opts, int device,
            void *stream, plm_ais_cb cb, void *user, plm_ais_result *result) {
    if (!opts || !result) return plm_fail(PLM_EINVAL, "NULL options or result");
    const int L = n_sites, q = n_states, C = opts->n_chains, K = opts->n_temps, n = opts->sweeps_per_temp;
    if (L < 1 || C < 1 || K < 1 || n < 1 || opts->steps_per_launch < 0)
        return plm_fail(PLM_EINVAL, "need n_sites >= 1, n_chains >= 1, n_temps >= 1, sweeps_per_temp >= 1, "
                                    "steps_per_launch >= 0 (got %d, %d, %d, %d, %d)", L, C, K, n, opts->steps_per_launch);
    PLM_TRY(gibbs::check_states(q, "annealed importance sampling"));
    if ((double)K * (double)n >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "n_temps x sweeps_per_temp must stay below 2^32 - 1 sweeps");
    if (opts->betas) {
        if (opts->betas[0] != 0.f) return plm_fail(PLM_EINVAL, "betas[0] must be 0 (got %g)", (double)opts->betas[0]);
        for (int k = 1; k <= K; k++)
            if (!isfinite(opts->betas[k]) || !(opts->betas[k] >= opts->betas[k - 1]))
                return plm_fail(PLM_EINVAL, "betas must be finite and non-decreasing (betas[%d] = %g after %g)", k,
                                (double)opts->betas[k], (double)opts->betas[k - 1]);
    }
    PLM_TRY(plm_check_device(device));
    // sizes first: nothing below this point is dereferenced before the device is known to hold the call
    const double table_b = gibbs::table_bytes(L, q);
    const double chain_b = (double)C * L + 16.0 * C + 4.0 * ((double)K + 1.0);
    PLM_TRY(plm_check_free(table_b + gibbs::canon_bytes(L, q) + chain_b, "annealed importance sampling", table_b));
    PLM_TRY(gibbs::check_chain_sites(C, L));
    if (!x_canonical) return plm_fail(PLM_EINVAL, "NULL model");
    gibbs::SweepPlan plan;
    PLM_TRY(gibbs::plan_sweeps(L, q, C, device, &plan));
    int n_cu = 0;
    PLM_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    const int per_launch = opts->steps_per_launch > 0 ? std::min(opts->steps_per_launch, K)
                                                      : gibbs::default_steps_per_launch(plan, L, C, n, K, n_cu);

    // log Z_0 = sum_i log sum_a exp h_i(a) in float64
    double log_z0 = 0.0;
    for (int i = 0; i < L; i++) {
        const float *h = x_canonical + (size_t)i * q;
        double m = h[0], s = 0.0;
        for (int a = 1; a < q; a++) m = std::max(m, (double)h[a]);
        for (int a = 0; a < q; a++) s += exp((double)h[a] - m);
        log_z0 += m + log(s);
    }
    std::vector<float> betas((size_t)K + 1);
    for (int k = 0; k <= K; k++) betas[k] = opts->betas ? opts->betas[k] : (float)((double)k / (double)K);

    hipStream_t st = (hipStream_t)stream;
    const size_t CL = (size_t)C * L;
    gibbs::DeviceModel model(L, q);
    float *d_betas = nullptr;
    int8_t *states = nullptr;
    double *d_e = nullptr, *d_logw = nullptr;
    DeviceBuffers mem;
    PLM_TRY(model.alloc_canon(mem));
    PLM_TRY(mem.alloc(&d_betas, betas.size()));
    PLM_TRY(model.alloc_table(mem));
    PLM_TRY(mem.alloc(&states, CL));
    PLM_TRY(mem.alloc(&d_e, (size_t)C));
    PLM_TRY(mem.alloc(&d_logw, (size_t)C));
    PLM_HIP(model.upload(st, x_canonical));
    PLM_HIP(hipMemcpyAsync(d_betas, betas.data(), betas.size() * sizeof(float), hipMemcpyHostToDevice, st));
    PLM_HIP(model.expand(st));
    AisArgs args = {model.W, L, q, C, d_betas, 0, 0, n, 1, plm_state_mask(q), opts->seed, states, d_e, d_logw};
    int steps_done = 0, status = PLM_STATUS_CONVERGED;
    while (steps_done < K) {
        args.k0 = steps_done;
        args.k1 = std::min(K, steps_done + per_launch);
        args.first = steps_done == 0;
        PLM_HIP(launch_steps(plan, st, args));
        steps_done = args.k1;
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
    if (result->e_j) PLM_HIP(hipMemcpyAsync(result->e_j, d_e, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (result->states) PLM_HIP(hipMemcpyAsync(result->states, states, CL, hipMemcpyDeviceToHost, st));
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
