// plm_ais.hip -- log Z of a Potts model by annealed importance sampling on gfx950 (DESIGN_NEXT_ROWS.md section 9.8).
// The path p_beta(x) ~ exp(sum_i h_i(x_i) + beta sum_{i<j} J_ij(x_i, x_j)) runs from the independent-site model of the
// fields (beta = 0, sampled exactly, log Z_0 in closed form) to the couplings scaled by the last beta.  Every chain makes
// Gibbs sweeps of plm_sample's contract with the temperature on the couplings only, and carries its coupling energy E
// and its log weight in float64: log w += (beta_k - beta_{k-1}) E before the sweeps at beta_k.
//
//   k_ais          the tiled form: the pipeline of k_gibbs (plm_gibbs_device.h) with U starting at zero, the field added
//                  after the loop, and E followed through U[a_new] - U[a_old], which the lane holds when it draws
//   k_ais_direct   the direct form: lanes = (chain, state), the two U by shuffles inside the group
// A launch runs the steps [k0, k1) of the schedule; the first one draws the start states and measures E there.
#include "plm_sample_internal.h"
#include "plm_gibbs_device.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace {

// The products and sums the contract states with one rounding each.  The _rn intrinsics of HIP are plain operators,
// which the compiler fuses into one multiply-add with a single rounding; the pragma keeps the two roundings.
__device__ __forceinline__ float field_plus_scaled(float h, float beta, float u) {
#pragma clang fp contract(off)
    const float p = beta * u;
    return h + p;
}
__device__ __forceinline__ double weight_step(double logw, double dbeta, double e) {
#pragma clang fp contract(off)
    const double p = dbeta * e;
    return logw + p;
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

// U[a] = sum_{j != i} J_ij(a, x_j) of the lane's chain in float32, j = 0 .. L-1, from zero: the loop of k_gibbs
#define AIS_SITE_U()                                                                    \
    const float4 *Wi = W + (int64_t)i * L * row4;                                       \
    float4 U[NV];                                                                       \
    _Pragma("unroll") for (int v = 0; v < NV; v++) U[v] = make_float4(0.f, 0.f, 0.f, 0.f); \
    PreSet pre0, pre1, pre2;                                                            \
    GS_FETCH(0, pre0);                                                                  \
    GS_FETCH(1, pre1);                                                                  \
    GS_FETCH(2, pre2);                                                                  \
    for (int base = 0; base < n_chunks; base += GS_DEPTH) {                             \
        GS_STEP(base, pre0);                                                            \
        GS_STEP(base + 1, pre1);                                                        \
        GS_STEP(base + 2, pre2);                                                        \
    }

// The LDS layout, the staging and the site order are those of k_gibbs.  states, E and logw are read (first == 0) and
// written back; first != 0: the start rule at beta = 1, logw = 0 and E from a measuring pass over the sites.
template <int NV, int TILE>
__global__ __launch_bounds__(TILE) void k_ais(const float4 *__restrict__ W, int L, int q, int C, int JC,
                                              const float *__restrict__ betas /* [K + 1] */, int k0, int k1, int n_per,
                                              int first, uint32_t allowed, uint32_t seed_lo, uint32_t seed_hi,
                                              int8_t *__restrict__ states /* [C][L] */, double *__restrict__ e_io /* [C] */,
                                              double *__restrict__ logw_io /* [C] */) {
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

    for (int k = tid; k < L4 * TILE; k += TILE) xw[k] = 0u;
    __syncthreads();
    double E = 0.0, logw = 0.0;
    if (first) {
        for (int i = 0; i < L; i++) {
            float4 Hi[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) Hi[v] = H[i * NV + v];
            const int a = draw_state<NV>(Hi, q, allowed, 1.0f, philox_word0((uint32_t)chain, 0u, GS_START_SWEEP,
                                                                            (uint32_t)i, seed_lo, seed_hi));
            xs[((i >> 2) * TILE + tid) * 4 + (i & 3)] = (uint8_t)a;
        }
        __syncthreads();
        for (int i = 0; i < L; i++) {                      // the measuring pass: no draws
            AIS_SITE_U()
            E += (double)pick_state<NV>(U, xs[((i >> 2) * TILE + tid) * 4 + (i & 3)]);
        }
        E *= 0.5;                                          // every pair was met from both of its sites
    } else {
        for (int k = tid; k < n_here * L; k += TILE) {
            const int c = k / L, j = k - c * L;
            xs[((j >> 2) * TILE + c) * 4 + (j & 3)] = (uint8_t)states[(int64_t)c0 * L + k];
        }
        if (chain < C) {
            E = e_io[chain];
            logw = logw_io[chain];
        }
        __syncthreads();
    }

    for (int k = k0; k < k1; k++) {
        const float beta = betas[k + 1];
        logw = weight_step(logw, (double)beta - (double)betas[k], E);
        for (int s = 0; s < n_per; s++) {
            const uint32_t sweep = (uint32_t)k * (uint32_t)n_per + (uint32_t)s;
            for (int i = 0; i < L; i++) {
                AIS_SITE_U()
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
    if (chain < C) {
        e_io[chain] = E;
        logw_io[chain] = logw;
    }
}

// Lanes = (chain, state) as in k_gibbs_direct: lane a holds U_a, the two U of the energy step come from the lanes a_new
// and a_old of the group.  Every lane of a group carries the same E and logw; lane 0 writes them.
template <int QP>
__global__ __launch_bounds__(256) void k_ais_direct(const float *__restrict__ Wf, int L, int q, int QS, int C,
                                                    const float *__restrict__ betas, int k0, int k1, int n_per, int first,
                                                    uint32_t allowed, uint32_t seed_lo, uint32_t seed_hi,
                                                    int8_t *__restrict__ states, double *__restrict__ e_io,
                                                    double *__restrict__ logw_io) {
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
    for (int k = tid; k < CPW * Lp; k += 256) xs[k] = 0;
    __syncthreads();
    double E = 0.0, logw = 0.0;
    if (first) {
        for (int i = 0; i < L; i++) {
            const float Hi = a < q ? Hf[i * QS + a] : 0.f;
            const int x = draw_group<QP>(Hi, a, q, allowed, 1.0f,
                                         philox_word0((uint32_t)chain, 0u, GS_START_SWEEP, (uint32_t)i, seed_lo, seed_hi));
            if (a == 0) xc[i] = (uint8_t)x;
        }
        __syncthreads();
        for (int i = 0; i < L; i++) {
            const float *Wi = Wf + (int64_t)i * L * q * QS;
            float U = 0.f;
            for (int j = 0; j < L; j++) {
                if (j == i) continue;
                const int x = xc[j];
                if (a < q) U += Wi[((int64_t)j * q + x) * QS + a];
            }
            E += (double)__shfl(U, lane0 + xc[i], 64);
        }
        E *= 0.5;
    } else {
        for (int k = tid; k < n_here * L; k += 256) {
            const int c = k / L, j = k - c * L;
            xs[c * Lp + j] = (uint8_t)states[(int64_t)c0 * L + k];
        }
        if (chain < C) {
            E = e_io[chain];
            logw = logw_io[chain];
        }
        __syncthreads();
    }
    for (int k = k0; k < k1; k++) {
        const float beta = betas[k + 1];
        logw = weight_step(logw, (double)beta - (double)betas[k], E);
        for (int s = 0; s < n_per; s++) {
            const uint32_t sweep = (uint32_t)k * (uint32_t)n_per + (uint32_t)s;
            for (int i = 0; i < L; i++) {
                const float *Wi = Wf + (int64_t)i * L * q * QS;
                float U = 0.f;
                for (int j = 0; j < L; j++) {
                    if (j == i) continue;
                    const int x = xc[j];
                    if (a < q) U += Wi[((int64_t)j * q + x) * QS + a];
                }
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
    if (a == 0 && chain < C) {
        e_io[chain] = E;
        logw_io[chain] = logw;
    }
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
    const uint32_t seed_lo = (uint32_t)(a.seed & 0xFFFFFFFFu), seed_hi = (uint32_t)(a.seed >> 32);
    return gibbs::dispatch(
        p,
        [&](auto nv, auto tile) {
            return gibbs::launch(k_ais<nv(), tile()>, (unsigned)((a.C + tile() - 1) / tile()), tile(), p, st, a.W, a.L, a.q,
                                 a.C, p.JC, a.betas, a.k0, a.k1, a.n_per, a.first, a.allowed, seed_lo, seed_hi, a.states, a.e,
                                 a.logw);
        },
        [&](auto qp) {
            const int cpw = 256 / qp();              // chains per workgroup
            return gibbs::launch(k_ais_direct<qp()>, (unsigned)((a.C + cpw - 1) / cpw), 256, p, st, (const float *)a.W, a.L,
                                 a.q, p.NV * 4, a.C, a.betas, a.k0, a.k1, a.n_per, a.first, a.allowed, seed_lo, seed_hi,
                                 a.states, a.e, a.logw);
        });
}

// Steps per launch that keep a launch near a second: a workgroup of the tiled form spends about 150 ns per pair of sites
// at q = 21 (13 ms per sweep of 300 sites, section 9.6), in proportion to the row width; the workgroups beyond one per CU
// queue; the direct form is taken as eight times slower.  An estimate: the result does not depend on it.
int default_steps_per_launch(const gibbs::SweepPlan &p, int L, int C, int n_per, int K, int n_cu) {
    const double rounds = std::ceil((double)((C + p.tile - 1) / p.tile) / std::max(n_cu, 1));
    double per_step = (double)n_per * rounds * (double)L * L * 150e-9 * p.NV / 6.0;
    if (p.direct) per_step *= 8.0;
    const double steps = 1.0 / std::max(per_step, 1e-9);
    return steps >= (double)K ? K : std::max(1, (int)steps);
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
                                                      : default_steps_per_launch(plan, L, C, n, K, n_cu);

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
    const size_t n_canon = (size_t)plm_n_canon(L, q), CL = (size_t)C * L;
    float *canon = nullptr, *d_betas = nullptr;
    float4 *W = nullptr;
    int8_t *states = nullptr;
    double *d_e = nullptr, *d_logw = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&canon, n_canon));
    PLM_TRY(mem.alloc(&d_betas, betas.size()));
    PLM_TRY(mem.alloc(&W, gibbs::table_float4(L, q)));
    PLM_TRY(mem.alloc(&states, CL));
    PLM_TRY(mem.alloc(&d_e, (size_t)C));
    PLM_TRY(mem.alloc(&d_logw, (size_t)C));
    PLM_HIP(hipMemcpyAsync(canon, x_canonical, n_canon * sizeof(float), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(d_betas, betas.data(), betas.size() * sizeof(float), hipMemcpyHostToDevice, st));
    PLM_HIP(gibbs::expand(st, canon, L, q, W));
    AisArgs args = {W, L, q, C, d_betas, 0, 0, n, 1, plm_state_mask(q), opts->seed, states, d_e,
                    d_logw};
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
    // log Z = log Z_0 + log mean w, the sums in chain order in float64
    double m = logw[0], s1 = 0.0, s2 = 0.0;
    for (int c = 1; c < C; c++) m = std::max(m, logw[c]);
    for (int c = 0; c < C; c++) {
        const double w = exp(logw[c] - m);
        s1 += w;
        s2 += w * w;
    }
    const double mean = s1 / C;
    result->log_z = log_z0 + m + log(mean);
    result->ess = s1 * s1 / s2;
    double var = 0.0;
    for (int c = 0; c < C; c++) {
        const double d = exp(logw[c] - m) - mean;
        var += d * d;
    }
    result->log_z_se = C > 1 ? sqrt(var / (C - 1)) / (sqrt((double)C) * mean) : 0.0;
    return PLM_OK;
}
