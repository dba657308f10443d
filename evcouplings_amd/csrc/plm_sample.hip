// plm_sample.hip -- Gibbs sampler of a fitted Potts model on gfx950: draw sequences from
//     P(x) ~ exp beta (sum_i h_i(x_i) + sum_{i<j} J_ij(x_i, x_j)).
// The reference has no sampler (its numba loops stop at _hamiltonians / _delta_hamiltonian, couplings/model.py:25-177);
// the contract, the random-number scheme and the layout are in DESIGN_NEXT_ROWS.md section 9.6.
//
//   k_sample_expand  canonical i<j blocks -> W[i][j][b][a] = J_ij(a, b) for every ordered pair, float32, a contiguous and
//                    padded to a multiple of 4 states, followed by the fields padded the same way
//   k_gibbs          a workgroup owns a tile of chains (one lane per chain, the conditional's q energies in VGPRs) and
//                    walks sweeps x sites itself; W rows reach the lanes through LDS in chunks of j
//   k_gibbs_direct   the other form: lanes = (chain, state), W rows read straight from global memory
//   k_field_energy   (H, H_J, H_h) of the field-only model (L = 1), which the forward GEMM of plm_hamiltonians cannot take
#include "plm_sample_internal.h"
#include "plm_gibbs_device.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace {

__device__ __forceinline__ int64_t pair_index(int i, int j, int L) {   // i < j, row-major
    return (int64_t)i * (2 * L - i - 1) / 2 + (j - i - 1);
}

// W[((i L + j) q + b) QS + a] = J_ij(a, b); zero for i == j and for the padding states a >= q.  The fields follow at
// W + L L q QS as [L][QS].  One thread per float4 of the output.
__global__ __launch_bounds__(256) void k_sample_expand(const float *__restrict__ canon, int L, int q, int QS,
                                                      float4 *__restrict__ W) {
    const int NV = QS >> 2;
    const int64_t n_w = (int64_t)L * L * q * NV, n_all = n_w + (int64_t)L * NV;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_all) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (t >= n_w) {
        const int64_t r = t - n_w;
        const int i = (int)(r / NV), a0 = (int)(r % NV) * 4;
        for (int k = 0; k < 4; k++)
            if (a0 + k < q) v[k] = canon[(int64_t)i * q + a0 + k];
    } else {
        const int a0 = (int)(t % NV) * 4;
        int64_t r = t / NV;
        const int b = (int)(r % q);
        r /= q;
        const int j = (int)(r % L), i = (int)(r / L);
        const float *J = canon + (int64_t)L * q;
        if (i != j)
            for (int k = 0; k < 4; k++) {
                const int a = a0 + k;
                if (a < q)
                    v[k] = i < j ? J[(pair_index(i, j, L) * q + a) * q + b] : J[(pair_index(j, i, L) * q + b) * q + a];
            }
    }
    W[t] = make_float4(v[0], v[1], v[2], v[3]);
}

// The frame (locals, the chain states in LDS, start rule, loads and stores) is GS_TILE_FRAME and its companions in
// plm_gibbs_device.h, shared with the tempered and the annealing kernels.  A chunk of JC blocks W[i][j0 .. j0+JC) is
// contiguous in global memory; the workgroup copies it into one of two LDS buffers (rows padded from NV to NVP float4
// so that 16 lanes with 16 different rows hit 16 different 4-bank groups of a ds_read_b128) while it computes from the
// other.  Sites are visited 0 .. L-1, and U accumulates in float32 over j = 0 .. L-1 without i: the order of the
// contract.  src == NULL: the chains start from the start rule (one draw per site of softmax beta h_i).
template <int NV, int TILE>
__global__ __launch_bounds__(TILE) void k_gibbs(const float4 *__restrict__ W, int L, int q, int C, int JC,
                                                const int8_t *__restrict__ src /* [C][L] or NULL: start rule */,
                                                const uint8_t *__restrict__ fixed /* [L] or NULL */, uint32_t allowed,
                                                float beta, uint32_t seed_lo, uint32_t seed_hi, uint32_t sweep0,
                                                int n_sweeps, int8_t *__restrict__ dst /* [C][L] */) {
    GS_TILE_FRAME()

    // ---- initial states ----
    GS_ZERO_STATES()
    __syncthreads();
    if (src) {
        GS_LOAD_STATES(src)
    } else {
        GS_DRAW_START(beta)
    }
    __syncthreads();

    GS_TILE_PIPE()
    for (int s = 0; s < n_sweeps; s++) {
        const uint32_t sweep = sweep0 + (uint32_t)s;
        for (int i = 0; i < L; i++) {
            if (fixed && fixed[i]) continue;                  // uniform over the workgroup
            GS_SITE_U(H[i * NV + v])
            const int a = draw_state<NV>(U, q, allowed, beta,
                                         philox_word0((uint32_t)chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
            xs[GS_XS(i, tid)] = (uint8_t)a;                   // a lane reads only its own chain: no barrier
        }
    }
    __syncthreads();
    GS_STORE_STATES(dst)
}

// The other form of the sweep: lanes = (chain, state), 256 / QP chains per workgroup, the row W[i][j][x_cj][.] read
// straight from global memory (every workgroup walks the same rows at about the same time, so they come from L2).  No
// staging and little LDS (the chain states, [chain][L] bytes), but 64 / QP chains per wave instead of 64.  It serves
// the lengths whose chain states do not fit the LDS in the tiled form, and PLM_SAMPLE_FORM=direct selects it for
// measurements (tests/probes/sample_probe.py).
template <int QP>
__global__ __launch_bounds__(256) void k_gibbs_direct(const float *__restrict__ Wf, int L, int q, int QS, int C,
                                                      const int8_t *__restrict__ src, const uint8_t *__restrict__ fixed,
                                                      uint32_t allowed, float beta, uint32_t seed_lo, uint32_t seed_hi,
                                                      uint32_t sweep0, int n_sweeps, int8_t *__restrict__ dst) {
    GS_DIRECT_FRAME()
    GS_DIRECT_ZERO()
    __syncthreads();
    if (src) {
        GS_DIRECT_LOAD(src)
    } else {
        GS_DIRECT_DRAW_START(beta)
    }
    __syncthreads();
    for (int s = 0; s < n_sweeps; s++) {
        const uint32_t sweep = sweep0 + (uint32_t)s;
        for (int i = 0; i < L; i++) {
            if (fixed && fixed[i]) continue;
            GS_DIRECT_XC()
            GS_DIRECT_SITE_U(a < q ? Hf[i * QS + a] : 0.f)
            const int x = draw_group<QP>(U, a, q, allowed, beta,
                                         philox_word0((uint32_t)chain, 0u, sweep, (uint32_t)i, seed_lo, seed_hi));
            if (a == 0) xc[i] = (uint8_t)x;
            __syncthreads();
        }
    }
    __syncthreads();
    GS_DIRECT_STORE(dst)
}

// (H, H_J, H_h) = (h(x), 0, h(x)) of the one-site model
__global__ void k_field_energy(const float *__restrict__ h, const int8_t *__restrict__ x, int64_t n, double *__restrict__ en) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const double v = (double)h[x[t]];
    en[3 * t + 0] = v;
    en[3 * t + 1] = 0.0;
    en[3 * t + 2] = v;
}

typedef gibbs::SweepPlan Plan;

const int TILES[3] = {64, 128, 256};            // chains per workgroup of the tiled form
const int CHUNKS[6] = {1, 2, 4, 8, 12, 16};     // sites j per staged chunk

// the row of a plan: float4 per q states, and the odd number of float4 the row takes in LDS
Plan plan_rows(int q) {
    Plan p = {};
    p.NV = (q + 3) / 4;
    p.NVP = (p.NV % 2 == 0) ? p.NV + 1 : p.NV;
    return p;
}

// The planner's own checks of one (tile, j-chunk): a chunk is at most GS_PF float4 per thread, and the two staging
// buffers and the chain states fit the LDS of a CU.  Nothing that fails them is ever launched.
bool tiled_fits(int L, int q, int tile, int JC, Plan *p) {
    if ((size_t)JC * q * p->NV > (size_t)GS_PF * tile) return false;
    const size_t lds = 2 * (size_t)JC * q * p->NVP * 16 + (size_t)((L + 3) / 4) * tile * 4;
    if (lds > GS_LDS_BYTES) return false;
    p->tile = tile;
    p->JC = JC;
    p->lds = lds;
    return true;
}

// tile of chains per workgroup, j-chunk and LDS size: the largest tile that still gives every CU a workgroup, limited
// by what the chain states leave of the LDS.  force_tile / force_jc != 0 (PLM_SAMPLE_TILE / PLM_SAMPLE_JC) replace the
// two preferences -- the spread over the CUs, and no chunk of 2 L sites or more -- and none of the checks.
bool make_plan(int L, int q, int C, int n_cu, int force_tile, int force_jc, Plan *out) {
    Plan p = plan_rows(q);
    for (int t = 2; t >= 0; t--) {
        const int tile = TILES[t];
        if (force_tile ? tile != force_tile : (tile > 64 && (C + tile - 1) / tile < n_cu)) continue;   // spread small calls over the CUs
        for (int c = 5; c >= 0; c--) {
            const int JC = CHUNKS[c];
            if (force_jc ? JC != force_jc : (JC > 1 && JC >= 2 * L)) continue;
            if (tiled_fits(L, q, tile, JC, &p)) {
                *out = p;
                return true;
            }
        }
    }
    return false;       // tile 64 with JC = 1 is the smallest plan there is: no other tile or chunk fits either
}

// lanes per chain of the direct form: the power of two >= q, and a larger one (fewer chains per workgroup, the lanes
// a >= q idle) where the states of that many chains would not fit the LDS
int direct_group(int L, int q) {
    int g = q <= 2 ? 2 : q <= 4 ? 4 : q <= 8 ? 8 : q <= 16 ? 16 : 32;
    while (g < 32 && (size_t)(256 / g) * ((L + 3) / 4 * 4) > GS_LDS_BYTES) g *= 2;
    return g;
}
size_t direct_lds(int L, int q) { return (size_t)(256 / direct_group(L, q)) * ((L + 3) / 4 * 4); }

// 0: the variable is not set; -1: it is set to something else than one of the values
int env_choice(const char *name, const int *values, int n) {
    const char *v = getenv(name);
    if (!v || !*v) return 0;
    char *end = nullptr;
    const long x = strtol(v, &end, 10);
    if (*end) return -1;
    for (int k = 0; k < n; k++)
        if (x == values[k]) return values[k];
    return -1;
}

// The one place a plan is made: plm_sample, plm_ais and plm_bm_fit (through gibbs::plan_sweeps) and plm_sample_plan.
// Host code.
int choose_plan(int L, int q, int C, int n_cu, Plan *out) {
    const int force_tile = env_choice("PLM_SAMPLE_TILE", TILES, 3), force_jc = env_choice("PLM_SAMPLE_JC", CHUNKS, 6);
    if (force_tile < 0) return plm_fail(PLM_EINVAL, "PLM_SAMPLE_TILE must be 64, 128 or 256 (got '%s')", getenv("PLM_SAMPLE_TILE"));
    if (force_jc < 0) return plm_fail(PLM_EINVAL, "PLM_SAMPLE_JC must be 1, 2, 4, 8, 12 or 16 (got '%s')", getenv("PLM_SAMPLE_JC"));
    // the tiled form wherever the chain states fit the LDS; the direct form for longer models, or on request
    // (PLM_SAMPLE_FORM=direct | tiled, measurements only: the two forms return the same states).  PLM_SAMPLE_TILE and
    // PLM_SAMPLE_JC (measurements and tests only) choose among the plans of the tiled form and say nothing when the
    // direct form is asked for.
    const char *form = getenv("PLM_SAMPLE_FORM");
    bool direct = form && !strcmp(form, "direct");
    Plan plan = {};
    if (!direct && !make_plan(L, q, C, n_cu, force_tile, force_jc, &plan)) {
        if (force_tile || force_jc)
            return plm_fail(PLM_EINVAL, "%s%s%s: no such plan for %d sites with %d states (a chunk needs JC q ceil(q/4) <= %d x tile "
                                        "and the workgroup at most %d bytes of LDS)", force_tile ? "PLM_SAMPLE_TILE" : "",
                            force_tile && force_jc ? " with " : "", force_jc ? "PLM_SAMPLE_JC" : "", L, q, GS_PF, GS_LDS_BYTES);
        if (form && !strcmp(form, "tiled"))
            return plm_fail(PLM_EUNSUPPORTED, "%d sites with %d states: the chain states of a workgroup do not fit the LDS of a CU", L, q);
        direct = true;
    }
    if (direct) {
        if (direct_lds(L, q) > GS_LDS_BYTES)
            return plm_fail(PLM_EUNSUPPORTED, "%d sites with %d states: the chain states of a workgroup do not fit the LDS of a CU", L, q);
        plan = plan_rows(q);
        plan.tile = 256 / direct_group(L, q);      // chains per workgroup
        plan.lds = direct_lds(L, q);
    }
    plan.direct = direct;
    *out = plan;
    return PLM_OK;
}

}  // namespace

namespace gibbs {

int check_states(int q, const char *who) {
    if (q < 2 || q > GS_Q) return plm_fail(PLM_EUNSUPPORTED, "%s supports 2..32 states (got %d)", who, q);
    return PLM_OK;
}

int check_chain_sites(int C, int L) {
    if ((double)C * L >= 2147483647.0) return plm_fail(PLM_EINVAL, "n_chains x n_sites must stay below 2^31");
    return PLM_OK;
}

double table_bytes(int L, int q) { return 16.0 * ((double)L * L * q + (double)L) * plan_rows(q).NV; }
double canon_bytes(int L, int q) { return 4.0 * plm_n_canon(L, q); }

int check_start(const int8_t *start, int C, int L, int q, uint32_t allowed, const uint8_t *fixed) {
    for (size_t k = 0; k < (size_t)C * L; k++) {
        const int v = start[k];
        const int site = (int)(k % (size_t)L);
        if (v < 0 || v >= q) return plm_fail(PLM_EINVAL, "start[%zu] = %d outside 0..%d", k, v, q - 1);
        if (!((allowed >> v) & 1u) && !(fixed && fixed[site]))
            return plm_fail(PLM_EINVAL, "start[%zu] = %d is not an allowed state and site %d is not fixed", k, v, site);
    }
    return PLM_OK;
}

int allowed_mask(int q, const uint8_t *flags, uint32_t *out) {
    uint32_t m = flags ? 0u : plm_state_mask(q);
    for (int a = 0; flags && a < q; a++)
        if (flags[a]) m |= 1u << a;
    if (!m) return plm_fail(PLM_EINVAL, "no state is allowed");
    *out = m;
    return PLM_OK;
}

int plan_sweeps(int L, int q, int C, int device, SweepPlan *out) {
    hipDeviceProp_t prop;
    PLM_HIP(hipGetDeviceProperties(&prop, device));
    return choose_plan(L, q, C, prop.multiProcessorCount, out);
}

size_t table_float4(int L, int q) { return ((size_t)L * L * q + (size_t)L) * plan_rows(q).NV; }

hipError_t expand(hipStream_t st, const float *canon, int L, int q, float4 *W) {
    hipLaunchKernelGGL(k_sample_expand, dim3((unsigned)((table_float4(L, q) + 255) / 256)), dim3(256), 0, st, canon, L, q,
                       plan_rows(q).NV * 4, W);
    return hipGetLastError();
}

hipError_t sweeps(const SweepPlan &p, hipStream_t st, const float4 *W, int L, int q, int C, const int8_t *src,
                  const uint8_t *fixed, uint32_t allowed, float beta, uint64_t seed, uint32_t sweep0, int n_sweeps,
                  int8_t *dst) {
    const Seed sd(seed);
    return dispatch(
        p,
        [&](auto nv, auto tile) {
            return launch_tiled(k_gibbs<nv(), tile()>, tile(), C, p, st, W, L, q, C, p.JC, src, fixed, allowed, beta, sd.lo,
                                sd.hi, sweep0, n_sweeps, dst);
        },
        [&](auto qp) {
            return launch_direct(k_gibbs_direct<qp()>, qp(), C, p, st, (const float *)W, L, q, p.NV * 4, C, src, fixed,
                                 allowed, beta, sd.lo, sd.hi, sweep0, n_sweeps, dst);
        });
}

// Steps per launch that keep a launch near a second: a workgroup of the tiled form spends about 150 ns per pair of sites
// at q = 21 (13 ms per sweep of 300 sites, section 9.6), in proportion to the row width; the workgroups beyond one per CU
// queue; the direct form is taken as eight times slower.  An estimate: no result depends on it.
int default_steps_per_launch(const SweepPlan &p, int L, int C, int n_per, int K, int n_cu) {
    const double rounds = std::ceil((double)((C + p.tile - 1) / p.tile) / std::max(n_cu, 1));
    double per_step = (double)n_per * rounds * (double)L * L * 150e-9 * p.NV / 6.0;
    if (p.direct) per_step *= 8.0;
    const double steps = 1.0 / std::max(per_step, 1e-9);
    return steps >= (double)K ? K : std::max(1, (int)steps);
}

int state_energies(const int8_t *rows, size_t n_rows, int L, int q, const float *x_canonical, int device, void *stream,
                   double *energies_out) {
    if (L == 1) {
        hipStream_t st = (hipStream_t)stream;
        float *h = nullptr;
        int8_t *x = nullptr;
        double *en = nullptr;
        DeviceBuffers mem;
        PLM_TRY(mem.alloc(&h, (size_t)q));
        PLM_TRY(mem.alloc(&x, n_rows));
        PLM_TRY(mem.alloc(&en, n_rows * 3));
        PLM_HIP(hipMemcpyAsync(h, x_canonical, (size_t)q * sizeof(float), hipMemcpyHostToDevice, st));
        PLM_HIP(hipMemcpyAsync(x, rows, n_rows, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_field_energy, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, h, x, (int64_t)n_rows, en);
        PLM_HIP(hipGetLastError());
        PLM_HIP(hipMemcpyAsync(energies_out, en, n_rows * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        PLM_HIP(hipStreamSynchronize(st));
        return PLM_OK;
    }
    // the code path of plm_hamiltonians, in row chunks that stay inside its limit on sequences per call
    const size_t Lp = ((size_t)L + 31) / 32 * 32;
    const size_t max_rows = std::max<size_t>(256, (((size_t)1 << 30) / Lp) / 256 * 256);
    int rc = PLM_OK;
    for (size_t r0 = 0; r0 < n_rows && rc == PLM_OK; r0 += max_rows) {
        const size_t n = std::min(max_rows, n_rows - r0);
        rc = plm_hamiltonians(rows + r0 * L, (int32_t)n, L, q, x_canonical, device, stream, energies_out + r0 * 3);
    }
    return rc;
}

}  // namespace gibbs

int plm_sample_plan(int32_t n_sites, int32_t n_states, int32_t n_chains, int32_t n_cu, plm_sample_plan_info *out) {
    if (!out) return plm_fail(PLM_EINVAL, "NULL plan");
    if (n_sites < 1 || n_chains < 1)
        return plm_fail(PLM_EINVAL, "need n_sites >= 1 and n_chains >= 1 (got %d, %d)", n_sites, n_chains);
    int rc = gibbs::check_states(n_states, "the sampler");
    if (rc) return rc;
    Plan plan;
    if (n_cu > 0) {
        rc = choose_plan(n_sites, n_states, n_chains, n_cu, &plan);      // no device, no HIP call
    } else {
        int device = 0;
        PLM_HIP(hipGetDevice(&device));
        rc = gibbs::plan_sweeps(n_sites, n_states, n_chains, device, &plan);
    }
    if (rc) return rc;
    out->direct = plan.direct ? 1 : 0;
    out->tile = plan.tile;
    out->jc = plan.direct ? 0 : plan.JC;
    out->nv = plan.NV;
    out->n_workgroups = (n_chains + plan.tile - 1) / plan.tile;
    out->lds_bytes = (int64_t)plan.lds;
    return PLM_OK;
}

int plm_sample(int32_t n_sites, int32_t n_states, const float *x_canonical, const plm_sample_opts *opts, int device,
               void *stream, int8_t *samples_out, double *energies_out) {
    if (!opts) return plm_fail(PLM_EINVAL, "NULL options");
    const int L = n_sites, q = n_states, C = opts->n_chains, K = opts->n_snapshots;
    if (L < 1 || C < 1 || K < 1 || opts->burn_in < 0 || (K > 1 && opts->thin < 1))
        return plm_fail(PLM_EINVAL, "need n_sites >= 1, n_chains >= 1, n_snapshots >= 1, burn_in >= 0, thin >= 1 "
                                    "(got %d, %d, %d, %d, %d)", L, C, K, opts->burn_in, opts->thin);
    PLM_TRY(gibbs::check_states(q, "the sampler"));
    if (!(opts->beta > 0.f) || !isfinite(opts->beta))
        return plm_fail(PLM_EINVAL, "beta must be finite and > 0 (got %g)", (double)opts->beta);
    const int thin = K > 1 ? opts->thin : 0;
    if ((double)opts->burn_in + (double)(K - 1) * thin >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "burn_in + (n_snapshots - 1) thin must stay below 2^32 - 1 sweeps");
    PLM_TRY(plm_check_device(device));
    // sizes first: nothing below this point is dereferenced before the device is known to hold the call
    const double table_b = gibbs::table_bytes(L, q);
    const double state_b = (double)C * L * ((double)K + 1.0) + L;
    const double energy_b = energies_out ? 24.0 * C : 0.0;
    PLM_TRY(plm_check_free(table_b + gibbs::canon_bytes(L, q) + state_b + energy_b, "the sampler", table_b));
    PLM_TRY(gibbs::check_chain_sites(C, L));
    if (!x_canonical || !samples_out) return plm_fail(PLM_EINVAL, "NULL argument");
    uint32_t allowed = 0;
    PLM_TRY(gibbs::allowed_mask(q, opts->allowed, &allowed));
    if (opts->start) PLM_TRY(gibbs::check_start(opts->start, C, L, q, allowed, opts->fixed));
    Plan plan;
    PLM_TRY(gibbs::plan_sweeps(L, q, C, device, &plan));
    hipStream_t st = (hipStream_t)stream;
    const size_t CL = (size_t)C * L;
    gibbs::DeviceModel model(L, q);
    int8_t *start = nullptr, *snaps = nullptr;
    uint8_t *fixed = nullptr;
    double *en = nullptr;
    DeviceBuffers mem;
    PLM_TRY(model.alloc_canon(mem));
    PLM_TRY(model.alloc_table(mem));
    PLM_TRY(mem.alloc(&snaps, CL * (size_t)K));
    if (opts->start) PLM_TRY(mem.alloc(&start, CL));
    if (opts->fixed) PLM_TRY(mem.alloc(&fixed, (size_t)L));
    if (energies_out && L == 1) PLM_TRY(mem.alloc(&en, CL * (size_t)K * 3));
    PLM_HIP(model.upload(st, x_canonical));
    if (start) PLM_HIP(hipMemcpyAsync(start, opts->start, CL, hipMemcpyHostToDevice, st));
    if (fixed) PLM_HIP(hipMemcpyAsync(fixed, opts->fixed, (size_t)L, hipMemcpyHostToDevice, st));
    PLM_HIP(model.expand(st));
    for (int k = 0; k < K; k++) {
        const int8_t *src = k == 0 ? start : snaps + (size_t)(k - 1) * CL;
        const uint32_t sweep0 = k == 0 ? 0u : (uint32_t)opts->burn_in + (uint32_t)(k - 1) * (uint32_t)thin;
        PLM_HIP(gibbs::sweeps(plan, st, model.W, L, q, C, src, fixed, allowed, opts->beta, opts->seed, sweep0,
                              k == 0 ? opts->burn_in : thin, snaps + (size_t)k * CL));
    }
    PLM_HIP(hipMemcpyAsync(samples_out, snaps, CL * (size_t)K, hipMemcpyDeviceToHost, st));
    if (en) {
        const int64_t n = (int64_t)CL * K;
        hipLaunchKernelGGL(k_field_energy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, model.canon, snaps, n, en);
        PLM_HIP(hipGetLastError());
        PLM_HIP(hipMemcpyAsync(energies_out, en, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    PLM_HIP(hipStreamSynchronize(st));
    mem.free_all();                          // before plm_hamiltonians allocates its own
    // the statistical energies of the snapshots at beta = 1
    if (energies_out && L > 1)
        return gibbs::state_energies(samples_out, (size_t)C * (size_t)K, L, q, x_canonical, device, stream, energies_out);
    return PLM_OK;
}
