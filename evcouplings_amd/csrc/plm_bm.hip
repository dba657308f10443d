// plm_bm.hip -- Boltzmann-machine refinement of a Potts model on gfx950 (plm_bm_fit): gradient ascent on the likelihood of
// target frequencies, the model's marginals estimated by persistent Gibbs chains.  The definition, the layout and the
// state of the measurements are in DESIGN_NEXT_ROWS.md section 9.7; the sweeps are those of plm_sample.hip
// (plm_sample_internal.h).
//
//   k_bm_transpose  chain states [C][L] -> site-major [L][Cp] (Cp = C rounded up to 4, the padding holds 0xFF)
//   k_bm_count      exact int32 counts n_i(a), n_ij(a, b): a workgroup owns site i and a block of sites j, keeps the
//                   q x q histograms of the block in LDS and reads four chains per lane with one dword load per site
//   k_bm_stats      p = n / C, and per workgroup max |fi - pi|, max |fij - pij|, sum (fij - pij)^2
//   k_bm_trace      the trace row from the partials, in a fixed order
//   k_bm_update     x <- x + lr ((f - p) - 2 lambda x)
#include "plm_sample_internal.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>

namespace {

#define BM_PAD 0xFFu            // state of the padding chains: no histogram takes it
#define BM_STAT_BLOCKS 1024     // workgroups of k_bm_stats at most: the order of the reduction depends on the size alone

// 64 x 64 tiles through LDS: rows of src (sites contiguous) in, rows of dst (chains contiguous) out
__global__ __launch_bounds__(256) void k_bm_transpose(const int8_t *__restrict__ x, int C, int L, int Cp,
                                                     uint8_t *__restrict__ xT) {
    __shared__ uint8_t tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, i = i0 + tx;
        tile[r][tx] = (c < C && i < L) ? (uint8_t)x[(int64_t)c * L + i] : (uint8_t)BM_PAD;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int i = i0 + r, c = c0 + tx;
        if (i < L && c < Cp) xT[(int64_t)i * Cp + c] = tile[tx][r];
    }
}

__device__ __forceinline__ int64_t pair_index(int i, int j, int L) {   // i < j, row-major
    return (int64_t)i * (2 * L - i - 1) / 2 + (j - i - 1);
}

// Workgroup (jb, i, z): sites j = jb JB .. jb JB + JB - 1 that are >= i, chain words [z per_z, (z + 1) per_z).  The
// histogram of (i, j) has q q bins; the block with j == i counts n_i on its diagonal.  LDS integer atomics, then one
// global integer atomic per bin that is not empty: integer sums do not depend on the order.
__global__ __launch_bounds__(256) void k_bm_count(const uint32_t *__restrict__ xTw /* [L][n4] */, int L, int q, int n4,
                                                 int JB, int per_z, int32_t *__restrict__ cnt_i,
                                                 int32_t *__restrict__ cnt_ij) {
    extern __shared__ int32_t hist[];                         // [JB][q q]
    const int i = blockIdx.y, j0 = blockIdx.x * JB;
    const int j1 = min(L, j0 + JB);
    if (j1 <= i) return;                                      // uniform: no site of the block is >= i
    const int jlo = max(j0, i);
    const int QQ = q * q;
    for (int k = threadIdx.x; k < JB * QQ; k += 256) hist[k] = 0;
    __syncthreads();
    const int u0 = blockIdx.z * per_z, u1 = min(n4, u0 + per_z);
    const uint32_t *xi = xTw + (int64_t)i * n4;
    for (int u = u0 + threadIdx.x; u < u1; u += 256) {
        const uint32_t wi = xi[u];
        const uint32_t a0 = wi & 0xff, a1 = (wi >> 8) & 0xff, a2 = (wi >> 16) & 0xff, a3 = wi >> 24;
#pragma unroll 4
        for (int j = jlo; j < j1; j++) {
            const uint32_t wj = xTw[(int64_t)j * n4 + u];
            const uint32_t b0 = wj & 0xff, b1 = (wj >> 8) & 0xff, b2 = (wj >> 16) & 0xff, b3 = wj >> 24;
            int32_t *h = hist + (j - j0) * QQ;
            // the states come from the sampler or were checked on the host; the comparison keeps the padding chains
            // (and anything else) out of the table
            if (a0 < (uint32_t)q && b0 < (uint32_t)q) atomicAdd(h + a0 * q + b0, 1);
            if (a1 < (uint32_t)q && b1 < (uint32_t)q) atomicAdd(h + a1 * q + b1, 1);
            if (a2 < (uint32_t)q && b2 < (uint32_t)q) atomicAdd(h + a2 * q + b2, 1);
            if (a3 < (uint32_t)q && b3 < (uint32_t)q) atomicAdd(h + a3 * q + b3, 1);
        }
    }
    __syncthreads();
    for (int j = jlo; j < j1; j++) {
        const int32_t *h = hist + (j - j0) * QQ;
        if (j == i) {
            for (int a = threadIdx.x; a < q; a += 256) {
                const int32_t v = h[a * q + a];
                if (v) atomicAdd(cnt_i + (int64_t)i * q + a, v);
            }
        } else {
            int32_t *dst = cnt_ij + pair_index(i, j, L) * QQ;
            for (int k = threadIdx.x; k < QQ; k += 256) {
                const int32_t v = h[k];
                if (v) atomicAdd(dst + k, v);
            }
        }
    }
}

// cnt, f, p: canonical layout (n_h field entries, then the pair entries).  part[blk] = (max_i, max_ij, sum of squares)
__global__ __launch_bounds__(256) void k_bm_stats(const int32_t *__restrict__ cnt, const float *__restrict__ f, int64_t n,
                                                 int64_t n_h, float chains, float *__restrict__ p,
                                                 double *__restrict__ part) {
    __shared__ float s_mi[256], s_mj[256];
    __shared__ double s_sq[256];
    float mi = 0.f, mj = 0.f;
    double sq = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const float pv = __fdiv_rn((float)cnt[t], chains);
        p[t] = pv;
        const float d = fabsf(__fsub_rn(f[t], pv));
        if (t < n_h) {
            mi = fmaxf(mi, d);
        } else {
            mj = fmaxf(mj, d);
            sq += (double)d * (double)d;
        }
    }
    s_mi[threadIdx.x] = mi;
    s_mj[threadIdx.x] = mj;
    s_sq[threadIdx.x] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_mi[threadIdx.x] = fmaxf(s_mi[threadIdx.x], s_mi[threadIdx.x + o]);
            s_mj[threadIdx.x] = fmaxf(s_mj[threadIdx.x], s_mj[threadIdx.x + o]);
            s_sq[threadIdx.x] += s_sq[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x + 0] = (double)s_mi[0];
        part[3 * blockIdx.x + 1] = (double)s_mj[0];
        part[3 * blockIdx.x + 2] = s_sq[0];
    }
}

// one workgroup: row = (max_i, max_ij, sqrt(sum / n_pair_entries), lr)
__global__ __launch_bounds__(256) void k_bm_trace(const double *__restrict__ part, int n_part, double n_pair_entries,
                                                 double lr, double *__restrict__ row) {
    __shared__ double s_mi[256], s_mj[256], s_sq[256];
    double mi = 0.0, mj = 0.0, sq = 0.0;
    for (int b = threadIdx.x; b < n_part; b += 256) {
        mi = fmax(mi, part[3 * b + 0]);
        mj = fmax(mj, part[3 * b + 1]);
        sq += part[3 * b + 2];
    }
    s_mi[threadIdx.x] = mi;
    s_mj[threadIdx.x] = mj;
    s_sq[threadIdx.x] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_mi[threadIdx.x] = fmax(s_mi[threadIdx.x], s_mi[threadIdx.x + o]);
            s_mj[threadIdx.x] = fmax(s_mj[threadIdx.x], s_mj[threadIdx.x + o]);
            s_sq[threadIdx.x] += s_sq[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        row[0] = s_mi[0];
        row[1] = s_mj[0];
        row[2] = n_pair_entries > 0.0 ? sqrt(s_sq[0] / n_pair_entries) : 0.0;
        row[3] = lr;
    }
}

// step 6, every operation rounded on its own (no contraction): x + lr ((f - p) - (2 lambda) x)
__global__ __launch_bounds__(256) void k_bm_update(float *__restrict__ x, const float *__restrict__ f,
                                                  const float *__restrict__ p, int64_t n, int64_t n_h, float lr,
                                                  float two_lambda_h, float two_lambda_j) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float xv = x[t];
    const float g = __fsub_rn(__fsub_rn(f[t], p[t]), __fmul_rn(t < n_h ? two_lambda_h : two_lambda_j, xv));
    x[t] = __fadd_rn(xv, __fmul_rn(lr, g));
}

bool bad(float v) { return !(v >= 0.f) || !isfinite(v); }

}  // namespace

int plm_bm_fit(int32_t n_sites, int32_t n_states, const float *fi, const float *fij, const float *x_start,
               const plm_bm_opts *opts, int device, void *stream, plm_bm_epoch_cb cb, void *user, plm_bm_result *result) {
    if (!opts) return plm_fail(PLM_EINVAL, "NULL options");
    if (!result) return plm_fail(PLM_EINVAL, "NULL result");
    const int L = n_sites, q = n_states, C = opts->n_chains, E = opts->n_epochs, K = opts->sweeps_per_epoch;
    const int e0 = opts->first_epoch, T = opts->lr_decay_after;
    if (L < 1 || C < 1 || E < 1 || K < 1 || e0 < 0 || T < 0)
        return plm_fail(PLM_EINVAL, "need n_sites >= 1, n_chains >= 1, n_epochs >= 1, sweeps_per_epoch >= 1, first_epoch >= 0, "
                                    "lr_decay_after >= 0 (got %d, %d, %d, %d, %d, %d)", L, C, E, K, e0, T);
    PLM_TRY(gibbs::check_states(q, "the sampler"));
    if (bad(opts->lr)) return plm_fail(PLM_EINVAL, "lr must be finite and >= 0 (got %g)", (double)opts->lr);
    if (bad(opts->lambda_h)) return plm_fail(PLM_EINVAL, "lambda_h must be finite and >= 0 (got %g)", (double)opts->lambda_h);
    if (bad(opts->lambda_j)) return plm_fail(PLM_EINVAL, "lambda_j must be finite and >= 0 (got %g)", (double)opts->lambda_j);
    if (bad(opts->tol)) return plm_fail(PLM_EINVAL, "tol must be finite and >= 0 (got %g)", (double)opts->tol);
    if (((double)e0 + (double)E) * (double)K >= 4294967295.0)
        return plm_fail(PLM_EINVAL, "(first_epoch + n_epochs) sweeps_per_epoch must stay below 2^32 - 1 sweeps");
    PLM_TRY(plm_check_device(device));
    // sizes first: nothing below this point is dereferenced before the device is known to hold the call
    const double table_b = gibbs::table_bytes(L, q);
    const double canon_b = 4.0 * gibbs::canon_bytes(L, q);                      // x, f, p and the counts
    const double state_b = 3.0 * ((double)C + 3.0) * L;                         // two chain buffers and the site-major copy
    const double small_b = 32.0 * E + 24.0 * BM_STAT_BLOCKS;
    PLM_TRY(plm_check_free(table_b + canon_b + state_b + small_b, "the refinement", table_b));
    PLM_TRY(gibbs::check_chain_sites(C, L));
    if (!fi) return plm_fail(PLM_EINVAL, "NULL fi");
    if (!fij && L > 1) return plm_fail(PLM_EINVAL, "NULL fij");
    if (!x_start) return plm_fail(PLM_EINVAL, "NULL x_start");
    const size_t CL = (size_t)C * L;
    const uint32_t allowed = plm_state_mask(q);
    if (opts->start) PLM_TRY(gibbs::check_start(opts->start, C, L, q, allowed, nullptr));
    gibbs::SweepPlan plan;
    PLM_TRY(gibbs::plan_sweeps(L, q, C, device, &plan));

    hipStream_t st = (hipStream_t)stream;
    const size_t n_h = (size_t)L * q, n = (size_t)plm_n_canon(L, q), n_j = n - n_h;
    const int Cp = (C + 3) / 4 * 4, n4 = Cp / 4;
    const int JB = q <= 22 ? 16 : 8;                                            // at most 32 KB of histograms
    const int n_jb = (L + JB - 1) / JB;
    // split the chains only as far as it takes to fill the device: about 1024 workgroups that do work
    const long useful = std::max<long>(1, (long)n_jb * L / 2);
    const int n_z = (int)std::min<long>(std::max<long>(1, (1024 + useful - 1) / useful), std::max(1, (n4 + 255) / 256));
    const int per_z = (n4 + n_z - 1) / n_z;
    const int n_stat = (int)std::min<size_t>(BM_STAT_BLOCKS, (n + 255) / 256);

    float *x = nullptr, *f = nullptr, *p = nullptr;
    float4 *W = nullptr;
    int32_t *cnt = nullptr;
    int8_t *ch[2] = {nullptr, nullptr};
    uint8_t *xT = nullptr;
    double *part = nullptr, *trace = nullptr, *row_host = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&x, n));
    PLM_TRY(mem.alloc(&f, n));
    PLM_TRY(mem.alloc(&p, n));
    PLM_TRY(mem.alloc(&W, gibbs::table_float4(L, q)));
    PLM_TRY(mem.alloc(&cnt, n));
    PLM_TRY(mem.alloc(&ch[0], CL));
    PLM_TRY(mem.alloc(&ch[1], CL));
    PLM_TRY(mem.alloc(&xT, (size_t)L * Cp));
    PLM_TRY(mem.alloc(&part, (size_t)3 * BM_STAT_BLOCKS));
    PLM_TRY(mem.alloc(&trace, (size_t)4 * E));
    PLM_TRY(mem.alloc_pinned(&row_host, 4));
    PLM_HIP(hipMemcpyAsync(x, x_start, n * sizeof(float), hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(f, fi, n_h * sizeof(float), hipMemcpyHostToDevice, st));
    if (n_j) PLM_HIP(hipMemcpyAsync(f + n_h, fij, n_j * sizeof(float), hipMemcpyHostToDevice, st));
    if (opts->start) PLM_HIP(hipMemcpyAsync(ch[0], opts->start, CL, hipMemcpyHostToDevice, st));

    const bool host_decides = cb != nullptr || opts->tol > 0.f;
    int cur = 0;                                   // ch[cur]: the states the next sweeps start from
    int done_epochs = 0, rows = 0, status = PLM_STATUS_MAXITER;
    for (int ep = 0; ep < E; ep++) {
        const int64_t g = (int64_t)e0 + ep;
        float lr_g = opts->lr;
        if (T > 0 && g + 1 > T) lr_g = (float)((double)opts->lr * (double)T / (double)(g + 1));
        PLM_HIP(gibbs::expand(st, x, L, q, W));
        const int8_t *src = (ep == 0 && !opts->start) ? nullptr : ch[cur];
        PLM_HIP(gibbs::sweeps(plan, st, W, L, q, C, src, nullptr, allowed, 1.0f, opts->seed, (uint32_t)(g * K), K, ch[cur ^ 1]));
        cur ^= 1;
        hipLaunchKernelGGL(k_bm_transpose, dim3((unsigned)((Cp + 63) / 64), (unsigned)((L + 63) / 64)), dim3(256), 0, st,
                           ch[cur], C, L, Cp, xT);
        PLM_HIP(hipGetLastError());
        PLM_HIP(hipMemsetAsync(cnt, 0, n * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_bm_count, dim3((unsigned)n_jb, (unsigned)L, (unsigned)n_z), dim3(256),
                           (size_t)JB * q * q * sizeof(int32_t), st, (const uint32_t *)xT, L, q, n4, JB, per_z, cnt,
                           cnt + n_h);
        PLM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_bm_stats, dim3((unsigned)n_stat), dim3(256), 0, st, cnt, f, (int64_t)n, (int64_t)n_h, (float)C,
                           p, part);
        PLM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_bm_trace, dim3(1), dim3(256), 0, st, part, n_stat, (double)n_j, (double)lr_g,
                           trace + (size_t)4 * ep);
        PLM_HIP(hipGetLastError());
        rows = ep + 1;
        if (host_decides) {
            PLM_HIP(hipMemcpyAsync(row_host, trace + (size_t)4 * ep, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
            PLM_HIP(hipStreamSynchronize(st));
            if (opts->tol > 0.f && row_host[0] <= (double)opts->tol && row_host[1] <= (double)opts->tol) {
                status = PLM_STATUS_CONVERGED;
                break;
            }
            if (cb && cb((int32_t)g, row_host[0], row_host[1], row_host[2], row_host[3], user)) {
                status = PLM_STATUS_INTERRUPTED;
                break;
            }
        }
        if (lr_g != 0.f) {
            hipLaunchKernelGGL(k_bm_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, f, p, (int64_t)n,
                               (int64_t)n_h, lr_g, 2.f * opts->lambda_h, 2.f * opts->lambda_j);
            PLM_HIP(hipGetLastError());
        }
        done_epochs = ep + 1;
    }
    if (result->x_out) PLM_HIP(hipMemcpyAsync(result->x_out, x, n * sizeof(float), hipMemcpyDeviceToHost, st));
    if (result->pi_out) PLM_HIP(hipMemcpyAsync(result->pi_out, p, n_h * sizeof(float), hipMemcpyDeviceToHost, st));
    if (result->pij_out && n_j) PLM_HIP(hipMemcpyAsync(result->pij_out, p + n_h, n_j * sizeof(float), hipMemcpyDeviceToHost, st));
    if (result->chains_out) PLM_HIP(hipMemcpyAsync(result->chains_out, ch[cur], CL, hipMemcpyDeviceToHost, st));
    if (result->trace) PLM_HIP(hipMemcpyAsync(result->trace, trace, (size_t)4 * rows * sizeof(double), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    result->epochs_done = done_epochs;
    result->status = status;
    return PLM_OK;
}
