// plm_model.hip -- the numeric analysis the reference's CouplingsModel runs after a fit, on gfx950.
//
// Replaces three host loops of evcouplings/couplings/model.py:
//   zero-sum gauge (:180-233) + Frobenius norm and mutual information of every pair (:777-827)   -- k_model_pair_scores
//   double-mutant matrix of the target sequence (:715-742)                                        -- k_double_mutants
//   per-site fmin_bfgs of the independent-site model (:882-927)                                   -- k_independent_fields
// Everything is float64, like the model's arrays.  Pair blocks arrive compact: the i<j blocks of the dense
// [L][L][q][q] array in row-major pair order (plm_pair_index), uploaded as the L-1 contiguous row tails J[i, i+1:].
#include "plm_internal.h"
#include "plm_host_util.h"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

#define MA_Q 32                  // largest alphabet (one lane per state in a 64-lane wave)
#define MA_LD (MA_Q + 1)         // LDS row stride of a q x q block (odd: row and column walks hit distinct banks)
#define MA_NEWTON_CAP 100        // Newton steps per site before k_independent_fields gives up

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// pair number -> (i, j), i < j (row-major, the decode of k_mf_di)
__device__ __forceinline__ void pair_decode(int64_t p, int L, int *i_out, int *j_out) {
    int i = 0;
    while (p >= L - 1 - i) { p -= L - 1 - i; i++; }
    *i_out = i;
    *j_out = i + 1 + (int)p;
}

// One 64-lane wave per pair i<j.  J0 = J - rowmean - colmean + mean over all q states (gap included, model.py:180-233),
// fn = |J0|_F; mi = sum over f_ij(a,b) > 0 of p log(p / (f_i(a) f_j(b))) (model.py:795-799).  IEEE as numpy: p > 0 with
// f_i(a) f_j(b) = 0 gives log(inf) = inf, so the pair's MI is +inf.  fi_f32: the product rounded to float32 (the f_i
// values are float32 then, so the double product is exact and one rounding gives numpy's float32 outer product).
__global__ __launch_bounds__(64) void k_model_pair_scores(const double *__restrict__ Jp, const double *__restrict__ Fp,
                                                         const double *__restrict__ fi, int L, int q, int fi_f32,
                                                         double *__restrict__ fn, double *__restrict__ mi) {
    __shared__ double W[MA_Q * MA_LD];
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    int i, j;
    pair_decode(p, L, &i, &j);
    const int qq = q * q;
    const double *Jb = Jp + p * qq, *Fb = Fp + p * qq;
    // mutual information straight from global memory (contiguous lanes); the block goes to LDS for the gauge
    double acc_mi = 0.0;
    for (int k = lane; k < qq; k += 64) {
        const int a = k / q, b = k - a * q;
        W[a * MA_LD + b] = Jb[k];
        const double pab = Fb[k];
        if (pab > 0.0) {
            double m = fi[(size_t)i * q + a] * fi[(size_t)j * q + b];
            if (fi_f32) m = (double)(float)m;
            acc_mi += pab * log(pab / m);
        }
    }
    __syncthreads();
    // lane a < q: mean of row a and of column a
    __shared__ double ra[MA_Q], cb[MA_Q];
    double rs = 0.0, cs = 0.0;
    if (lane < q)
        for (int b = 0; b < q; b++) {
            rs += W[lane * MA_LD + b];
            cs += W[b * MA_LD + lane];
        }
    const double avg_ab = wave_sum(rs) / (double)qq;
    if (lane < q) {
        ra[lane] = rs / (double)q;
        cb[lane] = cs / (double)q;
    }
    __syncthreads();
    double acc_fn = 0.0;
    for (int k = lane; k < qq; k += 64) {
        const int a = k / q, b = k - a * q;
        const double v = W[a * MA_LD + b] - ra[a] - cb[b] + avg_ab;
        acc_fn += v * v;
    }
    acc_fn = wave_sum(acc_fn);
    acc_mi = wave_sum(acc_mi);
    if (lane == 0) {
        const double f = sqrt(acc_fn);
        fn[(size_t)i * L + j] = fn[(size_t)j * L + i] = f;
        mi[(size_t)i * L + j] = mi[(size_t)j * L + i] = acc_mi;
    }
}

// D[i,j,a,b] = smm[i,a] + smm[j,b] + J_ij[a,b] - J_ij[a,t_j] - J_ij[t_i,b] + J_ij[t_i,t_j]   (model.py:724-740, the
// reference's order of operations), D[j,i] = D[i,j]^T.  Blocks P .. P+L-1 of the grid zero the diagonal blocks.  The
// block is built in LDS so that both the block and its mirror leave with consecutive lanes on consecutive addresses.
__global__ __launch_bounds__(256) void k_double_mutants(const double *__restrict__ Jp, const double *__restrict__ smm,
                                                       const int8_t *__restrict__ target, int L, int q,
                                                       double *__restrict__ D) {
    __shared__ double W[MA_Q * MA_LD];
    const int qq = q * q;
    const int64_t n_pairs = (int64_t)L * (L - 1) / 2;
    const int64_t p = blockIdx.x;
    if (p >= n_pairs) {
        const int64_t d = p - n_pairs;
        double *out = D + (d * L + d) * qq;
        for (int k = threadIdx.x; k < qq; k += 256) out[k] = 0.0;
        return;
    }
    int i, j;
    pair_decode(p, L, &i, &j);
    const double *Jb = Jp + p * qq;
    const int ti = target[i], tj = target[j];
    const double jtt = Jb[ti * q + tj];
    for (int k = threadIdx.x; k < qq; k += 256) {
        const int a = k / q, b = k - a * q;
        W[a * MA_LD + b] = smm[(size_t)i * q + a] + smm[(size_t)j * q + b] + Jb[k] - Jb[a * q + tj] - Jb[ti * q + b] + jtt;
    }
    __syncthreads();
    double *out = D + ((int64_t)i * L + j) * qq, *mir = D + ((int64_t)j * L + i) * qq;
    for (int k = threadIdx.x; k < qq; k += 256) {
        const int a = k / q, b = k - a * q;
        out[k] = W[a * MA_LD + b];
        mir[k] = W[b * MA_LD + a];          // D[j,i](a, b) = D[i,j](b, a)
    }
}

// Independent-site model of one site per wave (lane a < q holds state a):
//   minimise F(x) = N (logZ(x) - f.x) + lambda |x|^2      (model.py:894-910)
// by damped Newton from x = 0.  H = N (diag P - P P^T) + 2 lambda I = D - N P P^T, D = diag(N P + 2 lambda), so
//   H^-1 g = D^-1 g + N D^-1 P (P^T D^-1 g) / (1 - N P^T D^-1 P)     (Sherman-Morrison; the denominator is > 0)
// Step length by Armijo backtracking on the f64 objective (max-shifted logsumexp); near the optimum, where the decrease
// drops below the rounding of F, a step that does not raise F beyond that rounding and shrinks |g|_inf is taken too.
// Converged when |g|_inf <= 1e-12 max(1, N).  iters[s] = Newton steps, or -1 if the cap was reached first.
__global__ __launch_bounds__(64) void k_independent_fields(const double *__restrict__ fi, int L, int q, double lambda,
                                                          double N, double *__restrict__ h, int32_t *__restrict__ iters) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool act = lane < q;
    const double f = act ? fi[(size_t)s * q + lane] : 0.0;
    const double tol = 1e-12 * fmax(1.0, N);
    // objective and (lane-held) probabilities at y
    auto eval = [&](double y, double *P) {
        const double m = wave_max(act ? y : -INFINITY);
        const double e = act ? exp(y - m) : 0.0;
        const double Z = wave_sum(e);
        *P = e / Z;
        const double lin = wave_sum(act ? f * y : 0.0), sq = wave_sum(act ? y * y : 0.0);
        return N * ((m + log(Z)) - lin) + lambda * sq;
    };
    double x = 0.0, P;
    double F = eval(x, &P);
    double g = act ? N * (P - f) + lambda * 2.0 * x : 0.0;
    double gmax = wave_max(fabs(g));
    int it = 0;
    bool ok = gmax <= tol;
    while (!ok && it < MA_NEWTON_CAP) {
        const double dinv = act ? 1.0 / (N * P + 2.0 * lambda) : 0.0;
        const double ptdg = wave_sum(P * dinv * g), ptdp = wave_sum(P * dinv * P);
        const double d = act ? -(dinv * g + N * dinv * P * ptdg / (1.0 - N * ptdp)) : 0.0;
        const double gd = wave_sum(g * d);
        if (!(gd < 0.0)) break;                       // not a descent direction: only rounding is left
        double t = 1.0, Pn = P, Fn = F, xn = x, gn = g, gnmax = gmax;
        bool taken = false;
        for (int ls = 0; ls < 60 && !taken; ls++, t *= 0.5) {
            xn = x + t * d;
            Fn = eval(xn, &Pn);
            gn = act ? N * (Pn - f) + lambda * 2.0 * xn : 0.0;
            gnmax = wave_max(fabs(gn));
            taken = Fn <= F + 1e-4 * t * gd ||
                    (Fn <= F + 8.0 * __DBL_EPSILON__ * fabs(F) && gnmax < gmax);
        }
        if (!taken) break;
        x = xn; P = Pn; F = Fn; g = gn; gmax = gnmax;
        it++;
        ok = gmax <= tol;
    }
    if (act) h[(size_t)s * q + lane] = x;
    if (lane == 0) iters[s] = ok ? it : -1;
}

// L-1 copies of the row tails J[i, i+1:] of a dense [L][L][q][q] host array into the compact pair buffer
int upload_pairs(const double *dense, int L, int q, double *dev, hipStream_t st) {
    const size_t qq = (size_t)q * q;
    size_t off = 0;
    for (int i = 0; i < L - 1; i++) {
        const size_t n = (size_t)(L - 1 - i) * qq;
        PLM_HIP(hipMemcpyAsync(dev + off, dense + ((size_t)i * L + i + 1) * qq, sizeof(double) * n, hipMemcpyHostToDevice, st));
        off += n;
    }
    return PLM_OK;
}

int check_shape(int L, int q) {
    if (L < 2) return plm_fail(PLM_EINVAL, "need at least 2 sites (got %d)", L);
    if (q < 2 || q > MA_Q) return plm_fail(PLM_EUNSUPPORTED, "model analysis supports 2..32 states (got %d)", q);
    return PLM_OK;
}

}  // namespace

int plm_model_pair_scores(const double *jij_full, const double *fij_full, const double *fi, int32_t n_sites,
                          int32_t n_states, int device, void *stream, double *fn_out, double *mi_out) {
    return plm_model_pair_scores_ex(jij_full, fij_full, fi, n_sites, n_states, 0, device, stream, fn_out, mi_out);
}

int plm_model_pair_scores_ex(const double *jij_full, const double *fij_full, const double *fi, int32_t n_sites,
                             int32_t n_states, int32_t flags, int device, void *stream, double *fn_out, double *mi_out) {
    if (flags & ~PLM_MODEL_FI_PRODUCT_F32) return plm_fail(PLM_EINVAL, "unknown flags 0x%x", flags);
    if (!jij_full || !fij_full || !fi || !fn_out || !mi_out) return plm_fail(PLM_EINVAL, "NULL argument");
    PLM_TRY(check_shape(n_sites, n_states));
    PLM_TRY(plm_check_device(device));
    const int L = n_sites, q = n_states;
    const size_t P = (size_t)L * (L - 1) / 2, qq = (size_t)q * q, LL = (size_t)L * L;
    PLM_TRY(plm_check_free(8.0 * (2.0 * P * qq + (double)L * q + 2.0 * LL), "pair scores"));
    hipStream_t st = (hipStream_t)stream;
    double *J = nullptr, *F = nullptr, *f = nullptr, *fn = nullptr, *mi = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&J, P * qq));
    PLM_TRY(mem.alloc(&F, P * qq));
    PLM_TRY(mem.alloc(&f, (size_t)L * q));
    PLM_TRY(mem.alloc(&fn, LL));
    PLM_TRY(mem.alloc(&mi, LL));
    PLM_TRY(upload_pairs(jij_full, L, q, J, st));
    PLM_TRY(upload_pairs(fij_full, L, q, F, st));
    PLM_HIP(hipMemcpyAsync(f, fi, sizeof(double) * L * q, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemsetAsync(fn, 0, sizeof(double) * LL, st));
    PLM_HIP(hipMemsetAsync(mi, 0, sizeof(double) * LL, st));
    hipLaunchKernelGGL(k_model_pair_scores, dim3((unsigned)P), dim3(64), 0, st, J, F, f, L, q, (flags & PLM_MODEL_FI_PRODUCT_F32) ? 1 : 0, fn, mi);
    PLM_HIP(hipGetLastError());
    PLM_HIP(hipMemcpyAsync(fn_out, fn, sizeof(double) * LL, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipMemcpyAsync(mi_out, mi, sizeof(double) * LL, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_double_mutants(const double *jij_full, const double *smm, const int8_t *target, int32_t n_sites,
                       int32_t n_states, int device, void *stream, double *dmm_out) {
    if (!jij_full || !smm || !target || !dmm_out) return plm_fail(PLM_EINVAL, "NULL argument");
    PLM_TRY(check_shape(n_sites, n_states));
    const int L = n_sites, q = n_states;
    for (int k = 0; k < L; k++)
        if (target[k] < 0 || target[k] >= q)
            return plm_fail(PLM_EINVAL, "target[%d] = %d outside 0..%d", k, (int)target[k], q - 1);
    PLM_TRY(plm_check_device(device));
    const size_t P = (size_t)L * (L - 1) / 2, qq = (size_t)q * q, LL = (size_t)L * L;
    PLM_TRY(plm_check_free(8.0 * ((double)P * qq + (double)LL * qq + (double)L * q) + L, "the double-mutant matrix"));
    hipStream_t st = (hipStream_t)stream;
    double *J = nullptr, *s = nullptr, *D = nullptr;
    int8_t *t = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&J, P * qq));
    PLM_TRY(mem.alloc(&s, (size_t)L * q));
    PLM_TRY(mem.alloc(&D, LL * qq));
    PLM_TRY(mem.alloc(&t, (size_t)L));
    PLM_TRY(upload_pairs(jij_full, L, q, J, st));
    PLM_HIP(hipMemcpyAsync(s, smm, sizeof(double) * L * q, hipMemcpyHostToDevice, st));
    PLM_HIP(hipMemcpyAsync(t, target, (size_t)L, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_double_mutants, dim3((unsigned)(P + L)), dim3(256), 0, st, J, s, t, L, q, D);
    PLM_HIP(hipGetLastError());
    PLM_HIP(hipMemcpyAsync(dmm_out, D, sizeof(double) * LL * qq, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}

int plm_independent_fields(const double *fi, int32_t n_sites, int32_t n_states, double lambda_h, double n_eff,
                           int device, void *stream, double *h_out, int32_t *iters_out) {
    if (!fi || !h_out || n_sites < 1) return plm_fail(PLM_EINVAL, "NULL argument or no sites");
    if (n_states < 2 || n_states > MA_Q)
        return plm_fail(PLM_EUNSUPPORTED, "independent fields support 2..32 states (got %d)", n_states);
    if (!(lambda_h > 0.0)) return plm_fail(PLM_EINVAL, "lambda_h must be > 0 (got %g): the optimum need not exist", lambda_h);
    if (!(n_eff >= 0.0) || !isfinite(n_eff)) return plm_fail(PLM_EINVAL, "N_eff must be finite and >= 0 (got %g)", n_eff);
    PLM_TRY(plm_check_device(device));
    const int L = n_sites, q = n_states;
    PLM_TRY(plm_check_free(8.0 * 2.0 * L * q + 4.0 * L, "independent fields"));
    hipStream_t st = (hipStream_t)stream;
    double *f = nullptr, *h = nullptr;
    int32_t *it = nullptr;
    DeviceBuffers mem;
    PLM_TRY(mem.alloc(&f, (size_t)L * q));
    PLM_TRY(mem.alloc(&h, (size_t)L * q));
    PLM_TRY(mem.alloc(&it, (size_t)L));
    PLM_HIP(hipMemcpyAsync(f, fi, sizeof(double) * L * q, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_independent_fields, dim3(L), dim3(64), 0, st, f, L, q, lambda_h, n_eff, h, it);
    PLM_HIP(hipGetLastError());
    std::vector<int32_t> own(iters_out ? 0 : L);
    int32_t *iters = iters_out ? iters_out : own.data();
    PLM_HIP(hipMemcpyAsync(h_out, h, sizeof(double) * L * q, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipMemcpyAsync(iters, it, sizeof(int32_t) * L, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < L; k++)
        if (iters[k] < 0)
            return plm_fail(PLM_ENUMERIC, "independent-site Newton solve of site %d did not reach |g| <= 1e-12 max(1, N_eff) "
                                          "in %d steps", k, MA_NEWTON_CAP);
    return PLM_OK;
}
