// plm_pca.hip -- principal components of an alignment's centred one-hot features and projections on them (plm_pca_fit,
// plm_pca_fit_cb, plm_pca_project); contract in include/plm_hip.h, notes in DESIGN_NEXT_ROWS.md section 9.20.
//
// The covariance C is never formed.  Features are addressed as d = i q + a over ALL states (Df = L q rows); the rows of
// the skipped state are kept at zero in every block, so the arithmetic is that of the D kept features.  Device image:
// column-major, one column of Np bytes per site (Np = N rounded up to 16, as in plm_triplets.hip) and the fixed-point
// weights wq [Np] u32 beside it.  One product Y = C V of a block V [Df][b]:
//   k_pca_meanproj  m[c] = sum_i (sum_a f_i(a) V[(i,a)][c])                  ascending a, then ascending i
//   k_pca_phiv      U[n][c] = (sum_i V[(i, x_ni)][c]) - m[c]                 ascending i
//   k_pca_slices    P[i][s][a][c] = sum_{n in slice s, x_ni = a} wq_n U[n][c]  ascending n, compensated (Kahan); a slice
//                   is PC_SLICE sequences
//   k_pca_combine   T = sum_s P (ascending s, compensated), S[c] = sum_a T[a][c] (ascending a),
//                   Y[(i,a)][c] = (T - f_i(a) S[c]) / W
// and the b x b products V^T Y, V^T V, Y^T Y over chunks of PC_ROWS rows (ascending rows in a chunk, then ascending
// chunks).  Every sum has one order, fixed by constants of this file: the launch plan (PLM_PCA_PLAN) only decides which
// workgroup computes which slice, sequence or chunk, so no output bit depends on it.  No float64 operation is contracted.
#include "plm_host_util.h"
#include "plm_gibbs_device.h"
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>

typedef uint32_t u32;
typedef unsigned long long u64;

namespace {

constexpr int PC_BLK = 256;                 // threads per workgroup, every kernel of this file
constexpr int PC_WAVES = PC_BLK / 64;
constexpr int PC_MAXB = 64;                 // columns of a block at most
constexpr int PC_SLICE = 256;               // sequences of one serial sum of k_pca_slices
constexpr int PC_ROWS = 32;                 // feature rows of one serial sum of the b x b products
constexpr int PC_MAX_GRID = 65535;
constexpr int PC_FILL_TRIES = 8;

// uniform in (-1, 1), never 0: the start block (tag 0) and the fill-in directions beyond the rank (tag 1 + attempt)
__device__ __forceinline__ double pca_draw(u32 feature, u32 column, u32 tag, u32 seed_lo, u32 seed_hi) {
    const u32 w = philox_word0(feature, column, tag, 0x50434131u, seed_lo, seed_hi);
    return ((double)w + 0.5) * 4.656612873077392578125e-10 - 1.0;
}

// The sum of x over the workgroup, the same value in every thread: the lanes of a wave, then the waves, one fixed order.
__device__ __forceinline__ double block_sum(double x, double *red) {
    for (int h = 32; h > 0; h >>= 1) x = x + __shfl_down(x, h);
    __syncthreads();                                   // red may still be read by the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < PC_WAVES; w++) s = s + red[w];
    return s;
}

__global__ __launch_bounds__(PC_BLK) void k_pca_init(double *__restrict__ V, int Df, int b, int q, int skip, u32 seed_lo,
                                                    u32 seed_hi) {
    const long long idx = (long long)blockIdx.x * PC_BLK + threadIdx.x;
    if (idx >= (long long)Df * b) return;
    const int d = (int)(idx / b), c = (int)(idx - (long long)d * b);
    V[idx] = (d % q) == skip ? 0.0 : pca_draw((u32)d, (u32)c, 0u, seed_lo, seed_hi);
}

// m[c] = sum_{i,a} f_i(a) V[(i,a)][c]: one workgroup; P [L][b] is scratch in global memory.
__global__ __launch_bounds__(PC_BLK) void k_pca_meanproj(const double *__restrict__ f, const double *__restrict__ V, int L,
                                                        int q, int b, double *__restrict__ P, double *__restrict__ m) {
#pragma clang fp contract(off)
    for (int idx = threadIdx.x; idx < L * b; idx += PC_BLK) {
        const int i = idx / b, c = idx - i * b;
        double p = 0.0;
        for (int a = 0; a < q; a++) p = p + f[i * q + a] * V[(size_t)(i * q + a) * b + c];
        P[idx] = p;
    }
    __threadfence_block();
    __syncthreads();
    if ((int)threadIdx.x < b) {
        double s = 0.0;
        for (int i = 0; i < L; i++) s = s + P[i * b + threadIdx.x];
        m[threadIdx.x] = s;
    }
}

// U = Phi V.  A thread owns (sequence, column): bp = b rounded up to a power of two lanes per sequence, PC_BLK / bp
// sequences in flight per workgroup, which walks the sequences blockIdx.x spw .. + spw - 1.
__global__ __launch_bounds__(PC_BLK) void k_pca_phiv(const int8_t *__restrict__ img, size_t Np, int N, int L, int q,
                                                    const double *__restrict__ V, int b, int bp,
                                                    const double *__restrict__ m, double *__restrict__ U, int spw) {
    const int gpb = PC_BLK / bp, g = threadIdx.x / bp, c = threadIdx.x - g * bp;
    const long long n0 = (long long)blockIdx.x * spw, n1 = min((long long)N, n0 + spw);
    if (c >= b) return;
    const double mc = m[c];
    for (long long n = n0 + g; n < n1; n += gpb) {
        double acc = 0.0;
        for (int i = 0; i < L; i++) {
            const int a = img[(size_t)i * Np + n];
            acc = acc + V[((size_t)i * q + a) * b + c];
        }
        U[(size_t)n * b + c] = acc - mc;
    }
}

// The slice sums of Phi^T diag(wq) U: workgroup (w, i) takes the slices w spw .. + spw - 1 of site i, one lane group of
// bp lanes per slice at a time.  A thread owns the accumulators [q] of its column in LDS, each with the compensation
// term of Kahan's summation (acc [gpb][2][q][bp]): the error of a slice sum does not grow with the slice.  The state of a
// sequence is uniform over the group.  partial [L][ns][q][b].
__global__ __launch_bounds__(PC_BLK) void k_pca_slices(const int8_t *__restrict__ img, size_t Np, const u32 *__restrict__ wq,
                                                      int N, int q, const double *__restrict__ U, int b, int bp,
                                                      double *__restrict__ partial, int ns, int spw) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int gpb = PC_BLK / bp, g = threadIdx.x / bp, c = threadIdx.x - g * bp;
    const int i = blockIdx.y;
    const int s0 = blockIdx.x * spw, s1 = min(ns, s0 + spw);
    double *mine = (double *)smem + (size_t)g * 2 * q * bp, *comp = mine + q * bp;
    const int8_t *col = img + (size_t)i * Np;
    if (c >= b) return;
    for (int s = s0 + g; s < s1; s += gpb) {
        for (int a = 0; a < q; a++) mine[a * bp + c] = comp[a * bp + c] = 0.0;
        const int n0 = s * PC_SLICE, n1 = min(N, n0 + PC_SLICE);
        for (int n = n0; n < n1; n++) {
            const int a = col[n];
            const double t = (double)wq[n] * U[(size_t)n * b + c];
            const double sum = mine[a * bp + c], y = t - comp[a * bp + c];
            const double next = sum + y;
            comp[a * bp + c] = (next - sum) - y;
            mine[a * bp + c] = next;
        }
        double *dst = partial + ((size_t)i * ns + s) * q * b;
        for (int a = 0; a < q; a++) dst[a * b + c] = mine[a * bp + c];
    }
}

// One workgroup per site: the slices in ascending order, the centring term, the division by W.  LDS: (q + 1) b doubles.
__global__ __launch_bounds__(PC_BLK) void k_pca_combine(const double *__restrict__ partial, int ns, const double *__restrict__ f,
                                                       double W, int q, int b, int skip, double *__restrict__ Y) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *T = (double *)smem, *S = T + q * b;
    const int i = blockIdx.x;
    const double *src = partial + (size_t)i * ns * q * b;
    for (int p = threadIdx.x; p < q * b; p += PC_BLK) {
        double t = 0.0, comp = 0.0;                       // Kahan again: ns grows with the alignment
        for (int s = 0; s < ns; s++) {
            const double y = src[(size_t)s * q * b + p] - comp;
            const double next = t + y;
            comp = (next - t) - y;
            t = next;
        }
        T[p] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < b) {
        double s = 0.0;
        for (int a = 0; a < q; a++) s = s + T[a * b + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < q * b; p += PC_BLK) {
        const int a = p / b, c = p - a * b;
        const double fs = f[i * q + a] * S[c];
        Y[((size_t)i * q + a) * b + c] = a == skip ? 0.0 : (T[p] - fs) / W;
    }
}

// V^T Y, V^T V and Y^T Y of the rows of one chunk: gpart [n_chunks][3][b b].  A workgroup takes cpw chunks.
__global__ __launch_bounds__(PC_BLK) void k_pca_gram(const double *__restrict__ V, const double *__restrict__ Y, int Df, int b,
                                                    int n_chunks, int cpw, double *__restrict__ gpart) {
#pragma clang fp contract(off)
    __shared__ double sv[PC_ROWS * PC_MAXB], sy[PC_ROWS * PC_MAXB];
    const int c0 = blockIdx.x * cpw, c1 = min(n_chunks, c0 + cpw), bb = b * b;
    for (int ch = c0; ch < c1; ch++) {
        const int d0 = ch * PC_ROWS, nr = min(PC_ROWS, Df - d0);
        __syncthreads();
        for (int p = threadIdx.x; p < nr * b; p += PC_BLK) {
            sv[p] = V[(size_t)d0 * b + p];
            sy[p] = Y[(size_t)d0 * b + p];
        }
        __syncthreads();
        for (int p = threadIdx.x; p < bb; p += PC_BLK) {
            const int r = p / b, c = p - r * b;
            double vy = 0.0, vv = 0.0, yy = 0.0;
            for (int row = 0; row < nr; row++) {
                const double vr = sv[row * b + r], vc = sv[row * b + c], yr = sy[row * b + r], yc = sy[row * b + c];
                vy = vy + vr * yc;
                vv = vv + vr * vc;
                yy = yy + yr * yc;
            }
            double *dst = gpart + (size_t)ch * 3 * bb;
            dst[p] = vy;
            dst[bb + p] = vv;
            dst[2 * bb + p] = yy;
        }
    }
}

// out[e] = sum over the chunks (ascending) of part[chunk][e], e < n
__global__ __launch_bounds__(PC_BLK) void k_pca_chunk_sum(const double *__restrict__ part, int n_chunks, int n,
                                                         double *__restrict__ out) {
    const int e = blockIdx.x * PC_BLK + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int ch = 0; ch < n_chunks; ch++) s = s + part[(size_t)ch * n + e];
    out[e] = s;
}

// Rayleigh-Ritz rotation of the rows of a chunk: X = V Q (the Ritz vectors), Z = Y Q (= C X), the squared residual
// entries (Z - X diag(theta))^2 summed over the rows of the chunk into rpart [n_chunks][b], and the next block
// V <- Y T2 in place.  Q, T2 [b][b] row-major, theta [b].
__global__ __launch_bounds__(PC_BLK) void k_pca_rotate(double *__restrict__ V, const double *__restrict__ Y,
                                                      double *__restrict__ X, const double *__restrict__ Q,
                                                      const double *__restrict__ T2, const double *__restrict__ theta, int Df,
                                                      int b, int n_chunks, int cpw, double *__restrict__ rpart) {
#pragma clang fp contract(off)
    __shared__ double sv[PC_ROWS * PC_MAXB], sy[PC_ROWS * PC_MAXB], se[PC_ROWS * PC_MAXB];
    const int c0 = blockIdx.x * cpw, c1 = min(n_chunks, c0 + cpw);
    for (int ch = c0; ch < c1; ch++) {
        const int d0 = ch * PC_ROWS, nr = min(PC_ROWS, Df - d0);
        __syncthreads();
        for (int p = threadIdx.x; p < nr * b; p += PC_BLK) {
            sv[p] = V[(size_t)d0 * b + p];
            sy[p] = Y[(size_t)d0 * b + p];
        }
        __syncthreads();
        for (int p = threadIdx.x; p < nr * b; p += PC_BLK) {
            const int row = p / b, c = p - row * b;
            double x = 0.0, z = 0.0, vn = 0.0;
            for (int j = 0; j < b; j++) {
                const double qj = Q[j * b + c], vj = sv[row * b + j], yj = sy[row * b + j];
                x = x + vj * qj;
                z = z + yj * qj;
                vn = vn + yj * T2[j * b + c];
            }
            const double tx = theta[c] * x;
            const double e = z - tx;
            se[p] = e * e;
            X[(size_t)d0 * b + p] = x;
            V[(size_t)d0 * b + p] = vn;
        }
        __syncthreads();
        if ((int)threadIdx.x < b) {
            double s = 0.0;
            for (int row = 0; row < nr; row++) s = s + se[row * b + threadIdx.x];
            rpart[(size_t)ch * b + threadIdx.x] = s;
        }
    }
}

// The first k Ritz vectors X[:, 0..k-1] (X [Df][b]) made orthonormal to rounding by modified Gram-Schmidt, twice, in
// one workgroup.  A column that is no unit vector (a dropped direction: zero) is drawn anew, orthogonalised against the
// columns before it and flagged in filled[c].  Then the sign rule.  F [Df][k] for the products, comp [k][Df] for the
// caller.  A thread reads and writes only the rows d = tid, tid + PC_BLK, ...: block_sum is the only exchange.
__global__ __launch_bounds__(PC_BLK) void k_pca_orth(const double *__restrict__ X, int b, double *__restrict__ F, int Df, int k,
                                                    int q, int skip, u32 seed_lo, u32 seed_hi, double *__restrict__ comp,
                                                    int32_t *__restrict__ filled) {
#pragma clang fp contract(off)
    __shared__ double red[PC_WAVES], red_m[PC_WAVES], red_v[PC_WAVES];
    __shared__ int red_i[PC_WAVES];
    const int tid = threadIdx.x;
    for (int c = 0; c < k; c++) {
        double s = 0.0;
        for (int d = tid; d < Df; d += PC_BLK) {
            const double x = X[(size_t)d * b + c];
            F[(size_t)d * k + c] = x;
            s = s + x * x;
        }
        double before = block_sum(s, red), after = 0.0;
        int fill = 0;
        for (int attempt = 0; attempt <= PC_FILL_TRIES; attempt++) {
            if (attempt > 0 || !(before > 0.25)) {
                fill = 1;
                s = 0.0;
                for (int d = tid; d < Df; d += PC_BLK) {
                    const double x = (d % q) == skip ? 0.0 : pca_draw((u32)d, (u32)c, 1u + (u32)attempt, seed_lo, seed_hi);
                    F[(size_t)d * k + c] = x;
                    s = s + x * x;
                }
                before = block_sum(s, red);
            }
            for (int pass = 0; pass < 2; pass++)
                for (int j = 0; j < c; j++) {
                    s = 0.0;
                    for (int d = tid; d < Df; d += PC_BLK) s = s + F[(size_t)d * k + j] * F[(size_t)d * k + c];
                    const double dot = block_sum(s, red);
                    for (int d = tid; d < Df; d += PC_BLK) {
                        const double t = dot * F[(size_t)d * k + j];
                        F[(size_t)d * k + c] = F[(size_t)d * k + c] - t;
                    }
                }
            s = 0.0;
            for (int d = tid; d < Df; d += PC_BLK) s = s + F[(size_t)d * k + c] * F[(size_t)d * k + c];
            after = block_sum(s, red);
            if (after > 1e-6 * before) break;          // else: the draw lay in the span of the columns before it
        }
        const double nrm = sqrt(after);
        double mx = -1.0, sv = 0.0;
        int mi = Df;
        for (int d = tid; d < Df; d += PC_BLK) {
            const double x = after > 0.0 ? F[(size_t)d * k + c] / nrm : 0.0;
            F[(size_t)d * k + c] = x;
            if (fabs(x) > mx) { mx = fabs(x); mi = d; sv = x; }
        }
        for (int h = 32; h > 0; h >>= 1) {              // the largest magnitude, the smallest index of a tie
            const double om = __shfl_down(mx, h), ov = __shfl_down(sv, h);
            const int oi = __shfl_down(mi, h);
            if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; sv = ov; }
        }
        __syncthreads();
        if ((tid & 63) == 0) { red_m[tid >> 6] = mx; red_i[tid >> 6] = mi; red_v[tid >> 6] = sv; }
        __syncthreads();
        mx = red_m[0]; mi = red_i[0]; sv = red_v[0];
        for (int w = 1; w < PC_WAVES; w++)
            if (red_m[w] > mx || (red_m[w] == mx && red_i[w] < mi)) { mx = red_m[w]; mi = red_i[w]; sv = red_v[w]; }
        const bool flip = sv < 0.0;
        for (int d = tid; d < Df; d += PC_BLK) {
            double x = F[(size_t)d * k + c];
            if (flip) x = -x;
            F[(size_t)d * k + c] = x;
            comp[(size_t)c * Df + d] = x;
        }
        if (tid == 0) filled[c] = fill;
    }
}

// lambda_c = (f_c . y_c) / (f_c . f_c), the Rayleigh quotient with the rounding of the normalisation taken out, and
// |y_c - lambda_c f_c| of the final vectors F with Y = C F, both [Df][k]: one workgroup.
__global__ __launch_bounds__(PC_BLK) void k_pca_final(const double *__restrict__ F, const double *__restrict__ Y, int Df, int k,
                                                     double *__restrict__ lam, double *__restrict__ res) {
#pragma clang fp contract(off)
    __shared__ double red[PC_WAVES];
    for (int c = 0; c < k; c++) {
        double s = 0.0, n = 0.0;
        for (int d = threadIdx.x; d < Df; d += PC_BLK) {
            s = s + F[(size_t)d * k + c] * Y[(size_t)d * k + c];
            n = n + F[(size_t)d * k + c] * F[(size_t)d * k + c];
        }
        const double fy = block_sum(s, red), ff = block_sum(n, red);
        const double l = fy / ff;
        s = 0.0;
        for (int d = threadIdx.x; d < Df; d += PC_BLK) {
            const double t = l * F[(size_t)d * k + c];
            const double e = Y[(size_t)d * k + c] - t;
            s = s + e * e;
        }
        const double r2 = block_sum(s, red);
        if (threadIdx.x == 0) { lam[c] = l; res[c] = sqrt(r2); }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------

// PLM_PCA_PLAN: comma-separated tokens that force the launch plan (measurements and tests): g<int> workgroups per site
// of k_pca_slices, s<int> sequences per workgroup of k_pca_phiv, r<int> row chunks per workgroup of k_pca_gram and
// k_pca_rotate.  0 = not forced.
struct PcaPlan { int g, s, r; };

int pca_forced_plan(PcaPlan *p) {
    *p = PcaPlan{0, 0, 0};
    const char *v = getenv("PLM_PCA_PLAN");
    if (!v) return PLM_OK;
    const char *s = v;
    bool ok = *s != 0;
    while (ok && *s) {
        const char key = *s++;
        if (key == 'g' || key == 's' || key == 'r') {
            char *end = nullptr;
            errno = 0;
            const long x = (*s >= '0' && *s <= '9') ? strtol(s, &end, 10) : -1;
            if (errno || x < 1 || x > INT_MAX) { ok = false; break; }
            s = end;
            if (key == 'g') { ok = x <= PC_MAX_GRID; p->g = (int)x; }
            else if (key == 's') { ok = x <= (1 << 20); p->s = (int)x; }
            else { ok = x <= PC_MAX_GRID; p->r = (int)x; }
        } else {
            ok = false;
        }
        if (ok && *s) { ok = *s == ',' && s[1] != 0; s++; }
    }
    if (!ok)
        return plm_fail(PLM_EINVAL, "PLM_PCA_PLAN must be a comma-separated list of g<int 1..65535>, s<int 1..1048576>, "
                                    "r<int 1..65535> (got '%s')", v);
    return PLM_OK;
}

int pca_check_shape(int N, int L, int q, const char *rows) {
    if (N < 1) return plm_fail(PLM_EINVAL, "%s must be at least 1 (got %d)", rows, N);
    if (L < 1) return plm_fail(PLM_EINVAL, "n_sites must be at least 1 (got %d)", L);
    if (L > PC_MAX_GRID) return plm_fail(PLM_EINVAL, "n_sites %d is above %d", L, PC_MAX_GRID);
    if (q < 2 || q > 32) return plm_fail(PLM_EINVAL, "n_states %d outside 2..32", q);
    if ((long long)N + 16 > INT_MAX) return plm_fail(PLM_EINVAL, "%s %d is too large", rows, N);
    return PLM_OK;
}

// the column-major byte image of the rows, every state checked
int pca_columns(const int8_t *msa, int N, int L, int q, const char *name, size_t Np, std::vector<int8_t> *cols) {
    for (int n = 0; n < N; n++)
        for (int i = 0; i < L; i++) {
            const int8_t v = msa[(size_t)n * L + i];
            if (v < 0 || v >= q) return plm_fail(PLM_EINVAL, "%s[%d][%d] = %d outside 0..%d", name, n, i, (int)v, q - 1);
        }
    cols->assign((size_t)L * Np, (int8_t)0);
    for (int n = 0; n < N; n++)
        for (int i = 0; i < L; i++) (*cols)[(size_t)i * Np + n] = msa[(size_t)n * L + i];
    return PLM_OK;
}

// Cyclic Jacobi for a symmetric n x n matrix (row-major; destroyed): eigenvalues w, eigenvectors in the columns of E.
void jacobi_eig(int n, std::vector<double> &A, std::vector<double> &E, std::vector<double> &w) {
    E.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) E[(size_t)i * n + i] = 1.0;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) A[(size_t)i * n + j] = A[(size_t)j * n + i] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; i++) {
            diag += A[(size_t)i * n + i] * A[(size_t)i * n + i];
            for (int j = i + 1; j < n; j++) off += A[(size_t)i * n + j] * A[(size_t)i * n + j];
        }
        if (off == 0.0 || off <= 1e-34 * diag) break;
        for (int p = 0; p < n; p++)
            for (int r = p + 1; r < n; r++) {
                const double apr = A[(size_t)p * n + r];
                if (apr == 0.0) continue;
                const double app = A[(size_t)p * n + p], arr = A[(size_t)r * n + r];
                const double tau = (arr - app) / (2.0 * apr);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                for (int x = 0; x < n; x++) {         // columns p and r
                    const double xp = A[(size_t)x * n + p], xr = A[(size_t)x * n + r];
                    A[(size_t)x * n + p] = c * xp - s * xr;
                    A[(size_t)x * n + r] = s * xp + c * xr;
                }
                for (int x = 0; x < n; x++) {         // rows p and r
                    const double px = A[(size_t)p * n + x], rx = A[(size_t)r * n + x];
                    A[(size_t)p * n + x] = c * px - s * rx;
                    A[(size_t)r * n + x] = s * px + c * rx;
                }
                A[(size_t)p * n + r] = A[(size_t)r * n + p] = 0.0;
                for (int x = 0; x < n; x++) {
                    const double xp = E[(size_t)x * n + p], xr = E[(size_t)x * n + r];
                    E[(size_t)x * n + p] = c * xp - s * xr;
                    E[(size_t)x * n + r] = s * xp + c * xr;
                }
            }
    }
    w.resize(n);
    for (int i = 0; i < n; i++) w[i] = A[(size_t)i * n + i];
}

// eigenvalues descending, the columns of E with them (stable)
void sort_descending(int n, std::vector<double> &E, std::vector<double> &w) {
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return w[x] > w[y]; });
    std::vector<double> E2((size_t)n * n), w2(n);
    for (int c = 0; c < n; c++) {
        w2[c] = w[order[c]];
        for (int r = 0; r < n; r++) E2[(size_t)r * n + c] = E[(size_t)r * n + order[c]];
    }
    E.swap(E2);
    w.swap(w2);
}

// M = X^T A X for n x n row-major matrices
std::vector<double> congruence(int n, const std::vector<double> &X, const std::vector<double> &A) {
    std::vector<double> AX((size_t)n * n, 0.0), M((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            double s = 0.0;
            for (int l = 0; l < n; l++) s += A[(size_t)i * n + l] * X[(size_t)l * n + j];
            AX[(size_t)i * n + j] = s;
        }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            double s = 0.0;
            for (int l = 0; l < n; l++) s += X[(size_t)l * n + i] * AX[(size_t)l * n + j];
            M[(size_t)i * n + j] = s;
        }
    return M;
}

// X P diag(sig)^-1/2 with the columns whose sig is not above floor * max(sig) set to zero (the dropped directions)
std::vector<double> whiten(int n, const std::vector<double> &X, const std::vector<double> &P, const std::vector<double> &sig,
                           double floor) {
    double smax = 0.0;
    for (int j = 0; j < n; j++) smax = std::max(smax, sig[j]);
    std::vector<double> T((size_t)n * n, 0.0);
    for (int j = 0; j < n; j++) {
        if (!(sig[j] > floor * smax) || !(sig[j] > 0.0)) continue;
        const double inv = 1.0 / sqrt(sig[j]);
        for (int i = 0; i < n; i++) {
            double s = 0.0;
            for (int l = 0; l < n; l++) s += X[(size_t)i * n + l] * P[(size_t)l * n + j];
            T[(size_t)i * n + j] = s * inv;
        }
    }
    return T;
}

struct PcaDevice {
    int N, L, q, Df, ns, skip;
    size_t Np;
    double W;
    int8_t *img = nullptr;
    u32 *wq = nullptr;
    double *f = nullptr, *P = nullptr, *m = nullptr, *U = nullptr, *partial = nullptr;
};

int pca_bp(int b) { int bp = 1; while (bp < b) bp *= 2; return bp; }

// m and U = Phi V for a block V [Df][b]
int pca_project_block(const PcaDevice &d, const PcaPlan &plan, const double *V, int b, hipStream_t st) {
    const int bp = pca_bp(b), gpb = PC_BLK / bp;
    const int spw = plan.s ? plan.s : gpb;
    hipLaunchKernelGGL(k_pca_meanproj, dim3(1), dim3(PC_BLK), 0, st, (const double *)d.f, V, d.L, d.q, b, d.P, d.m);
    PLM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pca_phiv, dim3((unsigned)((d.N + spw - 1) / spw)), dim3(PC_BLK), 0, st, (const int8_t *)d.img, d.Np, d.N,
                       d.L, d.q, V, b, bp, (const double *)d.m, d.U, spw);
    PLM_HIP(hipGetLastError());
    return PLM_OK;
}

// Y = C V for a block V [Df][b] (U is left holding Phi V)
int pca_product(const PcaDevice &d, const PcaPlan &plan, const double *V, int b, double *Y, hipStream_t st) {
    PLM_TRY(pca_project_block(d, plan, V, b, st));
    const int bp = pca_bp(b), gpb = PC_BLK / bp;
    int spw = gpb;
    if (plan.g) spw = (d.ns + std::min(plan.g, d.ns) - 1) / std::min(plan.g, d.ns);
    const int G = (d.ns + spw - 1) / spw;
    const size_t lds = sizeof(double) * 2 * (size_t)gpb * d.q * bp;          // 4096 q bytes: 128 KB at q = 32
    if (lds > 65536)
        PLM_HIP(hipFuncSetAttribute((const void *)k_pca_slices, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_pca_slices, dim3(G, d.L), dim3(PC_BLK), lds, st,
                       (const int8_t *)d.img, d.Np, (const u32 *)d.wq, d.N, d.q, (const double *)d.U, b, bp, d.partial, d.ns, spw);
    PLM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pca_combine, dim3(d.L), dim3(PC_BLK), sizeof(double) * (size_t)(d.q + 1) * b, st,
                       (const double *)d.partial, d.ns, (const double *)d.f, d.W, d.q, b, d.skip, Y);
    PLM_HIP(hipGetLastError());
    return PLM_OK;
}

int pca_upload_image(PcaDevice *d, DeviceBuffers &mem, const std::vector<int8_t> &cols, const std::vector<u32> *wq,
                     const double *f, int b, bool products, hipStream_t st) {
    PLM_TRY(mem.alloc(&d->img, cols.size()));
    PLM_HIP(hipMemcpyAsync(d->img, cols.data(), cols.size(), hipMemcpyHostToDevice, st));
    if (wq) {
        PLM_TRY(mem.alloc(&d->wq, wq->size()));
        PLM_HIP(hipMemcpyAsync(d->wq, wq->data(), sizeof(u32) * wq->size(), hipMemcpyHostToDevice, st));
    }
    PLM_TRY(mem.alloc(&d->f, (size_t)d->Df));
    PLM_HIP(hipMemcpyAsync(d->f, f, sizeof(double) * d->Df, hipMemcpyHostToDevice, st));
    PLM_TRY(mem.alloc(&d->P, (size_t)d->L * b));
    PLM_TRY(mem.alloc(&d->m, (size_t)b));
    PLM_TRY(mem.alloc(&d->U, (size_t)d->N * b));
    if (products) PLM_TRY(mem.alloc(&d->partial, (size_t)d->L * d->ns * d->q * b));
    return PLM_OK;
}

}  // namespace

int plm_pca_fit_cb(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                   const plm_pca_opts *opts, double *mean, double *components, double *eigenvalues, double *residuals,
                   double *total_variance, uint64_t *total, int32_t *iterations, int32_t *converged, double *scores,
                   int device, void *stream, plm_pca_cb cb, void *user, int32_t *status) {
    const int N = n_seqs, L = n_sites, q = n_states;
    PLM_TRY(pca_check_shape(N, L, q, "n_seqs"));
    if (!msa || !opts) return plm_fail(PLM_EINVAL, "NULL msa or opts");
    if (!mean || !components || !eigenvalues || !residuals)
        return plm_fail(PLM_EINVAL, "NULL mean, components, eigenvalues or residuals");
    const int skip = opts->skip_state, k = opts->n_components;
    if (skip < -1 || skip >= q) return plm_fail(PLM_EINVAL, "skip_state %d outside -1..%d", skip, q - 1);
    const long long D = (long long)L * (skip >= 0 ? q - 1 : q);
    if (k < 1 || k > D) return plm_fail(PLM_EINVAL, "n_components %d outside 1..%lld (the number of features)", k, D);
    if (k > PC_MAXB) return plm_fail(PLM_EINVAL, "n_components %d is above %d", k, PC_MAXB);
    if (opts->oversample < 0) return plm_fail(PLM_EINVAL, "oversample %d is negative", opts->oversample);
    if (opts->max_iter < 1) return plm_fail(PLM_EINVAL, "max_iter must be at least 1 (got %d)", opts->max_iter);
    if (!(opts->tol > 0.0) || !std::isfinite(opts->tol)) return plm_fail(PLM_EINVAL, "tol must be positive (got %g)", opts->tol);
    const size_t Np = ((size_t)N + 15) / 16 * 16;
    std::vector<u32> wq;
    uint64_t Wi = 0;
    PLM_TRY(plm_quantise_weights(weights, N, Np, &wq, &Wi));
    if (wq.empty()) { wq.assign(Np, 0u); std::fill(wq.begin(), wq.begin() + N, 1u); }
    std::vector<int8_t> cols;
    PLM_TRY(pca_columns(msa, N, L, q, "msa", Np, &cols));
    PcaPlan plan;
    PLM_TRY(pca_forced_plan(&plan));

    // frequencies and the total variance from exact integer counts
    const int Df = L * q;
    const double W = (double)Wi;
    std::vector<uint64_t> cnt((size_t)Df, 0);
    for (int i = 0; i < L; i++)
        for (int n = 0; n < N; n++) cnt[(size_t)i * q + cols[(size_t)i * Np + n]] += wq[n];
    std::vector<double> f((size_t)Df);
    double tv = 0.0;
    for (int d = 0; d < Df; d++) {
        f[d] = (double)cnt[d] / W;
        if (d % q != skip) tv += f[d] * (1.0 - f[d]);
    }

    const int b = (int)std::min<long long>(std::min<long long>((long long)k + opts->oversample, D), PC_MAXB);
    const int ns = (N + PC_SLICE - 1) / PC_SLICE, n_chunks = (Df + PC_ROWS - 1) / PC_ROWS, bb = b * b;
    const double gram_floor = (double)D * 5.6843418860808015e-14;        // D 2^-44, relative to the largest Gram eigenvalue

    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    PLM_TRY(plm_check_free((double)cols.size() + 4.0 * Np + 8.0 * ((double)Df * (1 + 4.0 * b) + (double)L * b + (double)N * b +
                           (double)L * ns * q * b + (double)n_chunks * (3.0 * bb + b) + 8.0 * bb), "plm_pca_fit"));
    DeviceBuffers mem;
    PcaDevice d;
    d.N = N; d.L = L; d.q = q; d.Df = Df; d.ns = ns; d.skip = skip; d.Np = Np; d.W = W;
    PLM_TRY(pca_upload_image(&d, mem, cols, &wq, f.data(), b, true, st));
    double *V = nullptr, *Y = nullptr, *X = nullptr, *F = nullptr, *gpart = nullptr, *rpart = nullptr, *small = nullptr;
    double *rot = nullptr, *dcomp = nullptr, *dlam = nullptr;
    int32_t *dfilled = nullptr;
    PLM_TRY(mem.alloc(&V, (size_t)Df * b));
    PLM_TRY(mem.alloc(&Y, (size_t)Df * b));
    PLM_TRY(mem.alloc(&X, (size_t)Df * b));
    PLM_TRY(mem.alloc(&F, (size_t)Df * k));
    PLM_TRY(mem.alloc(&gpart, (size_t)n_chunks * 3 * bb));
    PLM_TRY(mem.alloc(&rpart, (size_t)n_chunks * b));
    PLM_TRY(mem.alloc(&small, (size_t)3 * bb + b));            // V^T Y, V^T V, Y^T Y, squared residuals
    PLM_TRY(mem.alloc(&rot, (size_t)2 * bb + b));              // Q, T2, theta
    PLM_TRY(mem.alloc(&dcomp, (size_t)k * Df));
    PLM_TRY(mem.alloc(&dlam, (size_t)2 * k));
    PLM_TRY(mem.alloc(&dfilled, (size_t)k));
    const u32 seed_lo = (u32)opts->seed, seed_hi = (u32)(opts->seed >> 32);
    hipLaunchKernelGGL(k_pca_init, dim3((unsigned)(((size_t)Df * b + PC_BLK - 1) / PC_BLK)), dim3(PC_BLK), 0, st, V, Df, b, q,
                       skip, seed_lo, seed_hi);
    PLM_HIP(hipGetLastError());
    PLM_HIP(hipMemsetAsync(X, 0, sizeof(double) * (size_t)Df * b, st));
    PLM_HIP(hipMemsetAsync(small, 0, sizeof(double) * ((size_t)3 * bb + b), st));

    const int cpw = plan.r ? plan.r : 1, chunk_grid = (n_chunks + cpw - 1) / cpw;
    std::vector<double> host((size_t)3 * bb + b), hrot((size_t)2 * bb + b), theta_prev(b, 0.0);
    std::vector<double> A(bb), G(bb), B(bb), Pg, gam, Qp, theta, Pb, sig;
    int it = 0, stat = PLM_STATUS_MAXITER;
    bool have_ritz = false;
    for (;;) {
        it++;
        PLM_TRY(pca_product(d, plan, V, b, Y, st));
        hipLaunchKernelGGL(k_pca_gram, dim3(chunk_grid), dim3(PC_BLK), 0, st, (const double *)V, (const double *)Y, Df, b,
                           n_chunks, cpw, gpart);
        PLM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pca_chunk_sum, dim3((3 * bb + PC_BLK - 1) / PC_BLK), dim3(PC_BLK), 0, st, (const double *)gpart,
                           n_chunks, 3 * bb, small);
        PLM_HIP(hipGetLastError());
        PLM_HIP(hipMemcpyAsync(host.data(), small, sizeof(double) * host.size(), hipMemcpyDeviceToHost, st));
        PLM_HIP(hipStreamSynchronize(st));            // the one synchronisation of the iteration
        // the residuals of the Ritz vectors of the iteration before (X on the device) arrive with this iteration's sums
        double worst = INFINITY;
        if (have_ritz) {
            worst = 0.0;
            for (int c = 0; c < k; c++) worst = std::max(worst, sqrt(std::max(0.0, host[(size_t)3 * bb + c])));
            const double l1 = std::max(theta_prev[0], 0.0);
            if (worst <= opts->tol * l1) { stat = PLM_STATUS_CONVERGED; break; }
            worst = l1 > 0.0 ? worst / l1 : INFINITY;
        }
        // Rayleigh-Ritz on span(V): V^T Y q = theta V^T V q, through the orthonormal basis V S
        std::copy(host.begin(), host.begin() + bb, A.begin());
        std::copy(host.begin() + bb, host.begin() + 2 * bb, G.begin());
        std::copy(host.begin() + 2 * bb, host.begin() + 3 * bb, B.begin());
        for (int i = 0; i < b; i++)
            for (int j = i + 1; j < b; j++) A[(size_t)i * b + j] = A[(size_t)j * b + i] = 0.5 * (A[(size_t)i * b + j] + A[(size_t)j * b + i]);
        std::vector<double> ident((size_t)bb, 0.0);
        for (int i = 0; i < b; i++) ident[(size_t)i * b + i] = 1.0;
        std::vector<double> Gc = G;
        jacobi_eig(b, Gc, Pg, gam);
        const std::vector<double> S = whiten(b, ident, Pg, gam, gram_floor);
        std::vector<double> As = congruence(b, S, A);
        jacobi_eig(b, As, Qp, theta);
        sort_descending(b, Qp, theta);
        std::vector<double> Qf((size_t)bb, 0.0);
        for (int i = 0; i < b; i++)
            for (int j = 0; j < b; j++) {
                double s = 0.0;
                for (int l = 0; l < b; l++) s += S[(size_t)i * b + l] * Qp[(size_t)l * b + j];
                Qf[(size_t)i * b + j] = s;
            }
        // the next block: Y Qf made orthonormal through the eigenvectors of its Gram matrix; directions under the floor dropped
        std::vector<double> Bt = congruence(b, Qf, B);
        jacobi_eig(b, Bt, Pb, sig);
        sort_descending(b, Pb, sig);
        const std::vector<double> T2 = whiten(b, Qf, Pb, sig, gram_floor);
        std::copy(Qf.begin(), Qf.end(), hrot.begin());
        std::copy(T2.begin(), T2.end(), hrot.begin() + bb);
        std::copy(theta.begin(), theta.end(), hrot.begin() + 2 * bb);
        PLM_HIP(hipMemcpyAsync(rot, hrot.data(), sizeof(double) * hrot.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pca_rotate, dim3(chunk_grid), dim3(PC_BLK), 0, st, V, (const double *)Y, X, (const double *)rot,
                           (const double *)(rot + bb), (const double *)(rot + 2 * bb), Df, b, n_chunks, cpw, rpart);
        PLM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pca_chunk_sum, dim3((b + PC_BLK - 1) / PC_BLK), dim3(PC_BLK), 0, st, (const double *)rpart, n_chunks,
                           b, small + 3 * bb);
        PLM_HIP(hipGetLastError());
        theta_prev = theta;
        have_ritz = true;
        if (cb) {
            PLM_HIP(hipStreamSynchronize(st));        // hrot is free again; the callback may take its time
            if (cb((int32_t)it, worst, user) != 0) { stat = PLM_STATUS_INTERRUPTED; break; }
        }
        if (it >= opts->max_iter) break;
    }

    // the answer: the first k Ritz vectors made orthonormal to rounding, evaluated once more, directly
    hipLaunchKernelGGL(k_pca_orth, dim3(1), dim3(PC_BLK), 0, st, (const double *)X, b, F, Df, k, q, skip, seed_lo, seed_hi, dcomp,
                       dfilled);
    PLM_HIP(hipGetLastError());
    PLM_TRY(pca_product(d, plan, F, k, Y, st));
    hipLaunchKernelGGL(k_pca_final, dim3(1), dim3(PC_BLK), 0, st, (const double *)F, (const double *)Y, Df, k, dlam, dlam + k);
    PLM_HIP(hipGetLastError());
    std::vector<double> comp((size_t)k * Df), lam((size_t)2 * k), sc(scores ? (size_t)N * k : 0);
    std::vector<int32_t> filled(k);
    PLM_HIP(hipMemcpyAsync(comp.data(), dcomp, sizeof(double) * comp.size(), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipMemcpyAsync(lam.data(), dlam, sizeof(double) * lam.size(), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipMemcpyAsync(filled.data(), dfilled, sizeof(int32_t) * k, hipMemcpyDeviceToHost, st));
    if (scores) PLM_HIP(hipMemcpyAsync(sc.data(), d.U, sizeof(double) * sc.size(), hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    // beyond the numerical rank: a direction that was dropped and drawn anew, or a Ritz vector of the null space (a block
    // that spans it finds those too), told by a Rayleigh quotient at the rounding level of the spectrum: eigenvalue 0,
    // residual 0
    for (int c = 0; c < k; c++)
        if (filled[c] || !(lam[c] > (double)D * 2.220446049250313e-16 * tv)) lam[c] = lam[k + c] = 0.0;
    std::vector<int> order(k);
    for (int c = 0; c < k; c++) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lam[x] > lam[y]; });
    bool conv = true;
    for (int c = 0; c < k; c++) {
        const int o = order[c];
        eigenvalues[c] = lam[o];
        residuals[c] = lam[k + o];
        memcpy(components + (size_t)c * Df, comp.data() + (size_t)o * Df, sizeof(double) * Df);
        if (scores)
            for (int n = 0; n < N; n++) scores[(size_t)n * k + c] = sc[(size_t)n * k + o];
        conv = conv && lam[k + o] <= opts->tol * std::max(lam[order[0]], 0.0);
    }
    memcpy(mean, f.data(), sizeof(double) * Df);
    if (stat == PLM_STATUS_INTERRUPTED) conv = false;
    else stat = conv ? PLM_STATUS_CONVERGED : PLM_STATUS_MAXITER;
    if (total_variance) *total_variance = tv;
    if (total) *total = Wi;
    if (iterations) *iterations = it;
    if (converged) *converged = conv ? 1 : 0;
    if (status) *status = stat;
    return PLM_OK;
}

int plm_pca_fit(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                const plm_pca_opts *opts, double *mean, double *components, double *eigenvalues, double *residuals,
                double *total_variance, uint64_t *total, int32_t *iterations, int32_t *converged, double *scores, int device,
                void *stream) {
    return plm_pca_fit_cb(msa, weights, n_seqs, n_sites, n_states, opts, mean, components, eigenvalues, residuals,
                          total_variance, total, iterations, converged, scores, device, stream, nullptr, nullptr, nullptr);
}

int plm_pca_project(const int8_t *seqs, int32_t n, int32_t n_sites, int32_t n_states, const double *mean,
                    const double *components, int32_t k, int32_t skip_state, double *scores, int device, void *stream) {
    const int N = n, L = n_sites, q = n_states;
    PLM_TRY(pca_check_shape(N, L, q, "n"));
    if (!seqs || !mean || !components || !scores) return plm_fail(PLM_EINVAL, "NULL seqs, mean, components or scores");
    if (skip_state < -1 || skip_state >= q) return plm_fail(PLM_EINVAL, "skip_state %d outside -1..%d", skip_state, q - 1);
    const long long D = (long long)L * (skip_state >= 0 ? q - 1 : q);
    if (k < 1 || k > D) return plm_fail(PLM_EINVAL, "k = %d outside 1..%lld (the number of features)", k, D);
    if (k > PC_MAXB) return plm_fail(PLM_EINVAL, "k = %d is above %d", k, PC_MAXB);
    const int Df = L * q;
    for (int d = 0; d < Df; d++)
        if (!std::isfinite(mean[d])) return plm_fail(PLM_EINVAL, "mean[%d] is not finite", d);
    for (size_t e = 0; e < (size_t)k * Df; e++)
        if (!std::isfinite(components[e])) return plm_fail(PLM_EINVAL, "components[%zu] is not finite", e);
    const size_t Np = ((size_t)N + 15) / 16 * 16;
    std::vector<int8_t> cols;
    PLM_TRY(pca_columns(seqs, N, L, q, "seqs", Np, &cols));
    PcaPlan plan;
    PLM_TRY(pca_forced_plan(&plan));
    std::vector<double> F((size_t)Df * k);                         // [Df][k], the skipped state contributes 0
    for (int c = 0; c < k; c++)
        for (int d = 0; d < Df; d++) F[(size_t)d * k + c] = (d % q) == skip_state ? 0.0 : components[(size_t)c * Df + d];
    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    PLM_TRY(plm_check_free((double)cols.size() + 8.0 * ((double)Df * (1 + k) + (double)L * k + (double)N * k), "plm_pca_project"));
    DeviceBuffers mem;
    PcaDevice d;
    d.N = N; d.L = L; d.q = q; d.Df = Df; d.ns = 0; d.skip = skip_state; d.Np = Np; d.W = 1.0;
    PLM_TRY(pca_upload_image(&d, mem, cols, nullptr, mean, k, false, st));
    double *dF = nullptr;
    PLM_TRY(mem.alloc(&dF, F.size()));
    PLM_HIP(hipMemcpyAsync(dF, F.data(), sizeof(double) * F.size(), hipMemcpyHostToDevice, st));
    PLM_TRY(pca_project_block(d, plan, dF, k, st));
    PLM_HIP(hipMemcpyAsync(scores, d.U, sizeof(double) * (size_t)N * k, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    return PLM_OK;
}
