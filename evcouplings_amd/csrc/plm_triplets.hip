// plm_triplets.hip -- three-site counts, frequencies and connected correlations of an alignment: the listed call
// (plm_triplet_stats) and the scan over every triplet of a selection (plm_triplet_scan); contract in include/plm_hip.h,
// notes in DESIGN_NEXT_ROWS.md section 9.12.
//
// Device image (trip_image): column-major, one column of Np bytes per (selected) site, Np = N rounded up to 16, and the
// fixed-point weights wq [Np] u32 beside it (absent for unit weights).  A lane reads one dword = 4 sequences of a column.
// Counting: the histogram of one triplet (q q cw cells, cw = the c values of this pass) lives in LDS, integer atomicAdd,
// 32-bit cells when W < 2^32 and 64-bit cells otherwise.  One closing pass (triplet_close) forms the marginals, f, C and
// the reductions from the integer counts; the fused scan kernel runs it on the LDS histogram, the listed call (and the
// scan where 64-bit cells of q^3 do not fit the LDS) on the merged u64 counts in global memory.  Same code, same
// integers: the float64 outputs do not depend on the plan.
#include "plm_host_util.h"
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>

typedef uint32_t u32;
typedef unsigned long long u64;

namespace {

constexpr int TR_BLK = 512;                 // threads per workgroup, every kernel of this file
constexpr int TR_WAVES = TR_BLK / 64;
constexpr int TR_HIST_BYTES = 131072;       // LDS of one histogram at most: q = 32 in 32-bit cells
constexpr int TR_MAX_SPLITS = 65535;        // grid.y
constexpr double TR_CHUNK_BYTES = 256e6;    // u64 counts of one chunk of the unfused scan

// LDS behind the histogram: marginal frequencies f_ij, f_ik, f_jk [q q] and f_i, f_j, f_k [q] as f64, then the
// reduction scratch (one f64 sum, one f64 maximum and one int cell per wave)
__host__ __device__ constexpr size_t close_lds_bytes(int q) {
    return sizeof(double) * (size_t)(3 * q * q + 3 * q) + (size_t)TR_WAVES * (2 * sizeof(double) + sizeof(int));
}

// Sequences n0 .. n1 - 1 (n0 a multiple of 4) of the triplet's three columns into hist[(a q + b) cw + c - c0], the
// cells with c outside c0 .. c0 + cw - 1 left to another pass.  The host has checked every state: 0 <= a, b, c < q.
template <typename CT, bool UNIT>
__device__ __forceinline__ void accumulate(CT *__restrict__ hist, const u32 *__restrict__ ci, const u32 *__restrict__ cj,
                                           const u32 *__restrict__ ck, const u32 *__restrict__ wq, int n0, int n1, int q,
                                           int c0, int cw) {
    for (int n = n0 + 4 * (int)threadIdx.x; n < n1; n += 4 * TR_BLK) {
        const u32 vi = ci[n >> 2], vj = cj[n >> 2], vk = ck[n >> 2];
        uint4 w4 = {1u, 1u, 1u, 1u};
        if constexpr (!UNIT) w4 = *(const uint4 *)(wq + n);      // Np is a multiple of 16: the load stays inside
        const u32 w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int a = (vi >> (8 * e)) & 0xff, b = (vj >> (8 * e)) & 0xff, c = (int)((vk >> (8 * e)) & 0xff) - c0;
            if (n + e < n1 && (unsigned)c < (unsigned)cw && w[e] != 0) atomicAdd(&hist[(a * q + b) * cw + c], (CT)w[e]);
        }
    }
}

struct CloseOut {      // where the closing pass of one triplet writes; any pointer may be null
    double *freq, *connected;       // [q q q] of this triplet
    double *norm2, *maxabs;         // one value of this triplet
    int32_t *argmax;
};

// The closing pass of one triplet over its q^3 integer counts cnt[(a q + b) q + c] (LDS or global), by the whole
// workgroup.  lds: close_lds_bytes(q) bytes.  Every float64 operation is written out and not contracted, so the result
// is a function of the integers alone.  Ends with a barrier: cnt and lds may be reused at once.
template <typename CT>
__device__ __forceinline__ void triplet_close(const CT *__restrict__ cnt, int q, double W, int skip, double *__restrict__ lds,
                                              const CloseOut &out) {
#pragma clang fp contract(off)
    const int q2 = q * q, q3 = q2 * q, tid = threadIdx.x;
    double *fij = lds, *fik = fij + q2, *fjk = fik + q2, *fi = fjk + q2, *fj = fi + q, *fk = fj + q;
    double *red_s = fk + q, *red_m = red_s + TR_WAVES;
    int *red_c = (int *)(red_m + TR_WAVES);
    for (int p = tid; p < 3 * q2; p += TR_BLK) {        // pair counts, kept as integers (bit patterns) for the next step
        const int which = p / q2, r = p - which * q2, x = r / q, y = r - x * q;
        u64 s = 0;
        if (which == 0) for (int z = 0; z < q; z++) s += (u64)cnt[(x * q + y) * q + z];
        else if (which == 1) for (int z = 0; z < q; z++) s += (u64)cnt[(x * q + z) * q + y];
        else for (int z = 0; z < q; z++) s += (u64)cnt[(z * q + x) * q + y];
        lds[p] = __longlong_as_double((long long)s);
    }
    __syncthreads();
    u64 single = 0;
    if (tid < 3 * q) {                                  // i: rows of ij; j: columns of ij; k: columns of ik
        const int which = tid / q, x = tid - which * q;
        for (int y = 0; y < q; y++)
            single += (u64)__double_as_longlong(which == 0 ? fij[x * q + y] : which == 1 ? fij[y * q + x] : fik[y * q + x]);
    }
    __syncthreads();
    for (int p = tid; p < 3 * q2; p += TR_BLK) lds[p] = (double)(u64)__double_as_longlong(lds[p]) / W;
    if (tid < 3 * q) fi[tid] = (double)single / W;
    __syncthreads();
    double s2 = 0.0, mx = -1.0;
    int mc = q3;
    for (int cell = tid; cell < q3; cell += TR_BLK) {
        const int a = cell / q2, r = cell - a * q2, b = r / q, c = r - b * q;
        const double f3 = (double)(u64)cnt[cell] / W;
        const double t1 = fij[a * q + b] * fk[c], t2 = fik[a * q + c] * fj[b], t3 = fjk[b * q + c] * fi[a];
        const double t4 = 2.0 * fi[a] * fj[b] * fk[c];
        const double cc = f3 - t1 - t2 - t3 + t4;
        if (out.freq) out.freq[cell] = f3;
        if (out.connected) out.connected[cell] = cc;
        if (a != skip && b != skip && c != skip) {
            s2 += cc * cc;
            if (fabs(cc) > mx) { mx = fabs(cc); mc = cell; }     // ascending cells: the smallest cell of a tie
        }
    }
    for (int h = 32; h > 0; h >>= 1) {                  // fixed order: the lanes of a wave, then the waves
        s2 = s2 + __shfl_down(s2, h);
        const double om = __shfl_down(mx, h);
        const int oc = __shfl_down(mc, h);
        if (om > mx || (om == mx && oc < mc)) { mx = om; mc = oc; }
    }
    if ((tid & 63) == 0) { red_s[tid >> 6] = s2; red_m[tid >> 6] = mx; red_c[tid >> 6] = mc; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TR_WAVES; w++) {
            s2 = s2 + red_s[w];
            if (red_m[w] > mx || (red_m[w] == mx && red_c[w] < mc)) { mx = red_m[w]; mc = red_c[w]; }
        }
        if (out.norm2) *out.norm2 = s2;
        if (out.maxabs) *out.maxabs = mx;
        if (out.argmax) *out.argmax = mc;
    }
    __syncthreads();
}

// Listed call, counting: workgroup (t, s, p) = triplet t, sequences s n_per .. , c values p cw .. ; the LDS histogram is
// flushed into counts[t][q q q] (u64, zeroed by the host) with integer atomics.
template <typename CT, bool UNIT>
__global__ __launch_bounds__(TR_BLK) void k_trip_count(const u32 *__restrict__ img, size_t col_dwords,
                                                      const u32 *__restrict__ wq, int N, int q,
                                                      const int32_t *__restrict__ trip, int n_per, int cw,
                                                      u64 *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    CT *hist = (CT *)smem;
    const int t = blockIdx.x, c0 = blockIdx.z * cw, cwe = min(cw, q - c0);
    const int n0 = blockIdx.y * n_per, n1 = min(N, n0 + n_per);
    const int cells = q * q * cwe;
    for (int p = threadIdx.x; p < cells; p += TR_BLK) hist[p] = 0;
    __syncthreads();
    accumulate<CT, UNIT>(hist, img + trip[3 * t] * col_dwords, img + trip[3 * t + 1] * col_dwords,
                         img + trip[3 * t + 2] * col_dwords, wq, n0, n1, q, c0, cwe);
    __syncthreads();
    u64 *dst = counts + (size_t)t * q * q * q;
    for (int p = threadIdx.x; p < cells; p += TR_BLK) {
        const CT v = hist[p];
        const int ab = p / cwe, c = p - ab * cwe;
        if (v) atomicAdd(&dst[ab * q + c0 + c], (u64)v);
    }
}

// Closing pass over merged counts in global memory: one workgroup per triplet.
__global__ __launch_bounds__(TR_BLK) void k_trip_close(const u64 *__restrict__ counts, int q, double W, int skip,
                                                      double *__restrict__ freq, double *__restrict__ connected,
                                                      double *__restrict__ norm2, double *__restrict__ maxabs,
                                                      int32_t *__restrict__ argmax) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t t = blockIdx.x, q3 = (size_t)q * q * q;
    const CloseOut out = {freq ? freq + t * q3 : nullptr, connected ? connected + t * q3 : nullptr,
                          norm2 ? norm2 + t : nullptr, maxabs ? maxabs + t : nullptr, argmax ? argmax + t : nullptr};
    triplet_close<u64>(counts + t * q3, q, W, skip, (double *)smem, out);
}

struct ScanPair { int32_t i, j; long long base; };    // positions i < j of the selection; base: index of (i, j, j + 1)

// Fused scan: workgroup (pair, y) keeps (i, j) and walks k = j + 1 + y, j + 1 + y + gridDim.y, ...: zero, count every
// sequence, close on the LDS histogram.
template <typename CT, bool UNIT>
__global__ __launch_bounds__(TR_BLK) void k_trip_scan(const u32 *__restrict__ img, size_t col_dwords,
                                                     const u32 *__restrict__ wq, int N, int q, int n_sel,
                                                     const ScanPair *__restrict__ pairs, double W, int skip,
                                                     double *__restrict__ norm2, double *__restrict__ maxabs,
                                                     int32_t *__restrict__ argmax) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    CT *hist = (CT *)smem;
    const int q3 = q * q * q;
    double *lds = (double *)(smem + (((size_t)q3 * sizeof(CT) + 15) & ~(size_t)15));
    const ScanPair pr = pairs[blockIdx.x];
    const u32 *ci = img + pr.i * col_dwords, *cj = img + pr.j * col_dwords;
    for (int k = pr.j + 1 + blockIdx.y; k < n_sel; k += gridDim.y) {
        for (int p = threadIdx.x; p < q3; p += TR_BLK) hist[p] = 0;
        __syncthreads();
        accumulate<CT, UNIT>(hist, ci, cj, img + k * col_dwords, wq, 0, N, q, 0, q);
        __syncthreads();
        const long long t = pr.base + (k - pr.j - 1);
        const CloseOut out = {nullptr, nullptr, norm2 ? norm2 + t : nullptr, maxabs ? maxabs + t : nullptr,
                              argmax ? argmax + t : nullptr};
        triplet_close<CT>(hist, q, W, skip, lds, out);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------

// PLM_TRIPLET_PLAN: comma-separated tokens that force the launch plan (measurements and tests): w32 / w64 the cell width,
// n<int> sequences per workgroup of the listed call, c<int> c values per pass of the listed call, k<int> workgroups that
// share the k range of one (i, j) of the scan, u the unfused scan.  0 = not forced.
struct TripPlan { int width, n_per, cw, ksplit, unfused; };

int trip_forced_plan(TripPlan *p) {
    *p = TripPlan{0, 0, 0, 0, 0};
    const char *v = getenv("PLM_TRIPLET_PLAN");
    if (!v) return PLM_OK;
    const char *s = v;
    bool ok = *s != 0;
    while (ok && *s) {
        const char key = *s++;
        if (key == 'u') {
            p->unfused = 1;
        } else if (key == 'w' || key == 'n' || key == 'c' || key == 'k') {
            char *end = nullptr;
            errno = 0;
            const long x = (*s >= '0' && *s <= '9') ? strtol(s, &end, 10) : -1;
            if (errno || x < 1 || x > INT_MAX) { ok = false; break; }
            s = end;
            if (key == 'w') { ok = x == 32 || x == 64; p->width = (int)x; }
            else if (key == 'n') p->n_per = (int)x;
            else if (key == 'c') { ok = x <= 32; p->cw = (int)x; }
            else { ok = x <= TR_MAX_SPLITS; p->ksplit = (int)x; }
        } else {
            ok = false;
        }
        if (ok && *s) { ok = *s == ',' && s[1] != 0; s++; }
    }
    if (!ok)
        return plm_fail(PLM_EINVAL, "PLM_TRIPLET_PLAN must be a comma-separated list of w32, w64, n<int>, c<int 1..32>, "
                                    "k<int 1..65535>, u (got '%s')", v);
    return PLM_OK;
}

struct TripImage {
    int N, n_cols, q;
    size_t Np;                       // bytes of a column
    std::vector<int8_t> cols;        // [n_cols][Np]
    std::vector<u32> wq;             // [Np], empty for unit weights
    u64 W;
};

// The checks every call shares, then the image of the columns `sites` (nullptr: all) and the fixed-point weights.
int trip_image(const int8_t *msa, const float *weights, int N, int L, int q, const int32_t *sites, int n_cols,
               const plm_triplet_opts *opts, TripImage *im) {
    if (N < 1) return plm_fail(PLM_EINVAL, "n_seqs must be at least 1 (got %d)", N);
    if (L < 3) return plm_fail(PLM_EINVAL, "n_sites must be at least 3 (got %d)", L);
    if (q < 2 || q > 32) return plm_fail(PLM_EINVAL, "n_states %d outside 2..32", q);
    if (!msa || !opts) return plm_fail(PLM_EINVAL, "NULL msa or opts");
    if (opts->skip_state < -1 || opts->skip_state >= q)
        return plm_fail(PLM_EINVAL, "skip_state %d outside -1..%d", opts->skip_state, q - 1);
    if ((long long)N + 16 > INT_MAX) return plm_fail(PLM_EINVAL, "n_seqs %d is too large", N);
    im->N = N; im->n_cols = n_cols; im->q = q;
    im->Np = ((size_t)N + 15) / 16 * 16;
    uint64_t W = 0;
    PLM_TRY(plm_quantise_weights(weights, N, im->Np, &im->wq, &W));
    im->W = W;
    for (int n = 0; n < N; n++)
        for (int i = 0; i < L; i++) {
            const int8_t v = msa[(size_t)n * L + i];
            if (v < 0 || v >= q) return plm_fail(PLM_EINVAL, "msa[%d][%d] = %d outside 0..%d", n, i, (int)v, q - 1);
        }
    im->cols.assign((size_t)n_cols * im->Np, (int8_t)0);
    for (int n = 0; n < N; n++) {
        const int8_t *src = msa + (size_t)n * L;
        for (int c = 0; c < n_cols; c++) im->cols[(size_t)c * im->Np + n] = src[sites ? sites[c] : c];
    }
    return PLM_OK;
}

// the cell width of this call: 32 bits while every sum fits, unless the plan forces 64
int trip_width(const TripPlan &plan, u64 W, int *width) {
    const int need = W < (1ull << 32) ? 32 : 64;
    if (plan.width == 32 && need == 64)
        return plm_fail(PLM_EINVAL, "PLM_TRIPLET_PLAN forces w32, but the total weight %llu needs 64-bit cells", W);
    *width = plan.width ? plan.width : need;
    return PLM_OK;
}

struct TripDevice { u32 *img = nullptr, *wq = nullptr; };

int trip_upload(const TripImage &im, DeviceBuffers &mem, hipStream_t st, TripDevice *d) {
    PLM_TRY(mem.alloc(&d->img, im.cols.size() / 4));
    PLM_HIP(hipMemcpyAsync(d->img, im.cols.data(), im.cols.size(), hipMemcpyHostToDevice, st));
    if (!im.wq.empty()) {
        PLM_TRY(mem.alloc(&d->wq, im.wq.size()));
        PLM_HIP(hipMemcpyAsync(d->wq, im.wq.data(), sizeof(u32) * im.wq.size(), hipMemcpyHostToDevice, st));
    }
    return PLM_OK;
}

template <typename... P, typename... A>
hipError_t trip_launch(void (*kern)(P...), dim3 grid, size_t lds, hipStream_t st, A... args) {
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(TR_BLK), lds, st, args...);
    return hipGetLastError();
}

// counts[T][q^3] (zeroed here) of the device triplet table `trip`
int trip_count(const TripImage &im, const TripDevice &d, const TripPlan &plan, int width, const int32_t *trip, int T,
               u64 *counts, hipStream_t st) {
    const int q = im.q, cell = width / 8;
    int cw = plan.cw ? std::min(plan.cw, q) : q;
    cw = std::min(cw, TR_HIST_BYTES / (q * q * cell));
    const int passes = (q + cw - 1) / cw;
    int n_per = plan.n_per;
    if (!n_per) {      // about 2048 workgroups, 4096 sequences each at least
        const long long want = std::max(1ll, 2048ll / ((long long)T * passes));
        n_per = (int)std::max(4096ll, ((long long)im.N + want - 1) / want);
    }
    n_per = (int)std::min<long long>(((long long)n_per + 3) / 4 * 4, (long long)im.Np);
    const int splits = (im.N + n_per - 1) / n_per;
    if (splits > TR_MAX_SPLITS)
        return plm_fail(PLM_EINVAL, "PLM_TRIPLET_PLAN: n%d splits %d sequences into more than %d ranges", plan.n_per, im.N,
                        TR_MAX_SPLITS);
    PLM_HIP(hipMemsetAsync(counts, 0, sizeof(u64) * (size_t)T * q * q * q, st));
    const dim3 grid(T, splits, passes);
    const size_t lds = (size_t)q * q * cw * cell, cd = im.Np / 4;
    const bool unit = im.wq.empty();
#define TRIP_COUNT(CT, UNIT) trip_launch(k_trip_count<CT, UNIT>, grid, lds, st, d.img, cd, d.wq, im.N, q, trip, n_per, cw, counts)
    if (width == 32) PLM_HIP(unit ? TRIP_COUNT(u32, true) : TRIP_COUNT(u32, false));
    else PLM_HIP(unit ? TRIP_COUNT(u64, true) : TRIP_COUNT(u64, false));
#undef TRIP_COUNT
    return PLM_OK;
}

}  // namespace

int plm_triplet_stats(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                      const int32_t *triplets, int32_t n_triplets, const plm_triplet_opts *opts, uint64_t *counts,
                      double *freq, double *connected, uint64_t *total, int device, void *stream) {
    if (n_triplets < 1) return plm_fail(PLM_EINVAL, "n_triplets must be at least 1 (got %d)", n_triplets);
    if (!triplets) return plm_fail(PLM_EINVAL, "NULL triplets");
    TripImage im;
    PLM_TRY(trip_image(msa, weights, n_seqs, n_sites, n_states, nullptr, std::max(n_sites, 0), opts, &im));
    for (int t = 0; t < n_triplets; t++) {
        const int32_t i = triplets[3 * t], j = triplets[3 * t + 1], k = triplets[3 * t + 2];
        if (!(0 <= i && i < j && j < k && k < n_sites))
            return plm_fail(PLM_EINVAL, "triplet %d = (%d, %d, %d) is not i < j < k inside 0..%d", t, i, j, k, n_sites - 1);
    }
    TripPlan plan;
    int width = 0;
    PLM_TRY(trip_forced_plan(&plan));
    PLM_TRY(trip_width(plan, im.W, &width));
    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    const int q = n_states, T = n_triplets;
    const size_t n_cells = (size_t)T * q * q * q;
    const bool want_f = freq && (opts->want & PLM_TRIPLET_FREQ), want_c = connected && (opts->want & PLM_TRIPLET_CONNECTED);
    const bool want_n = counts && (opts->want & PLM_TRIPLET_COUNTS);
    PLM_TRY(plm_check_free((double)im.cols.size() + 4.0 * im.wq.size() + 12.0 * T +
                           8.0 * (double)n_cells * (1 + (want_f ? 1 : 0) + (want_c ? 1 : 0)), "plm_triplet_stats"));
    DeviceBuffers mem;
    TripDevice d;
    int32_t *dtrip = nullptr;
    u64 *dcounts = nullptr;
    double *dfreq = nullptr, *dconn = nullptr;
    PLM_TRY(trip_upload(im, mem, st, &d));
    PLM_TRY(mem.alloc(&dtrip, (size_t)3 * T));
    PLM_TRY(mem.alloc(&dcounts, n_cells));
    if (want_f) PLM_TRY(mem.alloc(&dfreq, n_cells));
    if (want_c) PLM_TRY(mem.alloc(&dconn, n_cells));
    PLM_HIP(hipMemcpyAsync(dtrip, triplets, sizeof(int32_t) * 3 * T, hipMemcpyHostToDevice, st));
    PLM_TRY(trip_count(im, d, plan, width, dtrip, T, dcounts, st));
    if (want_f || want_c)
        PLM_HIP(trip_launch(k_trip_close, dim3(T), close_lds_bytes(q), st, (const u64 *)dcounts, q, (double)im.W,
                            (int)opts->skip_state, dfreq, dconn, (double *)nullptr, (double *)nullptr, (int32_t *)nullptr));
    if (want_n) PLM_HIP(hipMemcpyAsync(counts, dcounts, sizeof(u64) * n_cells, hipMemcpyDeviceToHost, st));
    if (want_f) PLM_HIP(hipMemcpyAsync(freq, dfreq, sizeof(double) * n_cells, hipMemcpyDeviceToHost, st));
    if (want_c) PLM_HIP(hipMemcpyAsync(connected, dconn, sizeof(double) * n_cells, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    if (total) *total = im.W;
    return PLM_OK;
}

int plm_triplet_scan(const int8_t *msa, const float *weights, int32_t n_seqs, int32_t n_sites, int32_t n_states,
                     const int32_t *sites, int32_t n_sel, const plm_triplet_opts *opts, double *norm2, double *maxabs,
                     int32_t *argmax, uint64_t *total, int device, void *stream) {
    if (sites) {
        if (n_sel < 3) return plm_fail(PLM_EINVAL, "the selection holds fewer than 3 sites (n_sel = %d)", n_sel);
        for (int c = 0; c < n_sel; c++)
            if (sites[c] < 0 || sites[c] >= n_sites || (c > 0 && sites[c] <= sites[c - 1]))
                return plm_fail(PLM_EINVAL, "sites[%d] = %d: the selection must be strictly ascending inside 0..%d", c,
                                sites[c], n_sites - 1);
    } else {
        n_sel = n_sites;
    }
    const long long T = n_sel > 4096 ? LLONG_MAX : (long long)n_sel * (n_sel - 1) / 2 * (n_sel - 2) / 3;
    if (n_sel >= 3 && T > INT_MAX) return plm_fail(PLM_EINVAL, "%d sites make more than 2^31 - 1 triplets", n_sel);
    TripImage im;
    PLM_TRY(trip_image(msa, weights, n_seqs, n_sites, n_states, sites, std::max(n_sel, 0), opts, &im));
    TripPlan plan;
    int width = 0;
    PLM_TRY(trip_forced_plan(&plan));
    PLM_TRY(trip_width(plan, im.W, &width));
    PLM_TRY(plm_check_device(device));
    hipStream_t st = (hipStream_t)stream;
    const int q = n_states;
    const size_t q3 = (size_t)q * q * q;
    const size_t fused_lds = ((q3 * (width / 8) + 15) & ~(size_t)15) + close_lds_bytes(q);
    const bool fused = !plan.unfused && q3 * (width / 8) <= (size_t)TR_HIST_BYTES && fused_lds <= 163840;
    const int chunk = (int)std::min<long long>(T, std::max(1ll, (long long)(TR_CHUNK_BYTES / (8.0 * q3))));
    const int n_pairs = (n_sel - 1) * (n_sel - 2) / 2;
    PLM_TRY(plm_check_free((double)im.cols.size() + 4.0 * im.wq.size() + 20.0 * T +
                           (fused ? 16.0 * n_pairs : (8.0 * q3 + 12.0) * chunk), "plm_triplet_scan"));
    DeviceBuffers mem;
    TripDevice d;
    double *dn2 = nullptr, *dmx = nullptr;
    int32_t *dam = nullptr;
    PLM_TRY(trip_upload(im, mem, st, &d));
    PLM_TRY(mem.alloc(&dn2, (size_t)T));
    PLM_TRY(mem.alloc(&dmx, (size_t)T));
    PLM_TRY(mem.alloc(&dam, (size_t)T));
    std::vector<ScanPair> pairs;
    std::vector<int32_t> table;
    if (fused) {
        long long base = 0;
        for (int i = 0; i < n_sel - 2; i++)
            for (int j = i + 1; j < n_sel - 1; j++) {
                pairs.push_back(ScanPair{i, j, base});
                base += n_sel - 1 - j;
            }
        ScanPair *dpairs = nullptr;
        PLM_TRY(mem.alloc(&dpairs, pairs.size()));
        PLM_HIP(hipMemcpyAsync(dpairs, pairs.data(), sizeof(ScanPair) * pairs.size(), hipMemcpyHostToDevice, st));
        int ksplit = plan.ksplit;
        if (!ksplit) ksplit = (int)std::max(1ll, 2048ll / n_pairs);      // small selections: spread the k range too
        ksplit = std::min(ksplit, n_sel - 2);
        const dim3 grid(n_pairs, ksplit);
        const size_t cd = im.Np / 4;
        const bool unit = im.wq.empty();
#define TRIP_SCAN(CT, UNIT) trip_launch(k_trip_scan<CT, UNIT>, grid, fused_lds, st, d.img, cd, d.wq, im.N, q, (int)n_sel, \
                                        (const ScanPair *)dpairs, (double)im.W, (int)opts->skip_state, dn2, dmx, dam)
        if (width == 32) PLM_HIP(unit ? TRIP_SCAN(u32, true) : TRIP_SCAN(u32, false));
        else PLM_HIP(unit ? TRIP_SCAN(u64, true) : TRIP_SCAN(u64, false));
#undef TRIP_SCAN
    } else {       // chunks of the lexicographic table through the kernels of the listed call
        table.reserve((size_t)3 * T);
        for (int i = 0; i < n_sel - 2; i++)
            for (int j = i + 1; j < n_sel - 1; j++)
                for (int k = j + 1; k < n_sel; k++) { table.push_back(i); table.push_back(j); table.push_back(k); }
        int32_t *dtrip = nullptr;
        u64 *dcounts = nullptr;
        PLM_TRY(mem.alloc(&dtrip, (size_t)3 * chunk));
        PLM_TRY(mem.alloc(&dcounts, q3 * chunk));
        for (long long t0 = 0; t0 < T; t0 += chunk) {
            const int tc = (int)std::min<long long>(chunk, T - t0);
            PLM_HIP(hipMemcpyAsync(dtrip, table.data() + 3 * t0, sizeof(int32_t) * 3 * tc, hipMemcpyHostToDevice, st));
            PLM_TRY(trip_count(im, d, plan, width, dtrip, tc, dcounts, st));
            PLM_HIP(trip_launch(k_trip_close, dim3(tc), close_lds_bytes(q), st, (const u64 *)dcounts, q, (double)im.W,
                                (int)opts->skip_state, (double *)nullptr, (double *)nullptr, dn2 + t0, dmx + t0, dam + t0));
        }
    }
    if (norm2) PLM_HIP(hipMemcpyAsync(norm2, dn2, sizeof(double) * T, hipMemcpyDeviceToHost, st));
    if (maxabs) PLM_HIP(hipMemcpyAsync(maxabs, dmx, sizeof(double) * T, hipMemcpyDeviceToHost, st));
    if (argmax) PLM_HIP(hipMemcpyAsync(argmax, dam, sizeof(int32_t) * T, hipMemcpyDeviceToHost, st));
    PLM_HIP(hipStreamSynchronize(st));
    if (total) *total = im.W;
    return PLM_OK;
}
