// plm_host_util.h -- the host-side plumbing every one-shot entry point of the library shares: the message recorder and
// the device check of plm_host.cpp, one error macro for HIP calls, a scope guard for device memory, the free-memory
// check that precedes the allocations, and the few size expressions the entry points have in common.  Host code only.
#pragma once
#include "../../include/plm_hip.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>

int plm_fail(int code, const char *fmt, ...);   // plm_host.cpp: records the message for plm_last_error()
int plm_check_device(int device);               // plm_host.cpp: visible gfx950 device, made current

// plm_meanfield.hip.  fi (L q raw frequencies), fij (raw i<j blocks) and the outputs are device pointers; any output may
// be null: hi [L q] f64, jfull [L L q q] f64, jpairs [pairs q q] f32, di [L L] f64.
int plm_meanfield_device(const float *fi, const float *fij, int L, int q, double pseudo_count, hipStream_t st,
                         double *hi, double *jfull, float *jpairs, double *di);
int plm_direct_information_device(const double *jdense, const double *rfi, int L, int q, hipStream_t st, double *di);

// A HIP call that must succeed: the message names the call and carries HIP's text; out of memory is PLM_ENOMEM (the
// runtime grants allocations beyond the HBM, and the failure then surfaces at a later call), everything else PLM_EDEVICE.
#define PLM_HIP(expr)                                                                                      \
    do {                                                                                                   \
        const hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess)                                                                             \
            return plm_fail(e__ == hipErrorOutOfMemory ? PLM_ENOMEM : PLM_EDEVICE, "%s failed: %s (%s:%d)", \
                            #expr, hipGetErrorString(e__), __FILE__, __LINE__);                            \
    } while (0)

#define PLM_TRY(expr)                  \
    do {                               \
        int rc__ = (expr);             \
        if (rc__ != PLM_OK) return rc__; \
    } while (0)

// n_elems of T on the device, 16 bytes at least; the caller owns the pointer (the members of a context)
template <typename T> int plm_dalloc(T **p, size_t n_elems) {
    void *b = nullptr;
    const hipError_t e = hipMalloc(&b, std::max<size_t>(n_elems * sizeof(T), 16));
    *p = e == hipSuccess ? (T *)b : nullptr;
    if (e != hipSuccess)
        return plm_fail(PLM_ENOMEM, "hipMalloc of %zu bytes failed: %s", n_elems * sizeof(T), hipGetErrorString(e));
    return PLM_OK;
}

// The device buffers (and at most one pinned host buffer) of one call: freed when the scope ends, or at free_all().
struct DeviceBuffers {
    std::vector<void *> dev;
    void *pinned = nullptr;
    DeviceBuffers() = default;
    DeviceBuffers(const DeviceBuffers &) = delete;
    DeviceBuffers &operator=(const DeviceBuffers &) = delete;
    ~DeviceBuffers() { free_all(); }
    template <typename T> int alloc(T **p, size_t n_elems) {
        const int rc = plm_dalloc(p, n_elems);
        if (rc == PLM_OK) dev.push_back(*p);
        return rc;
    }
    template <typename T> int alloc_pinned(T **p, size_t n_elems) {
        const hipError_t e = pinned ? hipErrorInvalidValue : hipHostMalloc(&pinned, n_elems * sizeof(T));
        *p = e == hipSuccess ? (T *)pinned : nullptr;
        if (e != hipSuccess)
            return plm_fail(PLM_ENOMEM, "hipHostMalloc of %zu bytes failed: %s", n_elems * sizeof(T), hipGetErrorString(e));
        return PLM_OK;
    }
    void free_all() {
        for (void *b : dev) (void)hipFree(b);
        dev.clear();
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr;
    }
};

// PLM_ENOMEM before any allocation when the call needs more device memory than is free.  table_bytes: the share of the
// expanded couplings of the sweep kernels, named in the message when it is given.
inline int plm_check_free(double need_bytes, const char *what, double table_bytes = 0) {
    size_t free_b = 0, total_b = 0;
    const hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess) return plm_fail(PLM_EDEVICE, "hipMemGetInfo failed: %s", hipGetErrorString(e));
    if (need_bytes <= (double)free_b) return PLM_OK;
    char share[64] = "";
    if (table_bytes > 0) snprintf(share, sizeof share, " (%.2f GB of it the expanded couplings)", table_bytes / 1e9);
    return plm_fail(PLM_ENOMEM, "%s needs %.2f GB of device memory%s, %.2f GB are free (of %.1f GB)", what,
                    need_bytes / 1e9, share, free_b / 1e9, total_b / 1e9);
}

// entries of the canonical layout, L q fields and the i<j blocks of q q couplings.  A double: the sizes are compared
// with the free memory before anything is known to fit a size_t (exact wherever the call goes on)
inline double plm_n_canon(int L, int q) { return (double)L * q + (double)L * (L - 1) / 2 * q * q; }

inline uint32_t plm_state_mask(int q) { return q == 32 ? 0xFFFFFFFFu : (1u << q) - 1u; }   // states 0 .. q-1

// What plm_ais and plm_rbm_ais return from the C log weights of their chains: log Z = log Z_0 + m + log mean w with
// w = exp(log w - m), m = max log w, the sums in chain order in float64; ess = (sum w)^2 / sum w^2; the standard error
// of log Z = std(w, ddof = 1) / (sqrt(C) mean w), 0 for C = 1.
inline void plm_ais_summary(const double *logw, int C, double log_z0, double *log_z, double *log_z_se, double *ess) {
    double m = logw[0], s1 = 0.0, s2 = 0.0;
    for (int c = 1; c < C; c++) m = std::max(m, logw[c]);
    for (int c = 0; c < C; c++) {
        const double w = exp(logw[c] - m);
        s1 += w;
        s2 += w * w;
    }
    const double mean = s1 / C;
    *log_z = log_z0 + m + log(mean);
    *ess = s1 * s1 / s2;
    double var = 0.0;
    for (int c = 0; c < C; c++) {
        const double d = exp(logw[c] - m) - mean;
        var += d * d;
    }
    *log_z_se = C > 1 ? sqrt(var / (C - 1)) / (sqrt((double)C) * mean) : 0.0;
}

// The fixed-point weights of the alignment statistics (include/plm_hip.h, three-site section): e = the largest integer
// <= 30 with max(w) 2^e <= 2^30, wq_n = llrint((double)w_n 2^e), W = sum wq_n.  wq: `padded` entries (>= N, the rest 0);
// weights == NULL: wq is left empty (every weight is 1) and W = N.  PLM_EINVAL for a weight that is negative or not
// finite, and for W = 0.
inline int plm_quantise_weights(const float *weights, int N, size_t padded, std::vector<uint32_t> *wq, uint64_t *W) {
    wq->clear();
    *W = (uint64_t)N;
    if (!weights) return PLM_OK;
    double wmax = 0.0;
    for (int n = 0; n < N; n++) {
        const double w = (double)weights[n];
        if (!std::isfinite(w) || w < 0.0) return plm_fail(PLM_EINVAL, "weights[%d] = %g is negative or not finite", n, w);
        wmax = std::max(wmax, w);
    }
    if (!(wmax > 0.0)) return plm_fail(PLM_EINVAL, "the weights are all zero (W = 0)");
    int e = 30;                                   // the largest e <= 30 with wmax 2^e <= 2^30
    while (std::ldexp(wmax, e) > 1073741824.0) e--;
    wq->assign(padded, 0u);
    uint64_t sum = 0;
    for (int n = 0; n < N; n++) {
        const long long v = llrint(std::ldexp((double)weights[n], e));
        (*wq)[n] = (uint32_t)v;
        sum += (uint64_t)v;
    }
    if (sum == 0) return plm_fail(PLM_EINVAL, "the fixed-point weights are all zero (W = 0)");
    *W = sum;
    return PLM_OK;
}

// The padded row-major host image of n sequences of L states that the forward kernels read: rows of row_len bytes,
// n_rows of them, `pad` wherever no sequence is.
inline std::vector<int8_t> plm_padded_rows(const int8_t *seqs, int n, int L, size_t n_rows, size_t row_len, int8_t pad) {
    std::vector<int8_t> rm(n_rows * row_len, pad);
    for (int s = 0; s < n; s++) memcpy(&rm[(size_t)s * row_len], seqs + (size_t)s * L, L);
    return rm;
}
