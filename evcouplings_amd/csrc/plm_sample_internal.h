// plm_sample_internal.h -- what plm_sample.hip shares with plm_ais.hip, plm_pt.hip, plm_anneal.hip and plm_bm.hip: the
// checks the five entry points (plm_sample, plm_ais, plm_pt, plm_anneal, plm_bm_fit) open with, the mask of the allowed
// states, the two words of a seed, the plan, the model on the device and the expansion of its couplings, the sweep
// launchers, the energies of the states returned, and the step from a plan to the template arguments and the grid of a
// sweep kernel.
#pragma once
#include "plm_host_util.h"
#include <type_traits>

namespace gibbs {

struct SweepPlan {
    int NV, NVP, tile, JC;      // the tiled form: float4 per row, padded row, chains per workgroup, j-chunk
    size_t lds;
    bool direct;                // the direct form instead (tile = chains per workgroup = 256 / lanes per chain)
};

// ---- the front matter of plm_sample, plm_ais, plm_pt and plm_bm_fit ----
int check_states(int q, const char *who);             // 2..32 states, or PLM_EUNSUPPORTED
int check_chain_sites(int C, int L);                  // n_chains x n_sites < 2^31, or PLM_EINVAL
double table_bytes(int L, int q);                     // the expanded table
double canon_bytes(int L, int q);                     // one float32 vector in the canonical layout
// start [C][L]: every state in 0 .. q-1 and, unless its site is fixed (fixed may be NULL), allowed; or PLM_EINVAL
int check_start(const int8_t *start, int C, int L, int q, uint32_t allowed, const uint8_t *fixed);
// flags [q] (NULL: every state) -> the bit mask of the states that may be drawn; PLM_EINVAL when there is none
int allowed_mask(int q, const uint8_t *flags, uint32_t *out);

// the two words of a seed, as the kernels take them
struct Seed {
    uint32_t lo, hi;
    explicit Seed(uint64_t seed) : lo((uint32_t)(seed & 0xFFFFFFFFu)), hi((uint32_t)(seed >> 32)) {}
};

// PLM_OK and the plan, or PLM_EDEVICE / PLM_EUNSUPPORTED / PLM_EINVAL (a PLM_SAMPLE_TILE or PLM_SAMPLE_JC without a
// valid plan) with the message recorded
int plan_sweeps(int L, int q, int C, int device, SweepPlan *out);

size_t table_float4(int L, int q);       // float4 of the expanded table (couplings and fields)

// W <- expansion of canon (k_sample_expand)
hipError_t expand(hipStream_t st, const float *canon, int L, int q, float4 *W);

// n_sweeps sweeps with the indices sweep0 .. from src (NULL: the start rule) into dst, both [C][L]
hipError_t sweeps(const SweepPlan &p, hipStream_t st, const float4 *W, int L, int q, int C, const int8_t *src,
                  const uint8_t *fixed, uint32_t allowed, float beta, uint64_t seed, uint32_t sweep0, int n_sweeps,
                  int8_t *dst);

// steps of n_per sweeps per launch, out of K, that keep a launch of plm_ais or plm_anneal near a second (an estimate)
int default_steps_per_launch(const SweepPlan &p, int L, int C, int n_per, int K, int n_cu);

// (H, H_J, H_h) of n_rows host rows of L states into energies_out [n_rows][3]: what plm_hamiltonians returns for them,
// and the field-only model (L == 1), which its forward GEMM cannot take.  Allocates: call it after the caller's buffers
// are freed.
int state_energies(const int8_t *rows, size_t n_rows, int L, int q, const float *x_canonical, int device, void *stream,
                   double *energies_out);

// ---- from a plan to a kernel ----
template <int V> using Int = std::integral_constant<int, V>;

template <int NV, typename F> hipError_t with_tile(int tile, F &f) {
    switch (tile) {
    case 64: return f(Int<NV>{}, Int<64>{});
    case 128: return f(Int<NV>{}, Int<128>{});
    case 256: return f(Int<NV>{}, Int<256>{});
    }
    return hipErrorInvalidValue;
}

// tiled(Int<NV>, Int<TILE>) for NV = 1 .. 8 and TILE = 64, 128, 256, or direct(Int<QP>) for QP = 2, 4, 8, 16, 32 lanes
// per chain: every plan the planner makes is one of these (tests/test_sampler_plan_host.py)
template <typename Tiled, typename Direct> hipError_t dispatch(const SweepPlan &p, Tiled tiled, Direct direct) {
    if (p.direct) switch (256 / p.tile) {
        case 2: return direct(Int<2>{});
        case 4: return direct(Int<4>{});
        case 8: return direct(Int<8>{});
        case 16: return direct(Int<16>{});
        case 32: return direct(Int<32>{});
        default: return hipErrorInvalidValue;
        }
    switch (p.NV) {
    case 1: return with_tile<1>(p.tile, tiled);
    case 2: return with_tile<2>(p.tile, tiled);
    case 3: return with_tile<3>(p.tile, tiled);
    case 4: return with_tile<4>(p.tile, tiled);
    case 5: return with_tile<5>(p.tile, tiled);
    case 6: return with_tile<6>(p.tile, tiled);
    case 7: return with_tile<7>(p.tile, tiled);
    case 8: return with_tile<8>(p.tile, tiled);
    }
    return hipErrorInvalidValue;
}

// one launch with the plan's dynamic LDS
template <typename... P, typename... A>
hipError_t launch(void (*kern)(P...), unsigned grid, unsigned block, const SweepPlan &p, hipStream_t st, A... args) {
    const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), p.lds, st, args...);
    return hipGetLastError();
}

// the launch of either form over C chains: a workgroup of the tiled form is a tile of chains, one of the direct form
// 256 lanes in groups of qp lanes per chain
template <typename... P, typename... A>
hipError_t launch_tiled(void (*kern)(P...), int tile, int C, const SweepPlan &p, hipStream_t st, A... args) {
    return launch(kern, (unsigned)((C + tile - 1) / tile), (unsigned)tile, p, st, args...);
}
template <typename... P, typename... A>
hipError_t launch_direct(void (*kern)(P...), int qp, int C, const SweepPlan &p, hipStream_t st, A... args) {
    const int cpw = 256 / qp;                    // chains per workgroup
    return launch(kern, (unsigned)((C + cpw - 1) / cpw), 256u, p, st, args...);
}

// The model of a call on the device: the canonical vector and the table expanded from it.  Two allocations, because an
// entry point's own buffers may sit between them, and the order decides which allocation fails first.
struct DeviceModel {
    const int L, q;
    float *canon = nullptr;
    float4 *W = nullptr;
    DeviceModel(int L_, int q_) : L(L_), q(q_) {}
    int alloc_canon(DeviceBuffers &mem) { return mem.alloc(&canon, (size_t)plm_n_canon(L, q)); }
    int alloc_table(DeviceBuffers &mem) { return mem.alloc(&W, table_float4(L, q)); }
    hipError_t upload(hipStream_t st, const float *x_canonical) const {
        return hipMemcpyAsync(canon, x_canonical, (size_t)plm_n_canon(L, q) * sizeof(float), hipMemcpyHostToDevice, st);
    }
    hipError_t expand(hipStream_t st) const { return gibbs::expand(st, canon, L, q, W); }
};

}  // namespace gibbs
