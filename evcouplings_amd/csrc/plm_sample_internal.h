// plm_sample_internal.h -- what plm_sample.hip lends to plm_bm.hip: the expansion of the couplings and the sweep
// launchers, with the choice between the tiled and the direct form that plm_sample makes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gibbs {

struct SweepPlan {
    int NV, NVP, tile, JC;      // the tiled form: float4 per row, padded row, chains per workgroup, j-chunk
    size_t lds;
    bool direct;                // the direct form instead
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

}  // namespace gibbs
