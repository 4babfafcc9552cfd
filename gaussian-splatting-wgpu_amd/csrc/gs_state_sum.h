// gs_state_sum.h -- a workgroup's count into the GS_STATE_SLOTS partial sums (gs_kernels.h): what the kernels of k_state.hip and
// k_attr.hip return as `matched` / `count`.  Wave sum (DPP), one LDS add per wave, one global add per workgroup, spread over the
// slots.  A kernel calls state_block_begin first (every thread), state_block_add last (every thread, once).
#pragma once
#include "gs_device.h"
#include "gs_kernels.h"

__shared__ uint32_t s_state_sum;
__device__ __forceinline__ void state_block_begin() {
    if (threadIdx.x == 0) s_state_sum = 0u;
    __syncthreads();
}
__device__ __forceinline__ void state_block_add(uint32_t hits, unsigned long long* slots) {
    const uint32_t ws = wave_sum(hits);
    if ((threadIdx.x & 63u) == 0u && ws) atomicAdd(&s_state_sum, ws);
    __syncthreads();
    if (threadIdx.x == 0 && s_state_sum) atomicAdd(slots + (blockIdx.x % GS_STATE_SLOTS) * GS_STATE_SLOT_STRIDE, (unsigned long long)s_state_sum);
}
