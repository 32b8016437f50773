// Exponential moving average of the trainable weights on gfx950 (definition: include/reid_hip.h, reid_ema_update / reid_ema_swap).
//
// The averaged set is described by a device table of its own (parameter, shadow, length), so buffers AdamW never sees -- the
// BN-neck's running statistics -- can be averaged by the same launch.  Both kernels are HBM-bound streaming kernels shaped as the
// ones of optim.hip: 16-byte accesses, grid-stride over each table entry, a scalar tail for n % 4, grid = EMA_BLOCKS x n_entries.
//   reid_ema_update  s += w (p - s): 12 bytes per element (read p, read s, write s)
//   reid_ema_swap    p <-> s in place, as 32-bit words
#include "common.h"

// The definition rounds the difference, the product and the sum once each so that a float32 loop on the host reproduces the bits: no
// fused multiply-adds in this file.
#pragma clang fp contract(off)

namespace {

struct EmaEntry {            // 24 bytes, mirrored by prcv2025reid_amd/trainer.py
    float* p; float* s;
    long long n;
};

constexpr int EMA_BLOCKS = 128;     // workgroups per table entry (grid = EMA_BLOCKS x n_entries)
constexpr int ST_STEP = 16;         // optim.hip's device-side step counter (advanced by reid_opt_adamw's tick)

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// w = (float)(1 - d_t), d_t = min(decay, (1 + t) / (10 + t)) under warm-up: evaluated in double here for the host step and for the
// device counter alike, so both give the same bits
__device__ __forceinline__ float ema_weight(float decay, int warmup, double t) {
    double d = (double)decay;
    if (warmup) d = fmin(d, (1.0 + t) / (10.0 + t));
    return (float)(1.0 - d);
}

__global__ __launch_bounds__(256) void ema_update_kernel(const EmaEntry* __restrict__ table, float decay, int warmup, int step,
                                                         const float* __restrict__ state) {
    const EmaEntry e = table[blockIdx.y];
    const float w = ema_weight(decay, warmup, step >= 1 ? (double)step : (double)state[ST_STEP]);
    const long long n4 = e.n >> 2;
    const f32x4* p4 = (const f32x4*)e.p;
    f32x4* s4 = (f32x4*)e.s;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 p = p4[i];
        f32x4 s = s4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = p[k] - s[k];
            const float wd = w * d;
            s[k] = s[k] + wd;
        }
        s4[i] = s;
    }
    if (blockIdx.x == 0) {
        for (long long i = (n4 << 2) + threadIdx.x; i < e.n; i += 256) {
            const float s = e.s[i];
            const float d = e.p[i] - s;
            const float wd = w * d;
            e.s[i] = s + wd;
        }
    }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(const EmaEntry* __restrict__ table) {
    const EmaEntry e = table[blockIdx.y];
    const long long n4 = e.n >> 2;
    u32x4 *p4 = (u32x4*)e.p, *s4 = (u32x4*)e.s;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const u32x4 p = p4[i], s = s4[i];
        p4[i] = s; s4[i] = p;
    }
    if (blockIdx.x == 0) {
        uint32_t *pw = (uint32_t*)e.p, *sw = (uint32_t*)e.s;
        for (long long i = (n4 << 2) + threadIdx.x; i < e.n; i += 256) {
            const uint32_t p = pw[i], s = sw[i];
            pw[i] = s; sw[i] = p;
        }
    }
}

}  // namespace

extern "C" int32_t reid_ema_entry_bytes(void) { return (int32_t)sizeof(EmaEntry); }

extern "C" int reid_ema_update(const void* table, int32_t n_entries, float decay, int32_t warmup, int32_t step, const float* state,
                               void* stream) {
    REID_CHECK_ARG(table && n_entries >= 1 && n_entries <= 65535, "reid_ema_update: bad args (table, 1 <= n_entries <= 65535)");
    REID_CHECK_ARG(decay > 0.f && decay < 1.f, "reid_ema_update: decay must lie in (0, 1)");
    REID_CHECK_ARG(step >= 1 || (step == 0 && state), "reid_ema_update: bad args (step counts from 1; 0 = device counter in state)");
    hipLaunchKernelGGL(ema_update_kernel, dim3(EMA_BLOCKS, n_entries), dim3(256), 0, (hipStream_t)stream, (const EmaEntry*)table, decay,
                       warmup != 0, step, state);
    REID_CHECK_LAUNCH("reid_ema_update");
    return REID_OK;
}

extern "C" int reid_ema_swap(const void* table, int32_t n_entries, void* stream) {
    REID_CHECK_ARG(table && n_entries >= 1 && n_entries <= 65535, "reid_ema_swap: bad args (table, 1 <= n_entries <= 65535)");
    hipLaunchKernelGGL(ema_swap_kernel, dim3(EMA_BLOCKS, n_entries), dim3(256), 0, (hipStream_t)stream, (const EmaEntry*)table);
    REID_CHECK_LAUNCH("reid_ema_swap");
    return REID_OK;
}
