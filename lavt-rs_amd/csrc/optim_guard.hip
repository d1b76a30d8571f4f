// The guard around the optimizer step: global gradient norm (two launches, no atomics, bitwise reproducible), the fp32[8] control block it
// leaves on the device, and the AdamW update that obeys it (clip coefficient, skip-if-non-finite, hold) -- every decision is taken on the
// device, so the whole sequence can sit inside a captured hipGraph.
#include "common.h"
#include "adamw_body.h"

namespace {

// Pass 1: workgroup c = chunk c of the update's own chunk table -> ws[c] = sum of squares of the chunk's gradient elements (fp32).
// Whole aligned chunks: 8 float4 loads per thread, all issued before the first use; every thread then adds its 32 squares in order, the
// wave reduces with shuffles (6 levels), the 4 waves meet through LDS (2 levels).
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const int64_t* __restrict__ desc, const int2* __restrict__ chunks, float* __restrict__ ws) {
    __shared__ float red[4];
    const int2 ch = chunks[blockIdx.x];
    const float* g = reinterpret_cast<const float*>(desc[6 * ch.x + 1]);
    const int64_t n = desc[6 * ch.x + 4];
    const int64_t e0 = (int64_t)ch.y * ADAMW_CE, e1 = min(n, e0 + ADAMW_CE);
    float acc = 0.f;
    if ((desc[6 * ch.x + 1] & 15) == 0 && e1 - e0 == ADAMW_CE) {
        float4 gg[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) gg[u] = *reinterpret_cast<const float4*>(g + e0 + u * 1024 + threadIdx.x * 4);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc = fmaf(gg[u].x, gg[u].x, acc); acc = fmaf(gg[u].y, gg[u].y, acc);
            acc = fmaf(gg[u].z, gg[u].z, acc); acc = fmaf(gg[u].w, gg[u].w, acc);
        }
    } else {                                   // a tensor's last chunk / unaligned tensors
        for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) acc = fmaf(g[i], g[i], acc);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Pass 2: ONE workgroup adds the partials in fp64 in a fixed order (thread t: partials t, t + 256, ... in sequence; then a fixed tree through
// LDS) and lane 0 writes ctl[0..2].  ctl[3] (skipped-step count) belongs to the guarded tick, ctl[4] (hold) to the host.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const float* __restrict__ ws, int nchunks, float* __restrict__ ctl, float max_norm, int skip_nonfinite) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 256) acc += (double)ws[i];
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(red[0]);
        const bool finite = isfinite(norm);
        ctl[0] = norm;
        ctl[1] = (max_norm > 0.f && finite) ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;      // torch.nn.utils.clip_grad_norm_'s coefficient
        ctl[2] = (skip_nonfinite && !finite) ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void adamw_chunks_guarded_kernel(const int64_t* __restrict__ desc, const float* __restrict__ hyper, const int2* __restrict__ chunks,
                                                                   const float* __restrict__ step, float total_steps, float power, const float* __restrict__ ctl) {
    adamw_chunk_update<true, false>(desc, nullptr, hyper, chunks, step, total_steps, power, ctl);
}

// AMSGrad (adamw_body.h: AMSGRAD): the same body with the max_exp_avg_sq stream behind vmax; GUARD = a control block was given
template <bool GUARD>
__global__ __launch_bounds__(256) void adamw_chunks_amsgrad_kernel(const int64_t* __restrict__ desc, const int64_t* __restrict__ vmax, const float* __restrict__ hyper,
                                                                   const int2* __restrict__ chunks, const float* __restrict__ step, float total_steps, float power,
                                                                   const float* __restrict__ ctl) {
    adamw_chunk_update<GUARD, true>(desc, vmax, hyper, chunks, step, total_steps, power, ctl);
}
__global__ void adamw_tick_kernel(float* step) { step[0] += 1.f; }          // the unguarded tick, as behind lavt_adamw_step_chunks

// the step counter advances only when the update ran; a skipped step is counted unless the optimizer is on hold
__global__ void adamw_tick_guarded_kernel(float* step, float* ctl) {
    const float skip = ctl[2], hold = ctl[4];
    if (skip == 0.f && hold == 0.f) step[0] += 1.f;
    if (hold == 0.f) ctl[3] += skip;
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int64_t lavt_grad_norm_ws(int nchunks) { return nchunks > 0 ? (int64_t)nchunks : 0; }

extern "C" int lavt_grad_norm(const int64_t* desc, const int32_t* chunks, int nchunks, float* ws, float* ctl, float max_norm, int skip_nonfinite, void* stream) {
    LAVT_CHECK_ARG(desc && chunks && ws && ctl && nchunks > 0, "lavt_grad_norm: bad arguments");
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(nchunks), dim3(256), 0, ST, desc, reinterpret_cast<const int2*>(chunks), ws);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, ST, ws, nchunks, ctl, max_norm, skip_nonfinite);
    LAVT_CHECK_LAUNCH("lavt_grad_norm");
    return LAVT_OK;
}

extern "C" int lavt_adamw_step_chunks_guarded(const int64_t* desc, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps, float power,
                                              float* ctl, void* stream) {
    LAVT_CHECK_ARG(desc && hyper && chunks && step && ctl && nchunks > 0, "lavt_adamw_step_chunks_guarded: bad arguments");
    hipLaunchKernelGGL(adamw_chunks_guarded_kernel, dim3(nchunks), dim3(256), 0, ST, desc, hyper, reinterpret_cast<const int2*>(chunks), step, total_steps, power, ctl);
    hipLaunchKernelGGL(adamw_tick_guarded_kernel, dim3(1), dim3(1), 0, ST, step, ctl);
    LAVT_CHECK_LAUNCH("lavt_adamw_step_chunks_guarded");
    return LAVT_OK;
}

extern "C" int lavt_adamw_step_chunks_amsgrad(const int64_t* desc, const int64_t* vmax, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps,
                                              float power, float* ctl, void* stream) {
    LAVT_CHECK_ARG(desc && vmax && hyper && chunks && step && nchunks > 0, "lavt_adamw_step_chunks_amsgrad: bad arguments");
    if (ctl) {
        hipLaunchKernelGGL(adamw_chunks_amsgrad_kernel<true>, dim3(nchunks), dim3(256), 0, ST, desc, vmax, hyper, reinterpret_cast<const int2*>(chunks), step, total_steps, power, ctl);
        hipLaunchKernelGGL(adamw_tick_guarded_kernel, dim3(1), dim3(1), 0, ST, step, ctl);
    } else {
        hipLaunchKernelGGL(adamw_chunks_amsgrad_kernel<false>, dim3(nchunks), dim3(256), 0, ST, desc, vmax, hyper, reinterpret_cast<const int2*>(chunks), step, total_steps, power, nullptr);
        hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, ST, step);
    }
    LAVT_CHECK_LAUNCH("lavt_adamw_step_chunks_amsgrad");
    return LAVT_OK;
}
