// The guard around the optimizer step: global gradient norm (two launches, no atomics, bitwise reproducible), the fp32[8] control block it
// leaves on the device, and the AdamW update that obeys it (clip coefficient, skip-if-non-finite, hold) -- every decision is taken on the
// device, so the whole sequence can sit inside a captured hipGraph.  Gradient accumulation adds a phase to the same block: lavt_grad_accumulate folds
// a micro-batch's flat gradient into a second flat buffer and sets ctl[5] while the cycle is open; norm, update and tick then do nothing but count the
// micro-step (ctl[6]).
#include "common.h"
#include "adamw_body.h"

namespace {

// Pass 1: workgroup c = chunk c of the update's own chunk table -> ws[c] = sum of squares of the chunk's gradient elements (fp32).
// Whole aligned chunks: 8 float4 loads per thread, all issued before the first use; every thread then adds its 32 squares in order, the
// wave reduces with shuffles (6 levels), the 4 waves meet through LDS (2 levels).
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const int64_t* __restrict__ desc, const int2* __restrict__ chunks, float* __restrict__ ws,
                                                                const float* __restrict__ ctl) {
    __shared__ float red[4];
    if (ctl[5] != 0.f) return;                 // an accumulating micro-step: the norm of the last applied cycle stays (wave-uniform, before the first load)
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
// LDS) and lane 0 writes ctl[0..2].  ctl[3] (skipped-step count) belongs to the guarded tick, ctl[4] (hold) to the host, ctl[5] (accumulating) to
// lavt_grad_accumulate: while it is set, ctl[0..2] keep the values of the last applied cycle.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const float* __restrict__ ws, int nchunks, float* __restrict__ ctl, float max_norm, int skip_nonfinite) {
    __shared__ double red[256];
    if (ctl[5] != 0.f) return;
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

// Weight EMA (adamw_body.h: EMA): the same body with the average's stream behind `ema`; vmax is read only with AMSGRAD, ctl only with GUARD
template <bool GUARD, bool AMSGRAD>
__global__ __launch_bounds__(256) void adamw_chunks_ema_kernel(const int64_t* __restrict__ desc, const int64_t* __restrict__ vmax, const int64_t* __restrict__ ema,
                                                               const float* __restrict__ hyper, const int2* __restrict__ chunks, const float* __restrict__ step,
                                                               float total_steps, float power, float decay, const float* __restrict__ ctl) {
    adamw_chunk_update<GUARD, AMSGRAD, true>(desc, vmax, hyper, chunks, step, total_steps, power, ctl, ema, decay);
}

// In-place exchange of p and e over the update's chunk table: workgroup c swaps elements [chunk * CE, (chunk + 1) * CE) of tensor chunks[c].x, every
// element is read and written by exactly one thread.  A bf16 compute copy (desc[.][5]) is written from the registers that hold the new p, as the
// update writes it.  Whole aligned chunks: two rounds of 4 float4 loads per stream and thread, a round's loads all issued before its first store.
__global__ __launch_bounds__(256) void ema_swap_kernel(const int64_t* __restrict__ desc, const int64_t* __restrict__ ema, const int2* __restrict__ chunks) {
    const int2 ch = chunks[blockIdx.x];
    const int t = ch.x;
    float* p = reinterpret_cast<float*>(desc[6 * t]);
    float* e = reinterpret_cast<float*>(ema[t]);
    const int64_t n = desc[6 * t + 4];
    bf16* cp = reinterpret_cast<bf16*>(desc[6 * t + 5]);
    const int64_t e0 = (int64_t)ch.y * ADAMW_CE, e1 = min(n, e0 + ADAMW_CE);
    const bool vec = ((desc[6 * t] | ema[t]) & 15) == 0 && (desc[6 * t + 5] & 7) == 0;
    if (vec && e1 - e0 == ADAMW_CE) {
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            float4 pp[4], ee[4];
            const int64_t base = e0 + (int64_t)round * 4096 + threadIdx.x * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                pp[u] = *reinterpret_cast<const float4*>(p + base + u * 1024); ee[u] = *reinterpret_cast<const float4*>(e + base + u * 1024);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = base + u * 1024;
                *reinterpret_cast<float4*>(p + i) = ee[u]; *reinterpret_cast<float4*>(e + i) = pp[u];
                if (cp) *reinterpret_cast<uint2*>(cp + i) = make_uint2(pack_bf16x2(ee[u].x, ee[u].y), pack_bf16x2(ee[u].z, ee[u].w));
            }
        }
    } else {                                   // a tensor's last chunk / unaligned tensors
        for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) {
            const float pv = p[i], ev = e[i];
            p[i] = ev; e[i] = pv;
            if (cp) cp[i] = from_f<bf16>(ev);
        }
    }
}

// the step counter advances only when the update ran; a skipped step is counted unless the optimizer is on hold.  Gradient accumulation: the tick is
// the last reader of the phase in a step, so it is also the one that moves the micro index -- an accumulating micro-step (ctl[5], set by
// lavt_grad_accumulate from m != k - 1) counts m up and nothing else (ctl[2] is the LAST cycle's skip flag then), the step that ends a cycle puts
// m back to 0: together (m + 1) % k.  Without accumulation ctl[5] and ctl[6] are 0 and stay 0.
__global__ void adamw_tick_guarded_kernel(float* step, float* ctl) {
    const float skip = ctl[2], hold = ctl[4], accumulating = ctl[5];
    if (hold != 0.f) return;
    if (accumulating != 0.f) {
        ctl[6] += 1.f;
        return;
    }
    if (skip == 0.f) step[0] += 1.f;
    ctl[3] += skip;
    ctl[6] = 0.f;
}

// One micro-batch's flat gradient folded into the accumulation buffer: acc = s * g on the first micro-step of a cycle (m == 0: SELECT, acc is never
// read -- whatever an earlier cycle left there, a NaN included, is gone and the buffer needs no zero fill), acc = fma(s, g, acc) on the others; s = 1 / k.
// hold (ctl[4]) and m (ctl[6]) are wave-uniform and read once per thread before the loop; nothing in this launch writes them.  Streaming, grid-stride,
// no atomics: every element is read and written by exactly one thread, so the result is bitwise reproducible.  Thread 0 of workgroup 0 leaves the
// phase for the kernels behind: ctl[5] = (m != k - 1).
// FIRST: acc is not read.  VEC: both bases 16-byte aligned -- float4 accesses over the first n / 4 * 4 elements, four independent loads of each
// stream in flight per thread before the first use; the n % 4 tail and unaligned bases go element by element.
template <bool FIRST, bool VEC>
__device__ __forceinline__ void grad_fold(const float* __restrict__ g, float* __restrict__ acc, int64_t n, float s, int64_t tid, int64_t stride) {
    auto sel4 = [&](float4 gg) { return make_float4(s * gg.x, s * gg.y, s * gg.z, s * gg.w); };
    auto fma4 = [&](float4 gg, float4 aa) { return make_float4(fmaf(s, gg.x, aa.x), fmaf(s, gg.y, aa.y), fmaf(s, gg.z, aa.z), fmaf(s, gg.w, aa.w)); };
    int64_t done = 0;                          // elements covered by the float4 part
    if constexpr (VEC) {
        const int64_t n4 = n >> 2;
        const float4* g4 = reinterpret_cast<const float4*>(g);
        float4* a4 = reinterpret_cast<float4*>(acc);
        // whole tiles of 1024 float4 per workgroup and trip: the four accesses of a thread lie at constant distances (256 float4) from each other
        const int64_t tiles = n4 >> 10;
        for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int64_t base = (t << 10) + threadIdx.x;
            float4 gg[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) gg[u] = g4[base + u * 256];
            if constexpr (FIRST) {
#pragma unroll
                for (int u = 0; u < 4; ++u) a4[base + u * 256] = sel4(gg[u]);
            } else {
                float4 aa[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) aa[u] = a4[base + u * 256];
#pragma unroll
                for (int u = 0; u < 4; ++u) a4[base + u * 256] = fma4(gg[u], aa[u]);
            }
        }
        int64_t i = (tiles << 10) + tid;       // the float4 behind the last whole tile
        for (; i < n4; i += stride) {
            if constexpr (FIRST) a4[i] = sel4(g4[i]);
            else a4[i] = fma4(g4[i], a4[i]);
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += stride) {
        if constexpr (FIRST) acc[i] = s * g[i];
        else acc[i] = fmaf(s, g[i], acc[i]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(const float* __restrict__ g, float* __restrict__ acc, int64_t n, float s, float last, float* __restrict__ ctl) {
    if (ctl[4] != 0.f) return;
    const float m = ctl[6];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (m == 0.f) grad_fold<true, VEC>(g, acc, n, s, tid, stride);
    else grad_fold<false, VEC>(g, acc, n, s, tid, stride);
    if (tid == 0) ctl[5] = m < last ? 1.f : 0.f;
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int64_t lavt_grad_norm_ws(int nchunks) { return nchunks > 0 ? (int64_t)nchunks : 0; }

extern "C" int lavt_grad_norm(const int64_t* desc, const int32_t* chunks, int nchunks, float* ws, float* ctl, float max_norm, int skip_nonfinite, void* stream) {
    LAVT_CHECK_ARG(desc && chunks && ws && ctl && nchunks > 0, "lavt_grad_norm: bad arguments");
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(nchunks), dim3(256), 0, ST, desc, reinterpret_cast<const int2*>(chunks), ws, ctl);
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

extern "C" int lavt_adamw_step_chunks_ema(const int64_t* desc, const int64_t* vmax, const int64_t* ema, const float* hyper, const int32_t* chunks, int nchunks, float* step,
                                          float total_steps, float power, float decay, float* ctl, void* stream) {
    LAVT_CHECK_ARG(desc && ema && hyper && chunks && step && nchunks > 0, "lavt_adamw_step_chunks_ema: bad arguments");
    LAVT_CHECK_ARG(decay > 0.f && decay < 1.f, "lavt_adamw_step_chunks_ema: the decay must lie in (0, 1)");
    const int2* ch = reinterpret_cast<const int2*>(chunks);
    const dim3 grid(nchunks), block(256);
    if (ctl) {
        if (vmax) hipLaunchKernelGGL((adamw_chunks_ema_kernel<true, true>), grid, block, 0, ST, desc, vmax, ema, hyper, ch, step, total_steps, power, decay, ctl);
        else hipLaunchKernelGGL((adamw_chunks_ema_kernel<true, false>), grid, block, 0, ST, desc, nullptr, ema, hyper, ch, step, total_steps, power, decay, ctl);
        hipLaunchKernelGGL(adamw_tick_guarded_kernel, dim3(1), dim3(1), 0, ST, step, ctl);
    } else {
        if (vmax) hipLaunchKernelGGL((adamw_chunks_ema_kernel<false, true>), grid, block, 0, ST, desc, vmax, ema, hyper, ch, step, total_steps, power, decay, nullptr);
        else hipLaunchKernelGGL((adamw_chunks_ema_kernel<false, false>), grid, block, 0, ST, desc, nullptr, ema, hyper, ch, step, total_steps, power, decay, nullptr);
        hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, ST, step);
    }
    LAVT_CHECK_LAUNCH("lavt_adamw_step_chunks_ema");
    return LAVT_OK;
}

extern "C" int lavt_ema_swap(const int64_t* desc, const int64_t* ema, const int32_t* chunks, int nchunks, void* stream) {
    LAVT_CHECK_ARG(desc && ema && chunks && nchunks > 0, "lavt_ema_swap: bad arguments");
    hipLaunchKernelGGL(ema_swap_kernel, dim3(nchunks), dim3(256), 0, ST, desc, ema, reinterpret_cast<const int2*>(chunks));
    LAVT_CHECK_LAUNCH("lavt_ema_swap");
    return LAVT_OK;
}

extern "C" int lavt_grad_accumulate(const float* g, float* acc, int64_t n, int k, float* ctl, void* stream) {
    LAVT_CHECK_ARG(g && acc && ctl && n > 0 && k >= 1 && k <= (1 << 20), "lavt_grad_accumulate: bad arguments (n > 0, 1 <= k <= 2^20)");
    LAVT_CHECK_ARG(g + n <= acc || acc + n <= g, "lavt_grad_accumulate: g and acc overlap");
    const float s = 1.f / (float)k, last = (float)(k - 1);
    const bool vec = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(acc)) & 15) == 0 && n >= 4;
    // memory-bound: at most 2048 workgroups (8 per CU), each thread 4 float4 per stream and trip; the grid-stride loop takes the rest
    const int64_t work = vec ? (n >> 2) : n, per_wg = vec ? 256 * 4 : 256;
    const int grid = (int)std::min<int64_t>(2048, (work + per_wg - 1) / per_wg);
    if (vec) hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3(grid), dim3(256), 0, ST, g, acc, n, s, last, ctl);
    else hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3(grid), dim3(256), 0, ST, g, acc, n, s, last, ctl);
    LAVT_CHECK_LAUNCH("lavt_grad_accumulate");
    return LAVT_OK;
}
