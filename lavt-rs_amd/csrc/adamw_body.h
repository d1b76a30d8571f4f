// The chunked multi-tensor AdamW update, shared by the plain kernel (elementwise.hip: adamw_chunks_kernel) and the guarded one
// (optim_guard.hip: adamw_chunks_guarded_kernel) so that the two cannot drift: one body, GUARD selects what surrounds it.
#pragma once
#include "common.h"

constexpr int ADAMW_CE = 8192;            // elements per chunk: 256 threads x 2 rounds x 4 float4

// Workgroup c updates elements [chunk * CE, (chunk + 1) * CE) of tensor chunks[c].x -- every workgroup has work
// (a per-tensor grid launches 256 workgroups per tensor: ~100 000 of them find nothing to do for the ~400 small tensors of a Swin-B LAVT)
// and all of a thread's loads are issued before the first use.  desc: int64 [count][6] = {param, grad, exp_avg, exp_avg_sq, numel, copy}: a
// non-zero `copy` is the parameter's bf16 compute copy in the same layout (Linear / 1x1 weights), written from the registers that hold the
// updated value -- the separate re-cast pass (a second read of every parameter) disappears.
// GUARD: ctl is the fp32[8] control block of lavt_grad_norm (wave-uniform, read once per workgroup): the workgroup returns before its first
// store when ctl[2] (skip), ctl[4] (hold) or ctl[5] (accumulating: lavt_grad_accumulate, this micro-step does not end its cycle) is set, and gradients are scaled by ctl[1] (the clip coefficient; x * 1.0f is exact, so a
// coefficient of 1 gives the unguarded bits).
// AMSGRAD: a fifth fp32 stream x = max_exp_avg_sq, addressed by vmax: int64 [count], one pointer per desc row (desc keeps its six columns: the norm
// kernel and the plain entry points read that layout).  torch.optim.AdamW(amsgrad=True), single-tensor form: x = max(x, v) with the UNcorrected v
// after its update, and x takes v's place in the denominator.  With AMSGRAD off, vmax is never read and the code is the four-stream update.
// EMA: one more fp32 stream e = the exponential moving average of the parameter, addressed by ema: int64 [count] exactly as vmax addresses x; the decay d
// is optimizer-wide.  torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)), applied after the parameter update from the registers
// that hold the new p: the first applied update (step counter 0) copies, e = p; every later one is e += (1 - d) * (p - e).  e is loaded with the other
// streams and stored next to m and v, so GUARD's early return covers it: a skipped, held or accumulating step leaves the average alone, as it leaves the
// moments.  With EMA off, ema and ema_decay are never read and the code is the four- / five-stream update.
template <bool GUARD, bool AMSGRAD, bool EMA = false>
__device__ __forceinline__ void adamw_chunk_update(const int64_t* __restrict__ desc, const int64_t* __restrict__ vmax, const float* __restrict__ hyper,
                                                   const int2* __restrict__ chunks, const float* __restrict__ step, float total_steps, float power,
                                                   const float* __restrict__ ctl, const int64_t* __restrict__ ema = nullptr, float ema_decay = 0.f) {
    float coef = 1.f;
    if constexpr (GUARD) {
        if (ctl[2] != 0.f || ctl[4] != 0.f || ctl[5] != 0.f) return;
        coef = ctl[1];
    }
    const int2 ch = chunks[blockIdx.x];
    const int t = ch.x;
    float* p = reinterpret_cast<float*>(desc[6 * t]);
    const float* g = reinterpret_cast<const float*>(desc[6 * t + 1]);
    float* m = reinterpret_cast<float*>(desc[6 * t + 2]);
    float* v = reinterpret_cast<float*>(desc[6 * t + 3]);
    const int64_t n = desc[6 * t + 4];
    bf16* cp = reinterpret_cast<bf16*>(desc[6 * t + 5]);
    const float b1 = hyper[5 * t + 2], b2 = hyper[5 * t + 3], eps = hyper[5 * t + 4], wd = hyper[5 * t + 1];
    const float k = step[0];
    const float sched = total_steps > 0.f ? powf(fmaxf(1.f - k / total_steps, 0.f), power) : 1.f;
    const float lr = hyper[5 * t] * sched;
    const float bc1 = 1.f - powf(b1, k + 1.f), bc2 = 1.f - powf(b2, k + 1.f);
    const float step_size = lr / bc1, rbc2 = rsqrtf(bc2), decay = 1.f - lr * wd;
    float unused = 0.f;                        // what the x arguments bind to when AMSGRAD is off: never read, never stored
    float* x = nullptr;
    if constexpr (AMSGRAD) x = reinterpret_cast<float*>(vmax[t]);
    float* e = nullptr;
    if constexpr (EMA) e = reinterpret_cast<float*>(ema[t]);
    const bool ema_first = k == 0.f;          // (a skipped step does not advance the counter: the first APPLIED update copies)
    const float ema_w = 1.f - ema_decay;
    auto avg = [&](float& ee, float pp) { ee = ema_first ? pp : ee + ema_w * (pp - ee); };
    auto upd = [&](float& pp, float gg, float& mm, float& vv, float& xx) {
        if constexpr (GUARD) gg *= coef;
        pp *= decay;
        mm = b1 * mm + (1.f - b1) * gg;
        vv = b2 * vv + (1.f - b2) * gg * gg;
        if constexpr (AMSGRAD) {
            xx = (vv > xx || vv != vv) ? vv : xx;          // torch.maximum: a NaN on either side stays (fmaxf would drop it)
            pp -= step_size * mm / (sqrtf(xx) * rbc2 + eps);
        } else {
            pp -= step_size * mm / (sqrtf(vv) * rbc2 + eps);
        }
    };
    const int64_t e0 = (int64_t)ch.y * ADAMW_CE, e1 = min(n, e0 + ADAMW_CE);
    bool vec = ((desc[6 * t] | desc[6 * t + 1] | desc[6 * t + 2] | desc[6 * t + 3]) & 15) == 0 && (desc[6 * t + 5] & 7) == 0;
    if constexpr (AMSGRAD) vec = vec && (vmax[t] & 15) == 0;
    if constexpr (EMA) vec = vec && (ema[t] & 15) == 0;
    if (vec && e1 - e0 == ADAMW_CE) {          // a whole chunk: no per-element conditions (a conditional load costs a branch and a full wait each)
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            float4 pp[4], gg[4], mm[4], vv[4], xx[AMSGRAD ? 4 : 1], ee[EMA ? 4 : 1];
            const int64_t base = e0 + (int64_t)round * 4096 + threadIdx.x * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = base + u * 1024;
                pp[u] = *reinterpret_cast<const float4*>(p + i); gg[u] = *reinterpret_cast<const float4*>(g + i);
                mm[u] = *reinterpret_cast<const float4*>(m + i); vv[u] = *reinterpret_cast<const float4*>(v + i);
                if constexpr (AMSGRAD) xx[u] = *reinterpret_cast<const float4*>(x + i);
                if constexpr (EMA) ee[u] = *reinterpret_cast<const float4*>(e + i);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = base + u * 1024;
                float4& xu = xx[AMSGRAD ? u : 0];          // (AMSGRAD off: bound, never read or stored)
                upd(pp[u].x, gg[u].x, mm[u].x, vv[u].x, xu.x); upd(pp[u].y, gg[u].y, mm[u].y, vv[u].y, xu.y);
                upd(pp[u].z, gg[u].z, mm[u].z, vv[u].z, xu.z); upd(pp[u].w, gg[u].w, mm[u].w, vv[u].w, xu.w);
                *reinterpret_cast<float4*>(p + i) = pp[u]; *reinterpret_cast<float4*>(m + i) = mm[u]; *reinterpret_cast<float4*>(v + i) = vv[u];
                if constexpr (AMSGRAD) *reinterpret_cast<float4*>(x + i) = xu;
                if constexpr (EMA) {
                    avg(ee[u].x, pp[u].x); avg(ee[u].y, pp[u].y); avg(ee[u].z, pp[u].z); avg(ee[u].w, pp[u].w);
                    *reinterpret_cast<float4*>(e + i) = ee[u];
                }
                if (cp) *reinterpret_cast<uint2*>(cp + i) = make_uint2(pack_bf16x2(pp[u].x, pp[u].y), pack_bf16x2(pp[u].z, pp[u].w));
            }
        }
    } else {                                   // a tensor's last chunk / unaligned tensors
        for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) {
            if constexpr (AMSGRAD) upd(p[i], g[i], m[i], v[i], x[i]);
            else upd(p[i], g[i], m[i], v[i], unused);
            if constexpr (EMA) avg(e[i], p[i]);
            if (cp) cp[i] = from_f<bf16>(p[i]);
        }
    }
}
