// The optimizer step, all of it: the multi-tensor AdamW update (per tensor, and over a chunk table with its GUARD / AMSGRAD / EMA forms), the ticks of
// the device step counter, the guard around it -- global gradient norm (two launches, no atomics, bitwise reproducible), the per-tensor norms, the
// fp32[8] control block they leave on the device (include/lavt_hip.h: LAVT_CTL_*), which the update obeys (clip coefficient, skip-if-non-finite, hold) --
// the fold of gradient accumulation and the swap of the weight average.  Every decision is taken on the device, so the whole sequence can sit inside
// a captured hipGraph.  Gradient accumulation adds a phase to the same block: lavt_grad_accumulate folds a micro-batch's flat gradient into a second
// flat buffer and sets ctl[5] while the cycle is open; norm, update and tick then do nothing but count the micro-step (ctl[6]).
#include "common.h"
#include "optim_protocol.h"

#define GRID_STRIDE(i, n) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

namespace {

constexpr int ADAMW_CE = 8192;            // elements per chunk: 256 threads x 2 rounds x 4 float4

// column `col` (LAVT_ADAMW_DESC_* / LAVT_ADAMW_HYPER_*) of row t of the chunked update's two tables
__device__ __forceinline__ int64_t desc_col(const int64_t* desc, int t, int col) { return desc[LAVT_ADAMW_DESC_COLS * t + col]; }
__device__ __forceinline__ float hyper_col(const float* hyper, int t, int col) { return hyper[LAVT_ADAMW_HYPER_COLS * t + col]; }

// ---- multi-tensor AdamW with the poly learning-rate schedule of the caller (train.py:688-700: torch.optim.AdamW + LambdaLR((1 - it/T)^0.9)).
// One launch for the whole parameter list: blockIdx.y = tensor, descriptor {param, grad, exp_avg, exp_avg_sq, numel} (fp32 pointers),
// per-tensor hyper-parameters {base_lr, weight_decay, beta1, beta2, eps}.  The step counter lives on the device (incremented by
// adamw_tick_kernel), so the optimizer step can be part of the captured hipGraph and still advance its schedule on every replay.
__global__ __launch_bounds__(256) void adamw_multi_kernel(const int64_t* __restrict__ desc, const float* __restrict__ hyper, int count,
                                                          const float* __restrict__ step, float total_steps, float power) {
    const int t = blockIdx.y;
    if (t >= count) return;
    float* p = reinterpret_cast<float*>(desc[5 * t]);
    const float* g = reinterpret_cast<const float*>(desc[5 * t + 1]);
    float* m = reinterpret_cast<float*>(desc[5 * t + 2]);
    float* v = reinterpret_cast<float*>(desc[5 * t + 3]);
    const int64_t n = desc[5 * t + 4];
    const float b1 = hyper[5 * t + 2], b2 = hyper[5 * t + 3], eps = hyper[5 * t + 4], wd = hyper[5 * t + 1];
    const float k = step[0];                                       // optimizer steps taken so far
    const float sched = total_steps > 0.f ? powf(fmaxf(1.f - k / total_steps, 0.f), power) : 1.f;
    const float lr = hyper[5 * t] * sched;
    const float bc1 = 1.f - powf(b1, k + 1.f), bc2 = 1.f - powf(b2, k + 1.f);
    const float step_size = lr / bc1, rbc2 = rsqrtf(bc2), decay = 1.f - lr * wd;
    auto upd = [&](float& pp, float gg, float& mm, float& vv) {
        pp *= decay;
        mm = b1 * mm + (1.f - b1) * gg;
        vv = b2 * vv + (1.f - b2) * gg * gg;
        pp -= step_size * mm / (sqrtf(vv) * rbc2 + eps);
    };
    const bool vec = ((desc[5 * t] | desc[5 * t + 1] | desc[5 * t + 2] | desc[5 * t + 3]) & 15) == 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        GRID_STRIDE(i, n4) {
            float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            upd(pp.x, gg.x, mm.x, vv.x); upd(pp.y, gg.y, mm.y, vv.y); upd(pp.z, gg.z, mm.z, vv.z); upd(pp.w, gg.w, mm.w, vv.w);
            reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
        }
        for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) upd(p[i], g[i], m[i], v[i]);
    } else {
        GRID_STRIDE(i, n) upd(p[i], g[i], m[i], v[i]);
    }
}
__global__ void adamw_tick_kernel(float* step) { step[0] += 1.f; }          // the unguarded tick

// ---- the same update over a CHUNK table: one kernel, GUARD / AMSGRAD / EMA select what surrounds the four-stream update, so the forms cannot drift.
// Workgroup c updates elements [chunk * CE, (chunk + 1) * CE) of tensor chunks[c].x -- every workgroup has work
// (a per-tensor grid launches 256 workgroups per tensor: ~100 000 of them find nothing to do for the ~400 small tensors of a Swin-B LAVT)
// and all of a thread's loads are issued before the first use.  desc: int64 [count][6] = {param, grad, exp_avg, exp_avg_sq, numel, copy}: a
// non-zero `copy` is the parameter's bf16 compute copy in the same layout (Linear / 1x1 weights), written from the registers that hold the
// updated value -- the separate re-cast pass (a second read of every parameter) disappears.
// GUARD: ctl is the fp32[8] control block of lavt_grad_norm (wave-uniform, read once per workgroup): the workgroup returns before its first
// store when ctl[2] (skip), ctl[4] (hold) or ctl[5] (accumulating: lavt_grad_accumulate, this micro-step does not end its cycle) is set, and gradients are scaled by ctl[1] (the clip coefficient; x * 1.0f is exact, so a
// coefficient of 1 gives the unguarded bits).  With GUARD off, ctl is never read.
// AMSGRAD: a fifth fp32 stream x = max_exp_avg_sq, addressed by vmax: int64 [count], one pointer per desc row (desc keeps its six columns: the norm
// kernel and the plain entry points read that layout).  torch.optim.AdamW(amsgrad=True), single-tensor form: x = max(x, v) with the UNcorrected v
// after its update, and x takes v's place in the denominator.  With AMSGRAD off, vmax is never read and the code is the four-stream update.
// EMA: one more fp32 stream e = the exponential moving average of the parameter, addressed by ema: int64 [count] exactly as vmax addresses x; the decay d
// is optimizer-wide.  torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)), applied after the parameter update from the registers
// that hold the new p: the first applied update (step counter 0) copies, e = p; every later one is e += (1 - d) * (p - e).  e is loaded with the other
// streams and stored next to m and v, so GUARD's early return covers it: a skipped, held or accumulating step leaves the average alone, as it leaves the
// moments.  With EMA off, ema and ema_decay are never read and the code is the four- / five-stream update.
template <bool GUARD, bool AMSGRAD, bool EMA>
__global__ __launch_bounds__(256) void adamw_update_kernel(const int64_t* __restrict__ desc, const int64_t* __restrict__ vmax, const int64_t* __restrict__ ema,
                                                           const float* __restrict__ hyper, const int2* __restrict__ chunks, const float* __restrict__ step,
                                                           float total_steps, float power, float ema_decay, const float* __restrict__ ctl) {
    float coef = 1.f;
    if constexpr (GUARD) {
        if (ctl_update_blocked(ctl)) return;
        coef = ctl[LAVT_CTL_CLIP];
    }
    const int2 ch = chunks[blockIdx.x];
    const int t = ch.x;
    float* p = reinterpret_cast<float*>(desc_col(desc, t, LAVT_ADAMW_DESC_PARAM));
    const float* g = reinterpret_cast<const float*>(desc_col(desc, t, LAVT_ADAMW_DESC_GRAD));
    float* m = reinterpret_cast<float*>(desc_col(desc, t, LAVT_ADAMW_DESC_EXP_AVG));
    float* v = reinterpret_cast<float*>(desc_col(desc, t, LAVT_ADAMW_DESC_EXP_AVG_SQ));
    const int64_t n = desc_col(desc, t, LAVT_ADAMW_DESC_NUMEL);
    bf16* cp = reinterpret_cast<bf16*>(desc_col(desc, t, LAVT_ADAMW_DESC_COPY));
    const float b1 = hyper_col(hyper, t, LAVT_ADAMW_HYPER_BETA1), b2 = hyper_col(hyper, t, LAVT_ADAMW_HYPER_BETA2), eps = hyper_col(hyper, t, LAVT_ADAMW_HYPER_EPS),
                wd = hyper_col(hyper, t, LAVT_ADAMW_HYPER_WEIGHT_DECAY);
    const float k = step[0];
    const float sched = poly_lr_factor(k, total_steps, power);
    const float lr = hyper_col(hyper, t, LAVT_ADAMW_HYPER_LR) * sched;
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
    bool vec = ((desc_col(desc, t, LAVT_ADAMW_DESC_PARAM) | desc_col(desc, t, LAVT_ADAMW_DESC_GRAD) | desc_col(desc, t, LAVT_ADAMW_DESC_EXP_AVG) |
                 desc_col(desc, t, LAVT_ADAMW_DESC_EXP_AVG_SQ)) & 15) == 0 && (desc_col(desc, t, LAVT_ADAMW_DESC_COPY) & 7) == 0;
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

// the step counter advances only when the update ran; a skipped step is counted unless the optimizer is on hold.  Gradient accumulation: the tick is
// the last reader of the phase in a step, so it is also the one that moves the micro index -- an accumulating micro-step (ctl[5], set by
// lavt_grad_accumulate from m != k - 1) counts m up and nothing else (ctl[2] is the LAST cycle's skip flag then), the step that ends a cycle puts
// m back to 0: together (m + 1) % k.  Without accumulation ctl[5] and ctl[6] are 0 and stay 0.
__global__ void adamw_tick_guarded_kernel(float* step, float* ctl) {
    const float skip = ctl[LAVT_CTL_SKIP], hold = ctl[LAVT_CTL_HOLD], accumulating = ctl[LAVT_CTL_ACCUMULATING];
    if (hold != 0.f) return;
    if (accumulating != 0.f) {
        ctl[LAVT_CTL_MICRO] += 1.f;
        return;
    }
    if (skip == 0.f) step[0] += 1.f;
    ctl[LAVT_CTL_SKIPPED] += skip;
    ctl[LAVT_CTL_MICRO] = 0.f;
}

// Pass 1: workgroup c = chunk c of the update's own chunk table -> ws[c] = sum of squares of the chunk's gradient elements (fp32).
// Whole aligned chunks: 8 float4 loads per thread, all issued before the first use; every thread then adds its 32 squares in order, the
// wave reduces with shuffles (6 levels), the 4 waves meet through LDS (2 levels).
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const int64_t* __restrict__ desc, const int2* __restrict__ chunks, float* __restrict__ ws,
                                                                const float* __restrict__ ctl) {
    __shared__ float red[4];
    // an accumulating micro-step: the norm of the last applied cycle stays (wave-uniform, before the first load).  Accumulating ONLY, not
    // ctl_cycle_open: under hold the norm is still computed and written.
    if (ctl[LAVT_CTL_ACCUMULATING] != 0.f) return;
    const int2 ch = chunks[blockIdx.x];
    const float* g = reinterpret_cast<const float*>(desc_col(desc, ch.x, LAVT_ADAMW_DESC_GRAD));
    const int64_t n = desc_col(desc, ch.x, LAVT_ADAMW_DESC_NUMEL);
    const int64_t e0 = (int64_t)ch.y * ADAMW_CE, e1 = min(n, e0 + ADAMW_CE);
    float acc = 0.f;
    if ((desc_col(desc, ch.x, LAVT_ADAMW_DESC_GRAD) & 15) == 0 && e1 - e0 == ADAMW_CE) {
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
    if (ctl[LAVT_CTL_ACCUMULATING] != 0.f) return;          // (accumulating only, as in pass 1)
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
        ctl[LAVT_CTL_NORM] = norm;
        ctl[LAVT_CTL_CLIP] = (max_norm > 0.f && finite) ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;      // torch.nn.utils.clip_grad_norm_'s coefficient
        ctl[LAVT_CTL_SKIP] = (skip_nonfinite && !finite) ? 1.f : 0.f;
    }
}

// Per-tensor sums of squares from pass 1's partials.  One workgroup of 16 waves; wave w takes tensors w, w + 16, ...  Lane l adds its tensor's partials
// first[t] + l, + 64, ... in sequence in fp64, the wave
// reduces with a fixed xor tree: a fixed order, bit-reproducible.  Four tensors per trip: their table entries, then the first partial of each lane for
// all four, are loaded before the first is used (most tensors have at most 64 chunks, so that is all of them).  A sum of squares is non-finite exactly
// when one of its fp32 partials is (they are >= 0, NaN or +Inf, and fp64 cannot overflow over them).
constexpr int TN_WAVES = 16, TN_BATCH = 4;
__global__ __launch_bounds__(TN_WAVES * 64) void grad_norm_tensors_kernel(const float* __restrict__ ws, int nchunks, const int32_t* __restrict__ first, int count,
                                                                          const float* __restrict__ ctl, double* __restrict__ out, int32_t* __restrict__ bad) {
    __shared__ int s_first[TN_WAVES], s_count[TN_WAVES];
    if (ctl_cycle_open(ctl)) return;          // hold / an accumulating micro-step: before any store (block-uniform); out and bad keep the last cycle's
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int sticky = bad[2];
    int my_first = INT32_MAX, my_count = 0;
    for (int t0 = w; t0 < count; t0 += TN_WAVES * TN_BATCH) {
        int a[TN_BATCH], b[TN_BATCH];
        float v[TN_BATCH];
#pragma unroll
        for (int u = 0; u < TN_BATCH; ++u) {
            const int t = t0 + u * TN_WAVES;
            a[u] = t < count ? max(first[t], 0) : 0;
            b[u] = t < count ? min(first[t + 1], nchunks) : 0;
        }
#pragma unroll
        for (int u = 0; u < TN_BATCH; ++u) v[u] = a[u] + lane < b[u] ? ws[a[u] + lane] : 0.f;
#pragma unroll
        for (int u = 0; u < TN_BATCH; ++u) {
            const int t = t0 + u * TN_WAVES;
            if (t >= count) break;          // (wave-uniform)
            double acc = (double)v[u];
            // a tensor of more than 64 chunks (a 3x3 convolution weight has hundreds): eight loads in flight per lane, added in the same index order
            int i = a[u] + 64 + lane;
            for (; i + 7 * 64 < b[u]; i += 8 * 64) {
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = ws[i + j * 64];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc += (double)x[j];
            }
            for (; i < b[u]; i += 64) acc += (double)ws[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (lane == 0) out[t] = acc;
            if (!isfinite(acc)) {
                my_first = min(my_first, t);
                my_count += 1;
            }
        }
    }
    if (lane == 0) { s_first[w] = my_first; s_count[w] = my_count; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int f = INT32_MAX, c = 0;
#pragma unroll
        for (int i = 0; i < TN_WAVES; ++i) { f = min(f, s_first[i]); c += s_count[i]; }
        bad[0] = c ? f : -1;
        bad[1] = c;
        bad[2] = c ? f : sticky;
    }
}

// In-place exchange of p and e over the update's chunk table: workgroup c swaps elements [chunk * CE, (chunk + 1) * CE) of tensor chunks[c].x, every
// element is read and written by exactly one thread.  A bf16 compute copy (desc[.][5]) is written from the registers that hold the new p, as the
// update writes it.  Whole aligned chunks: two rounds of 4 float4 loads per stream and thread, a round's loads all issued before its first store.
__global__ __launch_bounds__(256) void ema_swap_kernel(const int64_t* __restrict__ desc, const int64_t* __restrict__ ema, const int2* __restrict__ chunks) {
    const int2 ch = chunks[blockIdx.x];
    const int t = ch.x;
    float* p = reinterpret_cast<float*>(desc_col(desc, t, LAVT_ADAMW_DESC_PARAM));
    float* e = reinterpret_cast<float*>(ema[t]);
    const int64_t n = desc_col(desc, t, LAVT_ADAMW_DESC_NUMEL);
    bf16* cp = reinterpret_cast<bf16*>(desc_col(desc, t, LAVT_ADAMW_DESC_COPY));
    const int64_t e0 = (int64_t)ch.y * ADAMW_CE, e1 = min(n, e0 + ADAMW_CE);
    const bool vec = ((desc_col(desc, t, LAVT_ADAMW_DESC_PARAM) | ema[t]) & 15) == 0 && (desc_col(desc, t, LAVT_ADAMW_DESC_COPY) & 7) == 0;
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
    if (ctl[LAVT_CTL_HOLD] != 0.f) return;          // hold ONLY, not ctl_cycle_open: this launch is the writer of accumulating
    const float m = ctl[LAVT_CTL_MICRO];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (m == 0.f) grad_fold<true, VEC>(g, acc, n, s, tid, stride);
    else grad_fold<false, VEC>(g, acc, n, s, tid, stride);
    if (tid == 0) ctl[LAVT_CTL_ACCUMULATING] = m < last ? 1.f : 0.f;
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

// The chunked update and the tick that belongs to it, for all four entry points: the instantiation follows from which tables the caller gave --
// ctl (GUARD, and the guarded tick), vmax (AMSGRAD), ema (EMA); a table that is absent is never read.
static void launch_adamw_update(const int64_t* desc, const int64_t* vmax, const int64_t* ema, const float* hyper, const int32_t* chunks, int nchunks, float* step,
                                float total_steps, float power, float decay, float* ctl, void* stream) {
    static constexpr decltype(&adamw_update_kernel<false, false, false>) kernels[2][2][2] = {          // [GUARD][AMSGRAD][EMA]
        {{adamw_update_kernel<false, false, false>, adamw_update_kernel<false, false, true>}, {adamw_update_kernel<false, true, false>, adamw_update_kernel<false, true, true>}},
        {{adamw_update_kernel<true, false, false>, adamw_update_kernel<true, false, true>}, {adamw_update_kernel<true, true, false>, adamw_update_kernel<true, true, true>}}};
    hipLaunchKernelGGL(kernels[ctl != nullptr][vmax != nullptr][ema != nullptr], dim3(nchunks), dim3(256), 0, ST, desc, vmax, ema, hyper, reinterpret_cast<const int2*>(chunks), step, total_steps, power, decay, ctl);
    if (ctl) hipLaunchKernelGGL(adamw_tick_guarded_kernel, dim3(1), dim3(1), 0, ST, step, ctl);
    else hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, ST, step);
}

extern "C" int lavt_adamw_step(const int64_t* desc, const float* hyper, int count, float* step, float total_steps, float power, void* stream) {
    LAVT_CHECK_ARG(desc && hyper && step && count > 0, "lavt_adamw_step: bad arguments");
    hipLaunchKernelGGL(adamw_multi_kernel, dim3(256, count), dim3(256), 0, ST, desc, hyper, count, step, total_steps, power);      // small tensors: surplus workgroups exit at once
    hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, ST, step);
    LAVT_CHECK_LAUNCH("lavt_adamw_step");
    return LAVT_OK;
}

extern "C" int lavt_adamw_chunk_elems(void) { return ADAMW_CE; }
extern "C" int lavt_adamw_step_chunks(const int64_t* desc, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps, float power, void* stream) {
    LAVT_CHECK_ARG(desc && hyper && chunks && step && nchunks > 0, "lavt_adamw_step_chunks: bad arguments");
    launch_adamw_update(desc, nullptr, nullptr, hyper, chunks, nchunks, step, total_steps, power, 0.f, nullptr, stream);
    LAVT_CHECK_LAUNCH("lavt_adamw_step_chunks");
    return LAVT_OK;
}

extern "C" int64_t lavt_grad_norm_ws(int nchunks) { return nchunks > 0 ? (int64_t)nchunks : 0; }

extern "C" int lavt_grad_norm(const int64_t* desc, const int32_t* chunks, int nchunks, float* ws, float* ctl, float max_norm, int skip_nonfinite, void* stream) {
    LAVT_CHECK_ARG(desc && chunks && ws && ctl && nchunks > 0, "lavt_grad_norm: bad arguments");
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(nchunks), dim3(256), 0, ST, desc, reinterpret_cast<const int2*>(chunks), ws, ctl);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, ST, ws, nchunks, ctl, max_norm, skip_nonfinite);
    LAVT_CHECK_LAUNCH("lavt_grad_norm");
    return LAVT_OK;
}

extern "C" int lavt_grad_norm_tensors(const float* ws, int nchunks, const int32_t* first, int count, const float* ctl, double* out, int32_t* bad, void* stream) {
    LAVT_CHECK_ARG(ws && first && ctl && out && bad && nchunks > 0 && count > 0, "lavt_grad_norm_tensors: bad arguments");
    hipLaunchKernelGGL(grad_norm_tensors_kernel, dim3(1), dim3(TN_WAVES * 64), 0, ST, ws, nchunks, first, count, ctl, out, bad);
    LAVT_CHECK_LAUNCH("lavt_grad_norm_tensors");
    return LAVT_OK;
}

extern "C" int lavt_adamw_step_chunks_guarded(const int64_t* desc, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps, float power,
                                              float* ctl, void* stream) {
    LAVT_CHECK_ARG(desc && hyper && chunks && step && ctl && nchunks > 0, "lavt_adamw_step_chunks_guarded: bad arguments");
    launch_adamw_update(desc, nullptr, nullptr, hyper, chunks, nchunks, step, total_steps, power, 0.f, ctl, stream);
    LAVT_CHECK_LAUNCH("lavt_adamw_step_chunks_guarded");
    return LAVT_OK;
}

extern "C" int lavt_adamw_step_chunks_amsgrad(const int64_t* desc, const int64_t* vmax, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps,
                                              float power, float* ctl, void* stream) {
    LAVT_CHECK_ARG(desc && vmax && hyper && chunks && step && nchunks > 0, "lavt_adamw_step_chunks_amsgrad: bad arguments");
    launch_adamw_update(desc, vmax, nullptr, hyper, chunks, nchunks, step, total_steps, power, 0.f, ctl, stream);
    LAVT_CHECK_LAUNCH("lavt_adamw_step_chunks_amsgrad");
    return LAVT_OK;
}

extern "C" int lavt_adamw_step_chunks_ema(const int64_t* desc, const int64_t* vmax, const int64_t* ema, const float* hyper, const int32_t* chunks, int nchunks, float* step,
                                          float total_steps, float power, float decay, float* ctl, void* stream) {
    LAVT_CHECK_ARG(desc && ema && hyper && chunks && step && nchunks > 0, "lavt_adamw_step_chunks_ema: bad arguments");
    LAVT_CHECK_ARG(decay > 0.f && decay < 1.f, "lavt_adamw_step_chunks_ema: the decay must lie in (0, 1)");
    launch_adamw_update(desc, vmax, ema, hyper, chunks, nchunks, step, total_steps, power, decay, ctl, stream);
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
