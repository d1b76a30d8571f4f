// Training meters that live on the device (include/lavt_hip.h "Training meters"): one small launch at the end of an iteration appends a record
// {loss, I, U, lr, grad_norm, flags, iou, it} to a ring and moves the epoch accumulators -- what the reference's training loop reads back every
// iteration (train.py:231-235, 463-477) stays on the device and follows graph replays; the host copies the block out when it wants to look.
// lavt_grad_norm_tensors: per-tensor gradient norms from the per-chunk partial sums lavt_grad_norm's first pass has already written.
// Both are latency-bound single-round launches: every load is issued before the first use.
#include "common.h"

namespace {

constexpr int HDR = LAVT_METER_HEADER_DOUBLES;

// header words (fp64), as include/lavt_hip.h numbers them
enum { H_CAPACITY = 0, H_HOLD, H_N, H_EPOCH_START, H_ITERS, H_LOSS_SUM, H_LOSS_COUNT, H_LOSS_NONFINITE, H_IOU_SUM, H_CUM_I, H_CUM_U, H_SEG0,
       H_APPLIED = H_SEG0 + 5, H_SKIPPED, H_ACCUMULATING, H_LR_SUM, H_NORM_SUM, H_NORM_COUNT };

struct meter_record {
    float loss, I, U, lr, grad_norm;
    uint32_t flags;
    double iou;
    int64_t it;
};
static_assert(sizeof(meter_record) == LAVT_METER_RECORD_BYTES, "the record layout is the contract of include/lavt_hip.h");

// One writer: lane 0 of one wave.  Launches are ordered on the stream, so no atomics; plain vector stores.
__global__ __launch_bounds__(64) void meter_append_kernel(const float* __restrict__ stats, const float* __restrict__ ctl, const float* __restrict__ step,
                                                          const float* __restrict__ hyper, float total_steps, float power, double* __restrict__ block, int capacity) {
    if (threadIdx.x != 0) return;
    // ---- every load, before the first use
    const float loss = stats[0], I = stats[2], U = stats[3];
    float c0 = 0.f, c2 = 0.f, c4 = 0.f, c5 = 0.f, k = 0.f, base_lr = 0.f;
    if (ctl) { c0 = ctl[0]; c2 = ctl[2]; c4 = ctl[4]; c5 = ctl[5]; }
    if (step) k = step[0];
    if (step && hyper) base_lr = hyper[0];
    double h[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) h[i] = block[i];
    // ---- hold: the block's own word (host-written) or the optimizer's -- nothing is stored
    if (h[H_HOLD] != 0.0 || c4 != 0.f) return;
    const double n = h[H_N];
    if (!(n >= 0.0 && n < 9.0e15) || capacity <= 0) return;          // (a block that was never initialised: no store outside it)
    const int64_t it = (int64_t)n;
    const double dI = (double)I, dU = (double)U;
    const double iou = (dI == 0.0 || dU == 0.0) ? 0.0 : dI / dU;          // train.py:64-76, in fp64
    // group 0's lr AFTER this iteration's tick (the step counter has been advanced by the update in front of this launch): adamw_body.h's expression
    float lr = 0.f;
    if (step && hyper) lr = base_lr * (total_steps > 0.f ? powf(fmaxf(1.f - k / total_steps, 0.f), power) : 1.f);
    const bool loss_ok = isfinite(loss);
    const bool accumulating = ctl && c5 != 0.f, skipped = ctl && !accumulating && c2 != 0.f, applied = step && !accumulating && !skipped;
    const uint32_t flags = (applied ? LAVT_METER_APPLIED : 0u) | (skipped ? LAVT_METER_SKIPPED : 0u) | (accumulating ? LAVT_METER_ACCUMULATING : 0u) |
                           (loss_ok ? 0u : LAVT_METER_LOSS_NONFINITE);
    meter_record* ring = reinterpret_cast<meter_record*>(block + HDR);
    meter_record r;
    r.loss = loss; r.I = I; r.U = U; r.lr = lr; r.grad_norm = ctl ? c0 : 0.f; r.flags = flags; r.iou = iou; r.it = it;
    ring[it % capacity] = r;
    // ---- the epoch accumulators, all fp64
    block[H_N] = n + 1.0;
    block[H_ITERS] = h[H_ITERS] + 1.0;
    if (loss_ok) {          // a non-finite loss is left out of the sum and counted (the ring keeps the raw value)
        block[H_LOSS_SUM] = h[H_LOSS_SUM] + (double)loss;
        block[H_LOSS_COUNT] = h[H_LOSS_COUNT] + 1.0;
    } else {
        block[H_LOSS_NONFINITE] = h[H_LOSS_NONFINITE] + 1.0;
    }
    block[H_IOU_SUM] = h[H_IOU_SUM] + iou;
    block[H_CUM_I] = h[H_CUM_I] + dI;
    block[H_CUM_U] = h[H_CUM_U] + dU;
    const double thr[5] = {0.5, 0.6, 0.7, 0.8, 0.9};
#pragma unroll
    for (int j = 0; j < 5; ++j)
        if (iou >= thr[j]) block[H_SEG0 + j] = h[H_SEG0 + j] + 1.0;
    if (applied) block[H_APPLIED] = h[H_APPLIED] + 1.0;
    if (skipped) block[H_SKIPPED] = h[H_SKIPPED] + 1.0;
    if (accumulating) block[H_ACCUMULATING] = h[H_ACCUMULATING] + 1.0;
    block[H_LR_SUM] = h[H_LR_SUM] + (double)lr;
    if (ctl && !accumulating && isfinite(c0)) {          // the norm of a cycle's gradient, once per cycle
        block[H_NORM_SUM] = h[H_NORM_SUM] + (double)c0;
        block[H_NORM_COUNT] = h[H_NORM_COUNT] + 1.0;
    }
}

// One workgroup of 16 waves; wave w takes tensors w, w + 16, ...  Lane l adds its tensor's partials first[t] + l, + 64, ... in sequence in fp64, the wave
// reduces with a fixed xor tree: a fixed order, bit-reproducible.  Four tensors per trip: their table entries, then the first partial of each lane for
// all four, are loaded before the first is used (most tensors have at most 64 chunks, so that is all of them).  A sum of squares is non-finite exactly
// when one of its fp32 partials is (they are >= 0, NaN or +Inf, and fp64 cannot overflow over them).
constexpr int TN_WAVES = 16, TN_BATCH = 4;
__global__ __launch_bounds__(TN_WAVES * 64) void grad_norm_tensors_kernel(const float* __restrict__ ws, int nchunks, const int32_t* __restrict__ first, int count,
                                                                          const float* __restrict__ ctl, double* __restrict__ out, int32_t* __restrict__ bad) {
    __shared__ int s_first[TN_WAVES], s_count[TN_WAVES];
    if (ctl[4] != 0.f || ctl[5] != 0.f) return;          // hold / an accumulating micro-step, exactly like lavt_grad_norm: before any store (block-uniform)
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

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int64_t lavt_meter_bytes(int capacity) {
    return capacity > 0 ? (int64_t)LAVT_METER_HEADER_DOUBLES * 8 + (int64_t)capacity * LAVT_METER_RECORD_BYTES : 0;
}

extern "C" int lavt_meter_append(const float* stats, const float* ctl, const float* step, const float* hyper, float total_steps, float power, void* block, int capacity,
                                 void* stream) {
    LAVT_CHECK_ARG(stats && block && capacity > 0, "lavt_meter_append: bad arguments (stats, block, capacity > 0)");
    LAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(block) & 7) == 0, "lavt_meter_append: the block must be 8-byte aligned");
    hipLaunchKernelGGL(meter_append_kernel, dim3(1), dim3(64), 0, ST, stats, ctl, step, hyper, total_steps, power, reinterpret_cast<double*>(block), capacity);
    LAVT_CHECK_LAUNCH("lavt_meter_append");
    return LAVT_OK;
}

extern "C" int lavt_grad_norm_tensors(const float* ws, int nchunks, const int32_t* first, int count, const float* ctl, double* out, int32_t* bad, void* stream) {
    LAVT_CHECK_ARG(ws && first && ctl && out && bad && nchunks > 0 && count > 0, "lavt_grad_norm_tensors: bad arguments");
    hipLaunchKernelGGL(grad_norm_tensors_kernel, dim3(1), dim3(TN_WAVES * 64), 0, ST, ws, nchunks, first, count, ctl, out, bad);
    LAVT_CHECK_LAUNCH("lavt_grad_norm_tensors");
    return LAVT_OK;
}
