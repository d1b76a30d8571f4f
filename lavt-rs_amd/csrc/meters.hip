// Training meters that live on the device (include/lavt_hip.h "Training meters"): one small launch at the end of an iteration appends a record
// {loss, I, U, lr, grad_norm, flags, iou, it} to a ring and moves the epoch accumulators -- what the reference's training loop reads back every
// iteration (train.py:231-235, 463-477) stays on the device and follows graph replays; the host copies the block out when it wants to look.
// A latency-bound single-round launch: every load is issued before the first use.  What it reads of the optimizer -- the control block's slots, the
// hyper row, the schedule -- it reads through optim_protocol.h and the LAVT_CTL_* / LAVT_ADAMW_HYPER_* names of the public header.
// The evaluation meter (include/lavt_hip.h "Evaluation meter") is its sibling behind a Predictor's mask kernel: the (I, U) rows of a prediction batch
// go into the accumulators of the reference's evaluation loop (test.py:84-108) and a ring of per-sample records.
// The hard-mask I / U pass (include/lavt_hip.h "Training meters": lavt_upsample_iu) makes the fp32[4] row the append reads for the criteria whose own
// statistics do not hold the argmax counts (mc_dice, dice_boundary): the pixel arithmetic of the cross-entropy kernel, counted in integers.
#include "internal.h"
#include "optim_protocol.h"

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
    float c_norm = 0.f, c_skip = 0.f, c_hold = 0.f, c_acc = 0.f, k = 0.f, base_lr = 0.f;
    if (ctl) { c_norm = ctl[LAVT_CTL_NORM]; c_skip = ctl[LAVT_CTL_SKIP]; c_hold = ctl[LAVT_CTL_HOLD]; c_acc = ctl[LAVT_CTL_ACCUMULATING]; }
    if (step) k = step[0];
    if (step && hyper) base_lr = hyper[LAVT_ADAMW_HYPER_LR];
    double h[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) h[i] = block[i];
    // ---- hold: the block's own word (host-written) or the optimizer's -- nothing is stored
    if (h[H_HOLD] != 0.0 || c_hold != 0.f) return;
    const double n = h[H_N];
    if (!(n >= 0.0 && n < 9.0e15) || capacity <= 0) return;          // (a block that was never initialised: no store outside it)
    const int64_t it = (int64_t)n;
    const double dI = (double)I, dU = (double)U;
    const double iou = (dI == 0.0 || dU == 0.0) ? 0.0 : dI / dU;          // train.py:64-76, in fp64
    // group 0's lr AFTER this iteration's tick (the step counter has been advanced by the update in front of this launch): the update's own factor
    float lr = 0.f;
    if (step && hyper) lr = base_lr * poly_lr_factor(k, total_steps, power);
    const bool loss_ok = isfinite(loss);
    const bool accumulating = ctl && c_acc != 0.f, skipped = ctl && !accumulating && c_skip != 0.f, applied = step && !accumulating && !skipped;
    const uint32_t flags = (applied ? LAVT_METER_APPLIED : 0u) | (skipped ? LAVT_METER_SKIPPED : 0u) | (accumulating ? LAVT_METER_ACCUMULATING : 0u) |
                           (loss_ok ? 0u : LAVT_METER_LOSS_NONFINITE);
    meter_record* ring = reinterpret_cast<meter_record*>(block + HDR);
    meter_record r;
    r.loss = loss; r.I = I; r.U = U; r.lr = lr; r.grad_norm = ctl ? c_norm : 0.f; r.flags = flags; r.iou = iou; r.it = it;
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
    if (ctl && !accumulating && isfinite(c_norm)) {          // the norm of a cycle's gradient, once per cycle
        block[H_NORM_SUM] = h[H_NORM_SUM] + (double)c_norm;
        block[H_NORM_COUNT] = h[H_NORM_COUNT] + 1.0;
    }
}

// ---------------------------------------------------------------------------------------------- evaluation meter (include/lavt_hip.h "Evaluation meter")
// What EvalMeter.update does for the (I, U) rows of one prediction batch (test.py:84-95), on the device.  One wave: every lane loads one slot's counts and
// liveness (all loads of a chunk of 64 slots in flight at once), lane 0 then walks the live slots in slot order -- the fp64 sum is sequential.
enum { E_CAPACITY = 0, E_HOLD, E_N, E_COUNT, E_IOU_SUM, E_CUM_I, E_CUM_U, E_CORRECT0 };

struct eval_record {
    int32_t I, U;
    int64_t sample;
};
static_assert(sizeof(eval_record) == LAVT_EVAL_METER_RECORD_BYTES, "the record layout is the contract of include/lavt_hip.h");
static_assert(E_CORRECT0 + 5 <= LAVT_EVAL_METER_HEADER_DOUBLES, "the header holds the five precision counters");

__global__ __launch_bounds__(64) void eval_meter_append_kernel(const int32_t* __restrict__ iu, const int32_t* __restrict__ image_of, int n_images, int n,
                                                               double* __restrict__ block, int capacity) {
    __shared__ int32_t sI[64], sU[64];
    const int lane = threadIdx.x;
    double h[E_CORRECT0 + 5];
#pragma unroll
    for (int i = 0; i < E_CORRECT0 + 5; ++i) h[i] = block[i];
    // hold (host-written), or a block that was never initialised: nothing is stored (uniform over the wave, so the barriers below are safe)
    if (h[E_HOLD] != 0.0 || !(h[E_N] >= 0.0 && h[E_N] < 9.0e15) || capacity <= 0) return;
    eval_record* ring = reinterpret_cast<eval_record*>(block + LAVT_EVAL_METER_HEADER_DOUBLES);
    const double thr[5] = {0.5, 0.6, 0.7, 0.8, 0.9};
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        bool live = s < n;
        if (live && image_of) {
            const int img = image_of[s];
            live = img >= 0 && img < n_images;
        }
        int32_t I = 0, U = 0;
        if (live) { I = iu[2 * s]; U = iu[2 * s + 1]; }
        sI[lane] = I;
        sU[lane] = U;
        const unsigned long long mask = __ballot(live);
        __syncthreads();
        if (lane == 0) {
            for (int j = 0; j < 64; ++j) {
                if (!((mask >> j) & 1ull)) continue;
                const int32_t cI = sI[j], cU = sU[j];
                const double iou = cU == 0 ? 0.0 : (double)cI / (double)cU;          // test.py:86-89: a true fp64 division
                const int64_t sample = (int64_t)h[E_N];
                eval_record r;
                r.I = cI; r.U = cU; r.sample = sample;
                ring[sample % capacity] = r;
                h[E_N] += 1.0;
                h[E_COUNT] += 1.0;
                h[E_IOU_SUM] += iou;
                h[E_CUM_I] += (double)cI;
                h[E_CUM_U] += (double)cU;
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (iou >= thr[k]) h[E_CORRECT0 + k] += 1.0;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (int i = E_N; i < E_CORRECT0 + 5; ++i) block[i] = h[i];
    }
}

// ---------------------------------------------------------------------------------------------- J&F meter (include/lavt_hip.h "J&F measure")
// The DAVIS 2017 sequence means over the count rows of lavt_boundary_counts.  One wave, as the evaluation meter: every lane loads one frame's six counts
// and liveness (a chunk of 64 frames in flight at once), lane 0 walks the frames in order -- every fp64 sum is sequential -- and closes a sequence
// behind every frames_per_seq-th frame.
enum { J_CAPACITY = 0, J_HOLD, J_N, J_SEQS, J_JSEQ_SUM, J_FSEQ_SUM, J_FRAMES, J_JFRAME_SUM, J_FFRAME_SUM, J_END };

struct jf_record {
    int32_t frames, zero;
    double J, F;
    int64_t seq;
};
static_assert(sizeof(jf_record) == LAVT_JF_METER_RECORD_BYTES, "the record layout is the contract of include/lavt_hip.h");
static_assert(J_END <= LAVT_JF_METER_HEADER_DOUBLES, "the header holds the accumulators");

__global__ __launch_bounds__(64) void jf_meter_append_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ live_of, int n, int T,
                                                             double* __restrict__ block, int capacity) {
    __shared__ int32_t sc[64][6];
    const int lane = threadIdx.x;
    double h[J_END];
#pragma unroll
    for (int i = 0; i < J_END; ++i) h[i] = block[i];
    // hold (host-written), or a block that was never initialised: nothing is stored (uniform over the wave, so the barriers below are safe)
    if (h[J_HOLD] != 0.0 || !(h[J_N] >= 0.0 && h[J_N] < 9.0e15) || capacity <= 0) return;
    jf_record* ring = reinterpret_cast<jf_record*>(block + LAVT_JF_METER_HEADER_DOUBLES);
    double js = 0.0, fs = 0.0;          // the open sequence: sums of J and F over its live frames, and their number
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const bool live = s < n && (!live_of || live_of[s] != 0);
        if (live) {
#pragma unroll
            for (int k = 0; k < 6; ++k) sc[lane][k] = counts[(int64_t)s * 8 + k];
        }
        const unsigned long long mask = __ballot(live);
        __syncthreads();
        if (lane == 0) {
            const int m = min(64, n - base);
            for (int j = 0; j < m; ++j) {
                if ((mask >> j) & 1ull) {
                    const int32_t I = sc[j][0], U = sc[j][1], nfg = sc[j][2], ngt = sc[j][3], mfg = sc[j][4], mgt = sc[j][5];
                    const double J = U == 0 ? 1.0 : (double)I / (double)U;          // db_eval_iou: two empty masks agree
                    double p, r;
                    if (nfg == 0 && ngt > 0) { p = 1.0; r = 0.0; }
                    else if (nfg > 0 && ngt == 0) { p = 0.0; r = 1.0; }
                    else if (nfg == 0 && ngt == 0) { p = 1.0; r = 1.0; }
                    else { p = (double)mfg / (double)nfg; r = (double)mgt / (double)ngt; }
                    const double F = (p + r == 0.0) ? 0.0 : ((2.0 * p) * r) / (p + r);
                    js += J;
                    fs += F;
                    cnt += 1;
                    h[J_FRAMES] += 1.0;
                    h[J_JFRAME_SUM] += J;
                    h[J_FFRAME_SUM] += F;
                }
                if ((base + j + 1) % T == 0) {          // the sequence ends here; one without a live frame stores nothing
                    if (cnt > 0) {
                        const int64_t seq = (int64_t)h[J_N];
                        jf_record rec;
                        rec.frames = cnt; rec.zero = 0; rec.J = js / (double)cnt; rec.F = fs / (double)cnt; rec.seq = seq;
                        ring[seq % capacity] = rec;
                        h[J_N] += 1.0;
                        h[J_SEQS] += 1.0;
                        h[J_JSEQ_SUM] += rec.J;
                        h[J_FSEQ_SUM] += rec.F;
                    }
                    js = 0.0; fs = 0.0; cnt = 0;
                }
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (int i = J_N; i < J_END; ++i) block[i] = h[i];
    }
}

// ---------------------------------------------------------------------------------------------- hard-mask I / U of a training batch (lavt_upsample_iu)
// train.py:64-76 on the low-resolution logits: every full-resolution pixel is recomputed from its four neighbours exactly as upsample_ce_fwd_kernel
// does (bl_coord / upce_at, common.h; pred = up1 > up0, a tie is class 0), pred && tgt and pred || tgt are counted per wave with ballot + popcount --
// wave-uniform integers -- and every workgroup stores ONE int32 pair.  A streaming pass over the int64 labels: consecutive lanes load consecutive
// 8-byte labels (512 contiguous bytes per wave), the label load is issued before the gather from the (L2-resident) logits map.  The loop bound is
// uniform over the workgroup, a lane past the end or on an unselected frame is a false predicate, not a branch around the ballots.
inline int iu_grid(int64_t n) { int64_t b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

template <typename T, bool SEL>
__global__ __launch_bounds__(256) void upsample_iu_kernel(const T* __restrict__ x, const int32_t* __restrict__ sel, int nfr, const int64_t* __restrict__ target,
                                                          int32_t* __restrict__ partial, int ns, int Hi, int Wi, int Ho, int Wo, float sh, float sw) {
    const int64_t n = (int64_t)ns * Ho * Wo, stride = (int64_t)gridDim.x * 256;
    int ci = 0, cu = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        bool pi = false, pu = false;
        if (i < n) {
            const int64_t t = target[i];
            const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho), b = sel_frame<SEL>(sel, (int)(i / Wo / Ho), nfr);
            if (!SEL || b >= 0) {          // an entry of sel outside [0, nfr): no logits are read, the sample counts nothing
                int y0, y1, x0, x1; float ly, lx;
                bl_coord(yo, sh, Hi, y0, y1, ly);
                bl_coord(xo, sw, Wi, x0, x1, lx);
                const UpCe u = upce_at<T>(x + (int64_t)b * Hi * Wi * 2, Wi, y0, y1, ly, x0, x1, lx);
                const bool pred = u.up1 > u.up0, tgt = t == 1;          // argmax picks class 0 on ties
                pi = pred && tgt;
                pu = pred || tgt;
            }
        }
        ci += __popcll(__ballot(pi));
        cu += __popcll(__ballot(pu));
    }
    __shared__ int red[4][2];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = ci; red[threadIdx.x >> 6][1] = cu; }
    __syncthreads();
    if (threadIdx.x < 2) partial[blockIdx.x * 2 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
// row = {loss_src ? loss_src[0] : 0, 0, I, U}: the pairs added in 64-bit integers in one fixed order (thread t takes pairs t, t + 256, ...; a xor tree
// joins the lanes, the four waves are added in wave order), each total converted to fp32 once.  The loss is copied as a bit pattern (a NaN keeps its payload).
__global__ __launch_bounds__(256) void upsample_iu_finish_kernel(const int32_t* __restrict__ partial, int nblk, const uint32_t* __restrict__ loss_src,
                                                                 float* __restrict__ row) {
    long long a[2] = {0, 0};
    for (int b = threadIdx.x; b < nblk; b += 256) { a[0] += partial[b * 2]; a[1] += partial[b * 2 + 1]; }
    __shared__ long long red[4][2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a[0]; red[threadIdx.x >> 6][1] = a[1]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t loss_bits = loss_src ? loss_src[0] : 0u;
        reinterpret_cast<uint32_t*>(row)[0] = loss_bits;
        row[1] = 0.f;
        row[2] = (float)(red[0][0] + red[1][0] + red[2][0] + red[3][0]);
        row[3] = (float)(red[0][1] + red[1][1] + red[2][1] + red[3][1]);
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

extern "C" int64_t lavt_eval_meter_bytes(int capacity) {
    return capacity > 0 ? (int64_t)LAVT_EVAL_METER_HEADER_DOUBLES * 8 + (int64_t)capacity * LAVT_EVAL_METER_RECORD_BYTES : 0;
}

extern "C" int lavt_eval_meter_append(const int32_t* iu, const int32_t* image_of, int n_images, int n, void* block, int capacity, void* stream) {
    LAVT_CHECK_ARG(iu && block && n > 0 && capacity > 0, "lavt_eval_meter_append: bad arguments (iu, block, n > 0, capacity > 0)");
    LAVT_CHECK_ARG(!image_of || n_images > 0, "lavt_eval_meter_append: image_of needs n_images > 0");
    LAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(block) & 7) == 0, "lavt_eval_meter_append: the block must be 8-byte aligned");
    hipLaunchKernelGGL(eval_meter_append_kernel, dim3(1), dim3(64), 0, ST, iu, image_of, n_images, n, reinterpret_cast<double*>(block), capacity);
    LAVT_CHECK_LAUNCH("lavt_eval_meter_append");
    return LAVT_OK;
}

extern "C" int64_t lavt_jf_meter_bytes(int capacity) {
    return capacity > 0 ? (int64_t)LAVT_JF_METER_HEADER_DOUBLES * 8 + (int64_t)capacity * LAVT_JF_METER_RECORD_BYTES : 0;
}

extern "C" int lavt_jf_meter_append(const int32_t* counts, const int32_t* live, int n, int frames_per_seq, void* block, int capacity, void* stream) {
    LAVT_CHECK_ARG(counts && block && n > 0 && capacity > 0, "lavt_jf_meter_append: bad arguments (counts, block, n > 0, capacity > 0)");
    LAVT_CHECK_ARG(frames_per_seq > 0 && n % frames_per_seq == 0, "lavt_jf_meter_append: %d frames are not whole sequences of %d", n, frames_per_seq);
    LAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(block) & 7) == 0, "lavt_jf_meter_append: the block must be 8-byte aligned");
    hipLaunchKernelGGL(jf_meter_append_kernel, dim3(1), dim3(64), 0, ST, counts, live, n, frames_per_seq, reinterpret_cast<double*>(block), capacity);
    LAVT_CHECK_LAUNCH("lavt_jf_meter_append");
    return LAVT_OK;
}

extern "C" int64_t lavt_upsample_iu_ws(int n, int Ho, int Wo) {
    return (n > 0 && Ho > 0 && Wo > 0) ? 2 * (int64_t)iu_grid((int64_t)n * Ho * Wo) : 0;
}

// SEL = false: B frames = B samples (sel, nsel unused); SEL = true: nsel samples out of the B frames of x
template <bool SEL>
static int upsample_iu(const char* who, int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, const float* loss_src, int32_t* ws,
                       int64_t ws_words, float* row, int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    const int ns = SEL ? nsel : B;
    const int blocks = iu_grid((int64_t)ns * Ho * Wo);
    LAVT_CHECK_ARG(dtype == LAVT_F32 || dtype == LAVT_BF16, "%s: bad dtype %d", who, dtype);
    LAVT_CHECK_ARG(ws_words >= lavt_upsample_iu_ws(ns, Ho, Wo), "%s: scratch of %d 32-bit words needed", who, 2 * blocks);
    LAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(target) & 7) == 0 && ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(row) |
                                                                       reinterpret_cast<uintptr_t>(loss_src) | reinterpret_cast<uintptr_t>(sel)) & 3) == 0,
                   "%s: target must be 8-byte aligned; sel, loss_src, ws and row 4-byte", who);
    const float sh = bl_scale(Hi, Ho), sw = bl_scale(Wi, Wo);
    if (dtype == LAVT_F32) hipLaunchKernelGGL((upsample_iu_kernel<float, SEL>), dim3(blocks), dim3(256), 0, ST, (const float*)x, sel, B, target, ws, ns, Hi, Wi, Ho, Wo, sh, sw);
    else hipLaunchKernelGGL((upsample_iu_kernel<bf16, SEL>), dim3(blocks), dim3(256), 0, ST, (const bf16*)x, sel, B, target, ws, ns, Hi, Wi, Ho, Wo, sh, sw);
    hipLaunchKernelGGL(upsample_iu_finish_kernel, dim3(1), dim3(256), 0, ST, ws, blocks, reinterpret_cast<const uint32_t*>(loss_src), row);
    LAVT_CHECK_LAUNCH(who);
    return LAVT_OK;
}

extern "C" int lavt_upsample_iu(int dtype, const void* x, const int64_t* target, const float* loss_src, int32_t* ws, int64_t ws_words, float* row, int B, int Hi,
                                int Wi, int Ho, int Wo, void* stream) {
    LAVT_CHECK_ARG(x && target && ws && row && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "lavt_upsample_iu: bad arguments");
    return upsample_iu<false>("lavt_upsample_iu", dtype, x, nullptr, B, target, loss_src, ws, ws_words, row, B, Hi, Wi, Ho, Wo, stream);
}

extern "C" int lavt_upsample_iu_sel(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, const float* loss_src, int32_t* ws,
                                    int64_t ws_words, float* row, int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    LAVT_CHECK_ARG(x && sel && target && ws && row && B > 0 && nsel > 0 && nsel <= B && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0,
                   "lavt_upsample_iu_sel: bad arguments (0 < nsel <= B)");
    return upsample_iu<true>("lavt_upsample_iu_sel", dtype, x, sel, nsel, target, loss_src, ws, ws_words, row, B, Hi, Wi, Ho, Wo, stream);
}
