// Inference-only kernels (reference test.py / test_ytvos.py under model.eval()): BatchNorm folded into the packed convolution weight, the split-K
// reduction with the folded bias + activation, and the final upsample fused with argmax and the I / U pixel counts.
#include "internal.h"

namespace {

inline int ew_grid(int64_t n) { int64_t b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }
#define GRID_STRIDE(i, n) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)
#define ST reinterpret_cast<hipStream_t>(stream)

// ---------------------------------------------------------------------------------------------- BatchNorm fold
// packed[co][tap][ci] = T(w[co][ci][tap] * s[co]),  s = gamma / sqrt(running_var + eps);  bias[co] = beta - running_mean * s  (all in fp32)
template <typename T>
__global__ void conv_bn_fold_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                                    const float* __restrict__ var, float eps, T* __restrict__ packed, float* __restrict__ bias, int Cout, int Cin, int taps) {
    const int64_t n = (int64_t)Cout * taps * Cin;
    GRID_STRIDE(i, n) {
        const int ci = (int)(i % Cin), tap = (int)((i / Cin) % taps), co = (int)(i / Cin / taps);
        const float s = (gamma ? gamma[co] : 1.f) / sqrtf(var[co] + eps);
        packed[i] = from_f<T>(w[((int64_t)co * Cin + ci) * taps + tap] * s);
        if (ci == 0 && tap == 0) bias[co] = (beta ? beta[co] : 0.f) - mean[co] * s;
    }
}

// ---------------------------------------------------------------------------------------------- split-K reduction + bias + activation
// the summation loop is splitk_reduce_kernel's (csrc/elementwise.hip): with bias == NULL and act == NONE the stored bytes are the same
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_epi_kernel(const float* __restrict__ parts, int splits, int64_t MN, int64_t chunks, int N, const float* __restrict__ bias,
                                                                int act, T* __restrict__ out, int64_t ldc) {
    GRID_STRIDE(i, chunks) {
        const int64_t e = i * 8;
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < splits; ++s) {
            const float4 v0 = *reinterpret_cast<const float4*>(parts + (int64_t)s * MN + e), v1 = *reinterpret_cast<const float4*>(parts + (int64_t)s * MN + e + 4);
            a[0] += v0.x; a[1] += v0.y; a[2] += v0.z; a[3] += v0.w; a[4] += v1.x; a[5] += v1.y; a[6] += v1.z; a[7] += v1.w;
        }
        const int64_t m = e / N;
        const int n = (int)(e - m * N);
        if (bias) {
            const float4 b0 = *reinterpret_cast<const float4*>(bias + n), b1 = *reinterpret_cast<const float4*>(bias + n + 4);
            a[0] += b0.x; a[1] += b0.y; a[2] += b0.z; a[3] += b0.w; a[4] += b1.x; a[5] += b1.y; a[6] += b1.z; a[7] += b1.w;
        }
        if (act == LAVT_ACT_RELU) {
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = fmaxf(a[k], 0.f);
        } else if (act == LAVT_ACT_GELU) {
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = std::is_same<T, bf16>::value ? gelu_f_fast(a[k]) : gelu_f(a[k]);
        } else if (act == LAVT_ACT_TANH) {
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = tanhf(a[k]);
        }
        if constexpr (std::is_same<T, float>::value) {
            *reinterpret_cast<float4*>(out + m * ldc + n) = make_float4(a[0], a[1], a[2], a[3]);
            *reinterpret_cast<float4*>(out + m * ldc + n + 4) = make_float4(a[4], a[5], a[6], a[7]);
        } else *reinterpret_cast<uint4*>(out + m * ldc + n) = f_to_chunk<bf16>(a);
    }
}

// ---------------------------------------------------------------------------------------------- upsample -> argmax mask (+ I / U)
// coordinate arithmetic of lavt_logits_up_fwd (bl_coord: common.h, bl_scale: internal.h), align_corners=True

template <typename T> __device__ __forceinline__ float2 ld_pair(const T* base, int64_t pix);
template <> __device__ __forceinline__ float2 ld_pair<float>(const float* base, int64_t pix) { return *reinterpret_cast<const float2*>(base + pix * 2); }
template <> __device__ __forceinline__ float2 ld_pair<bf16>(const bf16* base, int64_t pix) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(base + pix * 2);
    return make_float2(__uint_as_float(w << 16), __uint_as_float(w & 0xFFFF0000u));
}

// both classes of one bilinear sample of the [Hi][Wi][2] rows
template <typename T> __device__ __forceinline__ float2 bl_sample(const T* base, int Wi, int y0, int y1, float ly, int x0, int x1, float lx) {
    const float2 f00 = ld_pair<T>(base, (int64_t)y0 * Wi + x0), f01 = ld_pair<T>(base, (int64_t)y0 * Wi + x1);
    const float2 f10 = ld_pair<T>(base, (int64_t)y1 * Wi + x0), f11 = ld_pair<T>(base, (int64_t)y1 * Wi + x1);
    return make_float2((1.f - ly) * ((1.f - lx) * f00.x + lx * f01.x) + ly * ((1.f - lx) * f10.x + lx * f11.x),
                       (1.f - ly) * ((1.f - lx) * f00.y + lx * f01.y) + ly * ((1.f - lx) * f10.y + lx * f11.y));
}

struct UpMaskDims {
    int B, Hi, Wi, Hm, Wm, Ho, Wo;
    float sh, sw;          // output -> sampled grid (the intermediate grid when Hm > 0, else the input)
    float mh, mw;          // intermediate -> input
};

template <typename T> __device__ __forceinline__ bool up_mask_pixel(const T* base, const UpMaskDims& d, int yo, int xo) {
    float2 v;
    if (d.Hm == 0) {
        int y0, y1, x0, x1; float ly, lx;
        bl_coord(yo, d.sh, d.Hi, y0, y1, ly);
        bl_coord(xo, d.sw, d.Wi, x0, x1, lx);
        v = bl_sample<T>(base, d.Wi, y0, y1, ly, x0, x1, lx);
    } else {
        // (Hi, Wi) -> (Hm, Wm) -> (Ho, Wo): the four corners on the intermediate grid are bilinear samples of the input themselves
        int my[2], mx[2]; float mly, mlx;
        bl_coord(yo, d.sh, d.Hm, my[0], my[1], mly);
        bl_coord(xo, d.sw, d.Wm, mx[0], mx[1], mlx);
        int y0[2], y1[2], x0[2], x1[2]; float ly[2], lx[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            bl_coord(my[k], d.mh, d.Hi, y0[k], y1[k], ly[k]);
            bl_coord(mx[k], d.mw, d.Wi, x0[k], x1[k], lx[k]);
        }
        const float2 c00 = bl_sample<T>(base, d.Wi, y0[0], y1[0], ly[0], x0[0], x1[0], lx[0]), c01 = bl_sample<T>(base, d.Wi, y0[0], y1[0], ly[0], x0[1], x1[1], lx[1]);
        const float2 c10 = bl_sample<T>(base, d.Wi, y0[1], y1[1], ly[1], x0[0], x1[0], lx[0]), c11 = bl_sample<T>(base, d.Wi, y0[1], y1[1], ly[1], x0[1], x1[1], lx[1]);
        v = make_float2((1.f - mly) * ((1.f - mlx) * c00.x + mlx * c01.x) + mly * ((1.f - mlx) * c10.x + mlx * c11.x),
                        (1.f - mly) * ((1.f - mlx) * c00.y + mlx * c01.y) + mly * ((1.f - mlx) * c10.y + mlx * c11.y));
    }
    return v.y > v.x;          // a tie is class 0, as argmax
}

// One thread = 4 consecutive pixels of the flat [B*Ho*Wo] mask (a group may run over a row or sample end), stored as one 32-bit word.  Counts: one
// ballot per pixel slot, popcounts added per wave, two integer atomics per wave when the whole wave lies in one sample (all but <= B - 1 waves).
// PAIRS (include/lavt_hip.h: the image_of contract): sample b is slot b of a pair list, live when image_of[b] lies in [0, n_images).  The liveness test
// is per pixel's sample, because a group of 4 and a wave run over sample ends: a pixel of an empty slot loads no logits (they may be NaN), stores a
// zero byte and is false in both ballots -- an empty slot's wave counts 0 and issues no atomic.  PAIRS = false is the plain kernel, the two arguments unused.
template <typename T, bool PAIRS>
__global__ __launch_bounds__(256) void upsample_mask_kernel(const T* __restrict__ x, UpMaskDims d, uint8_t* __restrict__ mask, const int64_t* __restrict__ target,
                                                            int* __restrict__ iu, const int32_t* __restrict__ image_of, int n_images) {
    const int64_t HW = (int64_t)d.Ho * d.Wo, total = d.B * HW;
    const int64_t g0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 4;
    uint32_t word = 0;
    bool pi[4] = {false, false, false, false}, pu[4] = {false, false, false, false};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t g = g0 + j;
        if (g < total) {
            const int b = (int)(g / HW);
            if constexpr (PAIRS) {
                const int img = image_of[b];
                if (img < 0 || img >= n_images) continue;
            }
            const int64_t r = g - b * HW;
            const int yo = (int)(r / d.Wo), xo = (int)(r - (int64_t)yo * d.Wo);
            const bool p = up_mask_pixel<T>(x + (int64_t)b * d.Hi * d.Wi * 2, d, yo, xo);
            word |= (p ? 1u : 0u) << (8 * j);
            if (target) {
                const bool t = target[g] != 0;
                pi[j] = p && t;
                pu[j] = p || t;
            }
        }
    }
    if (g0 + 3 < total) *reinterpret_cast<uint32_t*>(mask + g0) = word;
    else
        for (int j = 0; j < 4 && g0 + j < total; ++j) mask[g0 + j] = (uint8_t)((word >> (8 * j)) & 1u);
    if (!target) return;
    // sample of the wave's first and last pixel (lanes are consecutive: 256 pixels per wave)
    const int64_t w0 = g0 - (int64_t)(threadIdx.x & 63) * 4;
    const int64_t wl = min(w0 + 255, total - 1);
    if (w0 >= total) return;
    const int bf = (int)(w0 / HW), bl = (int)(wl / HW);
    if (bf == bl) {
        int ci = 0, cu = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ci += __popcll(__ballot(pi[j]));
            cu += __popcll(__ballot(pu[j]));
        }
        if ((threadIdx.x & 63) == 0) {
            if (ci) atomicAdd(iu + bf * 2, ci);
            if (cu) atomicAdd(iu + bf * 2 + 1, cu);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t g = g0 + j;
            if (g < total && pu[j]) {
                const int b = (int)(g / HW);
                if (pi[j]) atomicAdd(iu + b * 2, 1);
                atomicAdd(iu + b * 2 + 1, 1);
            }
        }
    }
}

}  // namespace

extern "C" int lavt_conv_bn_fold(const float* w, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int dtype,
                                 void* w_packed, float* bias, int Cout, int Cin, int taps, void* stream) {
    LAVT_CHECK_ARG(w && running_mean && running_var && w_packed && bias && Cout > 0 && Cin > 0 && taps > 0, "lavt_conv_bn_fold: bad arguments");
    const int64_t n = (int64_t)Cout * Cin * taps;
    if (dtype == LAVT_F32) hipLaunchKernelGGL(conv_bn_fold_kernel<float>, dim3(ew_grid(n)), dim3(256), 0, ST, w, gamma, beta, running_mean, running_var, eps, (float*)w_packed, bias, Cout, Cin, taps);
    else if (dtype == LAVT_BF16) hipLaunchKernelGGL(conv_bn_fold_kernel<bf16>, dim3(ew_grid(n)), dim3(256), 0, ST, w, gamma, beta, running_mean, running_var, eps, (bf16*)w_packed, bias, Cout, Cin, taps);
    else { lavt_set_error("lavt_conv_bn_fold: bad dtype %d", dtype); return LAVT_ERR_INVALID; }
    LAVT_CHECK_LAUNCH("lavt_conv_bn_fold");
    return LAVT_OK;
}

extern "C" int lavt_splitk_reduce_epi(int dtype, const float* parts, int splits, int64_t M, int N, const float* bias, int act, void* out, int64_t ldc, void* stream) {
    LAVT_CHECK_ARG(parts && out && splits > 0 && M > 0 && N > 0 && N % 8 == 0 && ldc % 8 == 0, "lavt_splitk_reduce_epi: bad arguments (N, ldc multiples of 8)");
    LAVT_CHECK_ARG(act == LAVT_ACT_NONE || act == LAVT_ACT_GELU || act == LAVT_ACT_RELU || act == LAVT_ACT_TANH, "lavt_splitk_reduce_epi: act must be NONE, GELU, RELU or TANH");
    LAVT_CHECK_ARG(!bias || ((uintptr_t)bias % 16) == 0, "lavt_splitk_reduce_epi: bias must be 16-byte aligned");
    const int64_t chunks = M * N / 8;
    if (dtype == LAVT_BF16) hipLaunchKernelGGL(splitk_reduce_epi_kernel<bf16>, dim3(ew_grid(chunks)), dim3(256), 0, ST, parts, splits, M * N, chunks, N, bias, act, (bf16*)out, ldc);
    else if (dtype == LAVT_F32) hipLaunchKernelGGL(splitk_reduce_epi_kernel<float>, dim3(ew_grid(chunks)), dim3(256), 0, ST, parts, splits, M * N, chunks, N, bias, act, (float*)out, ldc);
    else { lavt_set_error("lavt_splitk_reduce_epi: bad dtype %d", dtype); return LAVT_ERR_INVALID; }
    LAVT_CHECK_LAUNCH("lavt_splitk_reduce_epi");
    return LAVT_OK;
}

static int upsample_mask_launch(const char* who, int dtype, const void* x, int B, int Hi, int Wi, int Hm, int Wm, int Ho, int Wo, uint8_t* mask, const int64_t* target,
                                int32_t* iu, const int32_t* image_of, int n_images, void* stream) {
    if (!(x && mask && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0)) { lavt_set_error("%s: bad arguments", who); return LAVT_ERR_INVALID; }
    if (!((Hm == 0 && Wm == 0) || (Hm > 0 && Wm > 0))) { lavt_set_error("%s: Hm, Wm are both 0 (one interpolation) or both positive", who); return LAVT_ERR_INVALID; }
    if (target && !iu) { lavt_set_error("%s: a target needs the iu output", who); return LAVT_ERR_INVALID; }
    if (((uintptr_t)mask % 4) != 0 || ((uintptr_t)x % 8) != 0) { lavt_set_error("%s: mask must be 4-byte, x 8-byte aligned", who); return LAVT_ERR_INVALID; }
    UpMaskDims d;
    d.B = B; d.Hi = Hi; d.Wi = Wi; d.Hm = Hm; d.Wm = Wm; d.Ho = Ho; d.Wo = Wo;
    if (Hm > 0) { d.sh = bl_scale(Hm, Ho); d.sw = bl_scale(Wm, Wo); d.mh = bl_scale(Hi, Hm); d.mw = bl_scale(Wi, Wm); }
    else { d.sh = bl_scale(Hi, Ho); d.sw = bl_scale(Wi, Wo); d.mh = d.mw = 0.f; }
    const int64_t groups = ((int64_t)B * Ho * Wo + 3) / 4, blocks = (groups + 255) / 256;
    if (blocks > 0x7fffffff) { lavt_set_error("%s: too many pixels for one launch", who); return LAVT_ERR_INVALID; }
    const dim3 grid((unsigned)blocks), block(256);
    if (dtype != LAVT_F32 && dtype != LAVT_BF16) { lavt_set_error("%s: bad dtype %d", who, dtype); return LAVT_ERR_INVALID; }
    if (image_of) {
        if (dtype == LAVT_F32) hipLaunchKernelGGL((upsample_mask_kernel<float, true>), grid, block, 0, ST, (const float*)x, d, mask, target, iu, image_of, n_images);
        else hipLaunchKernelGGL((upsample_mask_kernel<bf16, true>), grid, block, 0, ST, (const bf16*)x, d, mask, target, iu, image_of, n_images);
    } else {
        if (dtype == LAVT_F32) hipLaunchKernelGGL((upsample_mask_kernel<float, false>), grid, block, 0, ST, (const float*)x, d, mask, target, iu, nullptr, 0);
        else hipLaunchKernelGGL((upsample_mask_kernel<bf16, false>), grid, block, 0, ST, (const bf16*)x, d, mask, target, iu, nullptr, 0);
    }
    LAVT_CHECK_LAUNCH(who);
    return LAVT_OK;
}

extern "C" int lavt_upsample_mask(int dtype, const void* x, int B, int Hi, int Wi, int Hm, int Wm, int Ho, int Wo, uint8_t* mask, const int64_t* target, int32_t* iu,
                                  void* stream) {
    return upsample_mask_launch("lavt_upsample_mask", dtype, x, B, Hi, Wi, Hm, Wm, Ho, Wo, mask, target, iu, nullptr, 0, stream);
}

extern "C" int lavt_upsample_mask_pairs(int dtype, const void* x, int B, int Hi, int Wi, int Hm, int Wm, int Ho, int Wo, uint8_t* mask, const int64_t* target, int32_t* iu,
                                        const int32_t* image_of, int n_images, void* stream) {
    LAVT_CHECK_ARG(image_of && n_images > 0 && ((uintptr_t)image_of % 4) == 0, "lavt_upsample_mask_pairs: image_of (4-byte aligned) and n_images > 0 are required");
    return upsample_mask_launch("lavt_upsample_mask_pairs", dtype, x, B, Hi, Wi, Hm, Wm, Ho, Wo, mask, target, iu, image_of, n_images, stream);
}
