// Shared device/host helpers for the LAVT gfx950 kernels.  CDNA4 only: wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/lavt_hip.h"

typedef __bf16 bf16;
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

#define LAVT_WAVE 64

// ---- error plumbing -------------------------------------------------------------------------
void lavt_set_error(const char* fmt, ...);
#define LAVT_CHECK_ARG(cond, ...)                 \
    do {                                          \
        if (!(cond)) {                            \
            lavt_set_error(__VA_ARGS__);          \
            return LAVT_ERR_INVALID;              \
        }                                         \
    } while (0)
#define LAVT_CHECK_LAUNCH(name)                                                  \
    do {                                                                         \
        hipError_t e__ = hipGetLastError();                                      \
        if (e__ != hipSuccess) {                                                 \
            lavt_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return LAVT_ERR_LAUNCH;                                              \
        }                                                                        \
    } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- dispatch switches (tuning.hip): the LAVT_* environment variables the test-suite forces, read once per process (lavt_tuning_reload() re-reads) ---------
struct lavt_tuning_t {
    bool bilinear_rows;
    int gemm_tile, gemm_stages, gemm_pipe, tn_pipe, tn_pipe_min_tiles, tn_pipe_stages, tn_pipe_min_ktiles;
};
const lavt_tuning_t& lavt_tuning();

// ---- scalar conversions -----------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<bf16>(bf16 v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 from_f<bf16>(float v) { return (bf16)v; }

// A 16-byte chunk of T: 4 floats or 8 bf16.
template <typename T> struct Chunk { static constexpr int N = 16 / sizeof(T); };

template <typename T> __device__ __forceinline__ void chunk_to_f(const uint4& c, float* f) {
    if constexpr (std::is_same<T, float>::value) {
        f[0] = __uint_as_float(c.x); f[1] = __uint_as_float(c.y); f[2] = __uint_as_float(c.z); f[3] = __uint_as_float(c.w);
    } else {
        const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(w[i] << 16);
            f[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
        }
    }
}
// (as a two-element vector conversion the pair is ONE v_cvt_pk_bf16_f32; converted one by one and joined with shift / or it was four instructions)
typedef __bf16 lavt_bf16x2 __attribute__((ext_vector_type(2)));
typedef float lavt_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(lavt_f32x2{lo, hi}, lavt_bf16x2));
}
template <typename T> __device__ __forceinline__ uint4 f_to_chunk(const float* f) {
    uint4 c;
    if constexpr (std::is_same<T, float>::value) {
        c.x = __float_as_uint(f[0]); c.y = __float_as_uint(f[1]); c.z = __float_as_uint(f[2]); c.w = __float_as_uint(f[3]);
    } else {
        c.x = pack_bf16x2(f[0], f[1]); c.y = pack_bf16x2(f[2], f[3]);
        c.z = pack_bf16x2(f[4], f[5]); c.w = pack_bf16x2(f[6], f[7]);
    }
    return c;
}

// ---- wave / block reductions ----------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- activations ------------------------------------------------------------------------------
// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7): 1 reciprocal (v_rcp_f32, 1 ulp: __frcp_rn / a division expand to the 11-instruction
// IEEE sequence, more than the rest of the function), 1 exponential, 7 fma -- the library erff is ~40 instructions, and inside a
// GEMM epilogue (two waves per SIMD, nothing to overlap with) the exact form cost 4-5 us on a 1800 x 2048 tile set (tools/gemm_cold_probe.py).
// Used on the bf16 path only (bf16 keeps 8 significant bits); the fp32 parity path keeps erff.
__device__ __forceinline__ float erf_fast(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
    const float poly = ((((1.061405429f * t - 1.453152027f) * t + 1.421413741f) * t - 0.284496736f) * t + 0.254829592f) * t;
    const float y = 1.0f - poly * __expf(-ax * ax);
    return copysignf(y, x);
}
__device__ __forceinline__ float gelu_f_fast(float x) { return 0.5f * x * (1.0f + erf_fast(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad_f_fast(float x) {
    const float cdf = 0.5f * (1.0f + erf_fast(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}
// GELU and its derivative together: Phi(x) from the fast erf, phi(x) from the SAME exponential (exp(-z^2) with z = x / sqrt 2 is exp(-x^2 / 2))
__device__ __forceinline__ float gelu_pair_fast(float x, float& d) {
    const float z = x * 0.70710678118654752440f, az = fabsf(z);
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * az);
    const float poly = ((((1.061405429f * t - 1.453152027f) * t + 1.421413741f) * t - 0.284496736f) * t + 0.254829592f) * t;
    const float e = __expf(-az * az);
    const float cdf = 0.5f * (1.0f + copysignf(1.0f - poly * e, z));
    d = cdf + x * (0.39894228040143267794f * e);
    return x * cdf;
}
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// ---- bilinear resize (align_corners=True): source rows / columns i0, i1 and the weight of i1 for output index o ---------------------
__device__ __forceinline__ void bl_coord(int o, float scale, int n_in, int& i0, int& i1, float& lam) {
    const float src = scale * (float)o;
    i0 = (int)src;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = min(i0 + 1, n_in - 1);
    lam = src - (float)i0;
}
// gather form of the transpose: the output rows / columns [lo, hi] that can have sampled input index i (a generous candidate range; bl_coord decides)
__device__ __forceinline__ void bl_range(int i, float scale, int n_in, int n_out, int& lo, int& hi) {
    if (scale <= 0.f) { lo = 0; hi = n_out - 1; return; }
    lo = max(0, (int)floorf((float)(i - 1) / scale) - 1);
    hi = min(n_out - 1, (int)ceilf((float)(i + 1) / scale) + 1);
}

// ---- the fused upsample + criterion kernels (elementwise.hip, boundary_loss.hip): one full-resolution pixel of the 2-class logits from its four
// low-resolution neighbours (x NHWC [.,Hi,Wi,2]) and its log-sum-exp
struct UpCe { float up0, up1, lse; };
// ---- frame selection (train.py:282-285, 366-369; test.py:182-205 of the reference: `index_select(output, 0, valid_indices)` in front of the criterion):
// with SEL the loss has nsel samples, sample j reads logits frame sel[j] of the nfr frames of x and target j.  sel is read on the device (a replayed
// graph follows the buffer); an entry outside [0, nfr) is never dereferenced.  SEL = false is the plain kernel: frame = sample.
template <bool SEL> __device__ __forceinline__ int sel_frame(const int32_t* __restrict__ sel, int j, int nfr) {          // frame read by sample j, -1 = none
    if constexpr (!SEL) return j;
    else { const int f = sel[j]; return (f >= 0 && f < nfr) ? f : -1; }
}
// Backward: the sample that frame b feeds, -1 = none (its dx is +0.0).  A scan of sel per frame -- nsel is a handful, b is uniform over a wave in both
// cross-entropy forms (over the workgroup in the tile form), so the scan is a few scalar loads.
template <bool SEL> __device__ __forceinline__ int sel_sample(const int32_t* __restrict__ sel, int nsel, int b) {
    if constexpr (!SEL) return b;
    else {
        int j = -1;
        for (int k = nsel - 1; k >= 0; --k) j = sel[k] == b ? k : j;          // (entries are distinct by contract; the first one wins otherwise)
        return j;
    }
}
template <typename T>
__device__ __forceinline__ UpCe upce_at(const T* base, int Wi, int y0, int y1, float ly, int x0, int x1, float lx) {
    const T* r0 = base + ((int64_t)y0 * Wi) * 2;
    const T* r1 = base + ((int64_t)y1 * Wi) * 2;
    const float a0 = to_f<T>(r0[x0 * 2]), a1 = to_f<T>(r0[x0 * 2 + 1]), b0 = to_f<T>(r0[x1 * 2]), b1 = to_f<T>(r0[x1 * 2 + 1]);
    const float c0 = to_f<T>(r1[x0 * 2]), c1 = to_f<T>(r1[x0 * 2 + 1]), d0 = to_f<T>(r1[x1 * 2]), d1 = to_f<T>(r1[x1 * 2 + 1]);
    UpCe u;
    u.up0 = (1.f - ly) * ((1.f - lx) * a0 + lx * b0) + ly * ((1.f - lx) * c0 + lx * d0);
    u.up1 = (1.f - ly) * ((1.f - lx) * a1 + lx * b1) + ly * ((1.f - lx) * c1 + lx * d1);
    const float m = fmaxf(u.up0, u.up1);
    u.lse = m + logf(expf(u.up0 - m) + expf(u.up1 - m));
    return u;
}
