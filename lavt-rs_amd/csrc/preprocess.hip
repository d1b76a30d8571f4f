// Device-side frame preprocessing (reference transforms.py:20-31, 83-87, 106-113; the per-frame host loop of test_ytvos.py:236-243): PIL's bilinear
// (antialiased) resize of uint8 RGB frames by its own fixed-point coefficient tables, finished as ((v / 255) - mean) / std into fp32 planes, and PIL's
// nearest resize of uint8 masks into int64.  The tables come from the host (lavt_hip/preprocess.py): the integer stage equals PIL bit for bit.
#include "common.h"

namespace {

#define ST reinterpret_cast<hipStream_t>(stream)
constexpr int PP_TW = 64;                         // output pixels of a tile along x: one wave-width, the coalesced store
constexpr int PP_ROW = 3 * PP_TW;                 // bytes of one horizontally resampled source row of a tile in LDS: [c][x]
constexpr int PP_BITS = 22;                       // PIL's PRECISION_BITS for 8-bit data
constexpr int PP_LDS_MAX = 64 * 1024;             // the default dynamic-LDS limit of a work-group

struct Norm3 { float mean[3], std[3]; };

__device__ __forceinline__ uint32_t pp_round_clip(uint32_t acc) {
    const uint32_t v = acc >> PP_BITS;            // coefficients and pixels are non-negative: only the upper clip can act
    return v > 255u ? 255u : v;
}

// One work-group = TH x 64 output pixels of one frame, 256 threads = 4 waves.  Lane = x within the tile in both passes.
//   pass 1: source rows y0 .. y1 (what the tile's output rows read) resampled along x into LDS as uint8 [row][c][x]
//   pass 2: output (row, channel) pairs, one per wave at a time, resampled along y out of LDS, normalised, stored along x
// `frame` = the work-group's source, `plane` = its output frame: everything here is block-uniform, and so are the exits in front of the barrier.
__device__ __forceinline__ void pp_tile(const uint8_t* __restrict__ frame, int Hs, int Ws, const int32_t* __restrict__ coef_x, const int32_t* __restrict__ bounds_x, int ksize_x,
                                        const int32_t* __restrict__ coef_y, const int32_t* __restrict__ bounds_y, int ksize_y, float* __restrict__ plane, int Ho, int Wo,
                                        int TH, int lds_rows, const Norm3& nm, uint8_t* rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * PP_TW + lane;
    const int r0 = blockIdx.y * TH, r1 = min(r0 + TH, Ho) - 1;          // first / last output row of the tile
    const int y0 = bounds_y[2 * r0], y1 = bounds_y[2 * r1] + bounds_y[2 * r1 + 1];          // xmin and xmin + n are non-decreasing in the output index
    const int span = y1 - y0;
    if (span > lds_rows || y0 < 0 || y1 > Hs) return;          // tables that do not belong to this launch: nothing is written (block-uniform)

    if (x < Wo) {
        const int xmin = bounds_x[2 * x], nx = bounds_x[2 * x + 1];
        const int n = (xmin >= 0 && nx <= ksize_x && xmin + nx <= Ws) ? nx : 0;          // never read outside the frame or the table row
        const int32_t* cx = coef_x + (int64_t)x * ksize_x;
        for (int r = wave; r < span; r += 4) {
            const uint8_t* p = frame + ((int64_t)(y0 + r) * Ws + xmin) * 3;
            uint32_t a0 = 1u << (PP_BITS - 1), a1 = a0, a2 = a0;
            for (int k = 0; k < n; ++k) {
                const uint32_t c = (uint32_t)cx[k];
                a0 += c * p[3 * k];
                a1 += c * p[3 * k + 1];
                a2 += c * p[3 * k + 2];
            }
            uint8_t* q = rows + r * PP_ROW + lane;
            q[0] = (uint8_t)pp_round_clip(a0);
            q[PP_TW] = (uint8_t)pp_round_clip(a1);
            q[2 * PP_TW] = (uint8_t)pp_round_clip(a2);
        }
    }
    __syncthreads();
    if (x >= Wo) return;
    const int nrows = r1 - r0 + 1;
    for (int j = wave; j < nrows * 3; j += 4) {
        const int ty = j / 3, c = j - ty * 3, y = r0 + ty;
        const int ymin = bounds_y[2 * y], ny = bounds_y[2 * y + 1];
        const int n = (ymin >= y0 && ny <= ksize_y && ymin + ny <= y1) ? ny : 0;          // never read outside the rows pass 1 wrote
        const int32_t* cy = coef_y + (int64_t)y * ksize_y;
        const uint8_t* q = rows + (ymin - y0) * PP_ROW + c * PP_TW + lane;
        uint32_t a = 1u << (PP_BITS - 1);
        for (int k = 0; k < n; ++k) a += (uint32_t)cy[k] * q[k * PP_ROW];
        // the reference's three fp32 operations in its order: to_tensor's / 255, then normalize's subtraction and division (not one multiply-add)
        const float v = (float)pp_round_clip(a) / 255.f;
        plane[((int64_t)c * Ho + y) * Wo + x] = (v - nm.mean[c]) / nm.std[c];
    }
}

__global__ __launch_bounds__(256) void resize_norm_u8_kernel(const uint8_t* __restrict__ src, int64_t frame_stride, int Hs, int Ws,
                                                             const int32_t* __restrict__ coef_x, const int32_t* __restrict__ bounds_x, int ksize_x,
                                                             const int32_t* __restrict__ coef_y, const int32_t* __restrict__ bounds_y, int ksize_y,
                                                             float* __restrict__ out, int Ho, int Wo, int TH, int lds_rows, Norm3 nm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rows[];
    pp_tile(src + (int64_t)blockIdx.z * frame_stride, Hs, Ws, coef_x, bounds_x, ksize_x, coef_y, bounds_y, ksize_y, out + (int64_t)blockIdx.z * 3 * Ho * Wo, Ho, Wo, TH, lds_rows,
            nm, rows);
}

__global__ __launch_bounds__(256) void resize_nearest_u8_kernel(const uint8_t* __restrict__ src, int64_t frame_stride, int Hs, int Ws, const int32_t* __restrict__ idx_y,
                                                                const int32_t* __restrict__ idx_x, int64_t* __restrict__ out, int Ho, int Wo, int64_t total) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
        const int64_t f = i / ((int64_t)Wo * Ho);
        const int ys = min(max(idx_y[yo], 0), Hs - 1), xs = min(max(idx_x[xo], 0), Ws - 1);          // (the tables are clamped already: never read outside the mask)
        out[i] = src[f * frame_stride + (int64_t)ys * Ws + xs];
    }
}

// ---- batched form: sources of mixed sizes, one descriptor per output frame (lavt_pp_item_t), every table an element offset into one int32 buffer ----
static_assert(sizeof(lavt_pp_item_t) == 64 && alignof(lavt_pp_item_t) == 8, "lavt_pp_item_t is 64 bytes (lavt_hip/_capi.py: PPItem, lavt_hip/preprocess.py: ITEM_DTYPE)");

// [off, off + len) lies inside a buffer of `total` elements
__host__ __device__ __forceinline__ bool pp_inside(int64_t off, int64_t len, int64_t total) { return off >= 0 && len >= 0 && off <= total - len; }

__host__ __device__ __forceinline__ bool pp_image_item_inside(const lavt_pp_item_t& it, int Ho, int Wo, int64_t table_elems, int64_t pixel_bytes) {
    return it.Hs > 0 && it.Ws > 0 && it.ksize_x > 0 && it.ksize_y > 0 && pp_inside(it.src_off, (int64_t)it.Hs * it.Ws * 3, pixel_bytes) &&
           pp_inside(it.coef_x, (int64_t)Wo * it.ksize_x, table_elems) && pp_inside(it.bounds_x, 2 * (int64_t)Wo, table_elems) &&
           pp_inside(it.coef_y, (int64_t)Ho * it.ksize_y, table_elems) && pp_inside(it.bounds_y, 2 * (int64_t)Ho, table_elems);
}

__host__ __device__ __forceinline__ bool pp_target_item_inside(const lavt_pp_item_t& it, int Ho, int Wo, int64_t table_elems, int64_t mask_bytes) {
    return it.Hs > 0 && it.Ws > 0 && pp_inside(it.mask_off, (int64_t)it.Hs * it.Ws, mask_bytes) && pp_inside(it.idx_y, Ho, table_elems) &&
           pp_inside(it.idx_x, Wo, table_elems);
}

// pp_tile with blockIdx.z = the descriptor: Hs, Ws, both ksize and the source-row span differ between the work-groups of one launch; TH and lds_rows
// are the launch's (the entry sized them for the worst item).  Everything read from the descriptor is block-uniform, so are the exits.
__global__ __launch_bounds__(256) void resize_norm_u8_batch_kernel(const lavt_pp_item_t* __restrict__ items, const int32_t* __restrict__ tables, int64_t table_elems,
                                                                   const uint8_t* __restrict__ pixels, int64_t pixel_bytes, float* __restrict__ out, int Ho, int Wo,
                                                                   int TH, int lds_rows, Norm3 nm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rows[];
    const lavt_pp_item_t it = items[blockIdx.z];
    if (!pp_image_item_inside(it, Ho, Wo, table_elems, pixel_bytes)) return;          // a descriptor that does not belong to these buffers: nothing is read, nothing written
    pp_tile(pixels + it.src_off, it.Hs, it.Ws, tables + it.coef_x, tables + it.bounds_x, it.ksize_x, tables + it.coef_y, tables + it.bounds_y, it.ksize_y,
            out + (int64_t)blockIdx.z * 3 * Ho * Wo, Ho, Wo, TH, lds_rows, nm, rows);
}

__global__ __launch_bounds__(256) void resize_nearest_u8_batch_kernel(const lavt_pp_item_t* __restrict__ items, const int32_t* __restrict__ tables, int64_t table_elems,
                                                                      const uint8_t* __restrict__ masks, int64_t mask_bytes, int64_t* __restrict__ out, int Ho, int Wo,
                                                                      int64_t total) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
        const lavt_pp_item_t it = items[i / ((int64_t)Wo * Ho)];
        if (!pp_target_item_inside(it, Ho, Wo, table_elems, mask_bytes)) continue;          // a descriptor that does not belong to these buffers: its frame is not written
        const int ys = min(max(tables[it.idx_y + yo], 0), it.Hs - 1), xs = min(max(tables[it.idx_x + xo], 0), it.Ws - 1);          // never read outside the mask
        out[i] = masks[it.mask_off + (int64_t)ys * it.Ws + xs];
    }
}

// ---- pseudo-video augmentation: Pillow's affine transform of uint8 sources into uint8 frames of the same size (lavt_pp_warp_t) ----
static_assert(sizeof(lavt_pp_warp_t) == 128 && alignof(lavt_pp_warp_t) == 8, "lavt_pp_warp_t is 128 bytes (lavt_hip/_capi.py: PPWarp, lavt_hip/preprocess.py: WARP_DTYPE)");
constexpr int PP_SIDE_MAX = 8192;
constexpr int PP_WARP_ROWS = 4;                   // output rows of a work-group: one per wave, lane = x

__host__ __device__ __forceinline__ bool pp_finite(double v) { return v - v == 0.0; }          // false for NaN and both infinities

__host__ __device__ __forceinline__ bool pp_warp_inside(const lavt_pp_warp_t& w, int channels, int64_t src_bytes, int64_t dst_bytes) {
    return w.Hs > 0 && w.Ws > 0 && w.Hs <= PP_SIDE_MAX && w.Ws <= PP_SIDE_MAX && pp_inside(w.src_off, (int64_t)w.Hs * w.Ws * channels, src_bytes) &&
           pp_inside(w.dst_off, (int64_t)w.Hs * w.Ws * channels, dst_bytes);
}

__host__ __device__ __forceinline__ bool pp_warp_finite(const lavt_pp_warp_t& w) {
    return pp_finite(w.a[0]) && pp_finite(w.a[1]) && pp_finite(w.a[2]) && pp_finite(w.a[3]) && pp_finite(w.a[4]) && pp_finite(w.a[5]);
}

// Pillow's fixed-point source coordinate of output (x, y), in 64 bits: what its 32-bit `int` holds wherever that does not overflow
__host__ __device__ __forceinline__ int64_t pp_fixed(int32_t c, int32_t cy, int32_t cx, int x, int y) { return (int64_t)c + (int64_t)cy * y + (int64_t)cx * x; }

__host__ __device__ __forceinline__ bool pp_fits_i32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

__host__ __device__ __forceinline__ bool pp_warp_fixed_fits(const lavt_pp_warp_t& w) {
    for (int cy = 0; cy < 2; ++cy)
        for (int cx = 0; cx < 2; ++cx)
            if (!pp_fits_i32(pp_fixed(w.A[2], w.A[1], w.A[0], cx * w.Ws, cy * w.Hs)) || !pp_fits_i32(pp_fixed(w.A[5], w.A[4], w.A[3], cx * w.Ws, cy * w.Hs))) return false;
    return true;
}

// Pillow's bilinear_filter32RGB behind affine_transform (Geometry.c), fp64.  Every product and sum is rounded on its own, as Pillow's build does:
// hipcc would contract a * b + c into one fma, which moves isolated pixels by one.
// Grid (x tiles of 64, row groups of 4, descriptor); lanes of a wave are neighbours along x, so their gathers fall into the same few source rows.
__global__ __launch_bounds__(256) void affine_u8_batch_kernel(const lavt_pp_warp_t* __restrict__ warps, const uint8_t* __restrict__ src, int64_t src_bytes,
                                                              uint8_t* __restrict__ dst, int64_t dst_bytes) {
#pragma clang fp contract(off)
    const lavt_pp_warp_t w = warps[blockIdx.z];
    if (!pp_warp_inside(w, 3, src_bytes, dst_bytes) || !pp_warp_finite(w)) return;          // a descriptor that does not belong to these buffers: nothing is read, nothing written
    const int x = blockIdx.x * PP_TW + (threadIdx.x & 63), y = blockIdx.y * PP_WARP_ROWS + (threadIdx.x >> 6);
    if (x >= w.Ws || y >= w.Hs) return;
    const uint8_t* p = src + w.src_off;
    uint8_t* q = dst + w.dst_off + ((int64_t)y * w.Ws + x) * 3;
    const double xc = x + 0.5, yc = y + 0.5;
    double xin = w.a[0] * xc + w.a[1] * yc + w.a[2];
    double yin = w.a[3] * xc + w.a[4] * yc + w.a[5];
    if (xin < 0.0 || xin >= (double)w.Ws || yin < 0.0 || yin >= (double)w.Hs) {
        q[0] = 0; q[1] = 0; q[2] = 0;
        return;
    }
    xin -= 0.5;
    yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);          // xin, yin lie in [-0.5, 8192): the casts are exact
    const int x0 = (int)fx, y0 = (int)fy;
    const double dx = xin - fx, dy = yin - fy;
    const int xa = min(max(x0, 0), w.Ws - 1), xb = min(max(x0 + 1, 0), w.Ws - 1);          // columns clamp ...
    const uint8_t* r1 = p + (int64_t)min(max(y0, 0), w.Hs - 1) * w.Ws * 3;
    const bool below = y0 + 1 >= 0 && y0 + 1 < w.Hs;                                        // ... the second row does not: past the last row v2 = v1
    const uint8_t* r2 = p + (int64_t)(below ? y0 + 1 : 0) * w.Ws * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a1 = r1[xa * 3 + c], b1 = r1[xb * 3 + c];
        const double v1 = a1 + (b1 - a1) * dx;
        double v2 = v1;
        if (below) {
            const double a2 = r2[xa * 3 + c], b2 = r2[xb * 3 + c];
            v2 = a2 + (b2 - a2) * dx;
        }
        q[c] = (uint8_t)(int)(v1 + (v2 - v1) * dy);          // (UINT8) of Pillow: truncation
    }
}

// Pillow's affine_fixed (general) and ImagingScaleAffine (axis-aligned, through the host's index tables) for single-channel masks
__global__ __launch_bounds__(256) void affine_nearest_u8_batch_kernel(const lavt_pp_warp_t* __restrict__ warps, const int32_t* __restrict__ tables, int64_t table_elems,
                                                                      const uint8_t* __restrict__ src, int64_t src_bytes, uint8_t* __restrict__ dst, int64_t dst_bytes) {
    const lavt_pp_warp_t w = warps[blockIdx.z];
    if (!pp_warp_inside(w, 1, src_bytes, dst_bytes)) return;
    const bool by_tables = w.mode == LAVT_WARP_TABLES;
    if (by_tables ? !(pp_inside(w.idx_x, w.Ws, table_elems) && pp_inside(w.idx_y, w.Hs, table_elems)) : (w.mode != LAVT_WARP_FIXED || !pp_warp_fixed_fits(w))) return;
    const int x = blockIdx.x * PP_TW + (threadIdx.x & 63), y = blockIdx.y * PP_WARP_ROWS + (threadIdx.x >> 6);
    if (x >= w.Ws || y >= w.Hs) return;
    int64_t xi, yi;
    if (by_tables) {
        xi = tables[w.idx_x + x];
        yi = tables[w.idx_y + y];
    } else {
        xi = pp_fixed(w.A[2], w.A[1], w.A[0], x, y) >> 16;
        yi = pp_fixed(w.A[5], w.A[4], w.A[3], x, y) >> 16;
    }
    const bool in = xi >= 0 && xi < w.Ws && yi >= 0 && yi < w.Hs;          // (also what keeps a table entry that does not belong from being followed)
    dst[w.dst_off + (int64_t)y * w.Ws + x] = in ? src[w.src_off + yi * w.Ws + xi] : (uint8_t)0;
}

}  // namespace

extern "C" int lavt_affine_u8_batch(const lavt_pp_warp_t* warps, const lavt_pp_warp_t* warps_host, int n, const uint8_t* src, int64_t src_bytes, uint8_t* dst,
                                    int64_t dst_bytes, void* stream) {
    LAVT_CHECK_ARG(warps && warps_host && src && dst, "lavt_affine_u8_batch: null pointer");
    LAVT_CHECK_ARG(n > 0 && n <= 65535 && src_bytes > 0 && dst_bytes > 0, "lavt_affine_u8_batch: bad sizes (1 <= n <= 65535)");
    int Hmax = 0, Wmax = 0;
    for (int i = 0; i < n; ++i) {
        const lavt_pp_warp_t& w = warps_host[i];
        LAVT_CHECK_ARG(w.Hs > 0 && w.Ws > 0 && w.Hs <= PP_SIDE_MAX && w.Ws <= PP_SIDE_MAX, "lavt_affine_u8_batch: warp %d: source %d x %d: sides are 1..%d", i, w.Hs, w.Ws, PP_SIDE_MAX);
        LAVT_CHECK_ARG(pp_inside(w.src_off, (int64_t)w.Hs * w.Ws * 3, src_bytes), "lavt_affine_u8_batch: warp %d: a %d x %d x 3 source at byte offset %lld lies outside the %lld bytes of pixels", i,
                       w.Hs, w.Ws, (long long)w.src_off, (long long)src_bytes);
        LAVT_CHECK_ARG(pp_inside(w.dst_off, (int64_t)w.Hs * w.Ws * 3, dst_bytes), "lavt_affine_u8_batch: warp %d: a %d x %d x 3 frame at byte offset %lld lies outside the %lld bytes of the destination",
                       i, w.Hs, w.Ws, (long long)w.dst_off, (long long)dst_bytes);
        LAVT_CHECK_ARG(pp_warp_finite(w), "lavt_affine_u8_batch: warp %d: a coefficient is not finite", i);
        Hmax = w.Hs > Hmax ? w.Hs : Hmax;
        Wmax = w.Ws > Wmax ? w.Ws : Wmax;
    }
    hipLaunchKernelGGL(affine_u8_batch_kernel, dim3(cdiv(Wmax, PP_TW), cdiv(Hmax, PP_WARP_ROWS), n), dim3(256), 0, ST, warps, src, src_bytes, dst, dst_bytes);
    LAVT_CHECK_LAUNCH("lavt_affine_u8_batch");
    return LAVT_OK;
}

extern "C" int lavt_affine_nearest_u8_batch(const lavt_pp_warp_t* warps, const lavt_pp_warp_t* warps_host, int n, const int32_t* tables, const int32_t* tables_host,
                                            int64_t table_elems, const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, void* stream) {
    LAVT_CHECK_ARG(warps && warps_host && src && dst, "lavt_affine_nearest_u8_batch: null pointer");
    LAVT_CHECK_ARG(n > 0 && n <= 65535 && src_bytes > 0 && dst_bytes > 0 && table_elems >= 0, "lavt_affine_nearest_u8_batch: bad sizes (1 <= n <= 65535)");
    LAVT_CHECK_ARG(table_elems == 0 || (tables && tables_host), "lavt_affine_nearest_u8_batch: %lld table elements, but no tables", (long long)table_elems);
    int Hmax = 0, Wmax = 0;
    for (int i = 0; i < n; ++i) {
        const lavt_pp_warp_t& w = warps_host[i];
        LAVT_CHECK_ARG(w.Hs > 0 && w.Ws > 0 && w.Hs <= PP_SIDE_MAX && w.Ws <= PP_SIDE_MAX, "lavt_affine_nearest_u8_batch: warp %d: mask %d x %d: sides are 1..%d", i, w.Hs, w.Ws, PP_SIDE_MAX);
        LAVT_CHECK_ARG(pp_inside(w.src_off, (int64_t)w.Hs * w.Ws, src_bytes), "lavt_affine_nearest_u8_batch: warp %d: a %d x %d mask at byte offset %lld lies outside the %lld bytes of masks", i, w.Hs,
                       w.Ws, (long long)w.src_off, (long long)src_bytes);
        LAVT_CHECK_ARG(pp_inside(w.dst_off, (int64_t)w.Hs * w.Ws, dst_bytes), "lavt_affine_nearest_u8_batch: warp %d: a %d x %d mask at byte offset %lld lies outside the %lld bytes of the destination", i,
                       w.Hs, w.Ws, (long long)w.dst_off, (long long)dst_bytes);
        LAVT_CHECK_ARG(w.mode == LAVT_WARP_FIXED || w.mode == LAVT_WARP_TABLES, "lavt_affine_nearest_u8_batch: warp %d: mode %d is neither LAVT_WARP_FIXED nor LAVT_WARP_TABLES", i, w.mode);
        if (w.mode == LAVT_WARP_FIXED) {
            LAVT_CHECK_ARG(pp_warp_fixed_fits(w), "lavt_affine_nearest_u8_batch: warp %d: the 16.16 fixed-point coordinates overflow int32 at a corner of the %d x %d frame", i, w.Hs, w.Ws);
        } else {
            LAVT_CHECK_ARG(pp_inside(w.idx_x, w.Ws, table_elems) && pp_inside(w.idx_y, w.Hs, table_elems),
                           "lavt_affine_nearest_u8_batch: warp %d: an index table (idx_x %d, idx_y %d) lies outside the %lld table elements", i, w.idx_x, w.idx_y, (long long)table_elems);
            const int32_t *ix = tables_host + w.idx_x, *iy = tables_host + w.idx_y;
            for (int x = 0; x < w.Ws; ++x)
                LAVT_CHECK_ARG(ix[x] >= -1 && ix[x] < w.Ws, "lavt_affine_nearest_u8_batch: warp %d: idx_x[%d] = %d is neither -1 nor a column of a %d-column mask", i, x, ix[x], w.Ws);
            for (int y = 0; y < w.Hs; ++y)
                LAVT_CHECK_ARG(iy[y] >= -1 && iy[y] < w.Hs, "lavt_affine_nearest_u8_batch: warp %d: idx_y[%d] = %d is neither -1 nor a row of a %d-row mask", i, y, iy[y], w.Hs);
        }
        Hmax = w.Hs > Hmax ? w.Hs : Hmax;
        Wmax = w.Ws > Wmax ? w.Ws : Wmax;
    }
    hipLaunchKernelGGL(affine_nearest_u8_batch_kernel, dim3(cdiv(Wmax, PP_TW), cdiv(Hmax, PP_WARP_ROWS), n), dim3(256), 0, ST, warps, tables, table_elems, src, src_bytes, dst, dst_bytes);
    LAVT_CHECK_LAUNCH("lavt_affine_nearest_u8_batch");
    return LAVT_OK;
}

extern "C" int lavt_resize_norm_u8_batch(const lavt_pp_item_t* items, const lavt_pp_item_t* items_host, int n, const int32_t* tables, const int32_t* tables_host,
                                         int64_t table_elems, const uint8_t* pixels, int64_t pixel_bytes, float* out, int Ho, int Wo, float mean0, float mean1,
                                         float mean2, float std0, float std1, float std2, void* stream) {
    LAVT_CHECK_ARG(items && items_host && tables && tables_host && pixels && out, "lavt_resize_norm_u8_batch: null pointer");
    LAVT_CHECK_ARG(n > 0 && n <= 65535 && Ho > 0 && Wo > 0 && table_elems > 0 && pixel_bytes > 0, "lavt_resize_norm_u8_batch: bad sizes (1 <= n <= 65535)");
    LAVT_CHECK_ARG(std0 != 0.f && std1 != 0.f && std2 != 0.f, "lavt_resize_norm_u8_batch: std must be nonzero");
    for (int i = 0; i < n; ++i) {
        const lavt_pp_item_t& it = items_host[i];
        LAVT_CHECK_ARG(it.Hs > 0 && it.Ws > 0 && it.ksize_x > 0 && it.ksize_y > 0, "lavt_resize_norm_u8_batch: item %d: source %d x %d with %d / %d taps: all must be positive", i,
                       it.Hs, it.Ws, it.ksize_x, it.ksize_y);
        LAVT_CHECK_ARG(pp_inside(it.src_off, (int64_t)it.Hs * it.Ws * 3, pixel_bytes), "lavt_resize_norm_u8_batch: item %d: a %d x %d x 3 source at byte offset %lld lies outside the %lld bytes of pixels",
                       i, it.Hs, it.Ws, (long long)it.src_off, (long long)pixel_bytes);
        LAVT_CHECK_ARG(pp_image_item_inside(it, Ho, Wo, table_elems, pixel_bytes),
                       "lavt_resize_norm_u8_batch: item %d: a table (coef_x %d, bounds_x %d, coef_y %d, bounds_y %d; %d / %d taps) lies outside the %lld table elements", i, it.coef_x,
                       it.bounds_x, it.coef_y, it.bounds_y, it.ksize_x, it.ksize_y, (long long)table_elems);
        const int32_t *bx = tables_host + it.bounds_x, *by = tables_host + it.bounds_y;
        for (int x = 0; x < Wo; ++x)
            LAVT_CHECK_ARG(bx[2 * x] >= 0 && bx[2 * x + 1] >= 0 && bx[2 * x + 1] <= it.ksize_x && bx[2 * x] + bx[2 * x + 1] <= it.Ws,
                           "lavt_resize_norm_u8_batch: item %d: bounds_x[%d] = (%d, %d) is not a column range of a %d-column source with %d taps", i, x, bx[2 * x], bx[2 * x + 1], it.Ws,
                           it.ksize_x);
        for (int y = 0; y < Ho; ++y) {
            const int ymin = by[2 * y], t = by[2 * y + 1];
            LAVT_CHECK_ARG(ymin >= 0 && t >= 0 && t <= it.ksize_y && ymin + t <= it.Hs && (y == 0 || (ymin >= by[2 * y - 2] && ymin + t >= by[2 * y - 2] + by[2 * y - 1])),
                           "lavt_resize_norm_u8_batch: item %d: bounds_y[%d] = (%d, %d) is not a row range of a %d-row source with %d taps", i, y, ymin, t, it.Hs, it.ksize_y);
        }
    }
    // one tile height for the launch: the largest whose source-row span fits the LDS request for EVERY item
    int TH = 0, lds_rows = 0, worst_item = 0;
    for (int th = 16; th >= 1 && !TH; th >>= 1) {
        int worst = 0;
        for (int i = 0; i < n; ++i) {
            const int32_t* by = tables_host + items_host[i].bounds_y;
            for (int r0 = 0; r0 < Ho; r0 += th) {
                const int r1 = (r0 + th < Ho ? r0 + th : Ho) - 1;
                const int span = by[2 * r1] + by[2 * r1 + 1] - by[2 * r0];
                if (span > worst) { worst = span; worst_item = i; }
            }
        }
        if ((int64_t)worst * PP_ROW <= PP_LDS_MAX) { TH = th; lds_rows = worst; }
    }
    LAVT_CHECK_ARG(TH > 0, "lavt_resize_norm_u8_batch: item %d: %d -> %d rows: one output row reads more source rows than fit %d bytes of LDS (%d bytes each)", worst_item,
                   items_host[worst_item].Hs, Ho, PP_LDS_MAX, PP_ROW);
    const int gy = cdiv(Ho, TH);
    LAVT_CHECK_ARG(gy <= 65535, "lavt_resize_norm_u8_batch: too many output rows for one launch");
    Norm3 nm;
    nm.mean[0] = mean0; nm.mean[1] = mean1; nm.mean[2] = mean2; nm.std[0] = std0; nm.std[1] = std1; nm.std[2] = std2;
    const size_t lds = (size_t)(lds_rows > 0 ? lds_rows : 1) * PP_ROW;
    hipLaunchKernelGGL(resize_norm_u8_batch_kernel, dim3(cdiv(Wo, PP_TW), gy, n), dim3(256), lds, ST, items, tables, table_elems, pixels, pixel_bytes, out, Ho, Wo, TH, lds_rows, nm);
    LAVT_CHECK_LAUNCH("lavt_resize_norm_u8_batch");
    return LAVT_OK;
}

extern "C" int lavt_resize_nearest_u8_batch(const lavt_pp_item_t* items, const lavt_pp_item_t* items_host, int n, const int32_t* tables, const int32_t* tables_host,
                                            int64_t table_elems, const uint8_t* masks, int64_t mask_bytes, int64_t* out, int Ho, int Wo, void* stream) {
    LAVT_CHECK_ARG(items && items_host && tables && tables_host && masks && out, "lavt_resize_nearest_u8_batch: null pointer");
    LAVT_CHECK_ARG(n > 0 && n <= 65535 && Ho > 0 && Wo > 0 && table_elems > 0 && mask_bytes > 0, "lavt_resize_nearest_u8_batch: bad sizes (1 <= n <= 65535)");
    for (int i = 0; i < n; ++i) {
        const lavt_pp_item_t& it = items_host[i];
        LAVT_CHECK_ARG(it.Hs > 0 && it.Ws > 0 && pp_inside(it.mask_off, (int64_t)it.Hs * it.Ws, mask_bytes),
                       "lavt_resize_nearest_u8_batch: item %d: a %d x %d mask at byte offset %lld lies outside the %lld bytes of masks", i, it.Hs, it.Ws, (long long)it.mask_off,
                       (long long)mask_bytes);
        LAVT_CHECK_ARG(pp_target_item_inside(it, Ho, Wo, table_elems, mask_bytes), "lavt_resize_nearest_u8_batch: item %d: an index table (idx_y %d, idx_x %d) lies outside the %lld table elements",
                       i, it.idx_y, it.idx_x, (long long)table_elems);
        const int32_t *iy = tables_host + it.idx_y, *ix = tables_host + it.idx_x;
        for (int y = 0; y < Ho; ++y)
            LAVT_CHECK_ARG(iy[y] >= 0 && iy[y] < it.Hs, "lavt_resize_nearest_u8_batch: item %d: idx_y[%d] = %d is not a row of a %d-row mask", i, y, iy[y], it.Hs);
        for (int x = 0; x < Wo; ++x)
            LAVT_CHECK_ARG(ix[x] >= 0 && ix[x] < it.Ws, "lavt_resize_nearest_u8_batch: item %d: idx_x[%d] = %d is not a column of a %d-column mask", i, x, ix[x], it.Ws);
    }
    const int64_t total = (int64_t)n * Ho * Wo, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(resize_nearest_u8_batch_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, ST, items, tables, table_elems, masks, mask_bytes, out, Ho, Wo,
                       total);
    LAVT_CHECK_LAUNCH("lavt_resize_nearest_u8_batch");
    return LAVT_OK;
}

extern "C" int lavt_resize_norm_u8(const uint8_t* src, int64_t frame_stride, int N, int Hs, int Ws, const int32_t* coef_x, const int32_t* bounds_x, int ksize_x,
                                   const int32_t* coef_y, const int32_t* bounds_y, int ksize_y, const int32_t* bounds_y_host, float* out, int Ho, int Wo,
                                   float mean0, float mean1, float mean2, float std0, float std1, float std2, void* stream) {
    LAVT_CHECK_ARG(src && coef_x && bounds_x && coef_y && bounds_y && bounds_y_host && out, "lavt_resize_norm_u8: null pointer");
    LAVT_CHECK_ARG(N > 0 && N <= 65535 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0 && ksize_x > 0 && ksize_y > 0, "lavt_resize_norm_u8: bad sizes (1 <= N <= 65535)");
    LAVT_CHECK_ARG(frame_stride >= (int64_t)Hs * Ws * 3, "lavt_resize_norm_u8: frame_stride %lld is less than one %d x %d x 3 frame", (long long)frame_stride, Hs, Ws);
    LAVT_CHECK_ARG(std0 != 0.f && std1 != 0.f && std2 != 0.f, "lavt_resize_norm_u8: std must be nonzero");
    for (int y = 0; y < Ho; ++y) {
        const int ymin = bounds_y_host[2 * y], n = bounds_y_host[2 * y + 1];
        LAVT_CHECK_ARG(ymin >= 0 && n >= 0 && n <= ksize_y && ymin + n <= Hs && (y == 0 || (ymin >= bounds_y_host[2 * y - 2] && ymin + n >= bounds_y_host[2 * y - 2] + bounds_y_host[2 * y - 1])),
                       "lavt_resize_norm_u8: bounds_y_host[%d] = (%d, %d) is not a row range of a %d-row source with %d taps", y, ymin, n, Hs, ksize_y);
    }
    // the largest tile height whose source-row span fits the LDS request
    int TH = 0, lds_rows = 0;
    for (int th = 16; th >= 1 && !TH; th >>= 1) {
        int worst = 0;
        for (int r0 = 0; r0 < Ho; r0 += th) {
            const int r1 = (r0 + th < Ho ? r0 + th : Ho) - 1;
            const int span = bounds_y_host[2 * r1] + bounds_y_host[2 * r1 + 1] - bounds_y_host[2 * r0];
            worst = span > worst ? span : worst;
        }
        if ((int64_t)worst * PP_ROW <= PP_LDS_MAX) { TH = th; lds_rows = worst; }
    }
    LAVT_CHECK_ARG(TH > 0, "lavt_resize_norm_u8: %d -> %d rows: one output row reads more source rows than fit %d bytes of LDS (%d bytes each)", Hs, Ho, PP_LDS_MAX, PP_ROW);
    const int gy = cdiv(Ho, TH);
    LAVT_CHECK_ARG(gy <= 65535, "lavt_resize_norm_u8: too many output rows for one launch");
    Norm3 nm;
    nm.mean[0] = mean0; nm.mean[1] = mean1; nm.mean[2] = mean2; nm.std[0] = std0; nm.std[1] = std1; nm.std[2] = std2;
    const size_t lds = (size_t)(lds_rows > 0 ? lds_rows : 1) * PP_ROW;
    hipLaunchKernelGGL(resize_norm_u8_kernel, dim3(cdiv(Wo, PP_TW), gy, N), dim3(256), lds, ST, src, frame_stride, Hs, Ws, coef_x, bounds_x, ksize_x, coef_y, bounds_y,
                       ksize_y, out, Ho, Wo, TH, lds_rows, nm);
    LAVT_CHECK_LAUNCH("lavt_resize_norm_u8");
    return LAVT_OK;
}

extern "C" int lavt_resize_nearest_u8(const uint8_t* src, int64_t frame_stride, int N, int Hs, int Ws, const int32_t* idx_y, const int32_t* idx_x, int64_t* out, int Ho,
                                      int Wo, void* stream) {
    LAVT_CHECK_ARG(src && idx_y && idx_x && out, "lavt_resize_nearest_u8: null pointer");
    LAVT_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "lavt_resize_nearest_u8: bad sizes");
    LAVT_CHECK_ARG(frame_stride >= (int64_t)Hs * Ws, "lavt_resize_nearest_u8: frame_stride %lld is less than one %d x %d mask", (long long)frame_stride, Hs, Ws);
    const int64_t total = (int64_t)N * Ho * Wo, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(resize_nearest_u8_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, ST, src, frame_stride, Hs, Ws, idx_y, idx_x, out, Ho, Wo, total);
    LAVT_CHECK_LAUNCH("lavt_resize_nearest_u8");
    return LAVT_OK;
}
