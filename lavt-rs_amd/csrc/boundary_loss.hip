// Fused bilinear upsample + DiceBoundaryLoss (reference losses.py:142-244, `--loss dice_boundary`, train.py:709-711) on the 2-class low-resolution
// logits: the Dice part is that of lavt_upsample_dice_* (elementwise.hip), the boundary part is a stencil -- per class c, with a = 1 - p_c and
// h = 1 - [t == c]:   pred_b = maxpool3(a) - a,  gt_b = maxpool3(h) - h,  pred_b_ext = maxpool5(pred_b),  gt_b_ext = maxpool5(gt_b)   (stride 1, windows
// clipped at the image border: the reference pads with -inf),   S1 = sum pred_b gt_b_ext, S2 = sum pred_b, S3 = sum pred_b_ext gt_b, S4 = sum gt_b,
// P = S1 / (S2 + 1e-7), R = S3 / (S4 + 1e-7), BF1 = 2 P R / (P + R + 1e-7), boundary = mean_{sample, class} (1 - BF1).
// One workgroup owns one BT x BT output tile of one sample and recomputes what the tile needs in LDS (the full-resolution probabilities are never
// written).  No floating-point atomics: partial rows + a finish kernel in a fixed order, gather-form gradients.
// Every window is clipped to the image; the LDS regions are the tile plus the halo its stage needs, so a clipped window never leaves them.
#include "common.h"
#include "internal.h"

namespace {

constexpr int BT = 32;                   // output tile side
constexpr int NT = 256;                  // threads per workgroup
constexpr int NS = 14;                   // sums per sample: 6 Dice {I0, I1, sum p0^2, sum p1^2, #t==0, #t==1} + per class {S1, S2, S3, S4}
constexpr int FH = 3, FA = BT + 2 * FH;  // forward: a / target on the tile + halo 3 (a 3x3 pool below a 5x5 pool); pred_b / gt_b on halo 2 of the same grid
constexpr int GH = 6, GA = BT + 2 * GH;  // backward: a on the tile + halo 6 (see dice_boundary_dz_kernel)
constexpr float BEPS = 1e-7f;

template <typename T>
__device__ __forceinline__ void probs_at(const T* __restrict__ base, int Hi, int Wi, float sh, float sw, int gy, int gx, float& p0, float& p1) {
    int y0, y1, x0, x1; float ly, lx;
    bl_coord(gy, sh, Hi, y0, y1, ly);
    bl_coord(gx, sw, Wi, x0, x1, lx);
    const UpCe u = upce_at<T>(base, Wi, y0, y1, ly, x0, x1, lx);
    p0 = expf(u.up0 - u.lse); p1 = expf(u.up1 - u.lse);          // (the Dice kernels' own expression)
}
__device__ __forceinline__ uint8_t label_of(int64_t t) { return t == 0 ? 0 : (t == 1 ? 1 : 2); }

// grid (tiles, samples); partial[(sample * tiles + tile) * NS + k].  All stages index ONE FA x FA grid whose origin is the tile's corner - FH.
template <typename T, bool SEL>
__global__ __launch_bounds__(NT) void dice_boundary_fwd_kernel(const T* __restrict__ x, const int32_t* __restrict__ sel, int nfr, const int64_t* __restrict__ target,
                                                               float* __restrict__ partial, int Hi, int Wi, int Ho, int Wo, float sh, float sw, int tiles_x) {
    __shared__ float A[2][FA * FA];           // a_c = 1 - p_c                (halo 3)
    __shared__ float PB[2][FA * FA];          // pred_b_c                     (halo 2)
    __shared__ uint8_t TG[FA * FA];           // label 0 / 1 / 2 = other      (halo 3)
    __shared__ uint8_t GB[2][FA * FA];        // gt_b_c                       (halo 2)
    __shared__ float red[NT / 64][NS];
    const int b = blockIdx.y, fr = sel_frame<SEL>(sel, b, nfr);
    const int oy = (int)(blockIdx.x / tiles_x) * BT - FH, ox = (int)(blockIdx.x % tiles_x) * BT - FH;
    float s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.f;
    if (!SEL || fr >= 0) {                    // (uniform over the workgroup; a sample without a frame leaves zero sums)
        const T* base = x + (int64_t)fr * Hi * Wi * 2;
        const int64_t* tb = target + (int64_t)b * Ho * Wo;
        for (int i = threadIdx.x; i < FA * FA; i += NT) {
            const int ly = i / FA, lx = i - ly * FA, gy = oy + ly, gx = ox + lx;
            if (gy < 0 || gy >= Ho || gx < 0 || gx >= Wo) continue;
            float p0, p1;
            probs_at<T>(base, Hi, Wi, sh, sw, gy, gx, p0, p1);
            A[0][i] = 1.f - p0; A[1][i] = 1.f - p1;
            const uint8_t t = label_of(tb[(int64_t)gy * Wo + gx]);
            TG[i] = t;
            if (ly >= FH && ly < FH + BT && lx >= FH && lx < FH + BT) {          // the tile proper: the Dice sums
                if (t == 0) { s[0] += p0; s[4] += 1.f; }
                if (t == 1) { s[1] += p1; s[5] += 1.f; }
                s[2] += p0 * p0; s[3] += p1 * p1;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < FA * FA; i += NT) {
            const int ly = i / FA, lx = i - ly * FA, gy = oy + ly, gx = ox + lx;
            if (ly < 1 || ly >= FA - 1 || lx < 1 || lx >= FA - 1 || gy < 0 || gy >= Ho || gx < 0 || gx >= Wo) continue;
            const int y0 = max(gy - 1, 0) - oy, y1 = min(gy + 1, Ho - 1) - oy, x0 = max(gx - 1, 0) - ox, x1 = min(gx + 1, Wo - 1) - ox;      // within [0, FA)
            float m0 = -INFINITY, m1 = -INFINITY;
            bool o0 = false, o1 = false;
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx) {
                    const int j = yy * FA + xx;
                    m0 = fmaxf(m0, A[0][j]); m1 = fmaxf(m1, A[1][j]);
                    o0 |= TG[j] != 0; o1 |= TG[j] != 1;
                }
            PB[0][i] = m0 - A[0][i]; PB[1][i] = m1 - A[1][i];
            GB[0][i] = (TG[i] == 0 && o0) ? 1 : 0; GB[1][i] = (TG[i] == 1 && o1) ? 1 : 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < BT * BT; i += NT) {
            const int ty = i / BT, ly = ty + FH, lx = i - ty * BT + FH, gy = oy + ly, gx = ox + lx;
            if (gy >= Ho || gx >= Wo) continue;
            const int y0 = max(gy - 2, 0) - oy, y1 = min(gy + 2, Ho - 1) - oy, x0 = max(gx - 2, 0) - ox, x1 = min(gx + 2, Wo - 1) - ox;      // within [1, FA - 1)
            float e0 = -INFINITY, e1 = -INFINITY;
            uint8_t g0 = 0, g1 = 0;
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx) {
                    const int j = yy * FA + xx;
                    e0 = fmaxf(e0, PB[0][j]); e1 = fmaxf(e1, PB[1][j]);
                    g0 |= GB[0][j]; g1 |= GB[1][j];
                }
            const int c = ly * FA + lx;
            const float pb0 = PB[0][c], pb1 = PB[1][c], gb0 = (float)GB[0][c], gb1 = (float)GB[1][c];
            s[6] += pb0 * (float)g0; s[7] += pb0; s[8] += e0 * gb0; s[9] += gb0;
            s[10] += pb1 * (float)g1; s[11] += pb1; s[12] += e1 * gb1; s[13] += gb1;
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NS; ++k) red[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x < NS) partial[((int64_t)b * gridDim.x + blockIdx.x) * NS + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// stats = {loss, dice, boundary, then per sample the NS sums}; a sample whose sel entry lies outside [0, nfr) adds no term (the means stay over n samples)
__global__ __launch_bounds__(NT) void dice_boundary_finish_kernel(const float* __restrict__ partial, int nblk, int n, float* __restrict__ stats,
                                                                  const int32_t* __restrict__ sel, int nfr, float dice_rate, float boundary_rate) {
    __shared__ float red[NT / 64][NS];
    __shared__ float dice_acc, bnd_acc;
    if (threadIdx.x == 0) { dice_acc = 0.f; bnd_acc = 0.f; }
    for (int b = 0; b < n; ++b) {
        float a[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) a[j] = 0.f;
        for (int k = threadIdx.x; k < nblk; k += NT)
#pragma unroll
            for (int j = 0; j < NS; ++j) a[j] += partial[((int64_t)b * nblk + k) * NS + j];
#pragma unroll
        for (int j = 0; j < NS; ++j) a[j] = wave_sum(a[j]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int j = 0; j < NS; ++j) red[threadIdx.x >> 6][j] = a[j];
        __syncthreads();
        if (threadIdx.x == 0) {
            float v[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) { v[j] = red[0][j] + red[1][j] + red[2][j] + red[3][j]; stats[3 + b * NS + j] = v[j]; }
            if (!sel || (sel[b] >= 0 && sel[b] < nfr)) {
                dice_acc += (1.f - 2.f * v[0] / (v[2] + v[4] + 1e-6f)) + (1.f - 2.f * v[1] / (v[3] + v[5] + 1e-6f));
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float* q = v + 6 + 4 * c;
                    const float P = q[0] / (q[1] + BEPS), R = q[2] / (q[3] + BEPS);
                    bnd_acc += 1.f - 2.f * P * R / (P + R + BEPS);
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        const float dice = dice_acc / (2.f * (float)n), bnd = bnd_acc / (2.f * (float)n);
        stats[0] = dice_rate * dice + boundary_rate * bnd; stats[1] = dice; stats[2] = bnd;
    }
}

// Backward, launch A: dz[sample][Ho][Wo] (fp32) = d loss / d (z1 - z0) per full-resolution pixel, gather form.  All stages index ONE GA x GA grid whose origin
// is the tile's corner - GH; "halo h" = the tile grown by h.  With G1 = dL/dS1, G2 = dL/dS2, G3 = dL/dS3 of the pixel's (sample, class):
//   a on halo 6;  pred_b and argmax3 (of a) on halo 5;  gt_b and, where gt_b = 1, argmax5 (of pred_b) on halo 3;
//   D(q) = dL/d pred_b(q) = gt_b_ext(q) G1 + G2 + G3 #{r in the 5x5 of q : gt_b(r) = 1, argmax5(r) = q}                         on halo 1;
//   dL/da(s) = -D(s) + sum_{q in the 3x3 of s, argmax3(q) = s} D(q)                                                              on the tile.
// The arg-max is torch's: the window scanned row-major, the first maximum wins (`val > max`) -- whole windows tie where the softmax saturates.
template <typename T, bool SEL>
__global__ __launch_bounds__(NT) void dice_boundary_dz_kernel(const T* __restrict__ x, const int32_t* __restrict__ sel, int nfr, int nsamp, const int64_t* __restrict__ target,
                                                              const float* __restrict__ stats, float* __restrict__ dz, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                              int tiles_x, float dice_rate, float boundary_rate) {
    __shared__ float A[2][GA * GA];           // a_c (halo 6); from stage 4 on: D_c (halo 1) -- a is last read in stage 2, two barriers earlier
    __shared__ float PB[2][GA * GA];          // pred_b_c (halo 5)
    __shared__ uint8_t A3[2][GA * GA];        // argmax3 of a as (dy + 1) * 3 + (dx + 1)                         (halo 5)
    __shared__ uint8_t A5[2][GA * GA];        // argmax5 of pred_b as (dy + 2) * 5 + (dx + 2); 255: gt_b = 0     (halo 3)
    __shared__ uint8_t TG[GA * GA];           // label (halo 6)
    const int b = blockIdx.y, fr = sel_frame<SEL>(sel, b, nfr);
    const int oy = (int)(blockIdx.x / tiles_x) * BT - GH, ox = (int)(blockIdx.x % tiles_x) * BT - GH;
    float* dzb = dz + (int64_t)b * Ho * Wo;
    if (SEL && fr < 0) {                      // (uniform) no frame: launch B never reads this sample's map; leave it defined all the same
        for (int i = threadIdx.x; i < BT * BT; i += NT) {
            const int ty = i / BT, gy = oy + GH + ty, gx = ox + GH + i - ty * BT;
            if (gy < Ho && gx < Wo) dzb[(int64_t)gy * Wo + gx] = 0.f;
        }
        return;
    }
    const T* base = x + (int64_t)fr * Hi * Wi * 2;
    const int64_t* tb = target + (int64_t)b * Ho * Wo;
    for (int i = threadIdx.x; i < GA * GA; i += NT) {
        const int ly = i / GA, lx = i - ly * GA, gy = oy + ly, gx = ox + lx;
        if (gy < 0 || gy >= Ho || gx < 0 || gx >= Wo) continue;
        float p0, p1;
        probs_at<T>(base, Hi, Wi, sh, sw, gy, gx, p0, p1);
        A[0][i] = 1.f - p0; A[1][i] = 1.f - p1;
        TG[i] = label_of(tb[(int64_t)gy * Wo + gx]);
    }
    __syncthreads();
    // stage 2: pred_b, argmax3 on halo 5
    for (int i = threadIdx.x; i < GA * GA; i += NT) {
        const int ly = i / GA, lx = i - ly * GA, gy = oy + ly, gx = ox + lx;
        if (ly < 1 || ly >= GA - 1 || lx < 1 || lx >= GA - 1 || gy < 0 || gy >= Ho || gx < 0 || gx >= Wo) continue;
        const int y0 = max(gy - 1, 0) - oy, y1 = min(gy + 1, Ho - 1) - oy, x0 = max(gx - 1, 0) - ox, x1 = min(gx + 1, Wo - 1) - ox;          // within [0, GA)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float m = -INFINITY;
            int code = (y0 - ly + 1) * 3 + (x0 - lx + 1);
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx) {
                    const float v = A[c][yy * GA + xx];
                    if (v > m) { m = v; code = (yy - ly + 1) * 3 + (xx - lx + 1); }
                }
            PB[c][i] = m - A[c][i];
            A3[c][i] = (uint8_t)code;
        }
    }
    __syncthreads();
    // stage 3: gt_b and argmax5 on halo 3
    for (int i = threadIdx.x; i < GA * GA; i += NT) {
        const int ly = i / GA, lx = i - ly * GA, gy = oy + ly, gx = ox + lx;
        if (ly < 3 || ly >= GA - 3 || lx < 3 || lx >= GA - 3 || gy < 0 || gy >= Ho || gx < 0 || gx >= Wo) continue;
        const int t = TG[i];
        A5[0][i] = 255; A5[1][i] = 255;
        if (t > 1) continue;                  // gt_b_c(i) = 1 needs t == c
        bool other = false;
        {
            const int y0 = max(gy - 1, 0) - oy, y1 = min(gy + 1, Ho - 1) - oy, x0 = max(gx - 1, 0) - ox, x1 = min(gx + 1, Wo - 1) - ox;      // within [2, GA - 2)
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx) other |= TG[yy * GA + xx] != t;
        }
        if (!other) continue;
        const int y0 = max(gy - 2, 0) - oy, y1 = min(gy + 2, Ho - 1) - oy, x0 = max(gx - 2, 0) - ox, x1 = min(gx + 2, Wo - 1) - ox;          // within [1, GA - 1)
        float m = -INFINITY;
        int code = (y0 - ly + 2) * 5 + (x0 - lx + 2);
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) {
                const float v = PB[t][yy * GA + xx];
                if (v > m) { m = v; code = (yy - ly + 2) * 5 + (xx - lx + 2); }
            }
        A5[t][i] = (uint8_t)code;
    }
    __syncthreads();
    // the gradients of the sample's sums (every thread: a handful of scalar loads)
    const float* sb = stats + 3 + b * NS;
    const float invn = 0.5f / (float)nsamp;                  // mean over (sample, class)
    float G1[2], G2[2], G3[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* q = sb + 6 + 4 * c;
        const float d2 = q[1] + BEPS, d4 = q[3] + BEPS, P = q[0] / d2, R = q[2] / d4, den = P + R + BEPS;
        const float k = -boundary_rate * invn, dP = k * 2.f * R * (R + BEPS) / (den * den), dR = k * 2.f * P * (P + BEPS) / (den * den);
        G1[c] = dP / d2; G2[c] = -dP * q[0] / (d2 * d2); G3[c] = dR / d4;
    }
    // stage 4: D on halo 1 (into A)
    for (int i = threadIdx.x; i < GA * GA; i += NT) {
        const int ly = i / GA, lx = i - ly * GA, gy = oy + ly, gx = ox + lx;
        if (ly < 5 || ly >= GA - 5 || lx < 5 || lx >= GA - 5 || gy < 0 || gy >= Ho || gx < 0 || gx >= Wo) continue;
        const int y0 = max(gy - 2, 0) - oy, y1 = min(gy + 2, Ho - 1) - oy, x0 = max(gx - 2, 0) - ox, x1 = min(gx + 2, Wo - 1) - ox;          // within [3, GA - 3)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            int cnt = 0;
            bool ext = false;
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx) {
                    const int code = A5[c][yy * GA + xx];
                    ext |= code != 255;
                    cnt += code == (ly - yy + 2) * 5 + (lx - xx + 2);
                }
            A[c][i] = (ext ? G1[c] : 0.f) + G2[c] + G3[c] * (float)cnt;
        }
    }
    __syncthreads();
    // stage 5: dL/da on the tile, the Dice term, the 2-class softmax Jacobian
    const float c0 = sb[2] + sb[4] + 1e-6f, c1 = sb[3] + sb[5] + 1e-6f, dn = dice_rate * invn;
    const float A0 = -2.f * dn / c0, A1 = -2.f * dn / c1, E0 = 2.f * dn * sb[0] / (c0 * c0), E1 = 2.f * dn * sb[1] / (c1 * c1);
    for (int i = threadIdx.x; i < BT * BT; i += NT) {
        const int ty = i / BT, ly = ty + GH, lx = i - ty * BT + GH, gy = oy + ly, gx = ox + lx;
        if (gy >= Ho || gx >= Wo) continue;
        const int y0 = max(gy - 1, 0) - oy, y1 = min(gy + 1, Ho - 1) - oy, x0 = max(gx - 1, 0) - ox, x1 = min(gx + 1, Wo - 1) - ox;          // within [5, GA - 5)
        const int ctr = ly * GA + lx;
        float da[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float acc = 0.f;
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx)
                    if ((int)A3[c][yy * GA + xx] == (ly - yy + 1) * 3 + (lx - xx + 1)) acc += A[c][yy * GA + xx];
            da[c] = acc - A[c][ctr];
        }
        float p0, p1;
        probs_at<T>(base, Hi, Wi, sh, sw, gy, gx, p0, p1);
        const int t = TG[ctr];
        const float g0 = (t == 0 ? A0 : 0.f) + 2.f * p0 * E0 - da[0], g1 = (t == 1 ? A1 : 0.f) + 2.f * p1 * E1 - da[1];          // dL/dp_c (a_c = 1 - p_c)
        dzb[(int64_t)gy * Wo + gx] = p0 * p1 * (g1 - g0);
    }
}

// Backward, launch B: the transposed bilinear of the dz map, gathered per low-resolution pixel (no atomics): dx[b, yi, xi, :] = dloss * (-s, +s).
// B = frames of x / dx, nsel = samples of the loss (SEL = false: the same number); a frame that feeds no sample gets +0.0
template <typename T, bool SEL>
__global__ __launch_bounds__(256) void dice_boundary_dx_kernel(const float* __restrict__ dz, const int32_t* __restrict__ sel, int nsel, const float* __restrict__ dloss,
                                                               T* __restrict__ dx, int B, int Hi, int Wi, int Ho, int Wo, float sh, float sw) {
    const int64_t n = (int64_t)B * Hi * Wi;
    const float g = dloss ? dloss[0] : 1.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int xi = (int)(i % Wi), yi = (int)((i / Wi) % Hi), b = (int)(i / Wi / Hi);
        const int js = sel_sample<SEL>(sel, nsel, b);
        if (SEL && js < 0) {
            dx[i * 2] = from_f<T>(0.f);
            dx[i * 2 + 1] = from_f<T>(0.f);
            continue;
        }
        int ylo, yhi, xlo, xhi;
        bl_range(yi, sh, Hi, Ho, ylo, yhi);
        bl_range(xi, sw, Wi, Wo, xlo, xhi);
        const float* m = dz + (int64_t)js * Ho * Wo;
        float acc = 0.f;
        for (int yo = ylo; yo <= yhi; ++yo) {
            int y0, y1; float ly;
            bl_coord(yo, sh, Hi, y0, y1, ly);
            const float wy = (y0 == yi ? 1.f - ly : 0.f) + (y1 == yi ? ly : 0.f);
            if (wy == 0.f) continue;
            for (int xo = xlo; xo <= xhi; ++xo) {
                int x0, x1; float lx;
                bl_coord(xo, sw, Wi, x0, x1, lx);
                const float wx = (x0 == xi ? 1.f - lx : 0.f) + (x1 == xi ? lx : 0.f);
                if (wx == 0.f) continue;
                acc += wy * wx * m[(int64_t)yo * Wo + xo];
            }
        }
        dx[i * 2] = from_f<T>(-acc * g);
        dx[i * 2 + 1] = from_f<T>(acc * g);
    }
}

}  // namespace

#define DISPATCH_T(dtype, NAME, ...)                                   \
    if (dtype == LAVT_F32) { using T = float; __VA_ARGS__; }           \
    else if (dtype == LAVT_BF16) { using T = bf16; __VA_ARGS__; }      \
    else { lavt_set_error(NAME ": bad dtype %d", dtype); return LAVT_ERR_INVALID; }
#define ST reinterpret_cast<hipStream_t>(stream)

static inline int64_t db_tiles(int Ho, int Wo) { return (int64_t)cdiv(Ho, BT) * cdiv(Wo, BT); }
static inline int64_t db_rows(int n, int Ho, int Wo) { return db_tiles(Ho, Wo) * NS * n; }

// scratch of one forward + backward over n samples: the partial rows (head, forward), then the dz map [n][Ho][Wo] (tail, backward)
extern "C" int64_t lavt_upsample_dice_boundary_ws(int n, int Ho, int Wo) {
    if (n <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return db_rows(n, Ho, Wo) + (int64_t)n * Ho * Wo;
}

#define DB_CHECK_SHAPE(name, ns)                                                                                                                          \
    LAVT_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && (ns) > 0 && (ns) <= 65535 && db_tiles(Ho, Wo) < (1LL << 31), name ": bad shape");     \
    LAVT_CHECK_ARG(ws_floats >= lavt_upsample_dice_boundary_ws(ns, Ho, Wo), name ": scratch of %lld floats needed (lavt_upsample_dice_boundary_ws)",       \
                   (long long)lavt_upsample_dice_boundary_ws(ns, Ho, Wo))

template <bool SEL>
static int dice_boundary_fwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float dice_rate, float boundary_rate, float* ws,
                             int64_t ws_floats, float* stats, int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    const int ns = SEL ? nsel : B, tiles = (int)db_tiles(Ho, Wo);
    DISPATCH_T(dtype, "lavt_upsample_dice_boundary_fwd", hipLaunchKernelGGL((dice_boundary_fwd_kernel<T, SEL>), dim3(tiles, ns), dim3(NT), 0, ST, (const T*)x, sel, B, target, ws, Hi, Wi, Ho, Wo, bl_scale(Hi, Ho), bl_scale(Wi, Wo), cdiv(Wo, BT)));
    hipLaunchKernelGGL(dice_boundary_finish_kernel, dim3(1), dim3(NT), 0, ST, ws, tiles, ns, stats, sel, B, dice_rate, boundary_rate);
    LAVT_CHECK_LAUNCH("lavt_upsample_dice_boundary_fwd");
    return LAVT_OK;
}
template <bool SEL>
static int dice_boundary_bwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float dice_rate, float boundary_rate, const float* stats,
                             const float* dloss, float* ws, void* dx, int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    const int ns = SEL ? nsel : B, tiles = (int)db_tiles(Ho, Wo);
    float* dz = ws + db_rows(ns, Ho, Wo);
    const int64_t n = (int64_t)B * Hi * Wi;
    const int64_t blocks = (n + 255) / 256;
    const int grid = (int)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
    DISPATCH_T(dtype, "lavt_upsample_dice_boundary_bwd",
               hipLaunchKernelGGL((dice_boundary_dz_kernel<T, SEL>), dim3(tiles, ns), dim3(NT), 0, ST, (const T*)x, sel, B, ns, target, stats, dz, Hi, Wi, Ho, Wo, bl_scale(Hi, Ho), bl_scale(Wi, Wo), cdiv(Wo, BT), dice_rate, boundary_rate);
               hipLaunchKernelGGL((dice_boundary_dx_kernel<T, SEL>), dim3(grid), dim3(256), 0, ST, dz, sel, ns, dloss, (T*)dx, B, Hi, Wi, Ho, Wo, bl_scale(Hi, Ho), bl_scale(Wi, Wo)));
    LAVT_CHECK_LAUNCH("lavt_upsample_dice_boundary_bwd");
    return LAVT_OK;
}

extern "C" int lavt_upsample_dice_boundary_fwd(int dtype, const void* x, const int64_t* target, float dice_rate, float boundary_rate, float* ws, int64_t ws_floats,
                                               float* stats, int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    LAVT_CHECK_ARG(x && target && ws && stats, "lavt_upsample_dice_boundary_fwd: bad arguments");
    DB_CHECK_SHAPE("lavt_upsample_dice_boundary_fwd", B);
    return dice_boundary_fwd<false>(dtype, x, nullptr, B, target, dice_rate, boundary_rate, ws, ws_floats, stats, B, Hi, Wi, Ho, Wo, stream);
}
extern "C" int lavt_upsample_dice_boundary_sel_fwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float dice_rate, float boundary_rate,
                                                   float* ws, int64_t ws_floats, float* stats, int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    LAVT_CHECK_ARG(x && sel && target && ws && stats && nsel <= B, "lavt_upsample_dice_boundary_sel_fwd: bad arguments (0 < nsel <= B)");
    DB_CHECK_SHAPE("lavt_upsample_dice_boundary_sel_fwd", nsel);
    return dice_boundary_fwd<true>(dtype, x, sel, nsel, target, dice_rate, boundary_rate, ws, ws_floats, stats, B, Hi, Wi, Ho, Wo, stream);
}
extern "C" int lavt_upsample_dice_boundary_bwd(int dtype, const void* x, const int64_t* target, float dice_rate, float boundary_rate, const float* stats,
                                               const float* dloss, float* ws, int64_t ws_floats, void* dx, int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    LAVT_CHECK_ARG(x && target && stats && ws && dx, "lavt_upsample_dice_boundary_bwd: bad arguments");
    DB_CHECK_SHAPE("lavt_upsample_dice_boundary_bwd", B);
    return dice_boundary_bwd<false>(dtype, x, nullptr, B, target, dice_rate, boundary_rate, stats, dloss, ws, dx, B, Hi, Wi, Ho, Wo, stream);
}
extern "C" int lavt_upsample_dice_boundary_sel_bwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float dice_rate, float boundary_rate,
                                                   const float* stats, const float* dloss, float* ws, int64_t ws_floats, void* dx, int B, int Hi, int Wi, int Ho,
                                                   int Wo, void* stream) {
    LAVT_CHECK_ARG(x && sel && target && stats && ws && dx && nsel <= B, "lavt_upsample_dice_boundary_sel_bwd: bad arguments (0 < nsel <= B)");
    DB_CHECK_SHAPE("lavt_upsample_dice_boundary_sel_bwd", nsel);
    return dice_boundary_bwd<true>(dtype, x, sel, nsel, target, dice_rate, boundary_rate, stats, dloss, ws, dx, B, Hi, Wi, Ho, Wo, stream);
}
