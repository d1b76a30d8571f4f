// The pixel counts of the DAVIS 2017 J&F measure (include/lavt_hip.h "J&F measure"): for every frame the region counts I, U and the boundary counts
// n_fg, n_gt, m_fg, m_gt of db_eval_boundary without void pixels -- boundary maps of prediction and ground truth, each dilated with a disk of radius
// bound_pix, matched against the other.  All of it is integer work on BIT ROWS: a frame row is ceil(W / 64) 64-bit words, bit c of word w = pixel
// 64 * w + c, bits past W are zero.
//   pack pass      one ballot turns 64 pixels of a row into a word (nonzero = foreground; uint8 or int64 target); every pixel is read exactly once,
//                  512 contiguous bytes of an int64 target per wave and load, four loads in flight per lane.  I and U are popcounts of the words.
//   boundary pass  one workgroup per tile of JF_TROWS x (64 * JF_TWORDS) pixels stages the words of its tile plus a halo of bound_pix (+1 row and
//                  +1 word for the shifted neighbours) in LDS for both masks, forms the boundary-map words there -- three shifted XORs, the shifts
//                  replicate the last row and column, which is what the overwrite of the toolkit's _seg2bmap amounts to -- and then every thread
//                  owns one word of the tile: dil(b) of that word is, for each run of dy that shares the half width k = floor(sqrt(r*r - dy*dy)),
//                  the OR of the rows at +-dy spread horizontally by k.  A spread is at most six shift-and-OR doublings per direction (1, 2, 4, 8, 16, 9)
//                  plus what the nearest set bit of the two neighbour words reaches.  A word with no boundary bit of its own skips the dilation of the other
//                  mask, and the walk over dy stops once every own bit is matched.  Counts are popcounts.
// Frames never see each other: every staged word is addressed by (frame, row, word) and is zero outside [0, H) x [0, ceil(W / 64)).
// The counts are added with integer atomics behind a zero-fill kernel of the same entry: order-independent, identical from run to run.
#include "internal.h"

namespace {

constexpr int JF_TROWS = 64, JF_TWORDS = 4;          // the tile of the boundary pass: 64 rows x 256 columns, one word per thread
constexpr int JF_MAXR = LAVT_BOUNDARY_MAX_RADIUS;
constexpr int JF_SROWS = JF_TROWS + 2 * JF_MAXR + 1, JF_SWORDS = JF_TWORDS + 3;          // staged mask words: rows -r .. TROWS + r, words -1 .. TWORDS + 1
constexpr int JF_BROWS = JF_TROWS + 2 * JF_MAXR, JF_BWORDS = JF_TWORDS + 2;              // boundary-map words: rows -r .. TROWS + r - 1, words -1 .. TWORDS
constexpr int JF_PACK_WORDS = 64;                    // words of one frame per workgroup of the pack pass: 16 per wave, 4 at a time
static_assert(JF_MAXR >= 40 && JF_MAXR < 64, "a spread reaches the adjacent word only");
static_assert(JF_TROWS * JF_TWORDS == 256, "one thread per word of the tile");

typedef unsigned long long u64;

// the zero fill of counts in front of the atomic adds: a kernel of this entry, so the same three nodes whether the call runs eagerly or is replayed
__global__ __launch_bounds__(256) void jf_zero_kernel(int32_t* __restrict__ counts, int words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < words) counts[i] = 0;
}

// ---------------------------------------------------------------------------------------------- pack pass
template <typename T>
__global__ __launch_bounds__(256) void jf_pack_kernel(const uint8_t* __restrict__ pred, const T* __restrict__ target, u64* __restrict__ pbits, u64* __restrict__ gbits,
                                                      int32_t* __restrict__ counts, int H, int W, int WW, int blocks_per_frame) {
    const int f = blockIdx.x / blocks_per_frame, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int FW = H * WW;                                                    // words of a frame (checked on the host: fits an int)
    const int w0 = (blockIdx.x % blocks_per_frame) * JF_PACK_WORDS + wave * (JF_PACK_WORDS / 4);
    const int64_t pix0 = (int64_t)f * H * W, word0 = (int64_t)f * FW;
    int ci = 0, cu = 0;
    for (int it = 0; it < JF_PACK_WORDS / 16; ++it) {
        uint8_t p[4];
        T t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {          // every load of the round before the first ballot
            const int idx = w0 + it * 4 + u, row = idx / WW, col = (idx - row * WW) * 64 + lane;
            p[u] = 0;
            t[u] = 0;
            if (idx < FW && col < W) {
                const int64_t at = pix0 + (int64_t)row * W + col;
                p[u] = pred[at];
                t[u] = target[at];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = w0 + it * 4 + u;
            const u64 pw = __ballot(p[u] != 0), gw = __ballot(t[u] != 0);
            if (idx < FW) {                    // (uniform over the wave)
                if (lane == 0) { pbits[word0 + idx] = pw; gbits[word0 + idx] = gw; }
                ci += __popcll(pw & gw);
                cu += __popcll(pw | gw);
            }
        }
    }
    __shared__ int red[4][2];
    if (lane == 0) { red[wave][0] = ci; red[wave][1] = cu; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (v) atomicAdd(counts + (int64_t)f * 8 + threadIdx.x, v);
    }
}

// ---------------------------------------------------------------------------------------------- boundary pass
// columns [-k, k] around every set bit of C, plus what the set bits of the left (L) and right (R) neighbour words reach into this word; 0 <= k < 64
__device__ __forceinline__ u64 jf_spread(u64 L, u64 C, u64 R, int k) {
    u64 up = C, dn = C;
    for (int w = 0; w < k;) {          // up covers [0, w], dn [-w, 0]; a shift by s <= w + 1 leaves no gap.  One direction each: what a shift drops at
        const int s = min(w + 1, k - w);          // the word's end could only have reached columns outside the word
        up |= up << s;
        dn |= dn >> s;
        w += s;
    }
    u64 d = up | dn;
    if (L) {          // the highest set bit of L is the column -(clz + 1): it reaches the bits 0 .. k - 1 - clz
        const int t = k - 1 - __clzll(L);
        if (t >= 0) d |= (2ull << t) - 1ull;
    }
    if (R) {          // the lowest set bit of R is the column 64 + ctz: it reaches the bits 64 - (k - ctz) .. 63
        const int t = k - (__ffsll(R) - 1);
        if (t > 0) d |= ~0ull << (64 - t);
    }
    return d;
}

// popcount of own & dil(other) for the word (row br, word bw) of the LDS boundary maps
__device__ __forceinline__ int jf_match(const u64 (*other)[JF_BWORDS], const uint8_t* hx, u64 own, int br, int bw, int r) {
    u64 dil = 0, aL = 0, aC = 0, aR = 0;
    for (int dy = 0; dy <= r; ++dy) {
        const u64* up = other[br - dy] + bw;
        const u64* dn = other[br + dy] + bw;
        aL |= up[-1] | dn[-1];
        aC |= up[0] | dn[0];
        aR |= up[1] | dn[1];
        if (dy == r || hx[dy + 1] != hx[dy]) {          // the rows +-dy of one run share the half width: one spread for the run
            if (aL | aC | aR) dil |= jf_spread(aL, aC, aR, hx[dy]);
            aL = aC = aR = 0;
            if ((own & ~dil) == 0) break;
        }
    }
    return __popcll(own & dil);
}

__global__ __launch_bounds__(256) void jf_boundary_kernel(const u64* __restrict__ pbits, const u64* __restrict__ gbits, int32_t* __restrict__ counts, int H, int W,
                                                          int WW, int r, int tiles_x, int tiles_y) {
    __shared__ u64 S[2][JF_SROWS][JF_SWORDS];
    __shared__ u64 B[2][JF_BROWS][JF_BWORDS];
    __shared__ uint8_t hx[JF_MAXR + 2];
    __shared__ int red[4][4];
    const int tid = threadIdx.x;
    const int tx_tile = blockIdx.x % tiles_x, ty_tile = (blockIdx.x / tiles_x) % tiles_y, f = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = ty_tile * JF_TROWS, wc0 = tx_tile * JF_TWORDS;
    const int64_t word0 = (int64_t)f * H * WW;
    if (tid <= r) {          // half width of the disk at |dy| = tid: the largest k with k*k + dy*dy <= r*r
        int k = 0;
        while ((k + 1) * (k + 1) + tid * tid <= r * r) ++k;
        hx[tid] = (uint8_t)k;
    }
    // ---- the mask words of the tile and its halo; zero outside the frame
    const int srows = JF_TROWS + 2 * r + 1, brows = JF_TROWS + 2 * r;
    for (int i = tid; i < 2 * srows * JF_SWORDS; i += 256) {
        const int m = i / (srows * JF_SWORDS), rem = i - m * (srows * JF_SWORDS), lr = rem / JF_SWORDS, j = rem - lr * JF_SWORDS;
        const int g = y0 - r + lr, w = wc0 - 1 + j;
        u64 v = 0;
        if (g >= 0 && g < H && w >= 0 && w < WW) v = (m ? gbits : pbits)[word0 + (int64_t)g * WW + w];
        S[m][lr][j] = v;
    }
    __syncthreads();
    // ---- boundary maps: b = (S ^ e) | (S ^ s) | (S ^ se), the neighbours of the last row and the last column being the pixel itself
    for (int i = tid; i < 2 * brows * JF_BWORDS; i += 256) {
        const int m = i / (brows * JF_BWORDS), rem = i - m * (brows * JF_BWORDS), lr = rem / JF_BWORDS, j = rem - lr * JF_BWORDS;
        const int g = y0 - r + lr, w = wc0 - 1 + j;
        u64 b = 0;
        if (g >= 0 && g < H && w >= 0 && w < WW) {
            const int ln = min(g + 1, H - 1) - (y0 - r);
            const u64 last = (w == WW - 1) ? 1ull << ((W - 1) & 63) : 0ull;
            const u64 s0 = S[m][lr][j], s1 = S[m][ln][j];
            const u64 e0 = (s0 >> 1) | (S[m][lr][j + 1] << 63) | (s0 & last), e1 = (s1 >> 1) | (S[m][ln][j + 1] << 63) | (s1 & last);
            b = (s0 ^ e0) | (s0 ^ s1) | (s0 ^ e1);
        }
        B[m][lr][j] = b;
    }
    __syncthreads();
    // ---- one word per thread
    const int tx = tid & (JF_TWORDS - 1), ty = tid / JF_TWORDS;
    int c[4] = {0, 0, 0, 0};          // n_fg, n_gt, m_fg, m_gt
    if (y0 + ty < H && wc0 + tx < WW) {
        const int br = ty + r, bw = tx + 1;
        const u64 bp = B[0][br][bw], bg = B[1][br][bw];
        c[0] = __popcll(bp);
        c[1] = __popcll(bg);
        if (bp) c[2] = jf_match(B[1], hx, bp, br, bw, r);
        if (bg) c[3] = jf_match(B[0], hx, bg, br, bw, r);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[tid >> 6][k] = c[k];
    }
    __syncthreads();
    if (tid < 4) {
        const int v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        if (v) atomicAdd(counts + (int64_t)f * 8 + 2 + tid, v);
    }
}

inline int64_t jf_words(int n, int H, int W) { return (int64_t)n * H * ((W + 63) / 64); }

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int64_t lavt_boundary_counts_ws(int n, int H, int W) { return (n > 0 && H > 0 && W > 0) ? 2 * jf_words(n, H, W) : 0; }

extern "C" int lavt_boundary_counts(const uint8_t* pred, const uint8_t* target_u8, const int64_t* target_i64, int n, int H, int W, int bound_pix, uint64_t* ws,
                                    int64_t ws_words, int32_t* counts, void* stream) {
    LAVT_CHECK_ARG(pred && counts && ws, "lavt_boundary_counts: null pred, ws or counts");
    LAVT_CHECK_ARG((target_u8 != nullptr) != (target_i64 != nullptr), "lavt_boundary_counts: exactly one of target_u8 / target_i64");
    LAVT_CHECK_ARG(n > 0 && H > 0 && W > 0, "lavt_boundary_counts: bad sizes n=%d H=%d W=%d", n, H, W);
    LAVT_CHECK_ARG(bound_pix >= 1 && bound_pix <= LAVT_BOUNDARY_MAX_RADIUS, "lavt_boundary_counts: bound_pix %d outside 1..%d", bound_pix, LAVT_BOUNDARY_MAX_RADIUS);
    LAVT_CHECK_ARG(ws_words >= lavt_boundary_counts_ws(n, H, W), "lavt_boundary_counts: scratch of %lld 64-bit words needed", (long long)lavt_boundary_counts_ws(n, H, W));
    LAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(target_i64) & 7) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3) == 0,
                   "lavt_boundary_counts: ws and an int64 target must be 8-byte aligned, counts 4-byte");
    const int WW = (W + 63) / 64;
    const int64_t FW = (int64_t)H * WW, bpf = (FW + JF_PACK_WORDS - 1) / JF_PACK_WORDS;
    const int tiles_x = (WW + JF_TWORDS - 1) / JF_TWORDS, tiles_y = (H + JF_TROWS - 1) / JF_TROWS;
    LAVT_CHECK_ARG(FW <= 0x7fffffffll && bpf * n <= 0x7fffffffll && (int64_t)n * 8 <= 0x7fffffffll && (int64_t)tiles_x * tiles_y * n <= 0x7fffffffll, "lavt_boundary_counts: %d frames of %dx%d exceed a grid", n, H, W);
    u64* pbits = reinterpret_cast<u64*>(ws);
    u64* gbits = pbits + jf_words(n, H, W);
    hipLaunchKernelGGL(jf_zero_kernel, dim3((unsigned)(((int64_t)n * 8 + 255) / 256)), dim3(256), 0, ST, counts, n * 8);
    if (target_u8) hipLaunchKernelGGL(jf_pack_kernel<uint8_t>, dim3((unsigned)(bpf * n)), dim3(256), 0, ST, pred, target_u8, pbits, gbits, counts, H, W, WW, (int)bpf);
    else hipLaunchKernelGGL(jf_pack_kernel<int64_t>, dim3((unsigned)(bpf * n)), dim3(256), 0, ST, pred, target_i64, pbits, gbits, counts, H, W, WW, (int)bpf);
    hipLaunchKernelGGL(jf_boundary_kernel, dim3((unsigned)(tiles_x * tiles_y * n)), dim3(256), 0, ST, pbits, gbits, counts, H, W, WW, bound_pix, tiles_x, tiles_y);
    LAVT_CHECK_LAUNCH("lavt_boundary_counts");
    return LAVT_OK;
}
