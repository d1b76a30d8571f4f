// Text side of lavt_one / lavt_video: the BERT-base encoder the reference builds with
// `BertModel.from_pretrained(args.ck_bert)` (lib/_utils.py:38-52; train.py:595-602; HF transformers 3.0.2 `modeling_bert.py`).
// Its Linear / LayerNorm / GELU / attention GEMMs run on the kernels of the visual path; this file adds what only the text side needs:
// the embedding sum (word + position + token type) with its scatter-add backward, the same sum with its LayerNorm and the attention mask's key bias as one
// inference launch (lavt_bert_embed_ln_fwd), inverted dropout with a caller-drawn keep mask, and the fused
// attention core for sentence-length sequences (lavt_sentence_attn_fwd / _bwd: one workgroup per (sample, head), one launch per direction).
// 20-22 tokens per sentence: latency-bound, a wave per token row, 16-byte accesses.
#include "common.h"

namespace {

// out[r][:] = word[ids[r]][:] + pos[r % N][:] + type[tt ? tt[r] : 0][:]          (BertEmbeddings.forward before LayerNorm)
template <typename T>
__global__ __launch_bounds__(256) void bert_embed_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tt, const float* __restrict__ word,
                                                             const float* __restrict__ pos, const float* __restrict__ type, T* __restrict__ out,
                                                             int rows, int N, int H) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* w = word + ids[row] * (int64_t)H;
    const float* p = pos + (int64_t)(row % N) * H;
    const float* t = type + (tt ? tt[row] : 0) * (int64_t)H;
    for (int c = lane * 4; c < H; c += 256) {
        const float4 a = *reinterpret_cast<const float4*>(w + c), b = *reinterpret_cast<const float4*>(p + c), d = *reinterpret_cast<const float4*>(t + c);
        T* o = out + (int64_t)row * H + c;
        // (word + type) + position: the order of BertEmbeddings.forward
        o[0] = from_f<T>((a.x + d.x) + b.x); o[1] = from_f<T>((a.y + d.y) + b.y); o[2] = from_f<T>((a.z + d.z) + b.z); o[3] = from_f<T>((a.w + d.w) + b.w);
    }
}

// The opening of the encoder in inference as ONE launch (lavt_bert_embed_ln_fwd):
//   out[r][:] = T(LayerNorm((word[ids[r]][:] + type[tt ? tt[r] : 0][:]) + pos[r % N][:]) * gamma + beta),  keybias[r] = (1 - mask[r]) * -10000.
// A wave per token row, 4 rows per workgroup; lane l holds the float4 chunks l, l + 64, ... of its row (MAXC of them: H <= 256 * MAXC) in registers
// between the two statistics passes -- mean first, then the mean of squared deviations about it -- so the row is read once and nothing goes through LDS.
// The sum stays fp32 from the tables to the store: one rounding to T.  The kernel cannot raise: an id outside [0, vocab) reads word row 0 (the pad
// row), a type outside [0, n_types) type row 0; r % N < N <= n_pos is the entry's check.
template <typename T, int MAXC>
__global__ __launch_bounds__(256) void bert_embed_ln_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tt, const int64_t* __restrict__ amask,
                                                                const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                T* __restrict__ out, float* __restrict__ keybias, int rows, int N, int H, int vocab, int n_types) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                               // (uniform over the wave: the reductions below are wave-local)
    int64_t id = ids[row], ty = tt ? tt[row] : 0;
    if ((uint64_t)id >= (uint64_t)vocab) id = 0;
    if ((uint64_t)ty >= (uint64_t)n_types) ty = 0;
    const float* w = word + id * (int64_t)H;
    const float* p = pos + (int64_t)(row % N) * H;
    const float* t = type + ty * (int64_t)H;
    const int nchunk = H >> 2;
    float4 v[MAXC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + 64 * c;
        v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ch < nchunk) {
            const float4 a = *reinterpret_cast<const float4*>(w + 4 * ch), b = *reinterpret_cast<const float4*>(p + 4 * ch),
                         d = *reinterpret_cast<const float4*>(t + 4 * ch);
            // (word + type) + position: the order of BertEmbeddings.forward
            v[c] = make_float4((a.x + d.x) + b.x, (a.y + d.y) + b.y, (a.z + d.z) + b.z, (a.w + d.w) + b.w);
            s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
        }
    }
    const float mu = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (lane + 64 * c < nchunk) {
            const float dx = v[c].x - mu, dy = v[c].y - mu, dz = v[c].z - mu, dw = v[c].w - mu;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    const float rs = 1.f / sqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + 4 * ch), be = *reinterpret_cast<const float4*>(beta + 4 * ch);
            const float y0 = (v[c].x - mu) * rs * g.x + be.x, y1 = (v[c].y - mu) * rs * g.y + be.y, y2 = (v[c].z - mu) * rs * g.z + be.z,
                        y3 = (v[c].w - mu) * rs * g.w + be.w;
            T* o = out + (int64_t)row * H + 4 * ch;
            if constexpr (std::is_same<T, float>::value) {
                *reinterpret_cast<float4*>(o) = make_float4(y0, y1, y2, y3);
            } else {
                *reinterpret_cast<uint2*>(o) = make_uint2(pack_bf16x2(y0, y1), pack_bf16x2(y2, y3));          // (H % 4 == 0: a chunk of a bf16 row starts on 8 bytes)
            }
        }
    }
    if (amask && lane == 0) keybias[row] = (1.f - (float)amask[row]) * -10000.f;          // get_extended_attention_mask of 3.0.2, literally
}

// dword[ids[r]] += dy[r], dpos[r % N] += dy[r], dtype[tt[r]] += dy[r]  (fp32 atomics: a few dozen rows, repeated ids / positions collide)
template <typename T>
__global__ __launch_bounds__(256) void bert_embed_bwd_kernel(const T* __restrict__ dy, const int64_t* __restrict__ ids, const int64_t* __restrict__ tt,
                                                             float* __restrict__ dword, float* __restrict__ dpos, float* __restrict__ dtype_, int rows, int N, int H) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* w = dword + ids[row] * (int64_t)H;
    float* p = dpos + (int64_t)(row % N) * H;
    float* t = dtype_ + (tt ? tt[row] : 0) * (int64_t)H;
    for (int c = lane; c < H; c += 64) {
        const float g = to_f<T>(dy[(int64_t)row * H + c]);
        atomicAdd(w + c, g);
        atomicAdd(p + c, g);
        atomicAdd(t + c, g);
    }
}

// The same sums without atomics (lavt_bert_embed_bwd_det): workgroup (r, which) serves target `which` (0 word, 1 position, 2 token type) of token row r.
// It owns the target row key(r) iff no earlier token row names the same one; the owner then adds the dy rows of every token row with that key in ascending
// row order and adds the total to the target row -- one writer per target row, one fixed order.  rows = B * N_l is a few hundred: the quadratic scan over
// the keys is a few thousand uniform loads.
template <typename T>
__global__ __launch_bounds__(256) void bert_embed_bwd_det_kernel(const T* __restrict__ dy, const int64_t* __restrict__ ids, const int64_t* __restrict__ tt,
                                                                 float* __restrict__ dword, float* __restrict__ dpos, float* __restrict__ dtype_, int rows, int N, int H) {
    const int r = blockIdx.x, which = blockIdx.y;
    auto key = [&](int q) -> int64_t { return which == 0 ? ids[q] : (which == 1 ? (int64_t)(q % N) : (tt ? tt[q] : 0)); };
    const int64_t mine = key(r);
    for (int q = 0; q < r; ++q)
        if (key(q) == mine) return;                    // (uniform over the workgroup)
    float* dst = (which == 0 ? dword : (which == 1 ? dpos : dtype_)) + mine * (int64_t)H;
    for (int c = threadIdx.x; c < H; c += 256) {
        float a = 0.f;
        for (int q = r; q < rows; ++q)
            if (key(q) == mine) a += to_f<T>(dy[(int64_t)q * H + c]);
        dst[c] += a;
    }
}

// y = x * keep * scale (+ r)   (nn.Dropout in training: keep ~ Bernoulli(1 - p) drawn by the caller, scale = 1 / (1 - p); the optional r is
// the residual BertSelfOutput / BertOutput add before their LayerNorm; backward of x is the same map without r)
template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, const uint8_t* __restrict__ keep, float scale, const T* __restrict__ r,
                                                      T* __restrict__ y, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = keep[i] ? to_f<T>(x[i]) * scale : 0.f;
        y[i] = from_f<T>(r ? v + to_f<T>(r[i]) : v);
    }
}

// ---- sentence attention: the BertSelfAttention core for one (sample, head) per workgroup, everything in LDS as fp32 ---------------------------------
// qkv token-major [B*N][3H] (q | k | v, each heads x 64), N <= 64 tokens.  A wave owns a query row: lane j holds key j's score, the row's max / sum are
// wave reductions, and the lanes turn into the 64 output columns for the value product.  Plain fp32 FMA: the problem is 20 x 20 x 64 per head.
constexpr int SA_HD = 64;            // head_dim the kernels are written for (a lane per column)
constexpr int SA_LDK = SA_HD + 1;    // row stride of the operands read with a lane per ROW (k, and v in the backward): odd, so 32 rows hit 32 banks

__host__ __device__ constexpr size_t sattn_fwd_lds(int N) { return ((size_t)N * (2 * SA_HD + SA_LDK) + 64) * sizeof(float); }
__host__ __device__ constexpr size_t sattn_bwd_lds(int N) { return ((size_t)N * (2 * SA_HD + 2 * SA_LDK + 2 * N) + 64) * sizeof(float); }

// head h of the token rows of sample b, column block `which` (0 q, 1 k, 2 v) -> dst[n * ld + d] as fp32
template <typename T>
__device__ __forceinline__ void sattn_stage(const T* __restrict__ src, int64_t row_stride, float* dst, int ld, int N) {
    for (int e = threadIdx.x; e < N * SA_HD; e += blockDim.x) {
        const int n = e >> 6, d = e & 63;
        dst[n * ld + d] = to_f<T>(src[n * row_stride + d]);
    }
}

// P[i][j] for lane j of the wave that owns query row i: softmax_j(q_i . k_j / sqrt(hd) + keybias[j]).  ONE function for forward and backward, so that the
// backward's recomputed probabilities are the forward's bits.  Lanes j >= N return 0.  A fully masked row keeps -10000 on every key (uniform), as HF does.
__device__ __forceinline__ float sattn_prob(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ kb, int i, int j, int N,
                                            float scale) {
    float s = -INFINITY;
    if (j < N) {
        float a = 0.f;
#pragma unroll 16
        for (int d = 0; d < SA_HD; ++d) a = fmaf(q[i * SA_HD + d], k[j * SA_LDK + d], a);
        s = fmaf(a, scale, kb[j]);
    }
    const float m = wave_max(s);
    const float e = j < N ? expf(s - m) : 0.f;
    return e / wave_sum(e);
}

__device__ __forceinline__ float sattn_drop(float x, const uint8_t* __restrict__ keep_row, int j, float drop_scale) {
    return keep_row ? (keep_row[j] ? x * drop_scale : 0.f) : x;
}

template <typename T>
__global__ __launch_bounds__(512) void sentence_attn_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ keybias, const uint8_t* __restrict__ keep,
                                                                float drop_scale, T* __restrict__ out, int N, int heads, float scale) {
    extern __shared__ float sa_lds[];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, H = heads * SA_HD;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    float* q = sa_lds;                       // [N][64]
    float* k = q + N * SA_HD;                // [N][65]
    float* v = k + N * SA_LDK;               // [N][64]
    float* kb = v + N * SA_HD;               // [64]
    const T* base = qkv + (int64_t)b * N * 3 * H + h * SA_HD;
    sattn_stage<T>(base, 3 * H, q, SA_HD, N);
    sattn_stage<T>(base + H, 3 * H, k, SA_LDK, N);
    sattn_stage<T>(base + 2 * H, 3 * H, v, SA_HD, N);
    if (threadIdx.x < N) kb[threadIdx.x] = keybias[b * N + threadIdx.x];
    __syncthreads();
    for (int i = wave; i < N; i += nwaves) {
        const float p = sattn_prob(q, k, kb, i, lane, N, scale);
        const uint8_t* keep_row = keep ? keep + ((int64_t)blockIdx.x * N + i) * N : nullptr;
        const float pd = lane < N ? sattn_drop(p, keep_row, lane, drop_scale) : 0.f;
        float o = 0.f;
        for (int j = 0; j < N; ++j) o = fmaf(__shfl(pd, j, 64), v[j * SA_HD + lane], o);          // lane = output column
        out[((int64_t)b * N + i) * H + h * SA_HD + lane] = from_f<T>(o);
    }
}

// dqkv of the same (sample, head): P is recomputed (sattn_prob), dP = dO V^T through the dropout mask, dS = P (dP - sum_j dP P); then
// dQ = dS K / sqrt(hd), dK = dS^T Q / sqrt(hd), dV = Pd^T dO with a wave per output row and a lane per column.  Every sum runs in index order.
template <typename T>
__global__ __launch_bounds__(512) void sentence_attn_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ keybias, const uint8_t* __restrict__ keep,
                                                                float drop_scale, const T* __restrict__ dout, T* __restrict__ dqkv, int N, int heads,
                                                                float scale) {
    extern __shared__ float sa_lds[];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, H = heads * SA_HD;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    float* q = sa_lds;                       // [N][64]
    float* k = q + N * SA_HD;                // [N][65]
    float* v = k + N * SA_LDK;               // [N][65]
    float* dO = v + N * SA_LDK;              // [N][64]
    float* dS = dO + N * SA_HD;              // [N][N]
    float* Pd = dS + N * N;                  // [N][N]   P after dropout
    float* kb = Pd + N * N;                  // [64]
    const T* base = qkv + (int64_t)b * N * 3 * H + h * SA_HD;
    sattn_stage<T>(base, 3 * H, q, SA_HD, N);
    sattn_stage<T>(base + H, 3 * H, k, SA_LDK, N);
    sattn_stage<T>(base + 2 * H, 3 * H, v, SA_LDK, N);
    sattn_stage<T>(dout + (int64_t)b * N * H + h * SA_HD, H, dO, SA_HD, N);
    if (threadIdx.x < N) kb[threadIdx.x] = keybias[b * N + threadIdx.x];
    __syncthreads();
    for (int i = wave; i < N; i += nwaves) {
        const float p = sattn_prob(q, k, kb, i, lane, N, scale);
        const uint8_t* keep_row = keep ? keep + ((int64_t)blockIdx.x * N + i) * N : nullptr;
        float dp = 0.f;
        if (lane < N) {
            float a = 0.f;
#pragma unroll 16
            for (int d = 0; d < SA_HD; ++d) a = fmaf(dO[i * SA_HD + d], v[lane * SA_LDK + d], a);
            dp = sattn_drop(a, keep_row, lane, drop_scale);
        }
        const float delta = wave_sum(dp * p);
        if (lane < N) {
            dS[i * N + lane] = p * (dp - delta);
            Pd[i * N + lane] = sattn_drop(p, keep_row, lane, drop_scale);
        }
    }
    __syncthreads();
    T* gbase = dqkv + (int64_t)b * N * 3 * H + h * SA_HD;
    for (int t = wave; t < 3 * N; t += nwaves) {
        const int which = t / N, r = t - which * N;
        float a = 0.f;
        if (which == 0) {
            for (int j = 0; j < N; ++j) a = fmaf(dS[r * N + j], k[j * SA_LDK + lane], a);
            a *= scale;
        } else if (which == 1) {
            for (int i = 0; i < N; ++i) a = fmaf(dS[i * N + r], q[i * SA_HD + lane], a);
            a *= scale;
        } else {
            for (int i = 0; i < N; ++i) a = fmaf(Pd[i * N + r], dO[i * SA_HD + lane], a);
        }
        gbase[(int64_t)r * 3 * H + which * H + lane] = from_f<T>(a);
    }
}

}  // namespace

#define DISPATCH_T(dtype, NAME, ...)                                 \
    if (dtype == LAVT_F32) { using T = float; __VA_ARGS__; }           \
    else if (dtype == LAVT_BF16) { using T = bf16; __VA_ARGS__; }      \
    else { lavt_set_error(NAME ": bad dtype %d", dtype); return LAVT_ERR_INVALID; }
#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int lavt_bert_embed_fwd(int dtype, const int64_t* ids, const int64_t* token_type, const float* word, const float* pos, const float* type,
                                   void* out, int rows, int N, int H, void* stream) {
    LAVT_CHECK_ARG(ids && word && pos && type && out && rows > 0 && N > 0 && H > 0 && H % 4 == 0, "lavt_bert_embed_fwd: bad arguments");
    DISPATCH_T(dtype, "lavt_bert_embed_fwd", hipLaunchKernelGGL(bert_embed_fwd_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, ST, ids, token_type, word, pos, type, (T*)out, rows, N, H));
    LAVT_CHECK_LAUNCH("lavt_bert_embed_fwd");
    return LAVT_OK;
}

extern "C" int lavt_bert_embed_ln_fwd(int dtype, const int64_t* ids, const int64_t* token_type, const int64_t* attn_mask, const float* word, const float* pos,
                                      const float* type, const float* gamma, const float* beta, float eps, void* out, float* keybias, int rows, int N, int H,
                                      int vocab, int n_pos, int n_types, void* stream) {
    LAVT_CHECK_ARG(ids && word && pos && type && gamma && beta && out, "lavt_bert_embed_ln_fwd: null pointer");
    LAVT_CHECK_ARG(rows > 0 && N > 0 && H > 0 && vocab > 0 && n_pos > 0 && n_types > 0, "lavt_bert_embed_ln_fwd: rows = %d, N = %d, H = %d, tables of %d / %d / %d rows",
                   rows, N, H, vocab, n_pos, n_types);
    LAVT_CHECK_ARG(H % 4 == 0 && H <= 2048, "lavt_bert_embed_ln_fwd: unsupported H=%d (a multiple of 4, at most 2048)", H);
    LAVT_CHECK_ARG(N <= n_pos, "lavt_bert_embed_ln_fwd: %d tokens but only %d positions", N, n_pos);
    LAVT_CHECK_ARG((keybias != nullptr) == (attn_mask != nullptr), "lavt_bert_embed_ln_fwd: keybias and attn_mask go together (both or neither)");
    const int nchunk = H / 4;
#define EMBED_LN(MAXC_) hipLaunchKernelGGL((bert_embed_ln_fwd_kernel<T, MAXC_>), dim3((rows + 3) / 4), dim3(256), 0, ST, ids, token_type, attn_mask, word, pos, type, gamma, beta, eps, (T*)out, keybias, rows, N, H, vocab, n_types)
    DISPATCH_T(dtype, "lavt_bert_embed_ln_fwd", if (nchunk <= 64) EMBED_LN(1); else if (nchunk <= 128) EMBED_LN(2); else if (nchunk <= 256) EMBED_LN(4); else EMBED_LN(8));
#undef EMBED_LN
    LAVT_CHECK_LAUNCH("lavt_bert_embed_ln_fwd");
    return LAVT_OK;
}

extern "C" int lavt_bert_embed_bwd(int dtype, const void* dy, const int64_t* ids, const int64_t* token_type, float* dword, float* dpos, float* dtype_,
                                   int rows, int N, int H, void* stream) {
    LAVT_CHECK_ARG(dy && ids && dword && dpos && dtype_ && rows > 0 && N > 0 && H > 0, "lavt_bert_embed_bwd: bad arguments");
    DISPATCH_T(dtype, "lavt_bert_embed_bwd", hipLaunchKernelGGL(bert_embed_bwd_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, ST, (const T*)dy, ids, token_type, dword, dpos, dtype_, rows, N, H));
    LAVT_CHECK_LAUNCH("lavt_bert_embed_bwd");
    return LAVT_OK;
}

extern "C" int lavt_bert_embed_bwd_det(int dtype, const void* dy, const int64_t* ids, const int64_t* token_type, float* dword, float* dpos, float* dtype_,
                                       int rows, int N, int H, void* stream) {
    LAVT_CHECK_ARG(dy && ids && dword && dpos && dtype_ && rows > 0 && N > 0 && H > 0, "lavt_bert_embed_bwd_det: bad arguments");
    DISPATCH_T(dtype, "lavt_bert_embed_bwd_det", hipLaunchKernelGGL(bert_embed_bwd_det_kernel<T>, dim3(rows, 3), dim3(256), 0, ST, (const T*)dy, ids, token_type, dword, dpos, dtype_, rows, N, H));
    LAVT_CHECK_LAUNCH("lavt_bert_embed_bwd_det");
    return LAVT_OK;
}

// the geometry the sentence-attention kernels are written for; everything else is the caller's composed route (lavt_hip.ops.sentence_attention)
#define SATTN_CHECK(NAME, ...)                                                                                                                   \
    LAVT_CHECK_ARG(__VA_ARGS__, NAME ": bad arguments");                                                                                         \
    LAVT_CHECK_ARG(hd == SA_HD && N >= 1 && N <= 64, NAME ": head_dim %d, %d tokens: the kernel covers head_dim 64 and 1..64 tokens", hd, N);    \
    LAVT_CHECK_ARG(B >= 1 && heads >= 1 && (int64_t)B * heads <= 0x7fffffff, NAME ": B = %d, heads = %d", B, heads)

extern "C" int lavt_sentence_attn_fwd(int dtype, const void* qkv, const float* keybias, const uint8_t* keep, float drop_scale, void* out, int B, int N,
                                      int heads, int hd, void* stream) {
    SATTN_CHECK("lavt_sentence_attn_fwd", qkv && keybias && out);
    const size_t lds = sattn_fwd_lds(N);          // <= 49,664 bytes
    const float scale = 0.125f;                   // 1 / sqrt(64)
    DISPATCH_T(dtype, "lavt_sentence_attn_fwd", hipLaunchKernelGGL(sentence_attn_fwd_kernel<T>, dim3(B * heads), dim3(512), lds, ST, (const T*)qkv, keybias, keep,
                                                                   drop_scale, (T*)out, N, heads, scale));
    LAVT_CHECK_LAUNCH("lavt_sentence_attn_fwd");
    return LAVT_OK;
}

template <typename T>
static int sattn_bwd_launch(const void* qkv, const float* keybias, const uint8_t* keep, float drop_scale, const void* dout, void* dqkv, int B, int N, int heads,
                            hipStream_t st) {
    const size_t lds = sattn_bwd_lds(N);          // 99,072 bytes at N = 64: past 64 KB (N >= 48) the kernel needs the attribute, as attention_mfma.hip's do
    static size_t reserved = 0;
    if (lds > 65536 && lds > reserved) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sentence_attn_bwd_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            lavt_set_error("lavt_sentence_attn_bwd: cannot reserve %zu bytes of LDS", lds);
            return LAVT_ERR_LAUNCH;
        }
        reserved = lds;
    }
    hipLaunchKernelGGL(sentence_attn_bwd_kernel<T>, dim3(B * heads), dim3(512), lds, st, (const T*)qkv, keybias, keep, drop_scale, (const T*)dout, (T*)dqkv, N, heads,
                       0.125f);
    return LAVT_OK;
}

extern "C" int lavt_sentence_attn_bwd(int dtype, const void* qkv, const float* keybias, const uint8_t* keep, float drop_scale, const void* dout, void* dqkv,
                                      int B, int N, int heads, int hd, void* stream) {
    SATTN_CHECK("lavt_sentence_attn_bwd", qkv && keybias && dout && dqkv);
    int rc = LAVT_OK;
    DISPATCH_T(dtype, "lavt_sentence_attn_bwd", rc = sattn_bwd_launch<T>(qkv, keybias, keep, drop_scale, dout, dqkv, B, N, heads, ST));
    if (rc != LAVT_OK) return rc;
    LAVT_CHECK_LAUNCH("lavt_sentence_attn_bwd");
    return LAVT_OK;
}

extern "C" int lavt_dropout(int dtype, const void* x, const uint8_t* keep, float scale, const void* residual, void* y, int64_t n, void* stream) {
    LAVT_CHECK_ARG(x && keep && y && n > 0, "lavt_dropout: bad arguments");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    DISPATCH_T(dtype, "lavt_dropout", hipLaunchKernelGGL(dropout_kernel<T>, dim3((int)blocks), dim3(256), 0, ST, (const T*)x, keep, scale, (const T*)residual, (T*)y, n));
    LAVT_CHECK_LAUNCH("lavt_dropout");
    return LAVT_OK;
}
