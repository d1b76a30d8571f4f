// Streaming (online-softmax) bf16 formulation of the shifted-window attention core for windows too large to keep in LDS
// (Video-Swin --window12: 8x12x12 = 1152 tokens; WindowAttention3D.forward, lib/video_swin_transformer.py:137-168).
// Same arithmetic contract as lavt_window_attn_fwd / _bwd (header block "Shifted-window attention core"): qkv [nwin*N][3C] windowed rows, head_dim 32,
// the bias from the FULL window's table (a clipped window uses the top-left N x N block of the index matrix), int8 region ids (unequal ids add -100),
// lse fp32 [nwin][heads][N] in the natural-log domain.
//
// Forward: one workgroup (4 waves) per (window, head, 64-query block).  A wave owns 16 queries; their Q fragment stays in registers.  K and V stream
//   through a two-stage LDS ring in tiles of 64 keys (one barrier per tile; the next tile's global loads are in flight while the current one is
//   computed).  Scores are computed transposed, S^T = K Q^T (lane: query c16, keys 4g + r), in the log2 domain; running max and sum per query row;
//   the P^T accumulators of two key sub-tiles are directly the B operand of O^T += V^T P^T (V^T by the transposing LDS read).
// Backward, no float atomics (bitwise reproducible):
//   dQ kernel: one workgroup (8 waves) per (head, 16-query tile), looping over ALL windows.  Wave w owns key pairs (32 keys) w, w + 8, ...; it recomputes
//     P from Q, K and lse, forms dS and dQ^T += K^T dS^T (K^T through a wave-private LDS slot and the transposing read) and adds dS into a register-
//     resident dense [16][N] accumulator whose lane <-> (i, j) map is fixed: plain adds.  The 8 partial dQ tiles are summed in wave order through LDS.
//     delta = rowsum(dO o O) is formed here and stored for the dK/dV kernel; the dense accumulator is stored ONCE at the end into [heads][N][ld] scratch
//     that lavt_relpos_reduce bins into the table gradient (deterministic).
//   dK/dV kernel: one workgroup (4 waves) per (window, head, 64-key block); a wave owns 16 keys (K, V rows in registers) and sweeps the query tiles,
//     which stream through an LDS ring (Q, dO rows + -lse, -delta) like K / V in the forward.
// LDS rows of 64 bytes with the 16-byte chunk swizzle of attention_mfma.hip (chunk c of row r at c ^ swz(r)): row reads and transposing reads conflict-free.
#include "attn_common.h"

namespace {

constexpr int SLD = 32;                 // bf16 elements per LDS row
constexpr int TILE = 64;                // keys (forward) / queries (dK/dV) per ring stage
constexpr int STREAM_MAX_N = 2048;
constexpr int LDS_BUDGET = 160 * 1024;
constexpr float MASK_LOG2 = -100.0f * LOG2E;

// A^T fragment (k = 32 rows of a 32-row LDS block, m = 16 columns 16u .. 16u + 15) by two transposing reads
__device__ __forceinline__ bf16x8 tr_frag(const bf16* blk, int rr, int tcol) {
    const bf16* p = blk + rr * SLD + tcol;
    return join4(__builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p), __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 16 * SLD)));
}
__device__ __forceinline__ uint2 pack4(f32x4 v, float s) { return make_uint2(pack_bf16x2(v[0] * s, v[1] * s), pack_bf16x2(v[2] * s, v[3] * s)); }

struct Geo {
    int R, centre;
};
__host__ __device__ __forceinline__ Geo geo(int wd, int wh, int ww) {
    return Geo{(2 * wd - 1) * (2 * wh - 1) * (2 * ww - 1), ((wd - 1) * (2 * wh - 1) + (wh - 1)) * (2 * ww - 1) + (ww - 1)};
}
// byte offset of token e's table-index base (full-window coordinates: the index-slice quirk of clipped windows, lib/video_swin_transformer.py:150)
__device__ __forceinline__ int token_base4(int e, int wh, int ww) {
    const int dz = e / (wh * ww), hy = (e / ww) % wh, wx = e % ww;
    return 4 * ((dz * (2 * wh - 1) + hy) * (2 * ww - 1) + wx);
}
// table column of head h * log2 e, then (run = true) centre + 1 entries of -1e30: a padded KEY carries the base -4 (R - centre), so that
// idx_i - idx_j + centre = R + idx_i lands in the run for every query i (its probability is exactly 0, no per-element select)
__device__ __forceinline__ void stage_table(float* tab, const float* table, int heads, int h, Geo G, bool run, int tid, int nthr) {
    const int n = run ? G.R + G.centre + 1 : G.R;
    for (int e = tid; e < n; e += nthr) tab[e] = e < G.R ? table[(int64_t)e * heads + h] * LOG2E : -1e30f;
}

// ================================================================================================ forward
template <bool REGION>
__global__ __launch_bounds__(256) void wattn_stream_fwd(const bf16* __restrict__ qkv, const float* __restrict__ table, const int8_t* __restrict__ region,
                                                        int nw_img, bf16* __restrict__ out, float* __restrict__ lse, int wd, int wh, int ww, int N, int heads,
                                                        float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int NT = (N + TILE - 1) / TILE, NP = NT * TILE;
    bf16* Kr = reinterpret_cast<bf16*>(smem_raw);                 // [2][TILE][SLD]
    bf16* Vr = Kr + 2 * TILE * SLD;                               // [2][TILE][SLD]
    int* bs = reinterpret_cast<int*>(Vr + 2 * TILE * SLD);        // [NP] byte offsets of the table-index base (key convention)
    uint8_t* Rs = reinterpret_cast<uint8_t*>(bs + NP);            // [NP] region ids
    float* tab = reinterpret_cast<float*>(Rs + ((NP + 15) & ~15));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int qb = blockIdx.x % NT, h = (blockIdx.x / NT) % heads, w = blockIdx.x / (NT * heads);
    const int C = heads * HD;
    const Geo G = geo(wd, wh, ww);
    const bf16* base = qkv + (int64_t)w * N * 3 * C + h * HD;

    // this thread's share of a ring stage: row tid / 4, chunk tid % 4 of K and of V
    const int srow = tid >> 2, sc = tid & 3, spc = (sc ^ swz(srow)) * 8;
    uint4 kreg, vreg;
    auto fetch = [&](int kt) {
        const int j = kt * TILE + srow;
        kreg = vreg = make_uint4(0, 0, 0, 0);
        if (j < N) {
            const bf16* r = base + (int64_t)j * 3 * C + sc * 8;
            kreg = *reinterpret_cast<const uint4*>(r + C);
            vreg = *reinterpret_cast<const uint4*>(r + 2 * C);
        }
    };
    auto put = [&](int stage) {
        *reinterpret_cast<uint4*>(Kr + (stage * TILE + srow) * SLD + spc) = kreg;
        *reinterpret_cast<uint4*>(Vr + (stage * TILE + srow) * SLD + spc) = vreg;
    };
    fetch(0);
    for (int e = tid; e < NP; e += 256) {
        bs[e] = e < N ? token_base4(e, wh, ww) : -4 * (G.R - G.centre);
        Rs[e] = (REGION && e < N) ? (uint8_t)region[(int64_t)(w % nw_img) * N + e] : 0;
    }
    stage_table(tab, table, heads, h, G, true, tid, 256);
    const int i = qb * TILE + 16 * wave + c16;
    const bool vi = i < N;
    bf16x8 qf;
    {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (vi) q = *reinterpret_cast<const uint4*>(base + (int64_t)i * 3 * C + 8 * g);
        qf = __builtin_bit_cast(bf16x8, q);
    }
    put(0);
    __syncthreads();

    const float sc2 = scale * LOG2E;
    const f32x4 sc4 = {sc2, sc2, sc2, sc2};
    const uint32_t bi = lds_addr(tab) + 4u * (uint32_t)G.centre + (uint32_t)(vi ? bs[i] : 0);     // + (-bs[j]): LDS address of tab[idx_i - idx_j + centre]
    const uint32_t ri4 = REGION ? 0x01010101u * Rs[vi ? i : 0] : 0u;
    const int kg = 8 * (g ^ swz(c16));
    const int rr = 4 * g + (c16 >> 2);
    const int tcol[2] = {(((c16 >> 1) & 1) ^ swz(rr)) * 8 + 4 * (c16 & 1), ((2 + ((c16 >> 1) & 1)) ^ swz(rr)) * 8 + 4 * (c16 & 1)};
    float m = -1e30f, l = 0.f;                  // running max (log2 domain, the whole row) and this lane's share of the running sum
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};

    for (int kt = 0; kt < NT; ++kt) {
        const int stage = kt & 1;
        if (kt + 1 < NT) fetch(kt + 1);
        const bf16* Ks = Kr + stage * TILE * SLD;
        const bf16* Vs = Vr + stage * TILE * SLD;
        f32x4 s[4];
        float tmax = -1e30f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_row8(Ks, SLD, 16 * t + c16, kg), qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            const int j0 = kt * TILE + 16 * t + 4 * g;
            const u32x4 bj = *reinterpret_cast<const u32x4*>(bs + j0);
            const f32x4 bb = {lds_f32_at(bi - bj[0]), lds_f32_at(bi - bj[1]), lds_f32_at(bi - bj[2]), lds_f32_at(bi - bj[3])};
            f32x4 v = __builtin_elementwise_fma(acc, sc4, bb);
            if constexpr (REGION) {
                const uint32_t x = *reinterpret_cast<const uint32_t*>(Rs + j0) ^ ri4;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (x & (0xFFu << (8 * r))) ? MASK_LOG2 : 0.f;
            }
            s[t] = v;
            tmax = fmaxf(fmaxf(tmax, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        // online-softmax rescale: the decision for this tile comes before its exponentials, and the previous tile's P V is complete
        const float mn = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        l *= alpha;
        o[0] *= alpha;
        o[1] *= alpha;
        const float nm = -mn;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f32x4 p0, p1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p0[r] = __builtin_amdgcn_exp2f(s[2 * ks][r] + nm);
                p1[r] = __builtin_amdgcn_exp2f(s[2 * ks + 1][r] + nm);
            }
            l += ((p0[0] + p0[1]) + (p0[2] + p0[3])) + ((p1[0] + p1[1]) + (p1[2] + p1[3]));
            u32x4 pw;
            pw[0] = pack_bf16x2(p0[0], p0[1]); pw[1] = pack_bf16x2(p0[2], p0[3]);
            pw[2] = pack_bf16x2(p1[0], p1[1]); pw[3] = pack_bf16x2(p1[2], p1[3]);
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
            const bf16* vb = Vs + 32 * ks * SLD;
            o[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(vb, rr, tcol[0]), pf, o[0], 0, 0, 0);
            o[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(vb, rr, tcol[1]), pf, o[1], 0, 0, 0);
        }
        if (kt + 1 < NT) put(stage ^ 1);          // (stage ^ 1 was last read in iteration kt - 1, before its closing barrier)
        __syncthreads();
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (vi && g == 0) lse[((int64_t)w * heads + h) * N + i] = (m + __log2f(l)) * LN2;
    const float inv = 1.f / l;
    store_head_row16(out + ((int64_t)w * N + (vi ? i : 0)) * C + h * HD, g, pack4(o[0], inv), pack4(o[1], inv), vi);
}

// ================================================================================================ backward: dQ + dense bias gradient
// PPW = key pairs (32 keys) per wave: the dense accumulator is PPW x 8 floats per lane.
template <int PPW, bool REGION>
__global__ __launch_bounds__(512) void wattn_stream_dq(const bf16* __restrict__ qkv, const float* __restrict__ table, const int8_t* __restrict__ region,
                                                       int nw_img, const bf16* __restrict__ out, const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                       bf16* __restrict__ dqkv, float* __restrict__ delta, float* __restrict__ dense, int ld, int wd, int wh,
                                                       int ww, int nwin, int N, int heads, float scale) {
    constexpr int WAVES = 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int NQT = (N + 15) / 16, NKP = (N + 31) / 32, NP = NKP * 32;
    bf16* slots = reinterpret_cast<bf16*>(smem_raw);              // [WAVES][32][SLD]: a wave's K pair for the transposing read, then its dQ partial
    int* bs = reinterpret_cast<int*>(slots + WAVES * 32 * SLD);   // [NP] (key convention: padded keys point into the -1e30 run)
    uint8_t* Rs = reinterpret_cast<uint8_t*>(bs + NP);            // [NP] region ids of the current window
    float* tab = reinterpret_cast<float*>(Rs + ((NP + 15) & ~15));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int qt = blockIdx.x % NQT, h = blockIdx.x / NQT;
    const int C = heads * HD;
    const Geo G = geo(wd, wh, ww);
    for (int e = tid; e < NP; e += 512) bs[e] = e < N ? token_base4(e, wh, ww) : -4 * (G.R - G.centre);
    stage_table(tab, table, heads, h, G, true, tid, 512);
    __syncthreads();

    const int i = 16 * qt + c16;
    const bool vi = i < N;
    const float sc2 = scale * LOG2E;
    const f32x4 sc4 = {sc2, sc2, sc2, sc2};
    const uint32_t bi = lds_addr(tab) + 4u * (uint32_t)G.centre + (uint32_t)(vi ? bs[i] : 0);
    const int kg = 8 * (g ^ swz(c16));
    const int rr = 4 * g + (c16 >> 2);
    const int tcol[2] = {(((c16 >> 1) & 1) ^ swz(rr)) * 8 + 4 * (c16 & 1), ((2 + ((c16 >> 1) & 1)) ^ swz(rr)) * 8 + 4 * (c16 & 1)};
    bf16* slot = slots + wave * 32 * SLD;
    f32x4 acc[PPW][2];
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) acc[pp][0] = acc[pp][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int w = 0; w < nwin; ++w) {
        const bf16* base = qkv + (int64_t)w * N * 3 * C + h * HD;
        if constexpr (REGION) {
            for (int e = tid; e < NP; e += 512) Rs[e] = e < N ? (uint8_t)region[(int64_t)(w % nw_img) * N + e] : 0;
        }
        uint4 q = make_uint4(0, 0, 0, 0), d = q, oo = q;
        float nl = -1e30f;
        if (vi) {
            const int64_t ro = ((int64_t)w * N + i) * C + h * HD + 8 * g;
            q = *reinterpret_cast<const uint4*>(base + (int64_t)i * 3 * C + 8 * g);
            d = *reinterpret_cast<const uint4*>(dout + ro);
            oo = *reinterpret_cast<const uint4*>(out + ro);
            nl = -lse[((int64_t)w * heads + h) * N + i] * LOG2E;
        }
        float dl;
        {
            float fd[8], fo[8];
            chunk_to_f<bf16>(d, fd);
            chunk_to_f<bf16>(oo, fo);
            dl = 0.f;
#pragma unroll
            for (int x = 0; x < 8; ++x) dl += fd[x] * fo[x];
            dl += __shfl_xor(dl, 16, 64);
            dl += __shfl_xor(dl, 32, 64);
        }
        const bf16x8 qf = __builtin_bit_cast(bf16x8, q), of = __builtin_bit_cast(bf16x8, d);
        const float ndl = -dl;
        __syncthreads();                              // region row staged; the previous window's slot reads are done
        const uint32_t ri4 = REGION ? 0x01010101u * Rs[vi ? i : 0] : 0u;
        f32x4 dq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int pp = 0; pp < PPW; ++pp) {
            const int p = wave + WAVES * pp;
            if (p >= NKP) break;                      // wave-uniform
            uint4 kr[2], vr[2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int j = 32 * p + 16 * hh + c16;
                kr[hh] = vr[hh] = make_uint4(0, 0, 0, 0);
                if (j < N) {
                    const bf16* r = base + (int64_t)j * 3 * C + 8 * g;
                    kr[hh] = *reinterpret_cast<const uint4*>(r + C);
                    vr[hh] = *reinterpret_cast<const uint4*>(r + 2 * C);
                }
            }
            u32x4 dsw;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const f32x4 st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kr[hh]), qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                const f32x4 dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vr[hh]), of, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                const int j0 = 32 * p + 16 * hh + 4 * g;
                const u32x4 bj = *reinterpret_cast<const u32x4*>(bs + j0);
                const f32x4 bb = {lds_f32_at(bi - bj[0]), lds_f32_at(bi - bj[1]), lds_f32_at(bi - bj[2]), lds_f32_at(bi - bj[3])};
                f32x4 a = __builtin_elementwise_fma(st, sc4, bb + nl);
                if constexpr (REGION) {
                    const uint32_t x = *reinterpret_cast<const uint32_t*>(Rs + j0) ^ ri4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] += (x & (0xFFu << (8 * r))) ? MASK_LOG2 : 0.f;
                }
                f32x4 pr;
#pragma unroll
                for (int r = 0; r < 4; ++r) pr[r] = __builtin_amdgcn_exp2f(a[r]);
                // (padded key: exp2(-1e30) = 0; padded query: nl = -1e30 -> 0; both give dS = 0)
                const f32x4 ds = pr * (dpt + ndl);
                acc[pp][hh] += ds;
                dsw[2 * hh] = pack_bf16x2(ds[0], ds[1]);
                dsw[2 * hh + 1] = pack_bf16x2(ds[2], ds[3]);
            }
            // K^T of the pair through this wave's LDS slot (rows 16 hh + c16, chunk g); the wave's LDS operations are ordered, the fences keep the
            // compiler from moving the stores across the previous pair's reads or the reads across these stores
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            *reinterpret_cast<uint4*>(slot + c16 * SLD + kg) = kr[0];
            *reinterpret_cast<uint4*>(slot + (16 + c16) * SLD + kg) = kr[1];
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bf16x8 ds8 = __builtin_bit_cast(bf16x8, dsw);
            dq[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(slot, rr, tcol[0]), ds8, dq[0], 0, 0, 0);
            dq[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(slot, rr, tcol[1]), ds8, dq[1], 0, 0, 0);
        }
        // the 8 partial dQ^T tiles, summed in wave order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float* sf = reinterpret_cast<float*>(slot) + lane * 8;
        *reinterpret_cast<f32x4*>(sf) = dq[0];
        *reinterpret_cast<f32x4*>(sf + 4) = dq[1];
        __syncthreads();
        if (wave == 0) {
            f32x4 t0 = dq[0], t1 = dq[1];
#pragma unroll
            for (int v = 1; v < WAVES; ++v) {
                const float* o2 = reinterpret_cast<const float*>(slots + v * 32 * SLD) + lane * 8;
                t0 += *reinterpret_cast<const f32x4*>(o2);
                t1 += *reinterpret_cast<const f32x4*>(o2 + 4);
            }
            store_head_row16(dqkv + ((int64_t)w * N + (vi ? i : 0)) * 3 * C + h * HD, g, pack4(t0, scale), pack4(t1, scale), vi);
            if (vi && g == 0) delta[((int64_t)w * heads + h) * N + i] = dl;
        }
    }
    if (vi) {
#pragma unroll
        for (int pp = 0; pp < PPW; ++pp) {
            const int p = wave + WAVES * pp;
            if (p >= NKP) break;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
                *reinterpret_cast<f32x4*>(dense + ((int64_t)h * N + i) * ld + 32 * p + 16 * hh + 4 * g) = acc[pp][hh];
        }
    }
}

// ================================================================================================ backward: dK, dV
template <bool REGION>
__global__ __launch_bounds__(256) void wattn_stream_dkv(const bf16* __restrict__ qkv, const float* __restrict__ table, const int8_t* __restrict__ region,
                                                        int nw_img, const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
                                                        bf16* __restrict__ dqkv, int wd, int wh, int ww, int N, int heads, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int NT = (N + TILE - 1) / TILE, NP = NT * TILE;
    bf16* Qr = reinterpret_cast<bf16*>(smem_raw);                 // [2][TILE][SLD]
    bf16* Or = Qr + 2 * TILE * SLD;                               // [2][TILE][SLD] dO
    float* nlr = reinterpret_cast<float*>(Or + 2 * TILE * SLD);   // [2][TILE] -lse * log2 e (-1e30 for padded queries)
    float* ndr = nlr + 2 * TILE;                                  // [2][TILE] -delta
    int* bs = reinterpret_cast<int*>(ndr + 2 * TILE);             // [NP] (query convention: padded queries carry base 0, a finite bias)
    uint8_t* Rs = reinterpret_cast<uint8_t*>(bs + NP);
    float* tab = reinterpret_cast<float*>(Rs + ((NP + 15) & ~15));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int kb = blockIdx.x % NT, h = (blockIdx.x / NT) % heads, w = blockIdx.x / (NT * heads);
    const int C = heads * HD;
    const Geo G = geo(wd, wh, ww);
    const bf16* base = qkv + (int64_t)w * N * 3 * C + h * HD;
    const int64_t lrow = ((int64_t)w * heads + h) * N;

    const int srow = tid >> 2, sc = tid & 3, spc = (sc ^ swz(srow)) * 8;
    uint4 qreg, dreg;
    float lreg = -1e30f, dlreg = 0.f;
    auto fetch = [&](int it) {
        const int r = it * TILE + srow;
        qreg = dreg = make_uint4(0, 0, 0, 0);
        if (r < N) {
            qreg = *reinterpret_cast<const uint4*>(base + (int64_t)r * 3 * C + sc * 8);
            dreg = *reinterpret_cast<const uint4*>(dout + ((int64_t)w * N + r) * C + h * HD + sc * 8);
        }
        if (tid < TILE) {
            const int rl = it * TILE + tid;
            lreg = rl < N ? -lse[lrow + rl] * LOG2E : -1e30f;
            dlreg = rl < N ? -delta[lrow + rl] : 0.f;
        }
    };
    auto put = [&](int stage) {
        *reinterpret_cast<uint4*>(Qr + (stage * TILE + srow) * SLD + spc) = qreg;
        *reinterpret_cast<uint4*>(Or + (stage * TILE + srow) * SLD + spc) = dreg;
        if (tid < TILE) { nlr[stage * TILE + tid] = lreg; ndr[stage * TILE + tid] = dlreg; }
    };
    fetch(0);
    for (int e = tid; e < NP; e += 256) {
        bs[e] = e < N ? token_base4(e, wh, ww) : 0;
        Rs[e] = (REGION && e < N) ? (uint8_t)region[(int64_t)(w % nw_img) * N + e] : 0;
    }
    stage_table(tab, table, heads, h, G, false, tid, 256);
    const int j = kb * TILE + 16 * wave + c16;
    const bool vj = j < N;
    bf16x8 kfr, vfr;
    {
        uint4 k = make_uint4(0, 0, 0, 0), v = k;
        if (vj) {
            const bf16* r = base + (int64_t)j * 3 * C + 8 * g;
            k = *reinterpret_cast<const uint4*>(r + C);
            v = *reinterpret_cast<const uint4*>(r + 2 * C);
        }
        kfr = __builtin_bit_cast(bf16x8, k);
        vfr = __builtin_bit_cast(bf16x8, v);
    }
    put(0);
    __syncthreads();

    const float sc2 = scale * LOG2E;
    const f32x4 sc4 = {sc2, sc2, sc2, sc2};
    const uint32_t bj = lds_addr(tab) + 4u * (uint32_t)G.centre - (uint32_t)(vj ? bs[j] : 0);      // + bs[i]: LDS address of tab[idx_i - idx_j + centre]
    const uint32_t rj4 = REGION ? 0x01010101u * Rs[vj ? j : 0] : 0u;
    const int kg = 8 * (g ^ swz(c16));
    const int rr = 4 * g + (c16 >> 2);
    const int tcol[2] = {(((c16 >> 1) & 1) ^ swz(rr)) * 8 + 4 * (c16 & 1), ((2 + ((c16 >> 1) & 1)) ^ swz(rr)) * 8 + 4 * (c16 & 1)};
    f32x4 dv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dk[2] = {dv[0], dv[0]};

    for (int it = 0; it < NT; ++it) {
        const int stage = it & 1;
        if (it + 1 < NT) fetch(it + 1);
        const bf16* Qs = Qr + stage * TILE * SLD;
        const bf16* Os = Or + stage * TILE * SLD;
        const float* nls = nlr + stage * TILE;
        const float* nds = ndr + stage * TILE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 ppw, dsw;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int t = 2 * ks + half;                          // 16-query sub-tile of the stage
                const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_row8(Qs, SLD, 16 * t + c16, kg), kfr, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_row8(Os, SLD, 16 * t + c16, kg), vfr, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                const int l0 = 16 * t + 4 * g, i0 = it * TILE + l0;     // lane: queries i0 + r, key j
                const f32x4 nl4 = *reinterpret_cast<const f32x4*>(nls + l0), nd4 = *reinterpret_cast<const f32x4*>(nds + l0);
                const u32x4 bi4 = *reinterpret_cast<const u32x4*>(bs + i0);
                const f32x4 bb = {lds_f32_at(bj + bi4[0]), lds_f32_at(bj + bi4[1]), lds_f32_at(bj + bi4[2]), lds_f32_at(bj + bi4[3])};
                f32x4 a = __builtin_elementwise_fma(s, sc4, bb + nl4);
                if constexpr (REGION) {
                    const uint32_t x = *reinterpret_cast<const uint32_t*>(Rs + i0) ^ rj4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] += (x & (0xFFu << (8 * r))) ? MASK_LOG2 : 0.f;
                }
                f32x4 p;
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(a[r]);
                // (a padded query row: -lse = -1e30 -> P = 0, dS = 0; a padded key lane: finite values in columns discarded with it)
                const f32x4 ds = p * (dp + nd4);
                ppw[2 * half] = pack_bf16x2(p[0], p[1]); ppw[2 * half + 1] = pack_bf16x2(p[2], p[3]);
                dsw[2 * half] = pack_bf16x2(ds[0], ds[1]); dsw[2 * half + 1] = pack_bf16x2(ds[2], ds[3]);
            }
            const bf16x8 pp = __builtin_bit_cast(bf16x8, ppw), ds8 = __builtin_bit_cast(bf16x8, dsw);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                dv[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(Os + 32 * ks * SLD, rr, tcol[u]), pp, dv[u], 0, 0, 0);
                dk[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(Qs + 32 * ks * SLD, rr, tcol[u]), ds8, dk[u], 0, 0, 0);
            }
        }
        if (it + 1 < NT) put(stage ^ 1);
        __syncthreads();
    }
    bf16* row = dqkv + ((int64_t)w * N + (vj ? j : 0)) * 3 * C + h * HD;
    store_head_row16(row + C, g, pack4(dk[0], scale), pack4(dk[1], scale), vj);
    store_head_row16(row + 2 * C, g, pack4(dv[0], 1.f), pack4(dv[1], 1.f), vj);
}

// ------------------------------------------------------------------------------------------------ host side
size_t fwd_lds(int N, Geo G) {
    const int NP = cdiv(N, TILE) * TILE;
    return (size_t)4 * TILE * SLD * 2 + (size_t)NP * 4 + ((NP + 15) & ~15) + (size_t)(G.R + G.centre + 1) * 4;
}
size_t dq_lds(int N, Geo G) {
    const int NP = cdiv(N, 32) * 32;
    return (size_t)8 * 32 * SLD * 2 + (size_t)NP * 4 + ((NP + 15) & ~15) + (size_t)(G.R + G.centre + 1) * 4;
}
size_t dkv_lds(int N, Geo G) {
    const int NP = cdiv(N, TILE) * TILE;
    return (size_t)4 * TILE * SLD * 2 + (size_t)4 * TILE * 4 + (size_t)NP * 4 + ((NP + 15) & ~15) + (size_t)G.R * 4;
}
int dense_ld(int N) { return cdiv(N, 32) * 32; }

// dynamic LDS above 64 KB must be allowed per kernel, once
template <typename F> bool allow_lds(F* fn) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BUDGET) == hipSuccess;
}

}  // namespace

extern "C" int lavt_window_attn_stream_ok(int dtype, int N, int wd, int wh, int ww, int heads, int head_dim) {
    if (dtype != LAVT_BF16 || head_dim != HD || N < 16 || N > STREAM_MAX_N || heads < 1 || wd < 1 || wh < 1 || ww < 1 || N > wd * wh * ww) return 0;
    const Geo G = geo(wd, wh, ww);
    return fwd_lds(N, G) <= LDS_BUDGET && dq_lds(N, G) <= LDS_BUDGET && dkv_lds(N, G) <= LDS_BUDGET ? 1 : 0;
}

extern "C" int lavt_window_attn_stream_fwd(int dtype, const void* qkv, const int8_t* region, int nw_img, void* out, float* lse, const float* table, int wd,
                                           int wh, int ww, int nwin, int N, int heads, int head_dim, float scale, void* stream) {
    LAVT_CHECK_ARG(lavt_window_attn_stream_ok(dtype, N, wd, wh, ww, heads, head_dim), "lavt_window_attn_stream_fwd: bf16, head_dim 32, 16 <= N=%d <= %d required",
                   N, STREAM_MAX_N);
    LAVT_CHECK_ARG(qkv && out && lse && table && nwin > 0 && (!region || nw_img > 0), "lavt_window_attn_stream_fwd: bad arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Geo G = geo(wd, wh, ww);
    const size_t lds = fwd_lds(N, G);
    static const bool ok = allow_lds(&wattn_stream_fwd<true>) && allow_lds(&wattn_stream_fwd<false>);
    if (!ok) { lavt_set_error("lavt_window_attn_stream_fwd: cannot reserve LDS"); return LAVT_ERR_LAUNCH; }
    const dim3 grid(nwin * heads * cdiv(N, TILE));
    if (region) hipLaunchKernelGGL(wattn_stream_fwd<true>, grid, dim3(256), lds, st, (const bf16*)qkv, table, region, nw_img, (bf16*)out, lse, wd, wh, ww, N, heads, scale);
    else hipLaunchKernelGGL(wattn_stream_fwd<false>, grid, dim3(256), lds, st, (const bf16*)qkv, table, region, nw_img, (bf16*)out, lse, wd, wh, ww, N, heads, scale);
    LAVT_CHECK_LAUNCH("lavt_window_attn_stream_fwd");
    return LAVT_OK;
}

// scratch: delta [nwin][heads][N], then the dense bias gradient [heads][N][ld], ld = N rounded up to a multiple of 32
extern "C" int64_t lavt_window_attn_stream_bwd_ws(int dtype, int nwin, int N, int heads, int wd, int wh, int ww) {
    if (!lavt_window_attn_stream_ok(dtype, N, wd, wh, ww, heads, HD) || nwin < 1) return 0;
    return (int64_t)nwin * heads * N + (int64_t)heads * N * dense_ld(N);
}

extern "C" int lavt_window_attn_stream_bwd(int dtype, const void* qkv, const int8_t* region, int nw_img, const void* out, const void* dout, const float* lse,
                                           void* dqkv, const float* table, float* dtable, float* ws, int64_t ws_floats, int wd, int wh, int ww, int nwin, int N,
                                           int heads, int head_dim, float scale, void* stream) {
    LAVT_CHECK_ARG(lavt_window_attn_stream_ok(dtype, N, wd, wh, ww, heads, head_dim), "lavt_window_attn_stream_bwd: bf16, head_dim 32, 16 <= N=%d <= %d required",
                   N, STREAM_MAX_N);
    LAVT_CHECK_ARG(qkv && out && dout && lse && dqkv && table && dtable && nwin > 0 && (!region || nw_img > 0), "lavt_window_attn_stream_bwd: bad arguments");
    LAVT_CHECK_ARG(ws && ws_floats >= lavt_window_attn_stream_bwd_ws(dtype, nwin, N, heads, wd, wh, ww), "lavt_window_attn_stream_bwd: scratch of lavt_window_attn_stream_bwd_ws floats required");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Geo G = geo(wd, wh, ww);
    float* delta = ws;
    float* dense = ws + (int64_t)nwin * heads * N;
    const int ld = dense_ld(N), NKP = cdiv(N, 32);
    const dim3 gq(heads * cdiv(N, 16));
    const size_t lq = dq_lds(N, G);
#define LAVT_DQ(PPW_)                                                                                                                              \
    do {                                                                                                                                           \
        static const bool ok = allow_lds(&wattn_stream_dq<PPW_, true>) && allow_lds(&wattn_stream_dq<PPW_, false>);                                \
        if (!ok) { lavt_set_error("lavt_window_attn_stream_bwd: cannot reserve LDS"); return LAVT_ERR_LAUNCH; }                                    \
        if (region) hipLaunchKernelGGL((wattn_stream_dq<PPW_, true>), gq, dim3(512), lq, st, (const bf16*)qkv, table, region, nw_img, (const bf16*)out, \
                                       (const bf16*)dout, lse, (bf16*)dqkv, delta, dense, ld, wd, wh, ww, nwin, N, heads, scale);                  \
        else hipLaunchKernelGGL((wattn_stream_dq<PPW_, false>), gq, dim3(512), lq, st, (const bf16*)qkv, table, region, nw_img, (const bf16*)out,    \
                                (const bf16*)dout, lse, (bf16*)dqkv, delta, dense, ld, wd, wh, ww, nwin, N, heads, scale);                         \
    } while (0)
    if (NKP <= 16) LAVT_DQ(2);
    else if (NKP <= 24) LAVT_DQ(3);
    else if (NKP <= 40) LAVT_DQ(5);
    else LAVT_DQ(8);
#undef LAVT_DQ
    LAVT_CHECK_LAUNCH("lavt_window_attn_stream_bwd(dq)");
    static const bool okkv = allow_lds(&wattn_stream_dkv<true>) && allow_lds(&wattn_stream_dkv<false>);
    if (!okkv) { lavt_set_error("lavt_window_attn_stream_bwd: cannot reserve LDS"); return LAVT_ERR_LAUNCH; }
    const dim3 gk(nwin * heads * cdiv(N, TILE));
    const size_t lk = dkv_lds(N, G);
    if (region) hipLaunchKernelGGL(wattn_stream_dkv<true>, gk, dim3(256), lk, st, (const bf16*)qkv, table, region, nw_img, (const bf16*)dout, lse, delta,
                                   (bf16*)dqkv, wd, wh, ww, N, heads, scale);
    else hipLaunchKernelGGL(wattn_stream_dkv<false>, gk, dim3(256), lk, st, (const bf16*)qkv, table, region, nw_img, (const bf16*)dout, lse, delta,
                            (bf16*)dqkv, wd, wh, ww, N, heads, scale);
    LAVT_CHECK_LAUNCH("lavt_window_attn_stream_bwd(dkv)");
    return lavt_relpos_reduce(dense, dtable, wd, wh, ww, N, heads, ld, stream);
}
