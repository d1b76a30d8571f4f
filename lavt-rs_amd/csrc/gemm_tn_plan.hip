// The planner of the TN (weight-gradient) GEMM family: which kernel, tile, K pieces, write form and LayerNorm rider lavt_gemm_tn and the grouped
// entries launch, decided in ONE place.  Host code only -- no __global__ function, no HIP runtime call, and no pointer of a problem is ever read
// through (pointers are tested for NULL and for alignment).  gemm.hip routes a problem or a group here and launches what the route names;
// gemm_tn_v2.hip and gemm_tn_pipe.hip fill their device structs from a route and map it to an instantiation.  A new tile, threshold or piece rule is
// an edit of this file; tests/test_gemm_tn_route_host.py holds the restatement in tests/gemm_tn_cases.py to this planner.
//
// Single problems (lavt_gemm_tn_route).  v2 = the bf16 LDS-DMA kernel of gemm_tn_v2.hip (tn_v2_eligible: zero page, 16-byte aligned rows, only
// 0 / constant row masks -- they can be folded into the row fetch --, no maps under taps or a second source, 32-bit element offsets), else the
// classic register-staged kernel of gemm.hip (fp32, and what v2 declines).
//   * v2 tile, measured (tools/gemm_bench.py tn): the 64x64 / 4-wave tile wins on every weight-gradient shape of the step, the conv wgrads included
//     (369 vs 230 TF/s for 128x128); conv weight gradients with long K and >= TN_BIG_MIN = 48 tiles of 128x128 (the Swin-T decoder's 384-channel
//     convolutions have 102) take 128x128 / 8 waves: the larger tile halves the L2->LDS bytes per MFMA (measured 303 vs 357 us on Swin-B's;
//     16.9 -> 16.1 ms per Swin-T step).  Two-stage ring only (3 / 4 stages cost a resident workgroup per CU and lost end to end in round 1).
//   * v2 split: the split-K factor trades workgroup count (latency hiding) against fp32 atomic traffic: ~3 (64-tile: 768) / ~1.5 (128-tile: 384)
//     workgroups per CU; no workgroup walks more than ~128 K tiles (long_k); >= tn_min_kt K tiles per piece.
//   * tn_min_kt: 8 K tiles per piece; batched problems -- the per-sample word-side reductions of the fused PWAM node: 2-4 output tiles -- are cut
//     down to 2: a piece is a serial chain of ~1 us per K tile on the 2-stage ring, and the launch sits on the critical chain.
//   * v2 column sums: on the matrix cores when the workgroups carrying them are a minority (64x64, >= 4 column tiles), the scalar walk otherwise.
//     convp: the kernel with the tap state (per-DMA coordinates, wrap tests); mapped problems are never convolutions, plain ones take the shorter loop.
//   * v2 write form: partial tiles instead of atomics when the caller lent scratch for every piece (no conv column permutation).
//   * classic: 128x128 only for I >= 256, J >= 1024, K >= 8192; split 768 / tiles, at least 4 K tiles per workgroup.
//
// Groups (lavt_gemm_tn_group_route), asked in the order PIPE, GROUP64, EACH.
//   PIPE (gemm_tn_pipe.hip).  Operands through one 2 GB buffer descriptor with 32-bit byte offsets, with room for the tiles issued beyond K
//   ((K + 1024) rows below 2^30 bytes); a MAPPED operand is addressed by source row: the rows its map may name must stay inside the descriptor as
//   well (a padded-window source or a large clip can be several times the reduction length -- beyond 2^31 bytes the hardware returns zeros).  A
//   group whose 128x128 tiles fill the chip (>= tn_pipe_min_tiles: the stage-2 / stage-3 Swin-block groups) runs uncut: one writer per output, chains
//   of <= 128 K tiles; short reductions stay on the 64x64 launch (tn_pipe_min_ktiles: at 8 K tiles -- the last stage's 450 tokens, 792 tiles -- a
//   workgroup that holds a CU alone spends more on its ring prologue and its 64 KB epilogue than on its K loop: 54 us against 49).  Otherwise
//   (LAVT_TN_PIPE=1: never; long reductions on few tiles: stage 0 / 1, PWAM's 1x1 convolutions) every member is cut through its partials scratch into
//   ONE round of workgroups of equal length (a workgroup holds a CU: 128 KB of LDS): the smallest piece length whose workgroup count stays inside
//   the chip (250) -- and leaves a fifth of it (208) to the LayerNorm riders when the launch carries them (they would otherwise queue behind the
//   tiles: +13 us at stage 0) ... unless giving the riders their fifth costs more than their own launch: with the measured 0.8 us per K tile, a
//   LayerNorm launch of ~4 us + its bytes at ~3 TB/s (Swin-T's stage 2 at 8 images: 117 tiles of 113 K tiles stay uncut under the rider budget
//   -- 96 us -- and take 57 K tiles + the reduction without riders: 63 + 16 us); the entry then launches the LayerNorm itself (AFTER).  A member
//   without a scratch for its pieces, pieces of > 128 K tiles or a workgroup count outside 96..256 keep the group on the 64x64 launch.  More than 8
//   pieces take tnp_reduce_pieces_deep.  The rider rides with one chunk per lane (C = 1024: two chunks per lane need 164 registers).
//   GROUP64 (gemm_tn_v2.hip): 64x64 tiles, 4 waves, 2-stage ring (rectangular 64 x 128 / 128 x 64 tiles measured level in round 4: 39.0 / 41.2 vs
//   39.0 us per stage-2 launch; an XCD-contiguous tile order and a 3-stage ring: 10.63 vs 10.64 and 10.81 vs 10.62 ms per step; none is kept).
//   Pieces per member: a member with a partials scratch may be cut as finely as its K allows -- the long-K weight gradients of PWAM (K = 28 800 rows
//   = 450 K tiles on 4 output tiles each) then run as ONE launch of ~1000 workgroups instead of four launches of ~230 at one workgroup per CU; a
//   member without one is cut into at most 4 pieces that meet through atomics (only if its C holds zeros: split_k < 0), and a chain of more than
//   128 K tiles without a scratch keeps the group from forming (it would run serially while the short members supply the tile count).
//   chain = 48 (32 / 48 / 64 / 128: video step 23.16 / 22.93 / 22.82 / 22.87 ms, image step level).  ... and only where cutting pays: a group whose
//   uncut 64x64 tiles already give every CU two workgroups (>= 512: the Swin-block launch at 4 images per GPU, K = 3600 = 57 K tiles) runs faster
//   uncut -- 64.9 vs 88.4 us (tools/wgrad_sk_time.py) -- unless a chain exceeds 128 K tiles; it is not cut through atomics either (two atomic
//   pieces per tile cost 12.60 vs 12.34 ms per step, and a plainly stored gradient needs no zero fill: engine.TrainStep).  More than 2048
//   workgroups: longer pieces (8 -> 64 K tiles).  Fewer than 256 workgroups are too few to fill the chip: EACH.  The rider rides only with column
//   sums (the rider kernels are CS = 2 instantiations) and when its scratch fits the idle tile ring.
//   SK (the stream-K entry): worth it when the 128x128 tiles alone cannot fill the chip in whole rounds but there is enough work for every run to
//   amortise its ring prologue (>= 6 K tiles per run, up to 512 runs, >= 128 runs, >= 32 tiles) -- the Swin-block launches of stages 1-3;
//   many-tile members (stage 0: K = 28 800) keep the piece form.  Scalar column sums: the matrix-core form costs 16 accumulator registers the
//   128-register tile does not have.
#include "internal.h"

namespace {

constexpr int TN_BIG_MIN = 48;
constexpr int GMAX = LAVT_TN_GROUP_MAX;
static_assert(sizeof(lavt_gemm_tn_route_t) == 40 && sizeof(lavt_gemm_tn_group_route_t) == 128, "lavt_hip/_capi.py declares these layouts");

inline int tn_ktiles(const lavt_gemm_tn_t& p) { return cdiv(p.K, 64); }
inline bool tn_maps(const lavt_gemm_tn_t& p) { return p.a_rowmap || p.a_rowscale || p.b_rowmap; }
inline int tn_min_kt(const lavt_gemm_tn_t& p) { return p.batch > 1 ? 2 : 8; }
inline int64_t tn_part_floats(const lavt_gemm_tn_t& p, int J) { return (int64_t)p.I * J + p.I; }          // one piece: its C tile and its column sums

bool tn_v2_eligible(const lavt_gemm_tn_t& p) {
    if (p.dtype != LAVT_BF16 || p.zeros == nullptr) return false;
    if (p.lda % 8 || p.ldb % 8 || (p.B2 && p.ldb2 % 8)) return false;
    if (p.a_rowscale && !p.a_rowscale_binary) return false;
    if (tn_maps(p) && (p.conv_kc > 0 || p.B2)) return false;                                      // the mapped K loop has no taps / second source
    if ((int64_t)p.K * (p.lda > p.ldb ? p.lda : p.ldb) >= (1LL << 31)) return false;                // 32-bit element offsets
    return true;
}
// a member of the two grouped launches of gemm_tn_v2.hip
bool tn_v2_member(const lavt_gemm_tn_t& p) { return tn_v2_eligible(p) && p.batch == 1 && p.conv_kc <= 0 && !p.B2 && p.I % 8 == 0 && p.J % 8 == 0; }

// `ns` pieces wanted -> pieces of equal length, none of them empty
void tn_cut(int ktiles, int ns, int32_t* pieces, int32_t* per) {
    *per = cdiv(ktiles, ns < 1 ? 1 : ns);
    *pieces = cdiv(ktiles, *per);
}

// (r.rider arrives as RIDES where a LayerNorm was offered and its geometry can ride, AFTER where it cannot; a planner may turn RIDES into AFTER)
bool tn_route_pipe(const lavt_gemm_tn_t* probs, int n, double ln_cells, lavt_gemm_tn_group_route_t& r) {
    const lavt_tuning_t& tun = lavt_tuning();
    if (tun.tn_pipe == 0) return false;
    int mt[GMAX], mj[GMAX], base_tiles = 0;          // 128x128 tiles and logical columns of a member
    long work = 0;                                   // (output tile, K tile) pairs of the launch
    for (int i = 0; i < n; ++i) {
        const lavt_gemm_tn_t& p = probs[i];
        const bool no_b = p.ldb == 0;                // (the column-sum-only side member: B = the zero page)
        if (p.dtype != LAVT_BF16 || p.batch != 1 || p.conv_kc > 0 || p.B2 || p.c_conv_permute) return false;
        if (p.I % 8 || p.J % 4 || p.lda % 8 || p.ldb % 8 || p.K < 8) return false;
        if ((int64_t)(p.K + 1024) * p.lda * 2 >= (1LL << 30) || (int64_t)(p.K + 1024) * p.ldb * 2 >= (1LL << 30)) return false;
        if (p.a_rowmap && p.a_src_rows > 0 && (p.a_src_rows + 1) * p.lda * 2 + 256 >= (1LL << 31)) return false;
        if (p.b_rowmap && p.b_src_rows > 0 && (p.b_src_rows + 1) * p.ldb * 2 + 256 >= (1LL << 31)) return false;
        if (p.a_rowscale && (!p.a_rowscale_binary || p.a_rowscale_div < 64 || cdiv(p.K, p.a_rowscale_div) > 64)) return false;          // a 64-bit keep mask over samples of >= 64 rows
        if (no_b ? !p.colsum : p.J % 8 != 0) return false;
        mj[i] = no_b ? 8 : p.J;
        mt[i] = cdiv(p.I, 128) * (no_b ? 1 : cdiv(p.J, 128));
        base_tiles += mt[i];
        work += (long)mt[i] * tn_ktiles(p);
    }
    const bool offered = r.rider != LAVT_TN_RIDER_NONE;
    int len = 128;                                   // uncut: chains of <= 128 K tiles
    if (base_tiles >= tun.tn_pipe_min_tiles) {
        if (work < (long)base_tiles * tun.tn_pipe_min_ktiles) return false;
        for (int i = 0; i < n; ++i)
            if (tn_ktiles(probs[i]) > 128) return false;
    } else {
        if (tun.tn_pipe < 2) return false;
        auto piece_len = [&](int budget) {
            int l = (int)((work + budget - 1) / budget);
            if (l < 8) l = 8;
            for (;; ++l) {
                long wgs = 0;
                for (int i = 0; i < n; ++i) wgs += (long)mt[i] * cdiv(tn_ktiles(probs[i]), l);
                if (wgs <= budget || l >= 128) break;
            }
            return l;
        };
        len = piece_len(offered ? 208 : 250);
        if (offered) {
            const int len_free = piece_len(250);
            const double ln_us = 4.0 + 6.0 * ln_cells / 3.0e6;
            if (0.8 * len > 0.8 * len_free + ln_us + 1.0) { len = len_free; r.rider = LAVT_TN_RIDER_AFTER; }
        }
    }
    int tiles = 0, max_ns = 1;
    int64_t max_total = 0;
    for (int i = 0; i < n; ++i) {
        const lavt_gemm_tn_t& p = probs[i];
        tn_cut(tn_ktiles(p), cdiv(tn_ktiles(p), len), &r.pieces[i], &r.kt_per_piece[i]);
        if (r.kt_per_piece[i] > 128) return false;
        if (r.pieces[i] > 1) {
            const int64_t tot = tn_part_floats(p, mj[i]);
            if (p.partials == nullptr || p.partials_floats < r.pieces[i] * tot) return false;
            r.parts[i] = r.any_parts = 1;
            max_total = max_total > tot ? max_total : tot;
            max_ns = max_ns > r.pieces[i] ? max_ns : r.pieces[i];
        }
        tiles += mt[i] * r.pieces[i];
    }
    if (base_tiles < tun.tn_pipe_min_tiles && (tiles < 96 || tiles > 256)) return false;
    r.launch = LAVT_TN_PIPE; r.stages = tun.tn_pipe_stages == 3 ? 3 : 4; r.workgroups = tiles;
    if (r.any_parts) { r.reducer = max_ns > 8 ? LAVT_TN_REDUCE_PIPE_DEEP : LAVT_TN_REDUCE_PIPE; r.reducer_grid_x = cdiv(max_total, max_ns > 8 ? 64 : 1024); }
    r.rider_wgs = (r.rider_blocks + 1) / 2;          // two 256-thread LayerNorm units per 512-thread workgroup
    return true;
}

bool tn_route_group64(const lavt_gemm_tn_t* probs, int n, lavt_gemm_tn_group_route_t& r) {
    constexpr int chain = 48, piece_tiles = 8;
    long uncut = 0;
    for (int i = 0; i < n; ++i) uncut += (long)cdiv(probs[i].I, 64) * cdiv(probs[i].J, 64);
    const bool cut_pays = uncut < 512;
    int tiles = 0;
    int64_t max_total = 0;
    for (int per_piece = piece_tiles; ; per_piece *= 2) {
        tiles = 0; r.any_parts = 0; max_total = 0;
        for (int i = 0; i < n; ++i) {
            const lavt_gemm_tn_t& p = probs[i];
            if (!tn_v2_member(p)) return false;
            const int ktiles = tn_ktiles(p), want = cdiv(ktiles, per_piece);
            const bool parts = p.partials != nullptr && !p.c_conv_permute && ktiles > chain && (cut_pays || ktiles > 128) && want > 1 &&
                               p.partials_floats >= want * tn_part_floats(p, p.J);
            if (!parts && ktiles > 128) return false;
            int ns = parts ? want : ((p.split_k < 0 && cut_pays) ? cdiv(ktiles, chain) : 1);
            if (!parts && ns > 4) ns = 4;
            tn_cut(ktiles, ns, &r.pieces[i], &r.kt_per_piece[i]);
            r.parts[i] = parts && r.pieces[i] > 1;
            if (r.parts[i]) { r.any_parts = 1; max_total = max_total > tn_part_floats(p, p.J) ? max_total : tn_part_floats(p, p.J); }
            tiles += cdiv(p.I, 64) * cdiv(p.J, 64) * r.pieces[i];
        }
        if (tiles <= 2048 || !r.any_parts || per_piece >= 64) break;
    }
    if (tiles < 256) return false;
    r.launch = LAVT_TN_GROUP64; r.stages = 2; r.workgroups = tiles;
    if (r.any_parts) { r.reducer = LAVT_TN_REDUCE_GROUP; r.reducer_grid_x = cdiv(max_total, 64); }
    // the rider kernels are CS = 2 instantiations (its scratch, 3 x lanes x 32 bytes <= 6 KB, always fits the idle 32 KB tile ring)
    if (!r.colsum_form && r.rider == LAVT_TN_RIDER_RIDES) r.rider = LAVT_TN_RIDER_AFTER;
    r.rider_wgs = r.rider_blocks;
    return true;
}

int tn_route_sk(const lavt_gemm_tn_t* probs, int n, lavt_gemm_tn_group_route_t& r) {
    int its = 0, tiles = 0;
    bool ok = n >= 2 && n <= GMAX;
    for (int i = 0; ok && i < n; ++i) {
        const lavt_gemm_tn_t& p = probs[i];
        ok = tn_v2_member(p) && !p.c_conv_permute;
        r.pieces[i] = 1; r.kt_per_piece[i] = tn_ktiles(p);
        its += cdiv(p.I, 128) * cdiv(p.J, 128) * tn_ktiles(p); tiles += cdiv(p.I, 128) * cdiv(p.J, 128);
    }
    int nw = 512;
    if (its / nw < 6) nw = its / 6;
    LAVT_CHECK_ARG(ok && nw >= 128 && tiles >= 32, "lavt_gemm_tn_grouped_sk: the group does not qualify (ask lavt_gemm_tn_grouped_sk_ws first)");
    r.launch = LAVT_TN_SK; r.stages = 2; r.workgroups = nw; r.colsum_form = r.colsum_form ? 1 : 0;
    r.scratch_floats = (int64_t)nw * 2 * (128 * 128 + 128);
    return LAVT_OK;
}

}  // namespace

extern "C" int lavt_gemm_tn_route(const lavt_gemm_tn_t* pp, lavt_gemm_tn_route_t* out) {
    LAVT_CHECK_ARG(pp != nullptr, "lavt_gemm_tn: null params");
    LAVT_CHECK_ARG(out != nullptr, "lavt_gemm_tn_route: null route");
    const lavt_gemm_tn_t& p = *pp;
    LAVT_CHECK_ARG(p.dtype == LAVT_F32 || p.dtype == LAVT_BF16, "lavt_gemm_tn: bad dtype %d", p.dtype);
    const int epc = p.dtype == LAVT_F32 ? 4 : 8;
    LAVT_CHECK_ARG(p.I > 0 && p.J > 0 && p.K > 0 && p.batch >= 1, "lavt_gemm_tn: bad shape");
    LAVT_CHECK_ARG(p.I % epc == 0 && p.J % epc == 0, "lavt_gemm_tn: I=%d, J=%d must be multiples of %d", p.I, p.J, epc);
    LAVT_CHECK_ARG(p.A && p.B && p.C, "lavt_gemm_tn: null operand");
    LAVT_CHECK_ARG(p.lda % epc == 0 && p.ldb % epc == 0, "lavt_gemm_tn: lda/ldb must be multiples of %d", epc);
    LAVT_CHECK_ARG(!p.B2 || (p.b_split % epc == 0 && p.ldb2 % epc == 0), "lavt_gemm_tn: bad b_split");
    if (p.conv_kc > 0)
        LAVT_CHECK_ARG(p.J == conv_taps_of(p) * p.conv_kc && p.conv_kc % epc == 0 && p.conv_h > 0 && p.conv_w > 0, "lavt_gemm_tn: bad conv geometry");
    lavt_gemm_tn_route_t r = {};
    r.dtype = p.dtype;
    const int force = lavt_tuning().gemm_tile;          // LAVT_GEMM_TILE=128|64 forces a tile configuration (tests exercise both)
    int split = p.split_k, ktiles;
    if (tn_v2_eligible(p)) {
        ktiles = tn_ktiles(p);
        const long tiles128 = (long)cdiv(p.I, 128) * cdiv(p.J, 128) * p.batch;
        const bool big = force ? force == 128 : (p.conv_kc > 0 && tiles128 >= TN_BIG_MIN && ktiles >= 64);
        const long tiles = big ? tiles128 : (long)cdiv(p.I, 64) * cdiv(p.J, 64) * p.batch;
        r.family = LAVT_TN_V2; r.tile = big ? 128 : 64; r.waves = big ? 8 : 4;
        if (split <= 0) {
            split = (int)(((big ? 384 : 768) + tiles / 2) / tiles);
            const int long_k = (ktiles + 127) / 128, max_split = cdiv(ktiles, tn_min_kt(p));
            if (split < long_k) split = long_k;
            if (split > max_split) split = max_split;
        }
        r.maps = tn_maps(p);
        r.colsum_form = !p.colsum ? 0 : ((!big && cdiv(p.J, 64) >= 4) ? 2 : 1);
        r.convp = !r.maps && (p.conv_kc > 0 || p.c_conv_permute);
    } else {
        LAVT_CHECK_ARG(!p.colsum_atomic, "lavt_gemm_tn: colsum_atomic needs the bf16 LDS-DMA kernel (bf16 operands, 16-byte aligned rows, zeros page)");
        ktiles = cdiv(p.K, p.dtype == LAVT_F32 ? 16 : 64);
        const bool big = force ? force == 128 : (p.I >= 256 && p.J >= 1024 && p.K >= 8192);
        r.family = LAVT_TN_CLASSIC; r.tile = big ? 128 : 64; r.waves = 4;
        if (split <= 0) {
            split = (int)(768 / ((long)cdiv(p.I, r.tile) * cdiv(p.J, r.tile) * p.batch));
            if (split > (ktiles + 3) / 4) split = (ktiles + 3) / 4;
        }
    }
    tn_cut(ktiles, split > ktiles ? ktiles : split, &r.pieces, &r.kt_per_piece);
    const bool parts = r.family == LAVT_TN_V2 && r.pieces > 1 && p.partials && !p.c_conv_permute && p.partials_floats >= (int64_t)p.batch * r.pieces * tn_part_floats(p, p.J);
    r.write = parts ? LAVT_TN_PARTS : ((r.pieces > 1 || p.accumulate || r.family == LAVT_TN_CLASSIC) ? LAVT_TN_ATOMIC : LAVT_TN_STORE);
    *out = r;
    return LAVT_OK;
}

extern "C" int lavt_gemm_tn_group_route(const lavt_gemm_tn_t* probs, int n, int entry, int ln_rows, int ln_C, lavt_gemm_tn_group_route_t* out) {
    LAVT_CHECK_ARG(probs != nullptr && n >= 1 && out != nullptr && (entry == LAVT_TN_ENTRY_GROUPED || entry == LAVT_TN_ENTRY_SK), "lavt_gemm_tn_group_route: bad arguments");
    lavt_gemm_tn_group_route_t r = {};
    for (int i = 0; i < n; ++i) {
        r.maps |= tn_maps(probs[i]) ? 1 : 0;
        r.colsum_form |= probs[i].colsum ? 2 : 0;
    }
    if (entry == LAVT_TN_ENTRY_SK) return tn_route_sk(probs, n, *out = r);
    if (ln_rows > 0) {          // the rider rides with 4 waves and one chunk per lane (C = 1024: two chunks per lane need 164 registers -- a fourth workgroup per CU no longer fits)
        int cpl = 0, waves = 0;
        r.rider_blocks = lavt_ln_bwd_geometry(LAVT_BF16, ln_rows, ln_C, &r.rider_lpr, &cpl, &waves);
        const bool can = waves == 4 && cpl == 1 && (r.rider_lpr == 16 || r.rider_lpr == 32 || r.rider_lpr == 64) && r.rider_blocks > 0;
        r.rider = can ? LAVT_TN_RIDER_RIDES : LAVT_TN_RIDER_AFTER;
    }
    bool formed = n >= 2 && n <= GMAX && (tn_route_pipe(probs, n, (double)ln_rows * ln_C, *out = r) || tn_route_group64(probs, n, *out = r));
    if (!formed) {          // one launch per problem, the LayerNorm after them
        *out = r;
        if (out->rider) out->rider = LAVT_TN_RIDER_AFTER;
        for (int i = 0; i < n; ++i) {
            lavt_gemm_tn_route_t one;
            const int rc = lavt_gemm_tn_route(&probs[i], &one);
            if (rc != LAVT_OK) return rc;
            if (i < GMAX) { out->pieces[i] = one.pieces; out->kt_per_piece[i] = one.kt_per_piece; out->parts[i] = one.write == LAVT_TN_PARTS; out->any_parts |= out->parts[i]; }
        }
    }
    if (out->rider != LAVT_TN_RIDER_RIDES) out->rider_lpr = out->rider_blocks = out->rider_wgs = 0;
    return LAVT_OK;
}

extern "C" int lavt_gemm_tn_v2_eligible(const lavt_gemm_tn_t* p) { return p != nullptr && tn_v2_eligible(*p) ? 1 : 0; }

extern "C" int lavt_gemm_tn_pieces(const lavt_gemm_tn_t* p) {
    if (!p || p->K <= 0) return 1;
    return cdiv(tn_ktiles(*p), tn_min_kt(*p));
}

extern "C" int64_t lavt_gemm_tn_grouped_sk_ws(const lavt_gemm_tn_t* probs, int n) {
    if (probs == nullptr || n < 1) return 0;
    for (int i = 0; i < n; ++i)
        if (!(probs[i].A && probs[i].B && probs[i].C && probs[i].I > 0 && probs[i].J > 0 && probs[i].K > 0)) return 0;
    lavt_gemm_tn_group_route_t r;
    return lavt_gemm_tn_group_route(probs, n, LAVT_TN_ENTRY_SK, 0, 0, &r) == LAVT_OK ? r.scratch_floats : 0;
}
