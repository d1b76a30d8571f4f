// The planner of the NT GEMM family: which kernel instantiation lavt_gemm_nt launches for a problem, decided in ONE place.  Host code only -- no
// __global__ function, no HIP runtime call, and no pointer of the struct is ever read through (pointers are tested for NULL and for alignment).
// lavt_gemm_nt (gemm.hip) checks and routes a problem here and then launches what the route names: gemm.hip (classic), gemm_v2.hip and
// gemm_nt_pipe.hip each map a route to their instantiation and decide nothing.  A new tile, ring depth or threshold is an edit of this file (and of
// the family's route -> instantiation switch); tests/test_gemm_nt_route_host.py holds the restatement in tests/gemm_nt_cases.py to this planner.
//
// The three families, in the order they are asked:
//   pipe     gemm_nt_pipe.hip, software-pipelined K loop, 8 waves: the 256x256 tile (2-stage ring, 128 KB of LDS, one workgroup per CU) and the
//            128x128 tile on long reductions.  bf16 and e4m3 operands, zero page required.
//   v2       gemm_v2.hip, LDS-DMA ring scheduled by the compiler: 128x128 / 8 waves and 64x64 / 4 waves, rings of 2 and 4 stages; the only home of the
//            LayerNorm-folded A operand (LNA), the fused activation gradient (DACT) and their stored-derivative forms (GD); e4m3 problems the
//            pipelined family does not take.
//   classic  gemm.hip, register-staged double buffer: fp32 (the parity path) and bf16 without a zero page or with rows that are not 16-byte aligned.
//
// Tile and ring depth (nt_tile_rule), measured on MI355X (tools/gemm_bench.py, hipGraph-timed):
//   * 128x128 tile with 8 waves (2 per SIMD: one wave's DMA issue and LDS reads hide under the other's MFMAs) once there are >= 200 such tiles, else
//     64x64 tiles / 4 waves (5 workgroups per CU): the backbone GEMMs of the batch-2 step are latency-bound, more workgroups per CU hide it better.
//   * long reductions on few tiles (3-D convolutions of SepTPWAM: K = 27 C on 144 tiles of 128x128) also take the 128x128 tile (K >= 4096 and
//     >= GEMM_BIG_LONG tiles): a launch lasts as long as its serial chain of K tiles, and the larger tile moves half the bytes per K tile and flop.
//   * ring depth: in isolation (operands L2-resident) 2 stages win everywhere; inside the training step the operands of the small GEMMs arrive cold
//     from HBM / Infinity Cache and a 4-deep ring is worth 0.8 ms per step.  For the 128x128 / 8-wave tile the 4-deep ring is 128 KB -- ONE workgroup
//     per CU -- so a launch of 257-600 such workgroups ran in two or three rounds of single workgroups; from S2_MIN128 = 257 workgroups up (more
//     workgroups than CUs) the 2-deep ring (64 KB, two co-resident workgroups whose barrier stalls overlap) wins: batch 4 11.70 -> 11.39 ms,
//     Video-Swin-B 19.55 -> 18.77, Swin-T batch 8 10.89 -> 10.73, headline 7.61 -> 7.58 (profiles/r05_zz_ring_depth_threshold_sweep.txt,
//     ..._rule_ab.txt).  Up to 256 workgroups (the M = 1800 GEMMs of batch 2) the 4-deep ring stays; 64x64 tiles switch at 512 workgroups.
//   * classic: 64x64 tiles win on every backbone GEMM of the batch-2 step; 128x128 pays only once there are >= 3 full waves of tiles (768).
// The pipelined family (nt_pipe_tile; tools/gemm_bench.py, tools/conv_small_probe.py): the 256x256 tile (128 flop per byte of LDS fill -- every CU
// ingests ~50 GB/s whatever the tile, so the 128x128 tile is fill-bound at half the rate) only when its tiles fill the 256 CUs well (whole rounds at
// >= 80 %) and K >= 1024; N within 1/16 of a multiple of 256 also takes it (Swin-T's 480-column data gradient of the concat convolution ran 439 us
// on 3600 128x128 tiles at 0.35 of peak; the columns beyond N are out-of-range offsets in the weight descriptor and masked stores).  The 128x128
// tile for long reductions (K >= 1024; LAVT_GEMM_PIPE=3: every 128x128 problem) where gemm_v2.hip would take its 8-wave 128x128 form.
//
// K walk (nt_kwalk; the kernels' MODE): plain = no conv taps, no concat source, K a multiple of the K tile: every lane's DMA source is a pointer that
// advances by a constant (the general decode made small GEMMs issue-bound: ~220 VALU/SALU instructions per K tile, 0.78 us per K tile at M = 2592,
// N = 512).  tap-walking = convolution taps with Cin (and the concat split) a multiple of the K tile, <= 32 taps (a bit per tap): the tap of a K
// tile is wave-uniform and walks with the loop.  partial-block = the tap walk for Cin % 64 != 0 (Swin-T's conv1_2: 384 + 96 = 480 input channels;
// the general decode ran at 0.19 of peak there), k-contiguous bf16 weights on the pipelined family only.  general = everything else, decoded per K
// tile.  The K tile is 64 bf16 or 128 e4m3 elements (the same 128 bytes).  The pipelined family addresses the tap walks through 32-bit buffer
// offsets, so every operand, halo margin included, has to stay below 2 GB there; gemm_v2.hip walks 64-bit pointers and has no such bound.
//
// Lean epilogues (nt_lean; gemm_common.h): instantiations without the features a launch does not use -- 1: bias / residual / row scale / row map
// only, 2: the bare store, 3: the bare store with the second output kept (split-output data gradient of a concat convolution, 256x256 tile).  The
// general walk and the DACT / LNA / gemm_v2 fp8 kernels have the full epilogue only.
#include "internal.h"

namespace {

// Workgroups of the 128x128 tile from which the 2-stage ring (two workgroups per CU) replaces the 4-stage one: more workgroups than the 256 CUs.
constexpr long S2_MIN128 = 257;
// Long reductions (K >= 4096) take the 128x128 tile from this many tiles up (below the general threshold of 200).
constexpr long GEMM_BIG_LONG = 128;

// The one tile / ring-depth rule of the two LDS-DMA families, and the two variants of it that exist today.
struct TileRule {
    bool forced;          // honours LAVT_GEMM_TILE / LAVT_GEMM_STAGES
    bool long_k;          // the long-K clause: K >= 4096 takes the 128x128 tile from GEMM_BIG_LONG tiles up
};
constexpr TileRule RULE_PLAIN = {true, true};          // plain bf16 problems of gemm_v2.hip and every problem of gemm_nt_pipe.hip
// LNA, DACT and fp8 problems of gemm_v2.hip: their launchers were cut-down copies of the rule that ignore the forced configuration and have no
// long-K clause (LNA and DACT reductions are a Swin block's width: K >= 4096 does not occur; for fp8 nobody has measured it -- see the PR text)
constexpr TileRule RULE_KIND = {false, false};

void nt_tile_rule(const lavt_gemm_nt_t& p, TileRule rule, int* tile, int* stages) {
    int force_tile = 0, force_stages = 0;
    if (rule.forced) { force_tile = lavt_tuning().gemm_tile; force_stages = lavt_tuning().gemm_stages; }          // (the RULE_KIND paths never read the tuning)
    const long tiles128 = (long)cdiv(p.M, 128) * cdiv(p.N, 128) * p.batch;          // (LNA problems have batch 1)
    const long tiles64 = (long)cdiv(p.M, 64) * cdiv(p.N, 64) * p.batch;
    const bool big = force_tile ? force_tile == 128 : ((tiles128 >= 200 || (rule.long_k && p.K >= 64 * 64 && tiles128 >= GEMM_BIG_LONG)) && p.N >= 128);
    const long wgs = big ? tiles128 : tiles64;
    *tile = big ? 128 : 64;
    *stages = (force_stages ? force_stages == 2 : wgs >= (big ? S2_MIN128 : 512)) ? 2 : 4;          // (a forced depth other than 2 means 4)
}

// K-walk mode.  f8: e4m3 operands (K tile of 128 elements of one byte); descriptors: the pipelined family's 32-bit buffer offsets (the 2 GB bound,
// and the only home of the partial-block walk).
int nt_kwalk(const lavt_gemm_nt_t& p, bool f8, bool descriptors) {
    const int bk = f8 ? 128 : 64, es = f8 ? 1 : 2;
    if (p.conv_kc <= 0) return (p.A2 == nullptr && p.K % bk == 0) ? LAVT_NT_WALK_PLAIN : LAVT_NT_WALK_GENERAL;
    const int taps = conv_taps_of(p);
    bool fits = true;
    if (descriptors) {
        const int64_t lim = (1ll << 31) - (1ll << 24);
        const int64_t a_rows = (int64_t)p.M + 2 * ((int64_t)(p.conv_h > 0 ? p.conv_h : 1) * p.conv_w + p.conv_w + 1);
        const int64_t b_rows = p.b_kmajor ? (int64_t)taps * p.conv_kc : p.N;
        fits = a_rows * p.lda * es < lim && (p.A2 == nullptr || a_rows * p.lda2 * es < lim) && b_rows * p.ldb * es + (int64_t)p.batch * p.strideB * es < lim;
    }
    const bool walkable = (p.A2 == nullptr || p.a_split % bk == 0) && taps <= 32 && fits;
    if (p.conv_kc % bk == 0 && walkable) return LAVT_NT_WALK_TAPS;
    // k-contiguous weights [Cout][taps][Cin] with Cin % 64 != 0 (Cin % 8 == 0; a concat boundary on a 64-channel block)
    if (descriptors && !f8 && !p.b_kmajor && p.conv_kc % 8 == 0 && walkable && p.conv_kc_split <= 0 && p.conv_tap_split <= 0 && p.batch == 1 &&
        p.K == taps * p.conv_kc && p.ldb >= (int64_t)taps * p.conv_kc)
        return LAVT_NT_WALK_PARTIAL;
    return LAVT_NT_WALK_GENERAL;
}

int nt_lean(const lavt_gemm_nt_t& p, const lavt_gemm_nt_route_t& r) {
    if (r.kwalk == LAVT_NT_WALK_GENERAL || r.family == LAVT_NT_CLASSIC || (r.family == LAVT_NT_V2 && r.kind != 0)) return 0;
    const bool bare = !p.bias && !p.R && !p.row_scale && !p.c_rowmap;
    const bool no_side = p.act == 0 && !p.mul && !p.Cpre;          // the lean predicate: no activation, multiplier or pre-activation output
    if (no_side && !p.C2) return bare ? 2 : 1;
    if (no_side && p.C2 && bare && r.tile == 256 && r.b_kmajor && r.kwalk == LAVT_NT_WALK_TAPS) return 3;
    return 0;
}

// Which tile of gemm_nt_pipe.hip a problem takes (0: none) and the ring depth (comments in the kernels know this as lavt_gemm_nt_pipe_tile).
int nt_pipe_tile(const lavt_gemm_nt_t& p, int* stages_out) {
    if ((p.dtype != LAVT_BF16 && p.dtype != LAVT_FP8) || p.zeros == nullptr) return 0;
    const lavt_tuning_t& tun = lavt_tuning();
    const int pipe = tun.gemm_pipe;                 // 0: gemm_v2 K loops only; 1: the 256x256 tile; 2: + 128x128 for K >= 1024; 3: + every 128x128 problem
    if (pipe < 1) return 0;
    if (p.dtype == LAVT_FP8) {          // e4m3 operands: k-contiguous, plain or tap-walking issue (anything else: gemm_v2.hip's fp8 form)
        if (p.b_kmajor || p.c_f32 || p.conv_kc_split > 0 || p.conv_tap_split > 0 || p.lda % 16 || p.ldb % 16 || (p.A2 && p.lda2 % 16)) return 0;
        if (nt_kwalk(p, true, true) == LAVT_NT_WALK_GENERAL) return 0;
    }
    if (p.lda % 8 || p.ldb % 8 || (p.A2 && p.lda2 % 8)) return 0;
    if (p.ln_wsum || p.dact_pre) return 0;
    if (p.conv_kc_split > 0) {          // the channel-split reduction exists in this family's tap-walking mode only
        *stages_out = 4;
        return 128;
    }
    int tile, stages;
    nt_tile_rule(p, RULE_PLAIN, &tile, &stages);
    const long tiles256x = (long)cdiv(p.M, 256) * cdiv(p.N, 256) * p.batch;
    const long rounds = (tiles256x + 255) / 256;
    const bool n_fits = p.N % 256 == 0 || (p.N % 8 == 0 && (long)p.N * 16 >= (long)cdiv(p.N, 256) * 256 * 15);
    const bool huge = tun.gemm_tile ? tun.gemm_tile == 512 : (n_fits && p.K >= 1024 && tiles256x >= 128 && tiles256x * 10 >= rounds * 256 * 8);
    if (huge) { *stages_out = 2; return 256; }
    if (tile == 128 && (pipe >= 3 || (pipe == 2 && p.K >= 1024))) { *stages_out = stages; return 128; }
    return 0;
}

}  // namespace

extern "C" int lavt_gemm_nt_route(const lavt_gemm_nt_t* pp, lavt_gemm_nt_route_t* out) {
    LAVT_CHECK_ARG(pp != nullptr, "lavt_gemm_nt: null params");
    LAVT_CHECK_ARG(out != nullptr, "lavt_gemm_nt_route: null route");
    const lavt_gemm_nt_t& p = *pp;
    // ---- the contract of include/lavt_hip.h ----------------------------------------------------------------------------------------------
    LAVT_CHECK_ARG(p.dtype == LAVT_F32 || p.dtype == LAVT_BF16 || p.dtype == LAVT_FP8, "lavt_gemm_nt: bad dtype %d", p.dtype);
    const int epc = p.dtype == LAVT_F32 ? 4 : (p.dtype == LAVT_FP8 ? 16 : 8);
    LAVT_CHECK_ARG(p.M > 0 && p.N > 0 && p.K > 0 && p.batch >= 1, "lavt_gemm_nt: bad shape M=%d N=%d K=%d batch=%d", p.M, p.N, p.K, p.batch);
    LAVT_CHECK_ARG(p.K % epc == 0, "lavt_gemm_nt: K=%d must be a multiple of %d", p.K, epc);
    LAVT_CHECK_ARG(p.A && p.B && p.C, "lavt_gemm_nt: null operand");
    LAVT_CHECK_ARG(p.lda % epc == 0 && p.ldb % epc == 0, "lavt_gemm_nt: lda/ldb must be multiples of %d", epc);
    LAVT_CHECK_ARG(p.ldc % 4 == 0, "lavt_gemm_nt: ldc must be a multiple of 4");
    LAVT_CHECK_ARG(!p.b_kmajor || p.N % epc == 0, "lavt_gemm_nt: k-major B needs N %% %d == 0", epc);
    LAVT_CHECK_ARG(!p.A2 || (p.a_split % epc == 0 && p.lda2 % epc == 0), "lavt_gemm_nt: bad a_split");
    LAVT_CHECK_ARG(!p.C2 || p.c_split % 4 == 0, "lavt_gemm_nt: bad c_split");
    if (p.conv_kc > 0) {
        const int taps = conv_taps_of(p);
        const int vox = (p.conv_d > 0 ? p.conv_d : 1) * p.conv_h * p.conv_w;
        if (p.conv_kc_split > 0) {
            int st_ = 0;
            LAVT_CHECK_ARG(p.dtype == LAVT_BF16 && p.conv_tap_split == 0 && p.conv_kc_split % 64 == 0 && p.batch * p.conv_kc_split == p.conv_kc && p.K == taps * p.conv_kc_split &&
                           p.strideB == 0 && taps <= 32 && (!p.A2 || p.a_split % 64 == 0) && p.zeros && nt_pipe_tile(p, &st_) == 128,
                           "lavt_gemm_nt: conv_kc_split needs batch * conv_kc_split == conv_kc, K == taps * conv_kc_split, strideB == 0 and the pipelined tap-walking kernel (bf16, conv_kc %% 64 == 0)");
        } else if (p.conv_tap_split > 0)
            LAVT_CHECK_ARG(p.dtype == LAVT_BF16 && p.K == p.conv_tap_split * p.conv_kc && p.batch * p.conv_tap_split == taps && p.conv_kc % 64 == 0 && taps <= 32 &&
                           (!p.A2 || p.a_split % 64 == 0) && p.zeros, "lavt_gemm_nt: conv_tap_split needs batch * conv_tap_split == taps and the tap-walking path (conv_kc %% 64 == 0)");
        else
            LAVT_CHECK_ARG(p.K == taps * p.conv_kc && p.conv_kc % epc == 0 && p.conv_h > 0 && p.conv_w > 0, "lavt_gemm_nt: bad conv geometry");
        LAVT_CHECK_ARG(p.M % vox == 0, "lavt_gemm_nt: conv rows %d not a multiple of D*H*W", p.M);
    }
    LAVT_CHECK_ARG((!p.R || p.ldr % 4 == 0) && (!p.Cpre || p.ldcpre % 4 == 0) && (!p.mul || p.ldmul % 4 == 0), "lavt_gemm_nt: ldr/ldcpre/ldmul must be multiples of 4");
    LAVT_CHECK_ARG(p.act != LAVT_ACT_GELU_D || (p.ln_wsum && p.Cpre && !p.mul && !p.C2 && !p.R && !p.row_scale && !p.c_rowmap),
                   "lavt_gemm_nt: LAVT_ACT_GELU_D exists in the LayerNorm-folded launch only (ln_wsum), needs Cpre and takes no multiplier / split / residual / row scale / row map");
    LAVT_CHECK_ARG(!p.res_first || (p.dact_pre && p.R), "lavt_gemm_nt: res_first orders the residual before the fused activation gradient (needs dact_pre and R)");

    lavt_gemm_nt_route_t r = {};
    r.dtype = p.dtype;
    r.b_kmajor = p.b_kmajor ? 1 : 0;
    // epi_wide bit 0: the 16-byte store form where every alignment holds; else the narrow 8-byte stores
    r.epi_wide = (p.dtype != LAVT_F32 && !p.c_f32 && p.ldc % 8 == 0 && (!p.C2 || (p.ldc2 % 8 == 0 && p.c_split % 8 == 0)) && (!p.R || p.ldr % 4 == 0) &&
                  (!p.Cpre || p.ldcpre % 8 == 0) && (!p.dact_pre || p.lddact % 4 == 0) && (!p.bias || (p.strideBias % 4 == 0 && ((uintptr_t)p.bias % 16) == 0)) &&
                  ((uintptr_t)p.C % 16) == 0 && (!p.C2 || ((uintptr_t)p.C2 % 16) == 0) && (!p.Cpre || ((uintptr_t)p.Cpre % 16) == 0) && (p.strideC % 8 == 0)) ? 1 : 0;
    // bit 1: the epilogue's side inputs are requested before the K loop (gemm_common.h NtSide)
    if (r.epi_wide && p.batch == 1) r.epi_wide |= 2;
    if (p.colstats) {
        int rpb = 0;
        LAVT_CHECK_ARG(lavt_gemm_nt_colstats_plan(&p, &rpb) > 0, "lavt_gemm_nt: colstats only where lavt_gemm_nt_colstats_plan accepts the problem (pipelined bf16 tiles, plain epilogue)");
    }

    // ---- the family, in order: pipe, v2, classic ---------------------------------------------------------------------------------------------
    const bool f8 = p.dtype == LAVT_FP8;
    if (const int pipe_tile = nt_pipe_tile(p, &r.stages)) {          // the 256x256 tile and the long-K 128x128 problems
        r.family = LAVT_NT_PIPE; r.tile = pipe_tile; r.waves = 8;
        r.kind = f8 ? LAVT_NT_F8 : 0;
        r.kwalk = nt_kwalk(p, f8, true);
    } else if (f8) {          // gemm_v2.hip's e4m3 form: k-contiguous A and B, 128-element K tiles
        if (p.b_kmajor || p.dact_pre || p.c_f32 || p.lda % 16 || p.ldb % 16 || (p.A2 && (p.lda2 % 16 || p.a_split % 16)) || p.K % 16 || (p.conv_kc > 0 && p.conv_kc % 16) || !p.zeros) {
            lavt_set_error("lavt_gemm_nt(fp8): needs k-contiguous e4m3 operands with 16-byte aligned rows (lda, ldb, K, conv_kc, a_split %% 16 == 0), bf16 C, no dact_pre");
            return LAVT_ERR_INVALID;
        }
        r.family = LAVT_NT_V2; r.kind = LAVT_NT_F8;
        nt_tile_rule(p, RULE_KIND, &r.tile, &r.stages);
        r.kwalk = nt_kwalk(p, true, false);
    } else if (p.dtype == LAVT_BF16 && p.zeros != nullptr && !(p.lda % 8 || p.ldb % 8 || (p.A2 && p.lda2 % 8))) {
        r.family = LAVT_NT_V2;
        if (p.ln_wsum) {
            // LayerNorm-folded A operand: plain k-contiguous problems whose workgroups see whole rows (every tile walks all of K)
            if (p.b_kmajor || p.conv_kc > 0 || p.A2 || p.a_rowmap || p.K % 64 || p.N % 4 || p.batch != 1 || p.dact_pre || !p.bias || p.alpha != 1.0f) {
                lavt_set_error("lavt_gemm_nt: ln_wsum (LayerNorm-folded A) needs a plain k-contiguous problem: no taps / concat / row gather / batch, K %% 64 == 0, bias = folded bias, alpha = 1");
                return LAVT_ERR_INVALID;
            }
            // (LAVT_ACT_GELU_D is its own instantiation: with the branch on p.act inside one kernel, the classic form ran 3 us per launch slower)
            const bool gd = p.act == LAVT_ACT_GELU_D && !p.mul && !p.C2 && !p.R && !p.row_scale && !p.c_rowmap;
            r.kind = LAVT_NT_LNA | (gd ? LAVT_NT_GD : 0);
            r.kwalk = LAVT_NT_WALK_PLAIN;
            nt_tile_rule(p, RULE_KIND, &r.tile, &r.stages);
        } else if (p.dact_pre) {
            // Fused activation-gradient epilogue: data gradients only (k-major B, plain K walk); a residual is taken in both orders the header states:
            // C * act'(pre) + R, and with res_first (C + R) * act'(pre).  Its own instantiations, so that no other kernel pays its registers (as a
            // run-time branch in every kernel it cost 12 VGPRs and 0.25 ms per step).
            if (!p.b_kmajor || p.conv_kc > 0 || p.A2 || p.K % 64 || p.lddact % 8 || p.c_f32 || p.C2 || p.Cpre || p.act || p.mul) {
                lavt_set_error("lavt_gemm_nt: dact_pre needs a plain k-major data-gradient problem (no taps / concat / activation / second output, K %% 64 == 0)");
                return LAVT_ERR_INVALID;
            }
            // the stored-derivative form (dact = LAVT_ACT_STORED) is its own instantiation (GD): a multiply, none of the transcendental forms; its wide
            // epilogue has no residual, bias or row map: any of them takes the general instantiation
            const bool gd = p.dact == LAVT_ACT_STORED && !p.R && !p.bias && !p.c_rowmap;
            r.kind = LAVT_NT_DACT | (gd ? LAVT_NT_GD : 0);
            r.kwalk = LAVT_NT_WALK_PLAIN;
            nt_tile_rule(p, RULE_KIND, &r.tile, &r.stages);
        } else {
            r.kwalk = nt_kwalk(p, false, false);
            nt_tile_rule(p, RULE_PLAIN, &r.tile, &r.stages);
        }
    } else {
        LAVT_CHECK_ARG(p.ln_wsum == nullptr, "lavt_gemm_nt: ln_wsum (LayerNorm-folded A operand) exists on the bf16 LDS-DMA path only");
        LAVT_CHECK_ARG(p.dact_pre == nullptr, "lavt_gemm_nt: dact_pre (fused activation gradient) exists on the bf16 LDS-DMA path only");
        const long tiles128 = (long)cdiv(p.M, 128) * cdiv(p.N, 128) * p.batch;
        const int force = lavt_tuning().gemm_tile;          // LAVT_GEMM_TILE=128|64 forces a tile configuration (tests exercise both)
        r.family = LAVT_NT_CLASSIC; r.waves = 4; r.stages = 2;
        r.tile = (force ? force == 128 : (tiles128 >= 768 && p.N >= 128)) ? 128 : 64;
        r.kwalk = LAVT_NT_WALK_GENERAL;
    }
    if (r.family == LAVT_NT_V2) r.waves = r.tile == 128 ? 8 : 4;
    r.lean = nt_lean(p, r);
    *out = r;
    return LAVT_OK;
}

extern "C" int lavt_gemm_nt_colstats_plan(const lavt_gemm_nt_t* pp, int* rows_per_block) {
    if (!pp || !rows_per_block) return 0;
    const lavt_gemm_nt_t& p = *pp;
    *rows_per_block = 0;
    if (p.batch != 1 || p.bias || p.act || p.R || p.row_scale || p.c_rowmap || p.c_f32 || p.C2 || p.Cpre || p.mul || p.N % 4 || p.M <= 0 || p.N <= 0) return 0;
    int stages = 0;
    const int tile = nt_pipe_tile(p, &stages);          // the statistics epilogue exists in the pipelined family only
    if (!tile) return 0;
    *rows_per_block = tile / 2;                      // a wave row of the 2 x 4 wave grid
    return cdiv(p.M, tile) * 2;
}
