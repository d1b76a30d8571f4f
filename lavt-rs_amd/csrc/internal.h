// Host-side declarations shared between the translation units of liblavt_hip.so: every function that is defined in one .hip file and called from
// another, the one struct they pass between them, and two small host helpers.  Included by the defining file AND its callers, so the compiler checks
// each definition against its declaration.  None of these names is exported with C linkage; the public surface is include/lavt_hip.h.
#pragma once
#include "common.h"

// ---- NT family ----------------------------------------------------------------------------------------------------------------------------------------
// gemm_nt_plan.hip (lavt_gemm_nt_route, include/lavt_hip.h) decides the kernel of a problem; gemm.hip launches the route's family.  The two LDS-DMA
// families map a route of theirs to its instantiation and launch it (a route naming no instantiation is LAVT_ERR_INVALID: the planner makes none).
int lavt_gemm_nt_v2(const lavt_gemm_nt_t& p, const lavt_gemm_nt_route_t& r, hipStream_t st);            // gemm_v2.hip
int lavt_gemm_nt_pipe(const lavt_gemm_nt_t& p, const lavt_gemm_nt_route_t& r, hipStream_t st);          // gemm_nt_pipe.hip
// the fields of a route that select an instantiation inside a family, as one switch value
constexpr unsigned lavt_nt_route_key(int tile, int stages, int b_kmajor, int kwalk, int kind, int lean) {
    return (unsigned)(tile / 64) | (stages == 2 ? 0u : 8u) | (b_kmajor ? 16u : 0u) | (unsigned)kwalk << 5 | (unsigned)lean << 7 | (unsigned)kind << 9;
}
// Dynamic LDS above 64 KiB has to be requested once per kernel; `*reserved` is the launcher's flag for its instantiation.
static inline int lavt_nt_reserve_lds(bool* reserved, const void* kernel, size_t lds, const char* who) {
    if (*reserved || lds <= 65536) return LAVT_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        lavt_set_error("%s: cannot reserve %zu bytes of LDS", who, lds);
        return LAVT_ERR_LAUNCH;
    }
    *reserved = true;
    return LAVT_OK;
}

// ---- TN family ----------------------------------------------------------------------------------------------------------------------------------------
// gemm_tn_v2.hip: bf16 LDS-DMA kernel.  Returns 1 when the problem is not for this kernel (the caller falls back to gemm.hip).
int lavt_gemm_tn_v2(const lavt_gemm_tn_t& p, hipStream_t st);

// A LayerNorm backward (the partial-sum form of lavt_layernorm_bwd_partial, bf16, no gather) offered to a grouped weight-gradient launch to run as
// rider workgroups.  Passed by pointer between gemm.hip, gemm_tn_v2.hip and gemm_tn_pipe.hip.
struct lavt_ln_rider_t { const void* dy; const void* x; const float* gamma; const float* mean; const float* rstd; void* dx; float* partials; const void* dres; int rows, C; };

// gemm_tn_v2.hip: n independent weight-gradient problems as one grouped launch without split-K when they qualify (bf16, plain / row-mapped operands,
// >= 256 output tiles in total).  Returns 1 when the group cannot run as one launch (the caller then issues the problems one by one).
// ln != NULL: a LayerNorm backward to run as rider workgroups of the launch; returns 3 when the group was launched WITHOUT it (the caller launches it).
int lavt_gemm_tn_grouped_v2(const lavt_gemm_tn_t* probs, int n, hipStream_t st, const lavt_ln_rider_t* ln);
// gemm_tn_pipe.hip: the grouped weight-gradient launch on 128x128 pipelined tiles.  Returns 1 when the group does not qualify (the caller takes
// gemm_tn_v2.hip's launch), LAVT_OK when it was launched (with the LayerNorm rider if `ln` was given), 3 when it was launched WITHOUT the rider it was offered.
int lavt_gemm_tn_grouped_pipe(const lavt_gemm_tn_t* probs, int n, hipStream_t st, const lavt_ln_rider_t* ln);
// The stream-K form of the grouped launch (gemm_tn_v2.hip): 128x128 tiles, the K-tile iterations of all members dealt in equal runs to persistent
// workgroups, split tiles through `scratch`.  _ws: floats of scratch the group wants, 0 = the group does not qualify (use lavt_gemm_tn_grouped).
// _sk_v2 returns 1 when the group does not qualify or the scratch is too small.
int64_t lavt_gemm_tn_grouped_sk_ws_v2(const lavt_gemm_tn_t* probs, int n);
int lavt_gemm_tn_grouped_sk_v2(const lavt_gemm_tn_t* probs, int n, float* scratch, int64_t scratch_floats, hipStream_t st);

// ---- LayerNorm backward (norm.hip) --------------------------------------------------------------------------------------------------------------------
// geometry of the plain (no gather, no xn output) partial-sum form, for the grouped weight-gradient launch that runs it in rider workgroups
int lavt_ln_bwd_geometry(int dtype, int rows, int C, int* lpr, int* cpl, int* waves);
// lavt_layernorm_bwd_partial without a gather map
int lavt_layernorm_bwd_partial_impl(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx, float* ws,
                                    int64_t ws_floats, const void* dres, int rows, int C, void* stream);

// ---- bf16 MFMA window attention (attention_mfma.hip), dispatched from attention.hip ---------------------------------------------------------------------
int lavt_window_attn_fwd_mfma(const void* qkv, const float* table, const int8_t* region, int nw_img, void* out, float* lse,
                              int wd, int wh, int ww, int nwin, int N, int heads, float scale, hipStream_t st);
// prev: the binning job of an EARLIER launch to run inside this one (8-wave variants; launched on its own in front otherwise); mine != NULL: this
// launch's own binning is NOT launched but described in *mine (the caller hands it to the next launch or to lavt_attn_dtable_run)
int lavt_window_attn_bwd_mfma(const void* qkv, const float* table, const int8_t* region, int nw_img, const void* out, const void* dout,
                              const float* lse, void* dqkv, float* dtable, int bias_ld, float* ws, float* parts, int wd, int wh, int ww, int nwin, int N,
                              int heads, float scale, hipStream_t st, const lavt_dtable_job_t* prev, lavt_dtable_job_t* mine);
int lavt_attn_dtable_run_mfma(const lavt_dtable_job_t* jb, hipStream_t st);
int lavt_window_attn_bwd_det_mfma(const void* qkv, const float* table, const int8_t* region, int nw_img, const void* out, const void* dout, const float* lse,
                                  void* dqkv, float* dtable, int bias_ld, float* ws, float* parts, int wd, int wh, int ww, int nwin, int N, int heads, float scale,
                                  hipStream_t st);
int lavt_attn_dtable_finish_multi_impl(const int64_t* desc, int n, int max_R, int max_heads, int total_heads, hipStream_t st);
int lavt_window_attn_bwd_pieces_mfma(int nwin, int N, int heads);
int64_t lavt_window_attn_bwd_ws_mfma(int nwin, int N, int heads, int bias_ld, int wd, int wh, int ww);

// ---- host helpers ---------------------------------------------------------------------------------------------------------------------------------------
// taps of an implicit-GEMM convolution problem (lavt_gemm_nt_t / lavt_gemm_tn_t): kd defaults to 1, kh and kw to 3
template <typename P> static inline int conv_taps_of(const P& p) {
    return (p.conv_kd > 0 ? p.conv_kd : 1) * (p.conv_kh > 0 ? p.conv_kh : 3) * (p.conv_kw > 0 ? p.conv_kw : 3);
}
// source step per output pixel of an align_corners=True bilinear resize (the `scale` of bl_coord, common.h)
static inline float bl_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }
