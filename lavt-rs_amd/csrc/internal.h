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
// gemm_tn_plan.hip (lavt_gemm_tn_route / lavt_gemm_tn_group_route, include/lavt_hip.h) decides kernel, pieces, write form and rider; gemm.hip launches
// what the route names.  The launchers below fill their device structs from a route of theirs and map it to an instantiation (a route naming no
// instantiation is LAVT_ERR_INVALID: the planner makes none).
int lavt_gemm_tn_v2(const lavt_gemm_tn_t& p, const lavt_gemm_tn_route_t& r, hipStream_t st);          // gemm_tn_v2.hip: LAVT_TN_V2

// A LayerNorm backward (the partial-sum form of lavt_layernorm_bwd_partial, bf16, no gather) offered to a grouped weight-gradient launch; it runs as
// rider workgroups of the launch where the route says LAVT_TN_RIDER_RIDES.  Passed by pointer between gemm.hip, gemm_tn_v2.hip and gemm_tn_pipe.hip.
struct lavt_ln_rider_t { const void* dy; const void* x; const float* gamma; const float* mean; const float* rstd; void* dx; float* partials; const void* dres; int rows, C; };

int lavt_gemm_tn_grouped_v2(const lavt_gemm_tn_t* probs, int n, const lavt_gemm_tn_group_route_t& r, hipStream_t st, const lavt_ln_rider_t* ln);          // gemm_tn_v2.hip: LAVT_TN_GROUP64
int lavt_gemm_tn_grouped_pipe(const lavt_gemm_tn_t* probs, int n, const lavt_gemm_tn_group_route_t& r, hipStream_t st, const lavt_ln_rider_t* ln);        // gemm_tn_pipe.hip: LAVT_TN_PIPE
int lavt_gemm_tn_grouped_sk_v2(const lavt_gemm_tn_t* probs, int n, const lavt_gemm_tn_group_route_t& r, float* scratch, hipStream_t st);                  // gemm_tn_v2.hip: LAVT_TN_SK

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
