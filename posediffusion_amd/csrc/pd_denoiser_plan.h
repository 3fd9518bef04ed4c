// pd_denoiser_plan.h -- which kernels one step of the default-shape denoiser launches, decided once per pd_denoiser_launch from
// (B, N, engine options) and read by every encoder layer.  Plain integers and booleans in, a plain struct out: no HIP call, no global.
// Every choice below selects between kernels with bitwise-equal results, except the path itself (rounding-level differences between the
// small-batch, exact streamed and split-precision GEMMs; the MMA attention kernel against the sequential one likewise).
#pragma once
#include "pd_qkv_attn.h"

// build switch of the fp16-plane path's strip GEMMs (pd_gemm_strip.h): a decision, not a kernel form (tools/den_ab.py runs both sides)
#ifndef PD_STRIP_RT3
#define PD_STRIP_RT3 1         // round 6: 96-row tiles for the 512-wide strip GEMMs when that takes them from more tiles than CUs to at most one per CU
#endif

enum PdDenPath {
    PD_DEN_SMALL,         // fewer than PD_STREAM_MIN_ROWS token rows (or an engine created for fewer): 32-row split-K tiles (pd_gemm_small.h)
    PD_DEN_STREAMED,      // exact fp32, 64 x 64 tiles streamed through LDS (pd_gemm_stream.h)
    PD_DEN_BF16_PLANES,   // PD_OPT_DENOISER_SPLIT = 1, the fast mode (pd_gemm_split.h)
    PD_DEN_F16_PLANES     // PD_OPT_DENOISER_SPLIT = 2
};

struct PdDenStepPlan {
    PdDenPath path;
    int M, MT;             // token rows; 32-row tiles of the small-batch GEMMs
    bool long_attn;        // every path: the key-tiled pd_attn_long_kernel (pd_attn_long.h) in place of the path's attention kernel -- above 64
                           //   frames always, below on request (PD_OPT_DENOISER_LONG_ATTN = 1: bitwise the kernel it replaces, except pd_attn_mma_kernel)
                           //   and whenever frame counts per sequence are set
    // PD_DEN_F16_PLANES only (zero on the other paths)
    bool fused_attn;       // in_proj + attention as ONE kernel (pd_qkv_attn.h), else the QKV GEMM and an attention kernel
    bool attn_mma;         // the attention kernel of the two-launch form: pd_attn_mma_kernel, else pd_attn_seq_kernel (or the long kernel, above)
    int rt_res, rt_ff1;    // 32-row tiles per workgroup (2 or 3) of the strip GEMMs: out-projection and FF2 (512 wide, residual epilogue); FF1
    int strip;             // PD_DEN_STRIP: bit mask {QKV, out, FF1, FF2} of the GEMMs on the strip kernel; the others run pd_gemm_split
};

// split / fused_attn: PD_OPT_DENOISER_SPLIT / PD_OPT_DENOISER_FUSED_ATTN; has_streamed: the engine was created for >= PD_STREAM_MIN_ROWS token
// rows; split_ready / split_h_ready: the bf16 / fp16 planes are built; knob_*: the development knobs PD_DEN_STRIP and PD_DEN_ATTN_MMA;
// long_attn: PD_OPT_DENOISER_LONG_ATTN; ragged: frame counts per sequence are set (pd_engine_set_frame_counts) -- the key-tiled kernel is the
// one attention kernel that takes a length per sequence, so it serves every N then (and the fused in_proj + attention kernel is not chosen)
static inline PdDenStepPlan pd_den_step_plan(int B, int N, int split, int fused_attn, int num_cus, bool has_streamed, bool split_ready,
                                             bool split_h_ready, int knob_strip, int knob_attn_mma, int long_attn = 0, bool ragged = false) {
    PdDenStepPlan p = {};
    p.M = B * N;
    p.MT = (p.M + 31) / 32;
    p.long_attn = N > 64 || long_attn != 0 || ragged;
    // >= 1024 token rows (52 sequences of 20 frames): the encoder GEMMs are large enough for 64 x 64 tiles streamed through LDS
    // (pd_gemm_stream.h; same sums in another order than the 32-row split-K tiles of the small path, i.e. rounding-level differences
    // between small and large batches)
    if (p.M < PD_STREAM_MIN_ROWS || !has_streamed) p.path = PD_DEN_SMALL;
    else if (split == 2 && split_h_ready) p.path = PD_DEN_F16_PLANES;
    else if (split == 1 && split_ready) p.path = PD_DEN_BF16_PLANES;
    else p.path = PD_DEN_STREAMED;
    if (p.path != PD_DEN_F16_PLANES) return p;
    const int cus = num_cus > 0 ? num_cus : 256;
    // the fused kernel holds a CU for ~38 us whatever the batch (one workgroup per 4 sequences and head): it wins when its workgroups
    // fill the chip's rounds (256 sequences = 256 workgroups: -76 us per step), not at 103 sequences (104 workgroups: +2 %)
    const int qa_wgs = pd_qkv_attn_wgs(B, N);
    const bool qa_fills = 4 * qa_wgs >= 3 * ((qa_wgs + cus - 1) / cus) * cus;
    p.fused_attn = qa_wgs > 0 && !p.long_attn && (fused_attn == 1 ? qa_fills : fused_attn == 2);   // (qa_wgs is 0 above 32 frames)
    p.attn_mma = N <= 32 && knob_attn_mma && !p.long_attn;
    // 512-wide outputs: 96-row tiles where 64-row tiles would give the busiest CUs two tiles and most CUs one (5 120 rows: 320 tiles on 256 CUs ->
    // 216 tiles of 1.5 x the work: the launch is as long as its busiest CU).  Same sums in the same order: bitwise the same C.
    const bool rt3 = PD_STRIP_RT3 && (((p.M + 63) / 64) * (DM / 128)) > cus && (((p.M + 95) / 96) * (DM / 128)) <= cus;
    p.rt_res = rt3 ? 3 : 2;
    p.rt_ff1 = 2;          // the 1 024-wide FF1 has 640 tiles at 64 rows, 432 at 96: three tiles of 1 or two of 1.5 on the busiest CU -- measured the same
    p.strip = knob_strip;
    return p;
}
