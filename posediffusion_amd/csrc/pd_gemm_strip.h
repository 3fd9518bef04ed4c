// pd_gemm_strip.h -- the strip GEMM of the fp16-plane mode: the large-batch denoiser's four encoder GEMMs (pd_denoiser.hip) and the image feature
// extractor's four Linear layers (pd_vit.hip); pd_qkv_attn.h runs the same product inside the fused in_proj + attention kernel and takes its pieces
// from here (the end of this header's first part).  The arithmetic is pd_gemm_split.h's fp16-plane mode: every fp32 operand as fp16 hi + fp16 lo, x * w ~= lo*hi + hi*lo
// + hi*hi with fp32 accumulation, power-of-two scales fixed by the caller (c_scale on the accumulator, out_scale on split-word outputs).
//
// vit_gemm_split_kernel is bound by operand delivery, not by the matrix pipe: both waves of a row block fetch the same weight fragments from L2 and the A rows
// make a global -> VGPR -> v_perm -> ds_write round trip.  Here a workgroup's tile is (32 RT) rows x 128 columns and each of its four waves owns a STRIP of 32
// columns over all RT 32-row tiles: no weight fragment is fetched twice (they go L2 -> registers, already in operand order), and the A rows -- raw split
// words -- go L2 -> LDS by LDS-DMA (global_load_lds_dwordx4, hand-issued as in pd_gemm_dma_kernel) and are un-zipped into hi / lo fragments when they are read.
//
// K loop: A chunks of 64 k per barrier (two 32-k blocks of the same LDS layout, two buffers), the weight fragments of a block requested half a chunk ahead into the
// registers the previous block just freed.  K must be a multiple of 64.
// MFMA shape: the wave's 32-column strip as two 16-column tiles, a row block as 2 RT 16-row tiles, one v_mfma_f32_16x16x32_f16 per (row tile, column tile,
// product) and 32-k block.  An operand fragment is 16 rows (or columns) x 32 k: lane = (row % 16) + 16 (k group), 8 consecutive k per lane.  The weight planes
// keep pd_frag_split_kernel's 32-column x 16-k order: a lane takes its 16 bytes from where that order has its (column, k group) -- four runs of 256 contiguous
// bytes per wave-wide load, the same cache lines as one run of 1 KiB.  32 k per instruction: a sum's rounding differs in the last bit from vit_gemm_split_kernel's
// two chained 16-k instructions -- the same operands, products and order otherwise.
// A rows in LDS: the 16-byte slots of a row XOR-ed with pd_strip_swz(row); a ds_read_b128 serves 16 lanes at a time -- rows {0-3, 12-15} at k group g with rows
// 4-11 at k group g ^ 1 --, so the 16-row x 4-k-group read wants bits {0, 2} of the swizzle from the row (bit 1 is the k groups' own).
// Superseded forms (32-k chunks, 32x32x16 products, the compiler's schedule, the 4-byte epilogue, bf16 planes, two column tiles per wave, 32- and 128-row tiles)
// and what each measured: DESIGN_LOG.md, "strip / fused-QKV forms removed from the source".
#pragma once
#include "pd_gemm_split.h"

#if defined(PD_STRIP_PIPE) || defined(PD_STRIP_RES_AHEAD) || defined(PD_STRIP_WIDE_EPI) || defined(PD_STRIP_MFMA16) || defined(PD_STRIP_NOPERM) || \
    defined(PD_STRIP_K64) || defined(PD_STRIP_RT1) || defined(PD_STRIP_RT3_FF1)
#error "PD_STRIP_PIPE / _RES_AHEAD / _WIDE_EPI / _MFMA16 / _NOPERM / _K64 / _RT1 / _RT3_FF1 selected strip-kernel forms that are no longer in the source; commit 522349f is the last that has them"
#endif

#ifdef PD_STRIP_LEGS      // tools/strip_legs_probe.hip only: cycle stamps of a workgroup's legs (VitSplitArgs::legs); nothing in the library
#define PD_LEG(i, v) do { if (g.legs && threadIdx.x == 0) g.legs[(size_t)blockIdx.x * 8 + (i)] = (long long)(v); } while (0)
#define PD_LEG_T0() leg_t0 = __builtin_amdgcn_s_memtime()
#define PD_LEG_ACC(v) v += __builtin_amdgcn_s_memtime() - leg_t0
#else
#define PD_LEG(i, v) do { } while (0)
#define PD_LEG_T0() do { } while (0)
#define PD_LEG_ACC(v) do { } while (0)
#endif

// ---- the pieces of the product that pd_qkv_attn_kernel shares ------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned pd_wv4 __attribute__((ext_vector_type(4)));       // a weight fragment as a native vector (an inline-asm register operand)
__device__ __forceinline__ int pd_strip_swz(int r) { return ((r >> 1) & 1) | ((r >> 1) & 4); }
// weights of 32-k block b at wq: 4 fragments {column tile 0 | 1} x {hi | lo} over the block's 32 k (the lo plane 1 KiB, the second column tile 16 lanes
// further) -- hand-issued like the DMA, so that every vector-memory operation of the loop is counted by the s_waitcnt below and by nothing else (the
// compiler's own waits assume it sees every load in flight)
#define PD_STRIP_WLOAD(wq, w0, w1, w2, w3, b)                                                                                        \
    do {                                                                                                                             \
        const uint4 *wp_ = (wq) + (size_t)(b) * 256;                                                                                 \
        asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %4, off offset:1024\n\t"                           \
                     "global_load_dwordx4 %2, %4, off offset:256\n\tglobal_load_dwordx4 %3, %4, off offset:1280"                     \
                     : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3) : "v"(wp_) : "memory");                                            \
    } while (0)
// the waits are tied to the registers they release: no use of a fragment moves above the wait that collects it
#define PD_STRIP_WAIT(n, w0, w1, w2, w3) asm volatile("s_waitcnt vmcnt(" #n ")" : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3) : : "memory")
#define PD_STRIP_WAITN(n, w0, w1, w2, w3) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3) : "n"(n) : "memory")
// two raw 16-byte words of a row (8 split words {hi | lo << 16} = 8 consecutive k) -> the hi and the lo fragment
template <class V>
__device__ __forceinline__ uint4 pd_unzip_hi(V p, V q) {
    return make_uint4(__builtin_amdgcn_perm(p.y, p.x, 0x05040100u), __builtin_amdgcn_perm(p.w, p.z, 0x05040100u),
                      __builtin_amdgcn_perm(q.y, q.x, 0x05040100u), __builtin_amdgcn_perm(q.w, q.z, 0x05040100u));
}
template <class V>
__device__ __forceinline__ uint4 pd_unzip_lo(V p, V q) {
    return make_uint4(__builtin_amdgcn_perm(p.y, p.x, 0x07060302u), __builtin_amdgcn_perm(p.w, p.z, 0x07060302u),
                      __builtin_amdgcn_perm(q.y, q.x, 0x07060302u), __builtin_amdgcn_perm(q.w, q.z, 0x07060302u));
}
__device__ __forceinline__ f32x4 pd_mma16(const uint4 &a, const pd_wv4 &b, const f32x4 &c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------
// dynamic LDS of a launch: two buffers of two 32-k blocks of 32 RT rows -- and no less than the epilogue's four per-wave patches
static constexpr size_t PD_STRIP_PATCH_BYTES = (size_t)4 * 32 * 36 * sizeof(float);
template <int RT>
static constexpr size_t pd_gemm_strip_lds() { return (size_t)16384 * RT; }
// EPI 0: C = A W^T * c_scale + bias (fp32); 2: C += that; 3 / 4: split words of gelu / relu (that) * out_scale.  RT 32-row tiles per workgroup.
template <int EPI, int RT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((RT == 3 ? 3 : 4) - (EPI == 2 ? 1 : 0))))
void pd_gemm_strip_kernel(VitSplitArgs g) {
    static_assert(EPI == 0 || EPI == 2 || EPI == 3 || EPI == 4, "the epilogues the library launches");
    static_assert(RT == 2 || RT == 3, "64- and 96-row tiles: pieces of 8 rows, RT per wave and 32-k block");
    constexpr int KC = 32, TM = 32 * RT, TN = 128, GROUP = RT == 3 ? 24 : 2048 / TM, CHA = TM * KC;     // words of A per 32-k block; GROUP row tiles (a multiple of
                                                                                                       //   8: a row block's column tiles share an XCD) per block group
    extern __shared__ __attribute__((aligned(1024))) unsigned strip_lds[];
    PD_LEG(0, wall_clock64());
    PD_LEG(2, __builtin_amdgcn_s_memtime());
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, kg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int MT = (g.M + TM - 1) / TM, NT = g.Nout / TN;
    int mtile, ntile;
    {
        const int b = blockIdx.x, full = (MT / GROUP) * GROUP * NT;
        if (b < full) {
            const int grp = b / (NT * GROUP), r = b - grp * (NT * GROUP);
            ntile = r / GROUP;
            mtile = grp * GROUP + r % GROUP;
        } else {
            const int r = b - full, rest = MT % GROUP;
            ntile = r / rest;
            mtile = (MT / GROUP) * GROUP + r % rest;
        }
    }
    const int m0 = mtile * TM, n0 = ntile * TN;
    // staging: pieces of 1 KiB = 8 rows x 32 words; a 32-k block has 4 RT of them, wave w moves pieces [RT w, RT (w + 1))
    const int prow = lane >> 3, pslot = lane & 7;
    unsigned oa[RT];
#pragma unroll
    for (int j = 0; j < RT; ++j) {
        const int r = 8 * (RT * wave + j) + prow;
        oa[j] = (unsigned)(((size_t)min(m0 + r, g.M - 1) * g.lda + 4 * (pslot ^ pd_strip_swz(r))) * sizeof(unsigned));
    }
    const unsigned lds_a = (unsigned)(size_t)(strip_lds + RT * wave * 256);
    const int KS = g.K / 16;
    const uint4 *wq = (const uint4 *)g.W + (size_t)(n0 / 32 + wave) * KS * 128 + ((kg >> 1) * 128 + (kg & 1) * 32 + l15);   // this wave's 32-column tile;
                                                                    //   the lane's (column % 16, k group) of a 32-k block in the planes' 32-column x 16-k order
    f32x4 acc4[2 * RT][2];                             // [16-row tile][16-column tile]
    pd_wv4 resid[EPI == 2 ? RT : 1][4];                // the residual tile of an EPI 2 product (resid_load, below)
#pragma unroll
    for (int t = 0; t < 2 * RT; ++t) acc4[t][0] = acc4[t][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    auto stage64 = [&](int c, int buf) {            // both 32-k blocks of chunk c: 2 RT pieces per wave
        const unsigned da = __builtin_amdgcn_readfirstlane(lds_a + buf * 2 * CHA * 4);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float *ab = (const float *)(g.A + (2 * c + h) * KC);
#pragma unroll
            for (int j = 0; j < RT; ++j) pd_dma_piece(ab, oa[j], da + h * CHA * 4 + j * 1024);
        }
    };
    // The steps of the K loop are scheduled by hand.  A wave issues in order and an MFMA holds its issue port for the matrix pipe's cycles unless something else is
    // there to issue: the compiler's schedule -- a step's un-zips and fragment reads in clumps, its MFMAs back to back -- ran the MFMAs and the other instructions
    // of a chunk in their SUM (tools/strip_legs_probe.hip: waits + barrier are 5 % of the loop, yet the matrix pipe was 41 - 55 % busy; neither later operands, nor
    // hidden LDS latency, nor moved DMA issue changed that).  Here every pair of MFMAs is preceded by the few instructions that fit its shadow: the four un-zips of its
    // own A fragment, or (second product) four un-zips + the NEXT step's two fragment reads of that row tile, or (third product) one LDS-DMA piece of the next
    // chunk; sched_barrier(0) pins the order.  Raw fragments double-buffered in registers, read one step ahead and waited for (lgkmcnt(0)) a step later.
    pd_wv4 raw[2][RT][2];
    const int swz = pd_strip_swz(l15);
    auto read_mi = [&](int rb, const unsigned *a, int st, int mi) {           // st = the 16-row half of 32-row tile mi, all 32 k of the block
        const unsigned p_ = (unsigned)(size_t)(a + (mi * 32 + st * 16) * KC + 4 * ((2 * kg) ^ swz));
        const unsigned q_ = (unsigned)(size_t)(a + (mi * 32 + st * 16) * KC + 4 * ((2 * kg + 1) ^ swz));
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(raw[rb][mi][0]), "=&v"(raw[rb][mi][1]) : "v"(p_), "v"(q_) : "memory");
    };
    auto wait_reads = [&](int rb) {
#pragma unroll
        for (int mi = 0; mi < RT; ++mi) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(raw[rb][mi][0]), "+v"(raw[rb][mi][1]) : : "memory");
    };
    // piece p (0 .. 2 RT - 1) of chunk dma_cn's rows -> buffer dma_nb (in the loop's vector-memory issue ORDER all 2 RT pieces come before the first block's
    // weight loads: the hand-counted vmcnt waits rest on it)
    int dma_cn = 0, dma_nb = 0;
    auto dma_piece_at = [&](int p) {
        const unsigned da = __builtin_amdgcn_readfirstlane(lds_a + dma_nb * 2 * CHA * 4);
        const int h = p / RT, j = p % RT;
        pd_dma_piece((const float *)(g.A + (2 * dma_cn + h) * KC), oa[j], da + h * CHA * 4 + j * 1024);
    };
    // a step is one 16-row half (h) of every 32-row tile over the block's 32 k, against both column tiles (w0 / w1 = tile 0 {hi | lo}, w2 / w3 = tile 1): per output
    // element lo x hi, hi x lo, hi x hi, in this order; two MFMAs of 16 cycles behind each group's un-zips / reads / DMA piece
    auto step16 = [&](int rb, int h, const pd_wv4 &w0, const pd_wv4 &w1, const pd_wv4 &w2, const pd_wv4 &w3, bool has_next, int nrb, const unsigned *na, int nst,
                      int dma_step) {
        uint4 ah[RT], al[RT];
#pragma unroll
        for (int mi = 0; mi < RT; ++mi) {
            const int t = 2 * mi + h;
            al[mi] = pd_unzip_lo(raw[rb][mi][0], raw[rb][mi][1]);
            __builtin_amdgcn_sched_barrier(0);
            acc4[t][0] = pd_mma16(al[mi], w0, acc4[t][0]);
            acc4[t][1] = pd_mma16(al[mi], w2, acc4[t][1]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mi = 0; mi < RT; ++mi) {
            const int t = 2 * mi + h;
            ah[mi] = pd_unzip_hi(raw[rb][mi][0], raw[rb][mi][1]);
            if (has_next) read_mi(nrb, na, nst, mi);
            __builtin_amdgcn_sched_barrier(0);
            acc4[t][0] = pd_mma16(ah[mi], w1, acc4[t][0]);
            acc4[t][1] = pd_mma16(ah[mi], w3, acc4[t][1]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mi = 0; mi < RT; ++mi) {
            const int t = 2 * mi + h;
            if (dma_step >= 0) dma_piece_at(dma_step * RT + mi);
            __builtin_amdgcn_sched_barrier(0);
            acc4[t][0] = pd_mma16(ah[mi], w0, acc4[t][0]);
            acc4[t][1] = pd_mma16(ah[mi], w2, acc4[t][1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    pd_wv4 a0, a1, a2, a3, b0, b1, b2, b3;               // weight fragments of the chunk's first / second 32-k block
    const int nk64 = g.K / 64;
    // The residual tile (EPI 2: C += ...) is requested at the end of the chunk BEFORE the last, in the epilogue's own 16-byte pattern (in-place C: inside the
    // epilogue the compiler cannot lift a row tile's loads over the previous tile's stores, so every row tile exposed a whole global-load latency).  Hand-issued,
    // counted by the loop's waits (`chunk`, below), 4 RT registers of 16 bytes.
    auto resid_load = [&]() {
        const int pr_ = lane >> 3, colb_ = n0 + wave * 32 + (lane & 7) * 4;
#pragma unroll
        for (int mi = 0; mi < RT; ++mi)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float *rp_ = (const float *)g.C + (size_t)min(m0 + mi * 32 + 8 * q + pr_, g.M - 1) * g.Nout + colb_;
                asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(resid[mi][q]) : "v"(rp_) : "memory");
            }
    };
    // the wait that collects the residual tile, tied to its registers like the weight fragments' waits to theirs: no use of them moves above it
    auto resid_wait = [&]() {
#pragma unroll
        for (int mi = 0; mi < ((EPI == 2) ? RT : 1); ++mi)
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(resid[mi][0]), "+v"(resid[mi][1]), "+v"(resid[mi][2]), "+v"(resid[mi][3]) : : "memory");
    };
    stage64(0, 0);
    PD_STRIP_WLOAD(wq, a0, a1, a2, a3, 0);
    PD_STRIP_WLOAD(wq, b0, b1, b2, b3, 1);
    PD_STRIP_WAIT(0, a0, a1, a2, a3);
    PD_STRIP_WAIT(0, b0, b1, b2, b3);
    __syncthreads();
    PD_LEG(3, __builtin_amdgcn_s_memtime());
#ifdef PD_STRIP_LEGS
    long long leg_t0 = 0, leg_wb = 0, leg_wa = 0, leg_bar = 0, leg_s0 = 0, leg_s1 = 0, leg_s2 = 0, leg_s3 = 0;
#endif
    // One 64-k chunk.  MODE 0: a chunk with a successor -- the successor's rows and weights are requested while this one is multiplied.  MODE 1: the one before the
    // last -- as 0, and (EPI 2) the residual tile is requested behind everything else, so that a whole chunk of matrix work hides it: returns are in order, the
    // end-of-chunk wait lets it fly (+ RESN) and so does the last chunk's first wait; the last chunk's end collects it.  MODE 2: the last chunk requests nothing
    // and leaves the closing barrier to the epilogue.
    constexpr int RESN = EPI == 2 ? 4 * RT : 0;
    auto chunk = [&](int c, auto mode_) {
        constexpr int MODE = decltype(mode_)::value;
        const int cn = c + 1;
        const unsigned *a = strip_lds + (c & 1) * 2 * CHA + l15 * KC;
        dma_cn = cn;                                         // in flight, oldest first: the second block's weights [4, from the previous turn], this DMA [2 RT]
        dma_nb = (c + 1) & 1;                                //   (its pieces are issued inside the first block's MFMA groups, below)
#pragma unroll
        for (int mi = 0; mi < RT; ++mi) read_mi(0, a, 0, mi);                // (the one exposed read per chunk: its rows were published by the barrier just passed)
        wait_reads(0);
        PD_LEG_T0();
        step16(0, 0, a0, a1, a2, a3, true, 1, a, 1, MODE == 2 ? -1 : 0);
        PD_LEG_ACC(leg_s0);
        wait_reads(1);
        PD_LEG_T0();
        step16(1, 1, a0, a1, a2, a3, true, 0, a + CHA, 0, MODE == 2 ? -1 : 1);
        PD_LEG_ACC(leg_s1);
        if constexpr (MODE != 2) PD_STRIP_WLOAD(wq, a0, a1, a2, a3, 2 * cn);     //   ... + the next chunk's first block [4]
        // the second block's weights must have landed; the DMA and the loads just issued may still be in flight (in-order returns)
        PD_LEG_T0();
        PD_STRIP_WAITN((MODE == 2 ? RESN : 2 * RT + 4), b0, b1, b2, b3);     // (2 RT DMA pieces + 4 weight loads may stay in flight; last chunk: the residual tile)
        PD_LEG_ACC(leg_wb);
        wait_reads(0);
        PD_LEG_T0();
        step16(0, 0, b0, b1, b2, b3, true, 1, a + CHA, 1, -1);
        PD_LEG_ACC(leg_s2);
        wait_reads(1);
        PD_LEG_T0();
        step16(1, 1, b0, b1, b2, b3, false, 0, a, 0, -1);
        PD_LEG_ACC(leg_s3);
        if constexpr (MODE != 2) {
            PD_STRIP_WLOAD(wq, b0, b1, b2, b3, 2 * cn + 1);      //   ... + the next chunk's second block [4]
            if constexpr (MODE == 1 && RESN > 0) resid_load();
            PD_LEG_T0();
            PD_STRIP_WAITN((MODE == 1 ? 4 + RESN : 4), a0, a1, a2, a3);      // the next chunk's rows and first block have landed; the second block (and the residual tile) may still fly
            PD_LEG_ACC(leg_wa);
            PD_LEG_T0();
            __syncthreads();
            PD_LEG_ACC(leg_bar);
        }
    };
    if constexpr (RESN > 0) {
        if (nk64 < 2) {                                      // (a single chunk: nothing to hide behind)
            resid_load();
            resid_wait();
        }
    }
    for (int c = 0; c < nk64 - 2; ++c) chunk(c, std::integral_constant<int, 0>());
    if (nk64 >= 2) chunk(nk64 - 2, std::integral_constant<int, 1>());
    chunk(nk64 - 1, std::integral_constant<int, 2>());
    PD_STRIP_WAIT(0, b0, b1, b2, b3);
    if constexpr (EPI == 2) resid_wait();
    PD_LEG(4, __builtin_amdgcn_s_memtime());
#ifdef PD_STRIP_LEGS
    PD_LEG(6, (leg_wb << 32) | (leg_wa & 0xffffffffll));
    PD_LEG(7, leg_bar);
#ifdef PD_STRIP_STEP_CLOCKS
    PD_LEG(0, (leg_s0 << 32) | (leg_s1 & 0xffffffffll));       // (overwrites the wall-clock stamps: the step-timing build of the probe does not print the timeline)
    PD_LEG(1, (leg_s2 << 32) | (leg_s3 & 0xffffffffll));
#endif
#endif
    // Epilogue with 16-byte accesses.  Every wave turns its 32 x 32 accumulator tile through a private 32 x 36 float patch of the (now idle) staging LDS: written
    // column-per-lane as the MFMA leaves it, read back as four consecutive columns of one row per lane, so that residual loads and stores are dwordx4 (four per row
    // tile; the 4-byte form -- sixteen, each covering two 128-byte row segments -- was 27 - 33 % of a workgroup's time, store-issue bound).
    static_assert(PD_STRIP_PATCH_BYTES <= pd_gemm_strip_lds<RT>(), "the four waves' patches live in the launch's dynamic LDS");
    __syncthreads();                               // every wave is past its last fragment read (the last chunk ends without a barrier): the staging buffers are free
    float *patch = (float *)strip_lds + wave * (32 * 36);
    const int pr = lane >> 3, pc = (lane & 7) * 4;
    // (One trip: the wave's one 32-column tile.  The loop is what is left of the two-tiles-per-wave form and stays for the machine code alone: the compiler expands
    //  colb from its induction variable after it has merged common subexpressions, so colb stays apart from resid_load's column.  As a plain expression the two
    //  merge and the register allocation of every instance moves; tools/kernel_isa_ab.py shows it.  Whoever changes the kernel's code anyway may drop it.)
#pragma unroll
    for (int c = 0; c < 1; ++c) {
        const int colb = n0 + (wave + c) * 32 + pc;
        const float4 bias4 = *(const float4 *)(g.bias + colb);
#pragma unroll
        for (int mi = 0; mi < RT; ++mi) {
            // 16x16 tiles: lane = column % 16 + 16 (row / 4), register = row % 4
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int i = 0; i < 4; ++i) patch[(16 * h + 4 * kg + i) * 36 + 16 * ct + l15] = acc4[2 * mi + h][ct][i];
            float4 res4[4];
            if constexpr (EPI == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) res4[q] = __builtin_bit_cast(float4, resid[mi][q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = m0 + mi * 32 + 8 * q + pr;
                const float4 a4 = *(const float4 *)(patch + (8 * q + pr) * 36 + pc);
                float v[4] = {a4.x, a4.y, a4.z, a4.w};
                const float b4[4] = {bias4.x, bias4.y, bias4.z, bias4.w};
                const float r4[4] = {EPI == 2 ? res4[q].x : 0.0f, EPI == 2 ? res4[q].y : 0.0f, EPI == 2 ? res4[q].z : 0.0f, EPI == 2 ? res4[q].w : 0.0f};
                unsigned o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = fmaf(v[e], g.c_scale, b4[e]);
                    if constexpr (EPI == 3) t = 0.5f * t * (1.0f + erff(t * 0.70710678118654752f));   // nn.GELU()'s exact form
                    if constexpr (EPI == 4) t = pd_relu(t);
                    if constexpr (EPI == 2) t += r4[e];
                    if constexpr (EPI == 3 || EPI == 4) o[e] = pd_split_word_as<2>(t, g.out_scale);
                    else o[e] = __float_as_uint(t);
                }
                if (row < g.M) *(uint4 *)((unsigned *)g.C + (size_t)row * g.Nout + colb) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
    }
#ifdef PD_STRIP_LEGS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the stores have left
    PD_LEG(5, __builtin_amdgcn_s_memtime());
#ifndef PD_STRIP_STEP_CLOCKS
    PD_LEG(1, wall_clock64());
#endif
#endif
}
template <int EPI, int RT>
static inline void pd_gemm_strip(const unsigned *A, int lda, const unsigned *W, int K, const float *bias, void *C, int M, int Nout, hipStream_t s,
                                 float c_scale = 1.0f, float out_scale = 1.0f) {
    VitSplitArgs g{A, W, bias, C, M, Nout, K, lda, c_scale, out_scale};
    constexpr int TM = 32 * RT;
    hipLaunchKernelGGL((pd_gemm_strip_kernel<EPI, RT>), dim3(((M + TM - 1) / TM) * (Nout / 128)), dim3(256), (pd_gemm_strip_lds<RT>()), s, g);
}
