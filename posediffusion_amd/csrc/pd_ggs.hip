// pd_ggs.hip -- Geometry-Guided Sampling as ONE persistent kernel per guided diffusion step.
//
// Replaces (paths relative to /root/reference/pose_diffusion/):
//   util/geometry_guided_sampling.py:14-64   geometry_guided_sampling  (5 optimisations)
//   util/geometry_guided_sampling.py:67-126  GGS_optimize  (clipped momentum SGD, early exit)
//   util/geometry_guided_sampling.py:129-172 compute_sampson_distance
//   util/get_fundamental_matrix.py:14-51     F for the frame pairs that own matches
//   util/camera_transform.py:80-97           pose decode (quat -> R, clamp(exp(logFL + 1.8)))
// plus torch autograd's backward of all of the above, derived by hand (DESIGN.md "GGS backward";
// the same derivation in fp64 numpy is oracle/pd_oracle.py:sampson_loss_grad_analytic).
//
// Mapping to CDNA4.  The reference launches ~1850 ATen kernels per iteration and 700 iterations
// per guided step; the chain is strictly sequential, so the design goal is launch-free, sync-cheap
// iterations:
//   * one launch runs every iteration of every stage; pose parameters, momentum and all per-frame
//     state live in registers/LDS of the owning workgroup(s);
//   * matches are pair-sorted at upload; a wavefront owns one (pair, <=512 matches) work item, the
//     pair's F is wave-uniform, the per-match Sampson residual + dL/dF is accumulated per lane and
//     reduced with a 64-lane butterfly (fixed order -> bitwise reproducible);
//   * k workgroups may cooperate on one sequence (k = ceil(items / 8) when CUs are free): each
//     publishes its 12 per-item sums as tagged 8-byte granules (write-through, data-is-the-flag,
//     guide section 6 G16 R2) and every workgroup gathers all of them, then redundantly runs the
//     tiny per-frame backward + SGD update, so there is exactly ONE cross-workgroup hop per
//     iteration and no broadcast of the new parameters.  All arithmetic orders are fixed, so the
//     replicas stay bitwise identical (and k = 1 and k > 1 give identical bits).
//   * blockIdx -> (sequence, workgroup) is XCD-aware: with B % 8 == 0 all workgroups of a sequence
//     sit on one XCD (dispatcher places block b on XCD b % 8) so the exchange stays in one L2.
//     That is a speed choice only; correctness uses agent-scope granules and bounded spins.
//
// This file: the one translation unit of the three GGS kernels -- its compiler flags (Makefile), the contraction pragma and the development
// switches below govern all of their code -- and the host code bound to them: pd_ggs_init, pd_ggs_plan, pd_ggs_launch.  The device code
// itself is in the headers included below: pd_ggs_lds.h (the LDS images and their sizes), pd_ggs_dev.h (cross-lane sums, pair geometry, pose
// decode), pd_ggs_sampson.h (the match pass), pd_ggs_kernels.h (pd_ggs_kernel, pd_ggs2_kernel), pd_ggs_lane.inc (pd_ggs_lane_kernel), and the
// statement fragments those include (pd_ggs_pairbwd.inc, pd_ggs_p3b.inc, pd_ggs_p4.inc, pd_ggs_p4_long.inc, pd_ggs_long_hop2.inc, pd_ggs_p4q.inc).  The match tables the kernels read are
// built elsewhere: on the host by pd_ggs_tables.hip (pd_ggs_set_matches), on the device by pd_ggs_ingest.hip; the stream events that order
// uploads against launches belong to pd_engine.hip.
#include "pd_internal.h"

#include <algorithm>
#include <math.h>
#include <stdlib.h>
#include <string.h>

// Floating-point contraction is decided per source expression in this file (not by the backend across statements, as
// -ffp-contract=fast allows): the GGS kernel exists in several template variants (resident / LDS-staged / register-streamed
// match pass, two-hop) whose results must agree BIT FOR BIT for the same sequence whatever the launch shape -- a backend
// that fuses a*b+c differently in two instantiations of the same source line would break that.
#pragma clang fp contract(on)

#ifndef PD_GGS_PROF12
#define PD_GGS_PROF12 0
#endif
#ifndef PD_GGS_ABLATE
#define PD_GGS_ABLATE 0   // development (tools/ab_ggs.py): bit mask of phases whose work is SKIPPED (1 P1, 2 P3a, 4 P3b, 8 P4, 16 match pass, 32 exchange
#endif                    // gather) -- garbage results, honest timing of what is left: the difference is a phase's share of the critical path

#ifndef PD_GGS_MIN_WAVES_PER_SIMD
#define PD_GGS_MIN_WAVES_PER_SIMD 2      // one 512-thread workgroup per CU; 4 = experiment: two workgroups per CU (<= 128 VGPRs)
#endif
// (-DPD_GGS_PROF2, no value: the timers INSIDE pd_ggs_kernel's match pass; the lane kernel's switches, PD_LANE_*, are in pd_ggs_lane.inc)

// device code (kept in this one translation unit: the switches above and the contraction pragma apply to all of it)
#include "pd_ggs_lds.h"        // the two LDS images: struct Lds, carve / carve_lane and the byte counts derived from them
#include "pd_ggs_dev.h"        // cross-lane sums, pair geometry, pose decode, quaternion Jacobian
#include "pd_ggs_sampson.h"    // the match pass: Sampson steps, item passes, LDS-DMA staging
#include "pd_ggs_kernels.h"    // pd_ggs_kernel, pd_ggs2_kernel, pd_ggs_long_kernel, pd_ggs_longm_kernel, pd_ggs_zero_kernel
#include "pd_ggs_lane.inc"     // pd_ggs_lane_kernel

// --------------------------------------------------------------------------------------------
// host side: init, launch plan, launch
// --------------------------------------------------------------------------------------------
// The one list of pd_ggs_kernel's instantiations: (pieces of LDS staging, matches resident in registers, waves per workgroup) -> kernel,
// nullptr where no such variant is built.  pd_ggs_launch picks from it and pd_ggs_init raises the dynamic-LDS limit of everything in it.
typedef void (*PdGgsKernel)(PdGgsParams, int, int, int, int);
static PdGgsKernel ggs_variant(int stage_p, bool resident, int waves) {
    if (resident) return stage_p == 0 && waves == PD_GGS_WAVES ? pd_ggs_kernel<0, true> : nullptr;
    if (waves == PD_GGS_WAVES) {
        switch (stage_p) {
        case 0: return pd_ggs_kernel<0, false>;
        case 3: return pd_ggs_kernel<3, false>;
        case 5: return pd_ggs_kernel<5, false>;
        case 6: return pd_ggs_kernel<6, false>;
        }
    } else if (waves == 12) {
        switch (stage_p) {
        case 3: return pd_ggs_kernel<3, false, 12>;
        case 5: return pd_ggs_kernel<5, false, 12>;
        case 6: return pd_ggs_kernel<6, false, 12>;
        }
    }
    return nullptr;
}

int pd_ggs_init() {
    for (bool resident : {true, false})
        for (int waves : {PD_GGS_WAVES, 12})
            for (int stage_p : {0, 3, 5, 6})
                if (PdGgsKernel f = ggs_variant(stage_p, resident, waves))
                    PD_HIP_CHECK(hipFuncSetAttribute((const void *)f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    PD_HIP_CHECK(hipFuncSetAttribute((const void *)pd_ggs2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    PD_HIP_CHECK(hipFuncSetAttribute((const void *)pd_ggs_long_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    PD_HIP_CHECK(hipFuncSetAttribute((const void *)pd_ggs_longm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    PD_HIP_CHECK(hipFuncSetAttribute((const void *)pd_ggs_lane_kernel<PD_LANE_RV>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (!lane_pinc_aligned()) {
        pd_set_error("pd_ggs: the lane kernel's LDS image puts its float4 rows off a 16-byte boundary");
        return PD_ERR_STATE;
    }
    return PD_OK;
}

// pd_ggs_plan, part 1: the arguments, and that every slot of the launch holds tables for N frames; returns the most work items of a slot
static int plan_check_slots(pd_engine *eng, int B, int N, const pd_ggs_cfg *cfg, PdGgsPlan *out, int &max_items) {
    PD_TRY(pd_ggs_frames_unsupported(eng, N, "pd_ggs"));       // more frames than the engine's GGS limit (64, or PD_OPT_GGS_MAX_FRAMES; the denoiser's is 256): a clean refusal
    if (!eng || !cfg || !out || B <= 0 || B > eng->max_B || N <= 0 || N > eng->max_N || N > eng->ggs_max_frames) {
        pd_set_error("pd_ggs: invalid arguments (B=%d N=%d)", B, N);
        return PD_ERR_INVALID_ARG;
    }
    // frame counts per sequence (pd_engine_set_frame_counts): slot b must hold tables for ITS count -- the kernels take the frame count of a
    // sequence from its descriptor and only the row stride of x from N
    const int *nf_dev = nullptr;
    PD_TRY(pd_frame_counts(eng, B, N, "pd_ggs", &nf_dev));
    max_items = 0;
    for (int b = 0; b < B; ++b) {
        const PdSeqDesc &d = eng->seqs[b].desc;
        if (d.M <= 0 || !eng->seqs[b].blob) {
            pd_set_error("pd_ggs: sequence slot %d has no matches (call pd_ggs_set_matches)", b);
            return PD_ERR_STATE;
        }
        const int n_b = nf_dev ? eng->nf_host[b] : N;
        if (d.n_frames != n_b) {
            if (nf_dev) pd_set_error("pd_ggs: slot %d matches were uploaded for %d frames, its frame count (pd_engine_set_frame_counts) is %d", b, d.n_frames, n_b);
            else pd_set_error("pd_ggs: slot %d matches were uploaded for %d frames, called with N=%d", b, d.n_frames, N);
            return PD_ERR_INVALID_ARG;
        }
        max_items = std::max(max_items, d.n_items);
    }
    return PD_OK;
}

// pd_ggs_plan, part 2: does the lane-per-item kernel take the launch?  (true: *out is its plan.)  It does on request (PD_GGS_CFG_LANE_ITEMS:
// what the pipeline sets wherever it gives a sequence ONE workgroup), or when the engine picks the shape and the launch holds more sequences
// than half the CUs (nothing to gain from several workgroups per sequence).
// An explicit wgs_per_seq without the flag keeps the wave-per-item kernels, whose results are bitwise independent of the workgroup
// count (the lane kernel sums in another fixed order: rounding-level differences).  Round 4: its stream goes through an
// LDS ring fed by LDS-DMA that never stops (pd_ggs_lane.inc) and it is 10 - 14 % faster than the 12-wave wave-per-item kernel at
// the bench shape (18.6 against 21.6 ms per 256-sequence launch, profiles/round4_lane_ring.txt); fully resident sequences 1.5 - 2 x.
static bool plan_lane(const pd_engine *eng, int B, int N, const pd_ggs_cfg *cfg, int device_cus, PdGgsPlan *out) {
    if ((cfg->reserved & PD_GGS_CFG_NO_LANE_ITEMS) ||
        !((cfg->reserved & PD_GGS_CFG_LANE_ITEMS) || (cfg->wgs_per_seq == 0 && device_cus / B <= 1)))
        return false;
    bool ok = N <= PD_GGS_FAST_FRAMES;
    int pairs = 0, steps = 0, deg = 0;
    for (int b = 0; b < B && ok; ++b) {
        const PdSeqDesc &d = eng->seqs[b].desc;
        ok = d.n_litems > 0 && d.n_pchunks == 1;
        pairs = std::max(pairs, d.n_pairs);
        steps = std::max(steps, d.l_max_steps);
        deg = std::max(deg, eng->seqs[b].max_deg);
    }
    if (!ok) return false;
    // rows of the pair backward at the fixed per-frame stride of the fast serial phases (pd_ggs_p3b.inc)
    const int pinc_rows = std::max(2 * std::min(PD_LANE_MAX_ITEMS, std::max(pairs, 1)), N * (((deg + 3) & ~3) + 1));
    const size_t lds = lane_lds_bytes(pinc_rows, PD_LANE_SLOTS);        // tables + the waves' rings (PD_LANE_RING steps of 2 KiB each)
    if (lds > 160 * 1024) return false;
    out->lane = 1;
    out->lane_rl = std::max(0, std::min(PD_LANE_RL, steps - PD_LANE_RV));     // (reported: steps of the longest wave that live in LDS for the launch, beside the ring)
    out->k = 1;
    out->waves = PD_LANE_WAVES;
    out->pinc_rows = pinc_rows;
    out->lds = (int)lds;
    out->max_items = PD_LANE_MAX_ITEMS;
    return true;
}

// pd_ggs_plan, part 3: the wave-per-item kernels -- one-hop or two-hop, workgroups per sequence (from the wanted k), item slots, the LDS
// image and the XCD-local placement of the exchange
static int plan_wave_items(const pd_engine *eng, int B, int N, const pd_ggs_cfg *cfg, int device_cus, int k, int max_items, PdGgsPlan *out) {
    // k > 1: every workgroup publishes one exchange line per work item in the sequence's [epoch][item] region of d_xchg
    // (pd_ggs_kernel, `xchg + epoch * xchg_stride + item * PD_XCHG_LINE`): a sequence with more items than the region holds
    // (2 max_N^2 + 512 lines, pd_engine_create) would write into the other epoch's lines or the next slot's -- one workgroup
    // per sequence then (no exchange at all).  The two-hop kernel checks its own, smaller line count below.
    if (k > 1 && (size_t)max_items * PD_XCHG_LINE > eng->xchg_granules) k = 1;
    // many frames (several chunks of pairs): the two-hop kernel distributes the backward over the workgroups instead of
    // replicating it -- needs one work item per pair and room for its exchange lines; it keeps only a workgroup's own
    // item sums in LDS, so it also covers item counts whose full table would not fit
    bool two_hop = k > 1 && !(cfg->reserved & PD_GGS_CFG_FORCE_ONE_HOP);
    for (int b = 0; b < B && two_hop; ++b) {
        const PdSeqDesc &d = eng->seqs[b].desc;
        two_hop = d.n_pchunks > 1 && d.single_item_pairs;
    }
    // one-hop kernel: backward rows of one chunk of pairs (both sides); LDS staging of the match pass when every item fits a
    // staging buffer (<= 384 matches) -- both only shrink / extend the LDS image, the arithmetic is the same
    int max_pairs = 0, max_len = 0;
    for (int b = 0; b < B; ++b) {
        max_pairs = std::max(max_pairs, eng->seqs[b].desc.n_pairs);
        max_len = std::max(max_len, eng->seqs[b].max_item_len);
    }
    int pinc_one_hop = std::min(PD_GGS_PINC_ROWS, 2 * std::min(PD_GGS_THREADS, std::max(max_pairs, 1)));
    // fast serial phases (<= PD_GGS_FAST_FRAMES frames, one chunk of pairs): rows at a fixed stride per frame -- N x (largest degree,
    // rounded up to 4, + 1) rows; about 2 x pairs for the complete graph of hloc's exhaustive pairs.  The kernel decides from the actual
    // tables; here only the room is made (dropped again below if the LDS image would not fit).
    int pinc_fast = 0;
    if (N <= PD_GGS_FAST_FRAMES) {
        int deg = 0;
        bool one_chunk = true;
        for (int b = 0; b < B; ++b) {
            deg = std::max(deg, eng->seqs[b].max_deg);
            one_chunk = one_chunk && eng->seqs[b].desc.n_pchunks <= 1;
        }
        if (one_chunk && deg > 0) pinc_fast = N * (((deg + 3) & ~3) + 1);     // (+ 1: the bank-conflict-free row stride, pd_ggs_kernel)
    }
    const int pinc_general = pinc_one_hop;
    if (pinc_fast <= PD_GGS_PINC_ROWS) pinc_one_hop = std::max(pinc_one_hop, pinc_fast);
    int stage_want = 0;
    if (!(cfg->reserved & PD_GGS_CFG_NO_LDS_STAGING) && max_len > 0) {
        const int pieces = (max_len + 63) / 64;
        stage_want = pieces <= 3 ? 3 : pieces <= 5 ? 5 : pieces <= 6 ? 6 : 0;
    }
    int n_slots = 0, pinc_rows = PD_GGS_PINC_ROWS, stage_p = 0;
    size_t lds = 0;
    // LDS image of a candidate shape; three waves per SIMD (12 waves, ONE staging buffer per wave) for the staged match pass at one
    // workgroup per sequence with several rounds of items per wave (the bench shape; A/B switch PD_GGS_CFG_WAVES8 keeps 8 waves)
    int waves = PD_GGS_WAVES;
    auto image = [&](int rows, int sp, int kk_, int slots, int &w_out) -> size_t {
        w_out = PD_GGS_WAVES;
        const size_t l8 = ggs_lds_bytes(slots, two_hop ? slots : max_items, rows, sp, PD_GGS_WAVES * 2);
        if (!two_hop && sp > 0 && kk_ == 1 && slots >= 3 * 12 && !(cfg->reserved & PD_GGS_CFG_WAVES8) && (PD_GGS_PROF12 || !eng->ggs_prof_on)) {
            const size_t l12 = ggs_lds_bytes(slots, max_items, rows, sp, 12);
            if (l12 <= 160 * 1024) {
                w_out = 12;
                return l12;
            }
        }
        return l8;
    };
    for (int pass = 0; pass < 2; ++pass) {
        int kk = k;
        for (;;) {
            const int rounds = (max_items + kk * PD_GGS_WAVES - 1) / (kk * PD_GGS_WAVES);
            n_slots = rounds * PD_GGS_WAVES;
            pinc_rows = two_hop ? PD_GGS_PINC_ROWS : pinc_one_hop;
            stage_p = (!two_hop && rounds > 1) ? stage_want : 0;     // one item per wave: matches are register resident
            lds = image(pinc_rows, stage_p, kk, n_slots, waves);
            if (lds > 160 * 1024 && !two_hop && pinc_rows > pinc_general) {   // the wider rows of the fast serial phases are optional
                pinc_one_hop = pinc_rows = pinc_general;
                lds = image(pinc_rows, stage_p, kk, n_slots, waves);
            }
            if (lds > 160 * 1024 && stage_p > 0) {                   // staging is optional: without it first
                stage_p = 0;
                lds = image(pinc_rows, 0, kk, n_slots, waves);
            }
            if (lds <= 160 * 1024 || kk >= device_cus / B) break;
            ++kk;
        }
        if (two_hop) {
            bool fits = lds <= 160 * 1024 && 2 * n_slots <= 512 && kk <= 256;
            for (int b = 0; b < B && fits; ++b)
                fits = (size_t)(2 * eng->seqs[b].desc.n_pairs + kk + N) * PD_XCHG_LINE <= eng->xchg_granules;
            if (!fits) {
                two_hop = false;   // size again for the single-exchange kernel
                continue;
            }
        }
        k = kk;
        break;
    }
    if (lds > 160 * 1024) {
        pd_set_error("pd_ggs: %d work items need %zu B of LDS per workgroup (> 160 KiB) at B=%d", max_items, lds, B);
        return PD_ERR_UNSUPPORTED;
    }
    if (k > 1 && !two_hop && (size_t)max_items * PD_XCHG_LINE > eng->xchg_granules) {   // (k grew again because one workgroup's LDS image did not fit)
        pd_set_error("pd_ggs: %d work items per sequence exceed the exchange region (%zu lines) and do not fit one workgroup's LDS at B=%d",
                     max_items, eng->xchg_granules / PD_XCHG_LINE, B);
        return PD_ERR_UNSUPPORTED;
    }
    // XCD-local placement of the exchange (k > 1, one-hop kernel): block b of a launch runs on XCD b % 8, so with the block -> (sequence,
    // workgroup) mapping padded to a multiple of 8 sequences all workgroups of a sequence share an XCD -- if its 32 CUs can hold them all at
    // once (they spin on each other: co-residency) and the handshake granules fit behind the items' lines.  PD_GGS_CFG_XCHG_SPREAD: A / B.
    const int seq_per_xcd = (B + 7) / 8;
    out->xchg_local = (k > 1 && !two_hop && device_cus == 256 && seq_per_xcd * k <= 32 && k <= 256 &&
                       (size_t)max_items * PD_XCHG_LINE + 256 <= eng->xchg_granules && !(cfg->reserved & PD_GGS_CFG_XCHG_SPREAD)) ? 1 : 0;
    out->waves = waves;
    out->pinc_rows = pinc_rows;
    out->stage_p = stage_p;
    out->k = k;
    out->n_slots = n_slots;
    out->lds = (int)lds;
    out->two_hop = two_hop ? 1 : 0;
    out->max_items = max_items;
    return PD_OK;
}

// pd_ggs_plan, part 4: pd_ggs_long_kernel / pd_ggs_longm_kernel -- more than PD_MAX_FRAMES frames in the launch (or in one of its slots, with frame counts per
// sequence), or PD_GGS_CFG_LONG_FRAMES.  One shape, no fall-back: what it needs and does not find is refused, naming the number.
static int plan_long(const pd_engine *eng, int B, int N, const pd_ggs_cfg *cfg, int device_cus, int max_items, PdGgsPlan *out) {
    // PD_OPT_GGS_LONG_PAIR_ITEMS and a slot whose pairs are not all one work item: pd_ggs_longm_kernel for the whole launch -- a slot is a
    // frame PAIR there, so the shape below is sized by the most pairs of a slot (== max_items wherever every pair is one item)
    bool multi = false;
    for (int b = 0; b < B; ++b) multi = multi || !eng->seqs[b].desc.single_item_pairs;
    multi = multi && eng->ggs_long_pair_items;
    if (multi) {
        max_items = 0;
        for (int b = 0; b < B; ++b) max_items = std::max(max_items, eng->seqs[b].desc.n_pairs);
    }
    for (int b = 0; b < B && !multi; ++b)
        if (!eng->seqs[b].desc.single_item_pairs) {
            pd_set_error("pd_ggs: slot %d holds a frame pair of more than %d matches (its longest work item has %d after the cut): the kernel for "
                         "more than %d frames takes at most %d matches per frame pair", b, PD_ITEM_MAX_MATCHES, eng->seqs[b].max_item_len,
                         PD_MAX_FRAMES, PD_ITEM_MAX_MATCHES);
            return PD_ERR_UNSUPPORTED;
        }
    if (cfg->wgs_per_seq == 1 || cfg->wgs_per_seq > PD_GGS_LONG_TOT_ROWS || device_cus / B < 2) {
        if (cfg->wgs_per_seq == 1 || cfg->wgs_per_seq > PD_GGS_LONG_TOT_ROWS)
            pd_set_error("pd_ggs: wgs_per_seq=%d: the kernel for more than %d frames runs 2 .. %d workgroups per sequence", cfg->wgs_per_seq,
                         PD_MAX_FRAMES, PD_GGS_LONG_TOT_ROWS);
        else
            pd_set_error("pd_ggs: B=%d leaves %d workgroup per sequence on %d CUs: the kernel for more than %d frames needs at least 2 (B <= %d)", B,
                         device_cus / B, device_cus, PD_MAX_FRAMES, device_cus / 2);
        return PD_ERR_UNSUPPORTED;
    }
    int k = cfg->wgs_per_seq > 0 ? cfg->wgs_per_seq : (max_items + PD_GGS_WAVES - 1) / PD_GGS_WAVES;
    k = std::max(2, std::min(k, std::min(device_cus / B, PD_GGS_LONG_TOT_ROWS)));
    const int n_slots = (max_items + k * PD_GGS_WAVES - 1) / (k * PD_GGS_WAVES) * PD_GGS_WAVES;
    const int n_batch = ggs_long_batch(n_slots);
    if (n_batch <= 0) {
        pd_set_error("pd_ggs: %d frame pairs on %d workgroups per sequence (B=%d) are %d item slots per workgroup: their tables alone need %zu B of "
                     "LDS (> 160 KiB) in the kernel for more than %d frames", max_items, k, B, n_slots, ggs_long_lds_bytes(n_slots, 64), PD_MAX_FRAMES);
        return PD_ERR_UNSUPPORTED;
    }
    const size_t lds = ggs_long_lds_bytes(n_slots, n_batch);
    for (int b = 0; b < B; ++b) {
        const PdSeqDesc &d = eng->seqs[b].desc;
        const size_t lines = (size_t)2 * d.n_pairs + k + d.n_frames;
        if (lines * PD_XCHG_LINE > eng->xchg_granules) {
            pd_set_error("pd_ggs: slot %d needs %zu exchange lines (2 x %d frame pairs + %d workgroups + %d frames), the region holds %zu", b, lines,
                         d.n_pairs, k, d.n_frames, eng->xchg_granules / PD_XCHG_LINE);
            return PD_ERR_UNSUPPORTED;
        }
    }
    (void)N;
    out->long_frames = multi ? 2 : 1;
    out->k = k;
    out->waves = PD_GGS_WAVES;
    out->n_slots = n_slots;
    out->pinc_rows = 2 * n_batch;      // (reported; the kernel's argument is n_batch)
    out->lds = (int)lds;
    out->max_items = max_items;
    return PD_OK;
}

// The launch shape of one GGS launch, derived from the uploaded match tables: workgroups per sequence, local item
// slots, dynamic LDS and which kernel.  Captured hipGraphs bake these in, so pd_sample_phase keys its graph cache on
// the plan (a re-upload with another item count must never replay the old shape: the kernel would index its LDS
// tables past their size).  Also validates what pd_ggs_launch validates, so a graph replay cannot skip the checks.
int pd_ggs_plan(pd_engine *eng, int B, int N, const pd_ggs_cfg *cfg, PdGgsPlan *out) {
    int max_items = 0;
    PD_TRY(plan_check_slots(eng, B, N, cfg, out, max_items));
    // workgroups per sequence: one item per wave if the chip has room (<= 256 resident workgroups)
    const int device_cus = eng->num_cus > 0 ? eng->num_cus : 256;
    int k = cfg->wgs_per_seq > 0 ? cfg->wgs_per_seq : (max_items + PD_GGS_WAVES - 1) / PD_GGS_WAVES;
    k = std::max(1, std::min(k, device_cus / B));
    memset(out, 0, sizeof(*out));
    // more than PD_MAX_FRAMES frames (with frame counts set: in any slot), or on request: the kernel with frame tables for 256 frames
    bool long_frames = (cfg->reserved & PD_GGS_CFG_LONG_FRAMES) != 0;
    if (eng->nf_B) {
        for (int b = 0; b < B; ++b) long_frames = long_frames || eng->nf_host[b] > PD_MAX_FRAMES;
    } else {
        long_frames = long_frames || N > PD_MAX_FRAMES;
    }
    if (long_frames) return plan_long(eng, B, N, cfg, device_cus, max_items, out);
    if (plan_lane(eng, B, N, cfg, device_cus, out)) return PD_OK;
    return plan_wave_items(eng, B, N, cfg, device_cus, k, max_items, out);
}

// pd_ggs_launch: the kernels' parameter block for the launch `plan` describes
static PdGgsParams launch_params(const pd_engine *eng, float *x, int B, int N, const PdGgsStage *stages, int n_stages, const pd_ggs_cfg *cfg,
                                 int eval_only, float *stats, float *trace, int trace_iters, float *loss_out, float *grad_out, const PdGgsPlan &plan) {
    PdGgsParams P;
    memset(&P, 0, sizeof(P));
    P.seqs = eng->d_seqs;
    P.x = x;
    P.N = N;                        // the row stride of x / grad_out; a sequence's own frame count is its descriptor's n_frames
    P.k = plan.k;
    for (int i = 0; i < n_stages; ++i) P.stages[i] = stages[i];
    P.n_stages = n_stages;
    P.alpha = cfg->alpha;
    P.lr = cfg->learning_rate;
    P.sampson_max = cfg->sampson_max;
    P.momentum = cfg->momentum;
    P.min_matches = cfg->min_matches;
    P.eval_only = eval_only;
    P.stats = stats;
    P.trace = trace;
    P.trace_iters = trace_iters;
    P.loss_out = loss_out;
    P.grad_out = grad_out;
    P.xchg = (plan.k > 1) ? eng->d_xchg : nullptr;
    P.xchg_stride = (int)eng->xchg_granules;
    P.err_flag = eng->d_err;
    P.prof = eng->ggs_prof_on ? (long long *)(eng->d_err + 2) : nullptr;
    P.prof_wave = eng->ggs_prof_on > 0 ? (eng->ggs_prof_on - 1) & 0x107 : 1;
    P.n_seqs = B;
    P.stamp = eng->d_stamps ? eng->d_stamps + 2 * (size_t)eng->stamp_slot : nullptr;
    P.xchg_local = plan.xchg_local;
    return P;
}

int pd_ggs_launch(pd_engine *eng, float *x, int B, int N, const PdGgsStage *stages, int n_stages,
                  const pd_ggs_cfg *cfg, int eval_only, float *stats, float *trace, int trace_iters,
                  float *loss_out, float *grad_out, hipStream_t s) {
    if (!eng || !x || !cfg || n_stages <= 0 || n_stages > PD_GGS_MAX_STAGES) {
        pd_set_error("pd_ggs: invalid arguments (B=%d N=%d stages=%d)", B, N, n_stages);
        return PD_ERR_INVALID_ARG;
    }
    if (trace && eng->nf_B) {       // a trace row is N x 9 + 3 floats of ONE frame count
        pd_set_error("pd_ggs_optimize: trace_out must be NULL while frame counts per sequence are set (pd_engine_set_frame_counts)");
        return PD_ERR_INVALID_ARG;
    }
    PdGgsPlan plan;
    PD_TRY(pd_ggs_plan(eng, B, N, cfg, &plan));
    PD_TRY(pd_wait_uploads(eng, s));
    const PdGgsParams P = launch_params(eng, x, B, N, stages, n_stages, cfg, eval_only, stats, trace, trace_iters, loss_out, grad_out, plan);
    if (plan.k > 1) {
        // tags restart at 1 every launch: zero every polled word first (guide G16 "re-initialise every call")
        const size_t n_zero = 2 * eng->xchg_granules * B;
        hipLaunchKernelGGL(pd_ggs_zero_kernel, dim3(256), dim3(256), 0, s, eng->d_xchg, n_zero);
    }
    const size_t lds = (size_t)plan.lds;
    const int B_map = plan.xchg_local ? ((B + 7) & ~7) : B;     // the kernels' block -> (sequence, workgroup) mapping
    if (plan.long_frames == 2)
        hipLaunchKernelGGL(pd_ggs_longm_kernel, dim3(B * plan.k), dim3(PD_GGS_THREADS), lds, s, P, B, plan.n_slots, plan.pinc_rows / 2);
    else if (plan.long_frames)
        hipLaunchKernelGGL(pd_ggs_long_kernel, dim3(B * plan.k), dim3(PD_GGS_THREADS), lds, s, P, B, plan.n_slots, plan.pinc_rows / 2);
    else if (plan.lane)
        hipLaunchKernelGGL(pd_ggs_lane_kernel<PD_LANE_RV>, dim3(B), dim3(PD_LANE_THREADS), lds, s, P, plan.pinc_rows);
    else if (plan.two_hop)
        hipLaunchKernelGGL(pd_ggs2_kernel, dim3(B * plan.k), dim3(PD_GGS_THREADS), lds, s, P, B, plan.n_slots);
    else {
        // one item slot per wave: the matches stay in registers (pd_ggs_plan gives that shape 8 waves and no staging)
        const PdGgsKernel kern = ggs_variant(plan.stage_p, plan.n_slots == PD_GGS_WAVES, plan.waves);
        if (!kern) {
            pd_set_error("pd_ggs: no pd_ggs_kernel variant for stage_p=%d n_slots=%d waves=%d", plan.stage_p, plan.n_slots, plan.waves);
            return PD_ERR_STATE;
        }
        hipLaunchKernelGGL(kern, dim3(B_map * plan.k), dim3(plan.waves * 64), lds, s, P, B_map, plan.n_slots, plan.pinc_rows, plan.max_items);
    }
    PD_HIP_CHECK(hipGetLastError());
    return pd_mark_use(eng, s);
}
