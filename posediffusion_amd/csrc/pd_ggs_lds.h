// pd_ggs_lds.h -- the three LDS images of the GGS kernels, each written down ONCE: carve() (pd_ggs_kernel, pd_ggs2_kernel), carve_lane()
// (pd_ggs_lane_kernel) and carve_long() (pd_ggs_long_kernel) hand out the pointers the kernels use, and the host reads the dynamic LDS size of a launch off those same pointers
// (ggs_lds_bytes, lane_lds_bytes, ggs_long_lds_bytes) -- a field added to a carve is in the byte count by construction.  The images fill the 160 KiB of a CU at
// the large shapes: a byte count that lagged behind its carve would let the kernel index past the LDS it was launched with.
#pragma once
#include "pd_internal.h"

#define PD_F_STRIDE 12    // floats per slot of the per-item F in LDS (9 used; 16-byte aligned rows)
// LDS carve (floats).  Everything lives in the one dynamic region (guide G17).
#define PD_GGS_PSUM_FLOATS (PD_GGS_FAST_FRAMES * 48 > 64 * 16 ? PD_GGS_FAST_FRAMES * 48 : 64 * 16)
#define PD_FR_STRIDE 12   // floats per frame in L.Rc: R_cv (9, row-major) | t_cv (3) -- three 16-byte LDS accesses per frame
#define PD_XS_STRIDE 12   // floats per frame in L.xst / L.mst: the 9 parameters / momenta (+ 3 unused), 16-byte accesses too
struct Lds {
    float *Rc;     // [64*12] per frame R_cv (9) | t_cv (3)  (opencv_from_cameras_projection)
    float *fl;     // [64*4]  per frame clamped focal (x, y) | clamp pass-through mask (1/0: x, y)
    float *cam;    // [8]     a0,a1,c0,c1,fbar_x,fbar_y
    float *gT;     // [64*3]  per-frame dL/dT  (un-normalised: not yet divided by n_valid)
    float *gR;     // [64*9]  per-frame dL/dR  (PyTorch3D R, un-normalised)
    float *gA;     // [64*4]  per-frame partial dL/dA {00,02,11,12}
    float *ctl;    // [8]     ctl[0] = stage done flag, ctl[1] = abort
    long long *prof;   // [16] phase cycle counters of the one wave that records them (pd_debug_ggs_prof): in LDS, not in 20 registers of every wave
    float *xst;    // [64*12] pose parameters per frame (lane = frame in P4) -- in LDS, not in registers: wave 0 touches them once per
    float *mst;    // [64*12] iteration, and 18 VGPRs held by every wave for the whole launch is what the match pass cannot spare
    float *pinc;   // [pinc_rows*16] backward results of the current chunk of pairs, one row per (pair, side), frame-sorted
                   //   (pinc_rows = 2 x pairs per chunk, at most PD_GGS_PINC_ROWS; the two-hop kernel always carves the maximum)
    float *psum;   // [PD_GGS_PSUM_FLOATS] general serial path (more than PD_GGS_FAST_FRAMES frames or several chunks of pairs): per-frame
                   //   partial sums across chunks [64*16]
    float *W;      // = psum, fast serial path: per frame the 4 x 9 Jacobian d(R entries)/d(quaternion) of the CURRENT parameters, rows
                   //   padded to 12 floats [PD_GGS_FAST_FRAMES*48] (jac_all)
    float *gq;     // = gR: [64*8] per frame {dL/dq (4), dL/dT (3), -} as P4 reads them (un-normalised: not yet divided by n_valid)
    int4 *itab;    // [n_slots] (first match, count, i, j) of the local items
    int *incoff;   // [PD_GGS_MAX_PCHUNKS][68] per chunk of pairs: CSR offsets of its incidences per frame
    float *F;      // [n_slots*PD_F_STRIDE]
    float *item;   // [n_items*12]
    float *stage;  // [8 waves][2 buffers][STAGE_P KiB] (or [12 waves][1 buffer]) LDS-DMA staging of the match pass (pd_ggs_kernel<STAGE_P > 0>), 1 KiB aligned
};

// (__host__ too: the host runs the same carve to size the launch, below)
__host__ __device__ __forceinline__ Lds carve(float *base, int n_slots, int pinc_rows, int n_items_cap) {
    Lds L;
    L.Rc = base;
    L.fl = L.Rc + 64 * PD_FR_STRIDE;
    L.cam = L.fl + 64 * 4;
    L.gT = L.cam + 8;
    L.gR = L.gT + 64 * 3;
    L.gA = L.gR + 64 * 9;
    L.ctl = L.gA + 64 * 4;
    L.prof = (long long *)(L.ctl + 8);
    L.xst = L.ctl + 8 + 32;
    L.mst = L.xst + 64 * PD_XS_STRIDE;
    L.pinc = L.mst + 64 * PD_XS_STRIDE;
    L.psum = L.pinc + pinc_rows * 16;
    L.W = L.psum;
    L.gq = L.gR;
    L.itab = (int4 *)(L.psum + PD_GGS_PSUM_FLOATS);
    L.incoff = (int *)(L.itab + n_slots);
    L.F = (float *)(L.incoff + PD_GGS_MAX_PCHUNKS * 68);
    L.item = L.F + n_slots * PD_F_STRIDE;
    L.stage = base + ((((L.item + n_items_cap * PD_ITEM_VALS) - base) + 255) & ~255);   // 1 KiB aligned (base is the LDS origin)
    return L;
}

// Host side of both images: the carve run on a stand-in for the LDS origin (1 KiB aligned like the origin; never dereferenced), and a
// carved pointer's distance from it in bytes.
static float *pd_ggs_lds_origin() { return (float *)(size_t)(1u << 20); }
static size_t pd_ggs_lds_offset(const void *p) { return (size_t)((const char *)p - (const char *)pd_ggs_lds_origin()); }

// dynamic LDS of a wave-per-item launch: up to the end of L.item, or (STAGE_P > 0) of the staging buffers -- 8 waves x 2 buffers, or 12 x 1
static size_t ggs_lds_bytes(int n_slots, int n_items, int pinc_rows, int stage_p, int stage_bufs = PD_GGS_WAVES * 2) {
    const Lds L = carve(pd_ggs_lds_origin(), n_slots, pinc_rows, n_items);
    if (stage_p > 0) return pd_ggs_lds_offset(L.stage) + (size_t)stage_bufs * stage_p * 1024;
    return pd_ggs_lds_offset(L.item + (size_t)n_items * PD_ITEM_VALS);
}

// The lane-per-item kernel's image (pd_ggs_lane.inc): the same struct, tables for 48 frame rows, no item table / F (a lane holds its own).
__host__ __device__ __forceinline__ Lds carve_lane(float *base, int pinc_rows) {
    Lds L;
    L.Rc = base;
    L.fl = L.Rc + 48 * PD_FR_STRIDE;
    L.cam = L.fl + 48 * 4;
    L.gT = L.cam + 8;
    L.gR = L.gT + 48 * 3;
    L.gA = L.gR + 48 * 9;
    L.ctl = L.gA + 48 * 4;
    L.xst = L.ctl + 8;
    L.mst = L.xst + 64 * PD_XS_STRIDE;
    L.psum = L.mst + 64 * PD_XS_STRIDE;                // [16] valid counts of the waves
    L.W = L.psum + 16;                                 // [PD_GGS_FAST_FRAMES * 48] quaternion Jacobians (jac_all)
    L.gq = L.gR;
    L.pinc = L.W + PD_GGS_FAST_FRAMES * 48;            // 16-byte aligned (what precedes it is a multiple of 4 floats: lane_pinc_aligned)
    L.incoff = (int *)(L.pinc + pinc_rows * 16);       // [68]
    L.item = (float *)(L.incoff + 68);                 // [PD_LANE_MAX_ITEMS][PD_LANE_ITEM_VALS]
    L.itab = nullptr;
    L.F = nullptr;
    L.stage = base + ((((L.item + PD_LANE_MAX_ITEMS * PD_LANE_ITEM_VALS) - base) + 255) & ~255);   // the waves' rings, 1 KiB aligned
    return L;
}
// dynamic LDS of a lane-per-item launch: the tables, then `wave_slots` 2 KiB slots per wave (PD_LANE_SLOTS: resident steps + the ring -- a
// parameter only because pd_ggs_lane.inc defines PD_LANE_SLOTS, with the kernel's other switches, after this header is included)
static size_t lane_lds_bytes(int pinc_rows, int wave_slots) {
    return pd_ggs_lds_offset(carve_lane(pd_ggs_lds_origin(), pinc_rows).stage) + (size_t)wave_slots * PD_LANE_WAVES * 2048;
}
// the float4 rows of L.pinc rest on the fields before it adding up to a multiple of 16 bytes (checked once, by pd_ggs_init)
static bool lane_pinc_aligned() { return pd_ggs_lds_offset(carve_lane(pd_ggs_lds_origin(), 0).pinc) % 16 == 0; }

// The image of the kernel for up to PD_GGS_LONG_FRAMES frames (pd_ggs_long_kernel): the same struct with frame tables for 256 frames, the hop
// windows of the two-hop scheme under names of their own, and only this workgroup's slots of the item tables.  L.pinc = the own rows (what
// pd_ggs_pairbwd.inc writes); L.prof / L.W / L.stage are not part of this image.
#define PD_GGS_LONG_FRAMES 256        // frames of the tables (thread = frame on waves 0 .. 3 in the serial phases)
#define PD_GGS_LONG_INCOFF 260        // CSR offsets of the incidence rows by frame: N + 1 entries, padded to 16 bytes
#define PD_GGS_LONG_FRAME_ROWS 512    // gathered rows of an owned frame: up to 2 (N - 1) = 510 when both orders of every pair occur
#define PD_GGS_LONG_TOT_ROWS 256      // gathered totals lines, one per workgroup of the sequence (k <= 256), 4 floats each
#define PD_GGS_LONG_RED 32            // cross-wave partial sums of the serial phases: 8 sums x the 4 frame waves
struct LdsLong : Lds {
    float *red;         // [PD_GGS_LONG_RED]
    float *tot_rows;    // [PD_GGS_LONG_TOT_ROWS][4]
    float *frame_rows;  // [PD_GGS_LONG_FRAME_ROWS][16]
    float *own_rows;    // [2 n_batch][16] results of a batch of this workgroup's pairs: row 2 s = side 0 of the batch's slot s, 2 s + 1 = side 1
    int *grow;          // [2 n_slots] exchange row of each local (pair, side)
    float *end;         // one past the image
};
// n_slots: item slots of a workgroup (L.itab, L.grow); n_batch <= n_slots: those whose F, item sums and rows are in LDS at a time
__host__ __device__ __forceinline__ LdsLong carve_long(float *base, int n_slots, int n_batch) {
    constexpr int NF = PD_GGS_LONG_FRAMES;
    LdsLong L;
    L.Rc = base;
    L.fl = L.Rc + NF * PD_FR_STRIDE;
    L.cam = L.fl + NF * 4;
    L.gT = L.cam + 8;
    L.gR = L.gT + NF * 3;
    L.gA = L.gR + NF * 9;
    L.ctl = L.gA + NF * 4;
    L.red = L.ctl + 8;
    L.xst = L.red + PD_GGS_LONG_RED;
    L.mst = L.xst + NF * PD_XS_STRIDE;
    L.psum = L.mst + NF * PD_XS_STRIDE;                 // [NF][16] the gathered frame sums
    L.incoff = (int *)(L.psum + NF * 16);
    L.tot_rows = (float *)(L.incoff + PD_GGS_LONG_INCOFF);
    L.frame_rows = L.tot_rows + PD_GGS_LONG_TOT_ROWS * 4;
    L.own_rows = L.frame_rows + PD_GGS_LONG_FRAME_ROWS * 16;
    L.pinc = L.own_rows;
    L.F = L.own_rows + 2 * n_batch * 16;
    L.item = L.F + n_batch * PD_F_STRIDE;
    L.itab = (int4 *)(L.item + n_batch * PD_ITEM_VALS);
    L.grow = (int *)(L.itab + n_slots);
    L.end = (float *)(L.grow + 2 * n_slots);
    L.prof = nullptr;
    L.W = nullptr;
    L.gq = L.gR;
    L.stage = nullptr;
    return L;
}
// dynamic LDS of a pd_ggs_long_kernel launch
static size_t ggs_long_lds_bytes(int n_slots, int n_batch) { return pd_ggs_lds_offset(carve_long(pd_ggs_lds_origin(), n_slots, n_batch).end); }
// Slots per batch for a workgroup of n_slots: all of them when that image fits the 160 KiB of a CU (and P3a's one thread per slot of a
// batch, <= PD_GGS_THREADS); else the largest multiple of 64 that fits (the lanes of the totals wave then keep their slots across
// batches); 0: not even 64.
static int ggs_long_batch(int n_slots) {
    if (n_slots <= PD_GGS_THREADS && ggs_long_lds_bytes(n_slots, n_slots) <= 160 * 1024) return n_slots;
    int nb = (n_slots < PD_GGS_THREADS ? n_slots : PD_GGS_THREADS) & ~63;
    while (nb > 0 && ggs_long_lds_bytes(n_slots, nb) > 160 * 1024) nb -= 64;
    return nb;
}
