/*
 * pd_engine_ingest.h -- extension of the C-ABI of libpd_engine.so (pd_engine.h): device-side match ingestion with one frame count per
 * sequence.  Same conventions as pd_engine.h (plain C, DEVICE pointers borrowed for the call, `stream` a hipStream_t as void*, 0 = PD_OK,
 * pd_last_error for the message).
 */
#ifndef PD_ENGINE_INGEST_H
#define PD_ENGINE_INGEST_H

#include "pd_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ingestion of pd_ggs_set_matches_csr_async (pd_engine.h) with ONE FRAME COUNT PER SEQUENCE: n_frames HOST [n_seqs], sequence b
 * (slot seq_first + b) has n_frames[b] frames;
 * one image size for the call.  Everything else is the contract of pd_ggs_set_matches_csr_async: device or pinned inputs in the
 * reference's dtypes, no host synchronisation, no allocation once a slot's buffer fits, launch shapes planned from capacities, the
 * descriptor written on the device, nothing enqueued unless the whole call can be launched.  This is the entry that takes
 *   - a ragged batch (e.g. 8 / 13 / 20-frame requests) in one call: a slot of <= 64 frames gets exactly the tables that call builds
 *     for its frame count (lane tables at <= 24 frames included), whatever shares the call with it;
 *   - sequences of 65 .. 256 frames (PD_OPT_GGS_MAX_FRAMES): such a slot gets the tables pd_ggs_set_matches writes there (pts, pair_ij,
 *     pair_item_off, items, gpos, ginc_off; no chunk tables, no lane tables, no limit on the chunks of pairs) from a stable two-pass
 *     sort by (j, then i) whose scratch is O(M + n_frames^2).  pd_ggs_long_kernel takes one work item per frame pair and the host
 *     never learns the counts, so a call that holds a count above 64 needs hints->max_matches_per_pair in 1 .. 512
 *     (PD_ERR_UNSUPPORTED naming the hint otherwise).  With the engine option PD_OPT_GGS_LONG_PAIR_ITEMS on, such a call also takes 0
 *     (unknown) or a value above 512: the slot's capacities are then P_cap + M / 512 + 1 work items and a host shadow that is not one
 *     item per pair, so its launches run pd_ggs_longm_kernel; a positive hint is still enforced on the device.
 * A frame index is checked against the sequence's OWN count: an index outside it, or a violated hint, empties THAT slot and raises
 * the asynchronous error word (bits 1 / 2); the other slots of the call are built.  Every count lies in
 * [1, min(max_N, PD_OPT_GGS_MAX_FRAMES)]: above the GGS limit in force PD_ERR_UNSUPPORTED (naming the limit), otherwise -- or with
 * n_frames == NULL -- PD_ERR_INVALID_ARG.  The slots' frame counts are what pd_engine_set_frame_counts / the GGS calls then expect.
 * Results are bitwise those of pd_ggs_set_matches on the same data. */
int pd_ggs_set_matches_csr_async_nf(pd_engine *eng, int seq_first, int n_seqs, const int64_t *seq_offsets, const double *kp1,
                                    const double *kp2, const int64_t *i12, const int *n_frames, int height, int width,
                                    const pd_match_hints *hints, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_ENGINE_INGEST_H */
