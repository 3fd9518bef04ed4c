// pd_ggs_ingest_layout.h -- the slot blob of a device-built sequence of more than 64 frames (pd_ggs_set_matches_csr_async_nf, the
// ingest_nf_* kernels of pd_ggs_ingest.hip).  Compiles on the host alone, like pd_ggs_lds.h (tests/test_ingest_layout_cpu.py runs it).
//
// The blob holds, each piece 256-byte aligned and in this order, the arrays the host builder writes for such a sequence (pd_blob_layout
// with no chunk and no lane tables) by CAPACITY -- M matches, P_cap frame pairs, I_cap work items, N frames --
//     pts  float4[M] | pair_ij  int2[P_cap] | pair_item_off  int[P_cap + 1] | items  int4[I_cap] | gpos  int2[P_cap] | ginc_off  int[N + 1]
// (pts .. items at the offsets of ingest_layout, so that ingest_interleave_kernel serves both), and behind them the scratch of the sort:
//     cnt   int[N * N + 1]     matches of a key (global integer atomics), then the first sorted row of the key
//     pex   int[N * N + 1]     frame pairs with matches before the key (the pair index of a key that has matches)
//     crk   int[N * N]         of key (i, j): pairs (a, j) with matches and a < i
//     keys  int[M]             i * N + j of every upload row, -1: a frame index out of range
//     src   int[M]             upload rows ordered by j (pass 1 of the two-pass sort)
//     hist  int[257][n_tiles]  per digit and tile of 1 024 rows: rows of the tile with that digit, then those of the earlier tiles; one
//                              array for both passes (256 frame digits + one for the rows without a key), n_tiles = ceil(M / 1 024)
//     btot  int[257]           rows per digit
// With al(v) = v rounded up to a multiple of 256 the total is
//     al(16 M) + al(8 P_cap) + al(4 (P_cap + 1)) + al(16 I_cap) + al(8 P_cap) + al(4 (N + 1))
//   + al(4 (N^2 + 1)) + al(4 (N^2 + 1)) + al(4 N^2) + al(4 M) + al(4 M) + al(4 x 257 x n_tiles) + al(4 x 257)
// i.e. a scratch of 8 bytes per match, 12 per key and 1 028 per tile: O(M + N^2), nothing of size n_tiles x N^2.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define PD_ING_HD __host__ __device__
#else
#define PD_ING_HD
#endif

#define PD_ING_TILE 1024          // upload rows per tile of the sort (= ING_TILE)
#define PD_ING_DIGITS 257         // a frame index (<= 256 frames), or 256: the row has no key

struct PdIngestNfLayout {
    size_t pts, pij, pio, itm, gps, gio, cnt, pex, crk, keys, src, hist, btot, total;
};

PD_ING_HD static inline size_t pd_ing_al256(size_t v) { return (v + 255) & ~(size_t)255; }
PD_ING_HD static inline size_t pd_ing_tiles(long long M) { return ((size_t)M + PD_ING_TILE - 1) / PD_ING_TILE; }

PD_ING_HD static inline void pd_ingest_nf_layout(long long M, int N, long long P_cap, long long I_cap, PdIngestNfLayout &L) {
    const size_t m = (size_t)M, n = (size_t)N, p = (size_t)P_cap, it = (size_t)I_cap, nn = n * n;
    L.pts = 0;
    L.pij = pd_ing_al256(L.pts + 16 * m);
    L.pio = pd_ing_al256(L.pij + 8 * p);
    L.itm = pd_ing_al256(L.pio + 4 * (p + 1));
    L.gps = pd_ing_al256(L.itm + 16 * it);
    L.gio = pd_ing_al256(L.gps + 8 * p);
    L.cnt = pd_ing_al256(L.gio + 4 * (n + 1));
    L.pex = pd_ing_al256(L.cnt + 4 * (nn + 1));
    L.crk = pd_ing_al256(L.pex + 4 * (nn + 1));
    L.keys = pd_ing_al256(L.crk + 4 * nn);
    L.src = pd_ing_al256(L.keys + 4 * m);
    L.hist = pd_ing_al256(L.src + 4 * m);
    L.btot = pd_ing_al256(L.hist + 4 * (size_t)PD_ING_DIGITS * pd_ing_tiles(M));
    L.total = pd_ing_al256(L.btot + 4 * (size_t)PD_ING_DIGITS);
}
