// pd_ggs_tables.hip -- the host builder of a sequence's match tables (pd_ggs_set_matches).  Host only: no kernel lives here.
//
// pd_build_seq_tables makes every array of the PdSeqDesc from the caller's matches as a sequence of named steps, each taking what
// it reads and returning what it makes; it calls neither HIP nor the engine.  pd_ggs_set_matches packs the result into the slot
// blob (pd_blob_layout, pd_internal.h) and writes the descriptor.  The device builder of the same tables, bit for bit, is
// pd_ggs_ingest.hip; the rules both follow (pd_cut_len, pd_lane_rank, pd_lane_pass_cost, pd_interleave_pair) are in pd_internal.h.
#include "pd_internal.h"

#include <algorithm>
#include <string.h>

// stable counting sort by pair key = i * N + j   (geometry_guided_sampling.py:26-27): key_off[q] = first sorted row of key q
static int sort_by_pair(const double *kp1, const double *kp2, const int64_t *i12, int64_t M, int N, std::vector<int> &key_off,
                        std::vector<float4> &pts) {
    std::vector<int> cnt((size_t)N * N + 1, 0);
    for (int64_t m = 0; m < M; ++m) {
        const int64_t a = i12[2 * m], c = i12[2 * m + 1];
        if (a < 0 || a >= N || c < 0 || c >= N) {
            pd_set_error("pd_ggs_set_matches: frame index (%lld,%lld) out of range [0,%d) at match %lld",
                         (long long)a, (long long)c, N, (long long)m);
            return PD_ERR_INVALID_ARG;
        }
        cnt[a * N + c + 1]++;
    }
    key_off.assign((size_t)N * N + 1, 0);
    for (int q = 0; q < N * N; ++q) key_off[q + 1] = key_off[q] + cnt[q + 1];
    pts.resize((size_t)M);
    std::vector<int> cur(key_off.begin(), key_off.end() - 1);
    for (int64_t m = 0; m < M; ++m) {
        const int key = (int)(i12[2 * m] * N + i12[2 * m + 1]);
        // .float() cast of geometry_guided_sampling.py:167 (round-to-nearest fp64 -> fp32)
        pts[cur[key]++] = make_float4((float)kp1[2 * m], (float)kp1[2 * m + 1], (float)kp2[2 * m], (float)kp2[2 * m + 1]);
    }
    return PD_OK;
}

// the frame pairs that own matches, each cut into balanced work items of <= PD_ITEM_MAX_MATCHES matches
static int cut_work_items(const std::vector<int> &key_off, int N, PdSeqTables &t) {
    for (int q = 0; q < N * N; ++q) {
        const int m = key_off[q + 1] - key_off[q];
        if (m == 0) continue;
        const int p = (int)t.pair_ij.size();
        t.pair_ij.push_back(make_int2(q / N, q % N));
        t.pair_item_off.push_back((int)t.items.size());
        const int nch = (m + PD_ITEM_MAX_MATCHES - 1) / PD_ITEM_MAX_MATCHES;
        int start = key_off[q];
        for (int c = 0; c < nch; ++c) {
            const int len = pd_cut_len(m, nch, c);
            t.items.push_back(make_int4(p, start, len, 0));
            start += len;
        }
    }
    t.pair_item_off.push_back((int)t.items.size());
    for (const int4 &it : t.items) t.max_item_len = std::max(t.max_item_len, it.z);
    for (size_t p = 0; p < t.pair_ij.size(); ++p)
        if (t.pair_item_off[p + 1] - t.pair_item_off[p] > 0xffff) {
            pd_set_error("pd_ggs_set_matches: a frame pair holds too many matches");
            return PD_ERR_UNSUPPORTED;
        }
    return PD_OK;
}

// per-pair table: positions of the pair's two incidences (side 0 under frame i, side 1 under frame j) among the
// incidences of its CHUNK of PD_GGS_THREADS pairs, sorted by frame; pchunk_off[chunk][n] = first position of frame n
static int chunk_incidences(int N, PdSeqTables &t) {
    const int n_pairs = (int)t.pair_ij.size();
    t.n_pchunks = (n_pairs + PD_GGS_THREADS - 1) / PD_GGS_THREADS;
    // most pairs incident to one frame: the row stride of the fast per-frame sums (pd_ggs_kernel)
    std::vector<int> deg(N, 0);
    for (int p = 0; p < n_pairs; ++p) {
        deg[t.pair_ij[p].x]++;
        deg[t.pair_ij[p].y]++;
    }
    for (int n = 0; n < N; ++n) t.max_deg = std::max(t.max_deg, deg[n]);
    // more than PD_MAX_FRAMES frames (PD_OPT_GGS_MAX_FRAMES): only pd_ggs_long_kernel runs, which reads the global tables (gpos, ginc_off) --
    // the chunk tables of the one-hop and lane kernels are not built (n_pchunks is still reported)
    if (N > PD_MAX_FRAMES) return PD_OK;
    if (t.n_pchunks > PD_GGS_MAX_PCHUNKS) {
        pd_set_error("pd_ggs_set_matches: %d frame pairs with matches (max %d)", n_pairs, PD_GGS_MAX_PCHUNKS * PD_GGS_THREADS);
        return PD_ERR_UNSUPPORTED;
    }
    t.ptab.resize(n_pairs);
    t.pchunk_off.assign((size_t)t.n_pchunks * (N + 1), 0);
    std::vector<int> pos0(n_pairs, 0), pos1(n_pairs, 0);
    for (int ck = 0; ck < t.n_pchunks; ++ck) {
        const int p_lo = ck * PD_GGS_THREADS, p_hi = std::min(n_pairs, p_lo + PD_GGS_THREADS);
        int q = 0;
        for (int n = 0; n < N; ++n) {
            t.pchunk_off[(size_t)ck * (N + 1) + n] = q;
            for (int p = p_lo; p < p_hi; ++p) {
                if (t.pair_ij[p].x == n) pos0[p] = q++;
                if (t.pair_ij[p].y == n) pos1[p] = q++;
            }
        }
        t.pchunk_off[(size_t)ck * (N + 1) + N] = q;
    }
    for (int p = 0; p < n_pairs; ++p)
        t.ptab[p] = make_int4(t.pair_ij[p].x | (t.pair_ij[p].y << 8), t.pair_item_off[p], t.pair_item_off[p + 1] - t.pair_item_off[p],
                              pos0[p] | (pos1[p] << 16));
    return PD_OK;
}

// the same positions among ALL incidences (two-hop kernel: one exchange line per (pair, side), grouped by frame)
static void global_incidences(int N, PdSeqTables &t) {
    const int n_pairs = (int)t.pair_ij.size();
    t.gpos.resize(n_pairs);
    t.ginc_off.assign(N + 1, 0);
    int q = 0;
    for (int n = 0; n < N; ++n) {
        t.ginc_off[n] = q;
        for (int p = 0; p < n_pairs; ++p) {
            if (t.pair_ij[p].x == n) t.gpos[p].x = q++;
            if (t.pair_ij[p].y == n) t.gpos[p].y = q++;
        }
    }
    t.ginc_off[N] = q;
    for (int p = 0; p < n_pairs; ++p)
        if (t.pair_item_off[p + 1] - t.pair_item_off[p] != 1) t.single_item_pairs = 0;
}

// smallest lane-item length with <= PD_LANE_MAX_ITEMS lane items in the sequence (n_pairs items at the longest pair's length)
static int lane_base_len(const std::vector<int> &key_off, int N) {
    int lo = 1, hi = 1;
    for (int q = 0; q < N * N; ++q) hi = std::max(hi, key_off[q + 1] - key_off[q]);
    auto count_items = [&](int len) {
        long long n = 0;
        for (int q = 0; q < N * N; ++q) n += pd_lane_items_of(key_off[q + 1] - key_off[q], len);
        return n;
    };
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (count_items(mid) <= PD_LANE_MAX_ITEMS) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// round 6: k more cuts for the spare / k - d pairs with the longest items, (k, d) by the modelled match pass (pd_lane_pass_cost).
// l_m = matches, l_nch = cuts at the base length of every pair; returns the cuts of the cheapest candidate
static std::vector<int> lane_cut_rule(const std::vector<int> &l_m, const std::vector<int> &l_nch, int spare) {
    const int n_pairs = (int)l_m.size();
    std::vector<int> rank(n_pairs, 0), nch_k(n_pairs), steps_k(n_pairs), best_nch = l_nch;
    for (int p = 0; p < n_pairs; ++p)
        if (l_nch[p] != 0 && l_m[p] > l_nch[p]) rank[p] = pd_lane_rank(l_m.data(), l_nch.data(), n_pairs, p, false);
    int best_cost = 0x7fffffff;
    for (int k = 1; k <= PD_LANE_MORE_MAX; ++k)
        for (int d = 0; d < PD_LANE_MORE_SLACK && (d == 0 || spare / k - d > 0); ++d) {
            int n_items = 0;
            for (int p = 0; p < n_pairs; ++p) {
                const bool elig = l_nch[p] != 0 && l_m[p] > l_nch[p] && rank[p] < spare / k - d;
                nch_k[p] = l_nch[p] + (elig ? std::min(k, l_m[p] - l_nch[p]) : 0);
                steps_k[p] = nch_k[p] ? (pd_lane_items_of(l_m[p], nch_k[p]) + 1) / 2 : 0;
                n_items += nch_k[p];
            }
            int T[PD_LANE_WAVES] = {}, Tmin[PD_LANE_WAVES] = {};
            for (int p = 0; p < n_pairs; ++p) {
                if (!nch_k[p]) continue;
                const int first = pd_lane_rank(steps_k.data(), nch_k.data(), n_pairs, p, true), end = first + nch_k[p];
                for (int w = (first + 63) / 64; w < PD_LANE_WAVES && 64 * w < end; ++w) T[w] = steps_k[p];                       // item 64 w: the wave's longest
                for (int w = first / 64; w < PD_LANE_WAVES && 64 * w < end; ++w)
                    if (std::min(64 * w + 63, n_items - 1) < end && std::min(64 * w + 63, n_items - 1) >= first) Tmin[w] = steps_k[p];   // its last item
            }
            const int cost = pd_lane_pass_cost(T, Tmin);
            if (cost < best_cost) {
                best_cost = cost;
                best_nch = nch_k;
            }
        }
    return best_nch;
}

// lane-per-item tables (pd_ggs_lane_kernel): every pair is cut into lane items of balanced size at the base length (+ the cut rule's
// extra cuts while lanes are left); lane item q belongs to thread q.  The items are ORDERED by length (steps of the pair's longest
// item, descending; pair; cut), 64 per wave: a wave runs as many steps as its longest item, and waves w and w + 4 share a SIMD
// (tools/simd_probe.hip), so long and short waves pair up.  A pair's items stay adjacent and in cut order (the pair backward sums
// them in that order).  A wave's stream holds max-over-its-lanes steps of two matches per lane (a lane past its item's end re-reads
// its last match, masked in the kernel).  Reads t.pts BEFORE its full groups are interleaved.
static void lane_tables(const std::vector<int> &key_off, int N, PdSeqTables &t) {
    const int n_pairs = (int)t.pair_ij.size();
    t.lptab = std::vector<int2>(n_pairs);
    if (!(n_pairs <= PD_LANE_MAX_ITEMS && t.n_pchunks == 1 && N <= PD_LANE_MAX_FRAMES)) return;
    t.l_item_len = lane_base_len(key_off, N);
    std::vector<int> l_m(n_pairs), l_nch(n_pairs), l_steps(n_pairs);
    int l_total = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int q = t.pair_ij[p].x * N + t.pair_ij[p].y;
        l_m[p] = key_off[q + 1] - key_off[q];
        l_nch[p] = pd_lane_items_of(l_m[p], t.l_item_len);
        l_total += l_nch[p];
    }
    l_nch = lane_cut_rule(l_m, l_nch, PD_LANE_MAX_ITEMS - l_total);
    for (int p = 0; p < n_pairs; ++p) l_steps[p] = l_nch[p] ? (pd_lane_items_of(l_m[p], l_nch[p]) + 1) / 2 : 0;
    std::vector<int4> &litems = t.litems;
    litems.assign((size_t)PD_LANE_MAX_ITEMS, make_int4(0, 0, 0, 0));
    int n_lit = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int q = t.pair_ij[p].x * N + t.pair_ij[p].y, m = l_m[p], nch = l_nch[p];
        const int first = pd_lane_rank(l_steps.data(), l_nch.data(), n_pairs, p, true);
        t.lptab[p] = make_int2(first, nch);
        int start = key_off[q];
        for (int c = 0; c < nch; ++c) {
            const int len = pd_cut_len(m, nch, c);
            litems[(size_t)first + c] = make_int4(t.pair_ij[p].x | (t.pair_ij[p].y << 8), len, p, start);
            start += len;
        }
        n_lit += nch;
    }
    litems.resize(n_lit);
    const int n_lw = ((int)litems.size() + 63) / 64;
    size_t base = 0;
    for (int w = 0; w < n_lw; ++w) {
        int steps = 0;
        for (int l = 0; l < 64 && w * 64 + l < (int)litems.size(); ++l) steps = std::max(steps, (litems[w * 64 + l].y + 1) / 2);
        t.lwave.push_back(make_int2((int)base, steps));
        t.l_max_steps = std::max(t.l_max_steps, steps);
        base += (size_t)steps * 128;
    }
    t.lstream.assign(base, make_float4(1.0f, 1.0f, 1.0f, 1.0f));
    for (int w = 0; w < n_lw; ++w)
        for (int s = 0; s < t.lwave[w].y; ++s)
            for (int l = 0; l < 64 && w * 64 + l < (int)litems.size(); ++l) {
                const int4 it = litems[w * 64 + l];
                const float4 a = t.pts[(size_t)it.w + std::min(2 * s, it.y - 1)], b2 = t.pts[(size_t)it.w + std::min(2 * s + 1, it.y - 1)];
                float4 q0, q1;
                pd_interleave_pair(a, b2, q0, q1);
                t.lstream[(size_t)t.lwave[w].x + (size_t)(2 * s) * 64 + l] = q0;
                t.lstream[(size_t)t.lwave[w].x + (size_t)(2 * s + 1) * 64 + l] = q1;
            }
}

// full 128-match groups of every work item: pair-interleaved in place (MatchRegs of the GGS kernels)
static void interleave_full_groups(PdSeqTables &t) {
    for (const int4 &it : t.items)
        for (int g = 0; g + 128 <= it.z; g += 128)
            for (int l = 0; l < 64; ++l) {
                float4 &a = t.pts[(size_t)it.y + g + l], &b = t.pts[(size_t)it.y + g + 64 + l];
                float4 q0, q1;
                pd_interleave_pair(a, b, q0, q1);
                a = q0;
                b = q1;
            }
}

int pd_build_seq_tables(const double *kp1, const double *kp2, const int64_t *i12, int64_t M, int n_frames, PdSeqTables &out) {
    out = PdSeqTables();
    std::vector<int> key_off;
    PD_TRY(sort_by_pair(kp1, kp2, i12, M, n_frames, key_off, out.pts));
    PD_TRY(cut_work_items(key_off, n_frames, out));
    PD_TRY(chunk_incidences(n_frames, out));
    global_incidences(n_frames, out);
    lane_tables(key_off, n_frames, out);
    interleave_full_groups(out);
    return PD_OK;
}

// the blob of the tables, sized by their exact counts; `o` receives the offsets of its arrays
static std::vector<char> pack_tables(const PdSeqTables &t, PdBlobArrays &o) {
    PdBlobArrays n;
    n.pts = t.pts.size();
    n.pij = t.pair_ij.size();
    n.pio = t.pair_item_off.size();
    n.itm = t.items.size();
    n.ptb = t.ptab.size();
    n.pco = t.pchunk_off.size();
    n.gps = t.gpos.size();
    n.gio = t.ginc_off.size();
    n.lit = t.litems.size();
    n.lwv = t.lwave.size();
    n.lpt = t.lptab.size();
    n.lst = t.lstream.size();
    std::vector<char> host(pd_blob_layout(n, o), 0);
    auto put = [&](size_t off, const auto &v) { if (!v.empty()) memcpy(host.data() + off, v.data(), sizeof(v[0]) * v.size()); };
    put(o.pts, t.pts);
    put(o.pij, t.pair_ij);
    put(o.pio, t.pair_item_off);
    put(o.itm, t.items);
    put(o.ptb, t.ptab);
    put(o.pco, t.pchunk_off);
    put(o.gps, t.gpos);
    put(o.gio, t.ginc_off);
    if (!t.litems.empty()) {
        put(o.lit, t.litems);
        put(o.lwv, t.lwave);
        put(o.lpt, t.lptab);
        put(o.lst, t.lstream);
    }
    return host;
}

void pd_ggs_free_seq(PdSeqHost &h) {
    if (h.blob) (void)hipFree(h.blob);
    h.blob = nullptr;
    h.blob_bytes = 0;
    memset(&h.desc, 0, sizeof(h.desc));
}

// one slot's descriptor -> device (other slots may hold descriptors the ingestion kernels wrote on the device)
static int upload_seq_desc(pd_engine *eng, int seq) {
    PD_HIP_CHECK(hipMemcpy(eng->d_seqs + seq, &eng->seqs[seq].desc, sizeof(PdSeqDesc), hipMemcpyHostToDevice));
    return PD_OK;
}

extern "C" int pd_ggs_set_matches(pd_engine *eng, int seq, const double *kp1, const double *kp2, const int64_t *i12,
                                  int64_t M, int n_frames, int height, int width) {
    if (!eng || seq < 0 || seq >= eng->max_B) {
        pd_set_error("pd_ggs_set_matches: bad engine or sequence slot %d", seq);
        return PD_ERR_INVALID_ARG;
    }
    if (M != 0) PD_TRY(pd_ggs_frames_unsupported(eng, n_frames, "pd_ggs_set_matches"));   // (M == 0 clears the slot whatever n_frames says)
    PD_HIP_CHECK(hipSetDevice(eng->device));
    // nothing of THIS engine in flight may still read the old tables; other engines (other batches of a pipeline) keep
    // running: no device-wide synchronisation here, and the blob is re-used when the new tables fit
    PD_TRY(pd_wait_uses(eng, nullptr, true));
    for (auto &e : eng->uploads) PD_HIP_CHECK(hipEventSynchronize(e.event));   // a pending device-side build of this slot
    PdSeqHost &h = eng->seqs[seq];
    h.device_built = false;
    if (M == 0) {
        pd_ggs_free_seq(h);
        return upload_seq_desc(eng, seq);
    }
    if (!kp1 || !kp2 || !i12 || M < 0 || n_frames <= 0 || n_frames > eng->ggs_max_frames || n_frames > eng->max_N ||
        height <= 0 || width <= 0) {
        pd_set_error("pd_ggs_set_matches: invalid arguments (M=%lld n_frames=%d h=%d w=%d; n_frames <= %d)",
                     (long long)M, n_frames, height, width, std::min(eng->ggs_max_frames, eng->max_N));
        return PD_ERR_INVALID_ARG;
    }
    PdSeqTables t;
    PD_TRY(pd_build_seq_tables(kp1, kp2, i12, M, n_frames, t));
    PdBlobArrays o;
    const std::vector<char> host = pack_tables(t, o);
    if (h.blob_bytes < host.size()) {
        pd_ggs_free_seq(h);
        PD_HIP_CHECK(hipMalloc(&h.blob, host.size()));
        h.blob_bytes = host.size();
    }
    memset(&h.desc, 0, sizeof(h.desc));
    PD_HIP_CHECK(hipMemcpy(h.blob, host.data(), host.size(), hipMemcpyHostToDevice));
    pd_desc_point_into(h.desc, (char *)h.blob, o);
    h.desc.n_pchunks = t.n_pchunks;
    h.desc.single_item_pairs = t.single_item_pairs;
    h.desc.n_litems = (int)t.litems.size();
    h.desc.n_lwaves = (int)t.lwave.size();
    h.desc.l_item_len = t.l_item_len;
    h.desc.l_max_steps = t.l_max_steps;
    h.desc.M = (int)M;
    h.desc.n_pairs = (int)t.pair_ij.size();
    h.desc.n_items = (int)t.items.size();
    h.desc.n_frames = n_frames;
    h.desc.sc = (float)std::min(height, width) / 2.0f;   // opencv_from_cameras_projection scale
    h.desc.cx = (float)width / 2.0f;
    h.desc.cy = (float)height / 2.0f;
    h.max_item_len = t.max_item_len;
    h.max_deg = t.max_deg;
    return upload_seq_desc(eng, seq);
}
