// P3b, hop 2, the frame gradients and the loss totals of one GGS iteration of pd_ggs_long_kernel and pd_ggs_longm_kernel (textually included by
// both, inside their iteration loop after hop 1): nothing here knows what a slot holds.  Reads xs, epoch, n_inc, wg, k, N, tid, lane, wave, L,
// frame_rows, tot_rows, P; declares `ok`; returns from the kernel when a bounded spin gave up.
            // ---- P3b: the owner of frame n sums that frame's rows in row order and publishes the frame line
            bool ok = true;
            for (int n = wg; n < N; n += k) {
                const int lo = L.incoff[n], cn = L.incoff[n + 1] - lo;   // <= 2 (N - 1) <= 510 rows: PD_GGS_LONG_FRAME_ROWS
                ok = ggs2_gather<1>(xs + (size_t)lo * PD_XCHG_LINE, tid, cn * 8, 8, epoch, frame_rows, 16, P.err_flag) && ok;
                __syncthreads();
                if (tid < 64) {
                    // the frame's rows summed in a FIXED order that does not depend on the workgroup count: the four 16-lane rows of wave 0 each sum
                    // every fourth row (rows p, p + 4, ...: eight LDS reads in flight at a time), then (p0 + p1) + (p2 + p3) on the permlane swaps.
                    // History (tools/ggs_prof_n50.py, round 5): a plain loop over the rows was a chain of <= 63 dependent LDS round trips -- 5 700 of the
                    // 22 100 cycles of an iteration at 50 frames; eight reads in flight on 16 lanes: 3 300; this form: see profiles/round5_ggs_n50_phase_clocks.txt
                    const int c16 = tid & 15, part = tid >> 4;
                    float a = 0.0f;
                    for (int e0 = part; e0 < cn; e0 += 32) {              // (cn <= 2 (N - 1) rows; the loop bound differs between the four parts: no cross-lane operation inside)
                        float r[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) r[u] = e0 + 4 * u < cn ? frame_rows[(e0 + 4 * u) * 16 + c16] : 0.0f;
#pragma unroll
                        for (int u = 0; u < 8; ++u) a += r[u];
                    }
                    a = add_xor16(a);
                    a = add_xor32(a);
                    if (tid < 16)
                        __hip_atomic_store(xs + (size_t)(n_inc + k + n) * PD_XCHG_LINE + tid, ((u64)epoch << 32) | (u64)__float_as_uint(a),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();
            }
            PD_PROF2H(q4);
            // ---- hop 2: everybody gathers the N frame lines and the k totals lines
            ok = ggs2_gather<2>(xs + (size_t)(n_inc + k) * PD_XCHG_LINE, tid, N * 8, 8, epoch, L.psum, 16, P.err_flag) && ok;
            ok = ggs2_gather<1>(xs + (size_t)n_inc * PD_XCHG_LINE, tid, k * 2, 2, epoch, tot_rows, 4, P.err_flag) && ok;
            if (!ok) {
                atomicOr(P.err_flag, 1u);
                L.ctl[1] = 1.0f;
            }
            __syncthreads();
            if (L.ctl[1] != 0.0f) return;
            PD_PROF2H(q5);
            // per-frame gradients back through tc = D T and Rc[a][b] = D[a] R[b][a]; totals in workgroup order
            for (int q = tid; q < N * 16; q += PD_GGS_THREADS) {
                const int n = q >> 4, c = q & 15;
                const float v = L.psum[n * 16 + c];
                if (c < 9) {
                    const int aa = c / 3, bb = c % 3;
                    L.gR[n * 9 + bb * 3 + aa] = (aa < 2 ? -v : v);
                } else if (c < 12) {
                    L.gT[n * 3 + (c - 9)] = (c - 9 < 2 ? -v : v);
                } else {
                    L.gA[n * 4 + (c - 12)] = v;
                }
            }
            if (wave >= PD_GGS_WAVES - 3) {                 // one wave per total (round 5: one wave ran the 3 x ceil(k / 64) reductions back to back)
                const int c = wave - (PD_GGS_WAVES - 3);
                float t = 0.0f;
                for (int w0 = 0; w0 < k; w0 += 64) {      // fixed order: 64 workgroups at a time, tree inside
                    const int w = w0 + lane;
                    t += wave_allsum(w < k ? tot_rows[w * 4 + c] : 0.0f);
                }
                if (lane == 0) *(c == 0 ? &L.cam[6] : (c == 1 ? &L.cam[7] : &L.ctl[2])) = t;
            }
            __syncthreads();
            PD_PROF2H(q6);
