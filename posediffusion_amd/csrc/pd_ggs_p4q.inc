// P4 of one GGS iteration for pd_ggs_kernel and pd_ggs_lane_kernel (textually included; the two-hop kernel keeps pd_ggs_p4.inc): wave 0,
// lane = frame.  The backward phase already turned the per-frame sums into dL/dq (through the Jacobian an idle wave prepared, jac_all)
// and the dL/dA partials arrive as one float4 per row wave, so what is left here is the short tail of GGS_optimize
// (geometry_guided_sampling.py:104-122): totals, early exit, the focal-length chain, masked-norm clip, momentum SGD, decode.
// In scope: L, P, S, D, N (the sequence's own frame count; P.N is the row stride of x and grad_out), b, wg, lane, wave, inv_M, stepped, trace_row.  Leaves {printed statistic, valid count, loss} in L.ctl[5..7].
// Reads L.gq [frame][8] = {dL/dq (4), dL/dT (3), -} (zeros where the stage leaves R / T alone), L.gA[0..3] (dL/dA totals, update_FL
// only: ga_parts partials of 4), L.cam[6] (sum s), L.cam[7] (n valid), L.ctl[2] (sum min(s, max)).
            if (wave == 0 && (PD_GGS_ABLATE & 8)) {
                if (lane == 0) L.ctl[0] = 0.0f;
            } else if (wave == 0) {
                float xr[9], mom[9];
                params_load(L.xst, lane, xr);
                params_load(L.mst, lane, mom);
                const float s_sum = L.cam[6], s_cnt = L.cam[7], s_cl = L.ctl[2];
                const float last_print = s_cl * inv_M;
                if (lane == 0) {
                    L.ctl[5] = last_print;
                    L.ctl[6] = s_cnt;
                }
                // len(valid) / n_frames < min_matches -> break   (geometry_guided_sampling.py:104-108)
                const bool done = (!P.eval_only) && P.min_matches > 0 && (s_cnt < (float)P.min_matches * (float)N);
                if (!done) {
                    const float inv_cnt = pd_rcp(s_cnt);
                    const float loss = s_sum * inv_cnt;                   // valid.mean()  :110
                    if (lane == 0) L.ctl[7] = loss;
                    float g[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c) g[c] = 0.0f;
                    if (lane < N) {
                        const float4 gq4 = *(const float4 *)&L.gq[lane * 8], gt4 = *(const float4 *)&L.gq[lane * 8 + 4];
                        g[0] = gt4.x * inv_cnt;
                        g[1] = gt4.y * inv_cnt;
                        g[2] = gt4.z * inv_cnt;
                        g[3] = gq4.x * inv_cnt;
                        g[4] = gq4.y * inv_cnt;
                        g[5] = gq4.z * inv_cnt;
                        g[6] = gq4.w * inv_cnt;
                        if (S.update_FL) {
                            // A00 = 1/(f sc), A02 = -cx/(f sc): dA/df ; mean over frames ; exp ; clamp mask
                            // dL/dA totals: the partials of the (<= 6) waves that summed the frames' rows, in wave order
                            float4 ga = *(const float4 *)&L.gA[0];
                            for (int w = 1; w < ga_parts; ++w) {
                                const float4 p4 = *(const float4 *)&L.gA[w * 4];
                                ga.x += p4.x;
                                ga.y += p4.y;
                                ga.z += p4.z;
                                ga.w += p4.w;
                            }
                            const float fbx = L.cam[4], fby = L.cam[5];
                            int n_op = N;
                            asm volatile("" : "+s"(n_op));            // (not hoisted out of the loop: see decode_all)
                            const float kx = pd_rcp(fbx * fbx * D.sc), ky = pd_rcp(fby * fby * D.sc), rNn = pd_rcp((float)n_op);
                            const float gfx = (ga.y * D.cx - ga.x) * kx;
                            const float gfy = (ga.w * D.cy - ga.z) * ky;
                            const float4 fl4 = *(const float4 *)&L.fl[lane * 4];      // (focal x, y | clamp masks x, y)
                            g[7] = gfx * rNn * fl4.x * fl4.z * inv_cnt;
                            g[8] = gfy * rNn * fl4.y * fl4.w * inv_cnt;
                        }
                    }
                    if (P.eval_only) {
                        if (lane < N) {
                            int lo_ = lane;
                            asm volatile("" : "+v"(lo_));     // address arithmetic of this rare branch stays here (not hoisted: registers)
#pragma unroll
                            for (int c = 0; c < 9; ++c) P.grad_out[((size_t)b * P.N + lo_) * 9 + c] = g[c];
                        }
                        if (lane == 0 && wg == 0) {
                            P.loss_out[b * 4 + 0] = loss;
                            P.loss_out[b * 4 + 1] = s_cnt;
                            P.loss_out[b * 4 + 2] = last_print;
                            P.loss_out[b * 4 + 3] = 0.0f;
                        }
                    } else {
                        // masked-norm clip (:114-121) + SGD momentum step (:122)
                        float gn2 = 0.0f, xn2 = 0.0f;
#pragma unroll
                        for (int c = 0; c < 9; ++c) {
                            gn2 += g[c] * g[c];
                            xn2 += (fabsf(g[c]) > 0.0f) ? xr[c] * xr[c] : 0.0f;
                        }
                        float gsum, xsum;
                        wave_allsum2(gn2, xn2, gsum, xsum);
                        const float gnorm = pd_sqrt(gsum), xnorm = pd_sqrt(xsum);
                        const float max_norm = P.alpha * xnorm * pd_rcp(P.lr);
                        const float coef = fminf(max_norm * pd_rcp(gnorm + 1e-6f), 1.0f);
#pragma unroll
                        for (int c = 0; c < 9; ++c) {
                            const float gc = g[c] * coef;
                            mom[c] = (stepped == 0) ? gc : P.momentum * mom[c] + gc;
                            xr[c] = xr[c] - P.lr * mom[c];
                        }
                        ++stepped;
                        if (P.trace && wg == 0 && trace_row < P.trace_iters) {
                            float *tr = P.trace + ((size_t)b * P.trace_iters + trace_row) * (N * 9 + 3);
                            if (lane < N) {
                                int lo_ = lane;
                                asm volatile("" : "+v"(lo_));
#pragma unroll
                                for (int c = 0; c < 9; ++c) tr[lo_ * 9 + c] = xr[c];
                            }
                            if (lane == 0) {
                                tr[N * 9 + 0] = loss;
                                tr[N * 9 + 1] = s_cnt;
                                tr[N * 9 + 2] = gnorm;
                            }
                        }
                        ++trace_row;
                        params_store(L.xst, lane, xr);
                        params_store(L.mst, lane, mom);
                        // only what this stage moves is decoded again (:144-151 detach the rest)
                        decode_all(L, xr, lane, N, D, S.update_R != 0, S.update_T != 0, S.update_FL != 0);
                    }
                }
                if (lane == 0) L.ctl[0] = (done || P.eval_only) ? 1.0f : 0.0f;
            }
