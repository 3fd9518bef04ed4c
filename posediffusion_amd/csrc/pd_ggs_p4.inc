// P4 of one GGS iteration (textually included by the GGS kernels of pd_ggs.hip): wave 0, lane = frame.
// In scope: L, P, S, D, N (the sequence's own frame count; P.N is the row stride of x and grad_out), b, wg, lane, wave, inv_M, stepped, trace_row, last_print, last_cnt, last_loss.  The parameters xr[9]
// and the momentum mom[9] of frame `lane` are loaded from / stored back to L.xst / L.mst here.
// Reads the per-frame gradients L.gR / L.gT / L.gA and the totals L.cam[6] (sum s), L.cam[7] (n valid), L.ctl[2].
            // ---- P4 (wave 0): totals, early exit, quaternion/focal chain, clip, momentum SGD ----
            if (wave == 0) {
                float xr[9], mom[9];
                params_load(L.xst, lane, xr);
                params_load(L.mst, lane, mom);
                const float s_sum = L.cam[6], s_cnt = L.cam[7], s_cl = L.ctl[2];
                float ga[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (S.update_FL) {                                        // (wave-uniform; only the focal-length chain reads them: 300 of the 700 iterations)
#pragma unroll
                    for (int c = 0; c < 4; ++c) ga[c] = wave_allsum(lane < N ? L.gA[lane * 4 + c] : 0.0f);
                }
                last_print = s_cl * inv_M;
                last_cnt = s_cnt;
                // len(valid) / n_frames < min_matches -> break   (geometry_guided_sampling.py:104-108)
                const bool done = (!P.eval_only) && P.min_matches > 0 && (s_cnt < (float)P.min_matches * (float)N);
                if (!done) {
                    const float inv_cnt = pd_rcp(s_cnt);
                    const float loss = s_sum * inv_cnt;                   // valid.mean()  :110
                    last_loss = loss;
                    float g[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c) g[c] = 0.0f;
                    if (lane < N) {
                        if (S.update_T) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) g[c] = L.gT[lane * 3 + c] * inv_cnt;
                        }
                        if (S.update_R) {
                            // R = I + two_s * Pm(q): chain rule to the (unnormalised) quaternion
                            const float r = xr[3], i = xr[4], j = xr[5], kq = xr[6];
                            const float n2 = r * r + i * i + j * j + kq * kq;
                            const float rn2 = pd_rcp(n2);
                            const float ts = 2.0f * rn2;
                            float gR[9];
#pragma unroll
                            for (int c = 0; c < 9; ++c) gR[c] = L.gR[lane * 9 + c];
                            const float gts = gR[0] * -(j * j + kq * kq) + gR[1] * (i * j - kq * r) + gR[2] * (i * kq + j * r) +
                                              gR[3] * (i * j + kq * r) + gR[4] * -(i * i + kq * kq) + gR[5] * (j * kq - i * r) +
                                              gR[6] * (i * kq - j * r) + gR[7] * (j * kq + i * r) + gR[8] * -(i * i + j * j);
                            float h[9];
#pragma unroll
                            for (int c = 0; c < 9; ++c) h[c] = ts * gR[c];
                            const float qs = gts * (-4.0f * rn2 * rn2);
                            const float gq_r = -kq * h[1] + j * h[2] + kq * h[3] - i * h[5] - j * h[6] + i * h[7] + qs * r;
                            const float gq_i = j * h[1] + kq * h[2] + j * h[3] - 2.0f * i * h[4] - r * h[5] + kq * h[6] +
                                               r * h[7] - 2.0f * i * h[8] + qs * i;
                            const float gq_j = -2.0f * j * h[0] + i * h[1] + r * h[2] + i * h[3] + kq * h[5] - r * h[6] +
                                               kq * h[7] - 2.0f * j * h[8] + qs * j;
                            const float gq_k = -2.0f * kq * h[0] - r * h[1] + i * h[2] + r * h[3] - 2.0f * kq * h[4] +
                                               j * h[5] + i * h[6] + j * h[7] + qs * kq;
                            g[3] = gq_r * inv_cnt;
                            g[4] = gq_i * inv_cnt;
                            g[5] = gq_j * inv_cnt;
                            g[6] = gq_k * inv_cnt;
                        }
                        if (S.update_FL) {
                            // A00 = 1/(f sc), A02 = -cx/(f sc): dA/df ; mean over frames ; exp ; clamp mask
                            const float fbx = L.cam[4], fby = L.cam[5];
                            const float kx = pd_rcp(fbx * fbx * D.sc), ky = pd_rcp(fby * fby * D.sc), rNn = pd_rcp((float)N);
                            const float gfx = (ga[1] * D.cx - ga[0]) * kx;
                            const float gfy = (ga[3] * D.cy - ga[2]) * ky;
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
                        const float gnorm = pd_sqrt(wave_allsum(gn2));
                        const float xnorm = pd_sqrt(wave_allsum(xn2));
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
                        // only what this stage moves is decoded again (:144-151 detach the rest; the parameters a stage leaves alone keep their bits)
                        decode_all(L, xr, lane, N, D, S.update_R != 0, S.update_T != 0, S.update_FL != 0);
                    }
                }
                if (lane == 0) L.ctl[0] = (done || P.eval_only) ? 1.0f : 0.0f;
            }
