// pd_cameras.hip -- ground-truth camera normalisation (include/pd_engine_cameras.h):
//   util/normalize_cameras.py:52-72     compute_optical_axis_intersection
//   util/normalize_cameras.py:75-114    normalize_cameras
//   util/normalize_cameras.py:118-128   normalize_Trans
//   util/normalize_cameras.py:132-148   first_camera_transform
// and, fused, util/camera_transform.py:108-129 camera_to_pose_encoding of the result (pd_pose_encode.h).
//
// One workgroup of PD_CAM_THREADS threads per sequence; thread t owns frames t, t + PD_CAM_THREADS, ...  A few microseconds of latency,
// not a throughput kernel: everything is fp64 and rounded once on store, which costs nothing here and gives a result closer to the exact
// one than the reference's own fp32 arithmetic.
//
// Order of the sums: a thread adds its frames in ascending order, a wave adds its lanes by a fixed shuffle tree, thread 0 adds the waves
// in ascending order through LDS.  The order depends on the sequence's frame count alone (not on N, B or the slot), no atomics.
//
// In place (R_out == R, T_out == T): frame 0 is the only frame other threads need, and it goes through LDS before the first barrier;
// every other frame is read and written by its owner alone, each pass reading it before the one store at the end.  This rests on the
// three frame loops of the kernel keeping ONE frame-to-thread mapping (i = tid, tid + PD_CAM_THREADS, ...): a pass that assigned frames
// differently would read rows another thread has already overwritten, and only the in-place case would show it.
#include "pd_internal.h"
#include "pd_pose_encode.h"
#include "../../include/pd_engine_cameras.h"

#define PD_CAM_THREADS 256
#define PD_CAM_WAVES (PD_CAM_THREADS / PD_WAVE)
#define PD_CAM_NSUM 10            // six of A, three of b, ||T||_F^2
#define PD_CAM_RANK_TOL 1e-10     // smallest Cholesky pivot over trace(A): the rule and its reasons are in include/pd_engine_cameras.h

struct PdCamArgs {
    const float *R, *T, *focal;
    const int32_t *n_frames;
    float *R_out, *T_out, *enc, *p_out, *scale_out, *dist, *foot, *axis;
    int32_t *status;
    int N, scale_mode, first_camera, normalize_T;
    float fl_bias, fl_min, fl_max;
};

struct PdCamShared {
    double part[PD_CAM_WAVES][PD_CAM_NSUM];
    double p[3], R0[9], T0[3], T0s[3];   // the intersection; frame 0 as given; frame 0's T after the scaling stage
    double div, s;                       // divisors of the scaling stage and of normalize_T
    int status, use_p;
};

// sum of v[k] over the workgroup, valid in thread 0 after the call (contains one barrier; sh.part must not be in use)
template <int K>
__device__ __forceinline__ void pd_cam_block_sum(double (&v)[K], PdCamShared &sh) {
    const int lane = threadIdx.x & (PD_WAVE - 1), wave = threadIdx.x / PD_WAVE;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = PD_WAVE / 2; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, PD_WAVE);
        if (lane == 0) sh.part[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = sh.part[0][k];
#pragma unroll
            for (int w = 1; w < PD_CAM_WAVES; ++w) t += sh.part[w][k];
            v[k] = t;
        }
    }
}

__device__ __forceinline__ void pd_cam_load(const PdCamArgs &a, size_t row, double (&R)[9], double (&T)[3]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double)a.R[row * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) T[k] = (double)a.T[row * 3 + k];
}

// camera centre C = -T R^T and the l2-normalised third column r of R
__device__ __forceinline__ void pd_cam_axis(const double (&R)[9], const double (&T)[3], double (&C)[3], double (&r)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) C[j] = -(T[0] * R[j * 3 + 0] + T[1] * R[j * 3 + 1] + T[2] * R[j * 3 + 2]);
    const double d0 = R[2], d1 = R[5], d2 = R[8];
    const double inv = 1.0 / sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    r[0] = d0 * inv;
    r[1] = d1 * inv;
    r[2] = d2 * inv;
}

// the scaling stage and first_camera_transform of one frame (normalize_T's division comes after)
__device__ __forceinline__ void pd_cam_frame(const double (&R)[9], const double (&T)[3], const PdCamShared &sh, int first_camera,
                                             double (&Ro)[9], double (&To)[3]) {
    double T1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v = T[c];
        if (sh.use_p) v += sh.p[0] * R[c] + sh.p[1] * R[3 + c] + sh.p[2] * R[6 + c];   // Translate(p) in front of the world-to-view transform
        T1[c] = v / sh.div;
    }
    if (first_camera == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Ro[k] = R[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) To[c] = T1[c];
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) Ro[a * 3 + c] = sh.R0[a] * R[c] + sh.R0[3 + a] * R[3 + c] + sh.R0[6 + a] * R[6 + c];   // R_0^T R_i
#pragma unroll
    for (int c = 0; c < 3; ++c)
        To[c] = first_camera == 1 ? T1[c] - (sh.T0s[0] * Ro[c] + sh.T0s[1] * Ro[3 + c] + sh.T0s[2] * Ro[6 + c]) : T1[c];
}

__device__ __forceinline__ bool pd_cam_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for inf and NaN

// thread 0: status, p and the scaling divisor from the reduced sums (acc: a00 a01 a02 a11 a12 a22 | b0 b1 b2 | ||T||_F^2)
__device__ __forceinline__ void pd_cam_decide(const double (&acc)[PD_CAM_NSUM], int bad, int scale_mode, PdCamShared &sh) {
    int status = PD_CAM_OK, use_p = 0;
    double div = 1.0, p[3] = {0.0, 0.0, 0.0};
    const double root_t = sqrt(sqrt(acc[9]));   // sqrt of the Frobenius norm (normalize_cameras.py:96-97, :104-105)
    bool sums_finite = true;                    // finite inputs can still give NaN sums: a zero third column has no direction (0 / 0)
#pragma unroll
    for (int k = 0; k < PD_CAM_NSUM; ++k) sums_finite = sums_finite && pd_cam_finite(acc[k]);
    if (bad || !sums_finite) {
        status = PD_CAM_NON_FINITE;
    } else if (scale_mode == 1) {
        // Cholesky of the symmetric positive semi-definite A, pivots d0, d1, d2
        const double a00 = acc[0], a01 = acc[1], a02 = acc[2], a11 = acc[3], a12 = acc[4], a22 = acc[5];
        const double tol = PD_CAM_RANK_TOL * (a00 + a11 + a22);
        const double d0 = a00, l00 = sqrt(d0), l10 = a01 / l00, l20 = a02 / l00;
        const double d1 = a11 - l10 * l10, l11 = sqrt(d1), l21 = (a12 - l20 * l10) / l11;
        const double d2 = a22 - l20 * l20 - l21 * l21, l22 = sqrt(d2);
        if (!(d0 > tol && d1 > tol && d2 > tol)) {
            status = PD_CAM_RANK;
        } else {
            const double y0 = acc[6] / l00, y1 = (acc[7] - l10 * y0) / l11, y2 = (acc[8] - l20 * y0 - l21 * y1) / l22;
            p[2] = y2 / l22;
            p[1] = (y1 - l21 * p[2]) / l11;
            p[0] = (y0 - l10 * p[1] - l20 * p[2]) / l00;
            if (!(pd_cam_finite(p[0]) && pd_cam_finite(p[1]) && pd_cam_finite(p[2]))) {
                status = PD_CAM_NON_FINITE;                                    // the reference's ValueError("p_intersect is NaN")
                p[0] = p[1] = p[2] = 0.0;
            } else {
                double C0[3], r0[3];
                pd_cam_axis(sh.R0, sh.T0, C0, r0);
                const double e0 = p[0] - C0[0], e1 = p[1] - C0[1], e2 = p[2] - C0[2];
                const double dist0 = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
                if (dist0 == 0.0) {                                             // the reference's degenerate case
                    if (root_t > 0.0 && pd_cam_finite(root_t)) {
                        status = PD_CAM_ZERO_SCALE;
                        div = root_t;
                    } else {
                        status = PD_CAM_NON_FINITE;
                    }
                } else if (pd_cam_finite(dist0)) {
                    div = dist0;
                    use_p = 1;
                } else {
                    status = PD_CAM_NON_FINITE;
                }
            }
        }
    } else if (scale_mode == 2) {
        if (root_t > 0.0 && pd_cam_finite(root_t)) div = root_t;
        else status = PD_CAM_NON_FINITE;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sh.p[k] = p[k];
        double v = sh.T0[k];
        if (use_p) v += p[0] * sh.R0[k] + p[1] * sh.R0[3 + k] + p[2] * sh.R0[6 + k];
        sh.T0s[k] = v / div;
    }
    sh.div = div;
    sh.s = 1.0;
    sh.status = status;
    sh.use_p = use_p;
}

__global__ __launch_bounds__(PD_CAM_THREADS) void pd_normalize_cameras_kernel(const PdCamArgs a) {
    __shared__ PdCamShared sh;
    const int tid = threadIdx.x, b = blockIdx.x, N = a.N;
    const int n = a.n_frames ? a.n_frames[b] : N;
    const size_t base = (size_t)b * N;
    const bool counted = n >= 1 && n <= N;

    // ---- pass 1: the sums, frame 0 into LDS ----
    if (counted) {
        double acc[PD_CAM_NSUM];
#pragma unroll
        for (int k = 0; k < PD_CAM_NSUM; ++k) acc[k] = 0.0;
        int bad = 0;
        for (int i = tid; i < n; i += PD_CAM_THREADS) {
            double R[9], T[3];
            pd_cam_load(a, base + i, R, T);
#pragma unroll
            for (int k = 0; k < 9; ++k) bad |= !pd_cam_finite(R[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) bad |= !pd_cam_finite(T[k]);
            if (i == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) sh.R0[k] = R[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) sh.T0[k] = T[k];
            }
            if (a.scale_mode == 1) {
                double C[3], r[3];
                pd_cam_axis(R, T, C, r);
                const double rc = r[0] * C[0] + r[1] * C[1] + r[2] * C[2];
                acc[0] += 1.0 - r[0] * r[0];
                acc[1] -= r[0] * r[1];
                acc[2] -= r[0] * r[2];
                acc[3] += 1.0 - r[1] * r[1];
                acc[4] -= r[1] * r[2];
                acc[5] += 1.0 - r[2] * r[2];
                acc[6] += C[0] - r[0] * rc;
                acc[7] += C[1] - r[1] * rc;
                acc[8] += C[2] - r[2] * rc;
            }
            acc[9] += T[0] * T[0] + T[1] * T[1] + T[2] * T[2];
        }
        bad = __syncthreads_or(bad);
        pd_cam_block_sum(acc, sh);
        if (tid == 0) pd_cam_decide(acc, bad, a.scale_mode, sh);
    } else if (tid == 0) {
        sh.status = PD_CAM_BAD_COUNT;
        sh.p[0] = sh.p[1] = sh.p[2] = 0.0;
        sh.div = 0.0;
        sh.s = 1.0;
        sh.use_p = 0;
    }
    __syncthreads();
    const int status = sh.status;
    const int n_real = counted ? n : 0;
    const bool solved = status <= PD_CAM_ZERO_SCALE;

    // ---- pass 2 (normalize_T): ||T[1:]||_F^2 of the transformed translations ----
    if (solved && a.normalize_T && n_real > 1) {
        double ss[1] = {0.0};
        for (int i = tid; i < n_real; i += PD_CAM_THREADS) {
            if (i == 0) continue;
            double R[9], T[3], Ro[9], To[3];
            pd_cam_load(a, base + i, R, T);
            pd_cam_frame(R, T, sh, a.first_camera, Ro, To);
            ss[0] += To[0] * To[0] + To[1] * To[1] + To[2] * To[2];
        }
        pd_cam_block_sum(ss, sh);
        if (tid == 0) {
            const double v = sqrt(ss[0]) / sqrt((double)(n_real - 1)) / 2.0;
            sh.s = v != v ? v : fmin(fmax(v, 0.01), 100.0);          // torch.clamp: NaN stays NaN
        }
        __syncthreads();
    }
    const double s = sh.s;
    const bool diag = solved && a.scale_mode == 1;

    // ---- pass 3: every row of every output ----
    for (int i = tid; i < N; i += PD_CAM_THREADS) {
        const size_t row = base + i;
        float Rf[9], Tf[3], dist = 0.0f, foot[3] = {0.0f, 0.0f, 0.0f}, axis[3] = {0.0f, 0.0f, 0.0f};
        const bool real = i < n_real;
        if (real && solved) {
            double R[9], T[3], Ro[9], To[3];
            pd_cam_load(a, row, R, T);
            pd_cam_frame(R, T, sh, a.first_camera, Ro, To);
#pragma unroll
            for (int k = 0; k < 9; ++k) Rf[k] = (float)Ro[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) Tf[k] = (float)(To[k] / s);
            if (diag) {
                double C[3], r[3];
                pd_cam_axis(R, T, C, r);
                const double e0 = sh.p[0] - C[0], e1 = sh.p[1] - C[1], e2 = sh.p[2] - C[2];
                const double along = e0 * r[0] + e1 * r[1] + e2 * r[2];
                dist = (float)sqrt(e0 * e0 + e1 * e1 + e2 * e2);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    foot[k] = (float)(C[k] + along * r[k]);
                    axis[k] = (float)r[k];
                }
            }
        } else if (real) {                                           // status 2, 3: the inputs, bit for bit
#pragma unroll
            for (int k = 0; k < 9; ++k) Rf[k] = a.R[row * 9 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) Tf[k] = a.T[row * 3 + k];
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Rf[k] = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) Tf[k] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) a.R_out[row * 9 + k] = Rf[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.T_out[row * 3 + k] = Tf[k];
        if (a.enc) {
            float e[9];
            if (real) {
                const float f[2] = {a.focal[row * 2 + 0], a.focal[row * 2 + 1]};
                pd_camera_to_pose_row(Rf, Tf, f, a.fl_bias, a.fl_min, a.fl_max, e);
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) e[k] = 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) a.enc[row * 9 + k] = e[k];
        }
        if (a.dist) a.dist[row] = dist;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (a.foot) a.foot[row * 3 + k] = foot[k];
            if (a.axis) a.axis[row * 3 + k] = axis[k];
        }
    }
    if (tid == 0) {
        a.status[b] = status;
        if (a.scale_out) a.scale_out[b] = status <= PD_CAM_ZERO_SCALE ? (float)sh.div : (status == PD_CAM_BAD_COUNT ? 0.0f : 1.0f);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (a.p_out) a.p_out[(size_t)b * 3 + k] = diag ? (float)sh.p[k] : 0.0f;
    }
}

extern "C" int pd_normalize_cameras(const float *R, const float *T, int B, int N, const int32_t *n_frames, const pd_cam_norm_cfg *cfg,
                                    float *R_out, float *T_out, const float *focal, float log_focal_length_bias, float min_focal_length,
                                    float max_focal_length, float *enc_out, float *p_intersect_out, float *scale_out, float *dist_out,
                                    float *foot_out, float *axis_out, int32_t *status_out, void *stream) {
    const char *null_arg = !R ? "R" : !T ? "T" : !cfg ? "cfg" : !R_out ? "R_out" : !T_out ? "T_out" : !status_out ? "status_out" : nullptr;
    if (null_arg) {
        pd_set_error("pd_normalize_cameras: %s is NULL", null_arg);
        return PD_ERR_INVALID_ARG;
    }
    if (B < 0 || N < 1) {
        pd_set_error("pd_normalize_cameras: B = %d must be >= 0 and N = %d must be >= 1", B, N);
        return PD_ERR_INVALID_ARG;
    }
    if (enc_out && !focal) {
        pd_set_error("pd_normalize_cameras: enc_out needs focal (the encoding holds the focal length)");
        return PD_ERR_INVALID_ARG;
    }
    if (cfg->scale_mode < 0 || cfg->scale_mode > 2 || cfg->first_camera < 0 || cfg->first_camera > 2 || cfg->normalize_T < 0 ||
        cfg->normalize_T > 1) {
        pd_set_error("pd_normalize_cameras: cfg holds an unknown mode (scale_mode %d of 0..2, first_camera %d of 0..2, normalize_T %d of 0..1)",
                     cfg->scale_mode, cfg->first_camera, cfg->normalize_T);
        return PD_ERR_INVALID_ARG;
    }
    if (B == 0) return PD_OK;
    PdCamArgs a;
    a.R = R, a.T = T, a.focal = focal, a.n_frames = n_frames;
    a.R_out = R_out, a.T_out = T_out, a.enc = enc_out, a.p_out = p_intersect_out, a.scale_out = scale_out;
    a.dist = dist_out, a.foot = foot_out, a.axis = axis_out, a.status = status_out;
    a.N = N, a.scale_mode = cfg->scale_mode, a.first_camera = cfg->first_camera, a.normalize_T = cfg->normalize_T;
    a.fl_bias = log_focal_length_bias, a.fl_min = min_focal_length, a.fl_max = max_focal_length;
    hipLaunchKernelGGL(pd_normalize_cameras_kernel, dim3(B), dim3(PD_CAM_THREADS), 0, (hipStream_t)stream, a);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}
