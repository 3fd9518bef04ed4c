// pd_images.hip -- training images of a whole batch (include/pd_engine_images.h): the crop, antialiased resize
// and colour draw of datasets/co3d_v2.py:get_data (:149, :205-214, :365-368), from decoded uint8 frames to [F, 3, S, S] fp32.
//
// Two kernels per call.
//   pd_img_resize_kernel   one workgroup per (band of output rows, frame).  The band's source rows are walked ONCE in chunks: a chunk's
//       picture bytes go to LDS with 16-byte loads (the unaligned head and tail of a row byte by byte), the horizontal pass turns them
//       into rows of S x 3 floats in LDS, the vertical pass adds those into the band's accumulators in LDS (each owned by one thread).
//       Neighbouring bands share the rows under the filter's overlap; with 8-row bands at S = 224 that is one row in eight read twice.
//       The weights are integers over a common denominator (see the header), formed on the fly from a running numerator: no weight table,
//       tap loops of any length; the sums stay un-normalised whole numbers (exact in fp32 while below 2^24) until the epilogue's one
//       division by (sum of the column's weights) x (sum of the row's weights) x 255.  The epilogue divides, stores, and -- for a frame
//       whose colour entry jitters -- applies the operations that precede contrast and leaves the band's fp64 sum of grey values in the
//       workspace.
//   pd_img_colour_kernel   one thread per output pixel of the frames that have a colour entry with something to do; the contrast mean is
//       the bands' partials added in ascending order.  Other frames are not touched: they keep the bits of the resize.
// No atomics; every order of summation is a function of the frame's own numbers and S.
//
// Contraction per source expression (Makefile): the colour operations are evaluated at two places (the first kernel's grey sums and the
// second kernel) and must agree; every fused multiply-add wanted is written as fmaf.
#include "pd_internal.h"
#include "../../include/pd_engine_images.h"

#define PD_IMG_THREADS 256
#define PD_IMG_WAVES (PD_IMG_THREADS / PD_WAVE)
#define PD_IMG_LDS_BYTES 65536
#define PD_IMG_STAGE_BYTES 18688      // >= 3 PD_IMG_MAX_SIDE + 32: one staged row at the longest side, head and tail padding included
#define PD_IMG_FIXED_BYTES 256        // row tables of the band and the reduction scratch
#define PD_IMG_MAX_BAND 16
#define PD_IMG_MAX_HROWS 32

static_assert(3 * PD_IMG_MAX_SIDE + 32 <= PD_IMG_STAGE_BYTES, "a staged row must fit");
static_assert(3 * PD_IMG_MAX_BAND * 4 + PD_IMG_WAVES * 8 <= PD_IMG_FIXED_BYTES, "fixed LDS region");

// how the LDS left after the staging area is cut for an image size (host; the kernels get the numbers as arguments)
struct PdImgPlan {
    int band, hrows, n_bands;
};
static bool pd_img_plan(int S, PdImgPlan *p) {
    const int col_bytes = 12 * S, row_bytes = 12 * S;   // lo, hi, tot per column; 3 S floats per row
    const int avail = (PD_IMG_LDS_BYTES - PD_IMG_STAGE_BYTES - PD_IMG_FIXED_BYTES - col_bytes) / row_bytes;
    if (avail < 2) return false;
    p->band = avail / 2 < PD_IMG_MAX_BAND ? avail / 2 : PD_IMG_MAX_BAND;
    if (p->band > S) p->band = S;
    p->hrows = avail - p->band < PD_IMG_MAX_HROWS ? avail - p->band : PD_IMG_MAX_HROWS;
    p->n_bands = (S + p->band - 1) / p->band;
    return true;
}
static_assert((PD_IMG_LDS_BYTES - PD_IMG_STAGE_BYTES - PD_IMG_FIXED_BYTES - 12 * PD_IMG_MAX_SIZE) / (12 * PD_IMG_MAX_SIZE) >= 2,
              "PD_IMG_MAX_SIZE must leave one accumulator row and one horizontal row");

// ---- the filter: exact integer windows and weights --------------------------------------------------------------------------------
// Everything is formed from side / G and S / G, G = gcd(side, S), and halved once more where that is exact (the header's n(i, j) are all
// multiples of G, and of 2 G when (S - side) / G is even): the ratios are the header's, the integers are the smallest there are.  A
// crop with side == S has the weights 1 and 0.
struct PdImgFilter {
    int side, Sr, sider, sh;   // the crop's side; S / G, side / G; 1 where the halving applies
    int D, step;               // 2 max(Sr, sider) >> sh: the weight at distance 0; 2 Sr >> sh: what one tap adds to the numerator
};
__device__ __forceinline__ PdImgFilter pd_img_filter(int side, int S) {
    int a = side, b = S;
    while (b) {
        const int t = a % b;
        a = b, b = t;
    }
    PdImgFilter f;
    f.side = side, f.Sr = S / a, f.sider = side / a;
    f.sh = ((f.Sr - f.sider) & 1) ? 0 : 1;
    f.D = (2 * (f.Sr > f.sider ? f.Sr : f.sider)) >> f.sh;
    f.step = (2 * f.Sr) >> f.sh;
    return f;
}
__device__ __forceinline__ int pd_img_floordiv(int a, int b) {   // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
// taps [lo, hi) of output index i
__device__ __forceinline__ void pd_img_window(const PdImgFilter &f, int i, int &lo, int &hi) {
    const int c2 = f.sider * (2 * i + 1), D2 = 2 * (f.Sr > f.sider ? f.Sr : f.sider);   // 2 S c and 2 S support, over G
    lo = pd_img_floordiv(c2 - D2 + f.Sr, 2 * f.Sr);
    hi = pd_img_floordiv(c2 + D2 + f.Sr, 2 * f.Sr);
    lo = lo < 0 ? 0 : lo;
    hi = hi > f.side ? f.side : hi;
}
// numerator of tap j's distance from the centre of output i (an even number where sh = 1); it grows by f.step per tap
__device__ __forceinline__ int pd_img_num(const PdImgFilter &f, int i, int j) { return ((2 * j + 1) * f.Sr - f.sider * (2 * i + 1)) >> f.sh; }
__device__ __forceinline__ float pd_img_weight(int D, int num) {
    const int n = D - (num < 0 ? -num : num);
    return (float)(n < 0 ? 0 : n);
}
// sum of a window's weights: below 2^32 (at most PD_IMG_MAX_SIDE + 2 taps of at most 2 PD_IMG_MAX_SIDE each), kept as an integer
__device__ __forceinline__ uint32_t pd_img_window_total(const PdImgFilter &f, int i, int lo, int hi) {
    uint32_t tot = 0;
    int num = pd_img_num(f, i, lo);
    for (int j = lo; j < hi; ++j, num += f.step) {
        const int n = f.D - (num < 0 ? -num : num);
        tot += (uint32_t)(n < 0 ? 0 : n);
    }
    return tot;
}

// ---- colour operations (torchvision's float-tensor definitions) -------------------------------------------------------------------
__device__ __forceinline__ float pd_img_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float pd_img_grey(const float (&x)[3]) { return 0.2989f * x[0] + 0.587f * x[1] + 0.114f * x[2]; }

__device__ __forceinline__ void pd_img_hue(float (&x)[3], float f) {
    const float r = x[0], g = x[1], b = x[2];
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float div = eqc ? 1.0f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = 2.0f + rc - bc;
    else h = 4.0f + gc - rc;
    h = h / 6.0f + 1.0f;
    h = h - floorf(h);            // fmod(., 1) of a positive number
    h = h + f;
    h = h - floorf(h);            // (h + f) mod 1, the sign of the divisor
    const float v = maxc;
    const float h6 = h * 6.0f;
    const float fl = floorf(h6);
    const float fr = h6 - fl;
    int i = (int)fl % 6;
    const float p = pd_img_clamp01(v * (1.0f - s));
    const float q = pd_img_clamp01(v * (1.0f - s * fr));
    const float t = pd_img_clamp01(v * (1.0f - s * (1.0f - fr)));
    x[0] = i == 0 || i == 5 ? v : (i == 1 ? q : (i == 4 ? t : p));
    x[1] = i == 1 || i == 2 ? v : (i == 0 ? t : (i == 3 ? q : p));
    x[2] = i == 3 || i == 4 ? v : (i == 2 ? t : (i == 5 ? q : p));
}

// one jitter operation; `mean` is read by contrast alone
__device__ __forceinline__ void pd_img_op(float (&x)[3], int op, const pd_img_colour &c, float mean) {
    if (op == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = pd_img_clamp01(c.brightness * x[k]);
    } else if (op == 1) {
        const float add = (1.0f - c.contrast) * mean;
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = pd_img_clamp01(c.contrast * x[k] + add);
    } else if (op == 2) {
        const float add = (1.0f - c.saturation) * pd_img_grey(x);
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = pd_img_clamp01(c.saturation * x[k] + add);
    } else {
        pd_img_hue(x, c.hue);
    }
}

// frame and colour entry checks, the same answer in every workgroup of the frame
__device__ __forceinline__ int pd_img_status(const pd_img_frame &fr, const pd_img_colour *colours, int n_colours, int S) {
    if (fr.side < 1 || fr.side > PD_IMG_MAX_SIDE) return PD_IMG_BAD_SIDE;
    if (fr.height < 1 || fr.width < 1 || fr.offset < 0) return PD_IMG_BAD_SIZE;
    if (fr.colour < -1 || fr.colour >= n_colours) return PD_IMG_BAD_COLOUR;
    if (fr.colour >= 0) {
        const pd_img_colour &c = colours[fr.colour];
        if (c.jitter) {
            int seen = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (c.order[k] < 0 || c.order[k] > 3) return PD_IMG_BAD_ORDER;
                seen |= 1 << c.order[k];
            }
            if (seen != 15) return PD_IMG_BAD_ORDER;
        }
        if (c.erase_h != 0) {
            if (c.erase_h < 0 || c.erase_w < 0 || c.erase_top < 0 || c.erase_left < 0 || c.erase_h > S || c.erase_w > S ||
                c.erase_top > S - c.erase_h || c.erase_left > S - c.erase_w)
                return PD_IMG_BAD_ERASE;
        }
    }
    return PD_IMG_OK;
}

struct PdImgArgs {
    const uint8_t *pixels;
    const pd_img_frame *frames;
    const pd_img_colour *colours;
    float *out;
    int32_t *status;
    double *partials;     // [F, n_bands]
    int n_colours, S, band, hrows, n_bands;
    float fill;
};

__global__ __launch_bounds__(PD_IMG_THREADS) void pd_img_resize_kernel(PdImgArgs a) {
    __shared__ __align__(16) unsigned char lds[PD_IMG_LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & (PD_WAVE - 1), wave = tid / PD_WAVE;
    const int f = blockIdx.y, bandi = blockIdx.x, S = a.S;
    const int o0 = bandi * a.band, nrow = (S - o0 < a.band) ? S - o0 : a.band;   // output rows [o0, o0 + nrow)
    const pd_img_frame fr = a.frames[f];
    float *out = a.out + (size_t)f * 3 * S * S;
    const int status = pd_img_status(fr, a.colours, a.n_colours, S);
    if (status != PD_IMG_OK) {
        for (int c = 0; c < 3; ++c)
            for (int e = tid; e < nrow * S; e += PD_IMG_THREADS) out[((size_t)c * S + o0) * S + e] = 0.0f;
        if (tid == 0) {
            a.partials[(size_t)f * a.n_bands + bandi] = 0.0;
            if (bandi == 0) a.status[f] = status;
        }
        return;
    }
    // LDS: staged bytes | row tables, reduction scratch | column tables | accumulators [band][3 S] | horizontal rows [hrows][3 S]
    unsigned char *stage = lds;
    int *row_lo = (int *)(lds + PD_IMG_STAGE_BYTES), *row_hi = row_lo + PD_IMG_MAX_BAND;
    uint32_t *row_tot = (uint32_t *)(row_hi + PD_IMG_MAX_BAND);
    double *red = (double *)(row_tot + PD_IMG_MAX_BAND);
    int *col_lo = (int *)(lds + PD_IMG_STAGE_BYTES + PD_IMG_FIXED_BYTES), *col_hi = col_lo + S;
    uint32_t *col_tot = (uint32_t *)(col_hi + S);
    float *acc = (float *)(col_tot + S);
    float *hbuf = acc + (size_t)a.band * 3 * S;

    const int side = fr.side;
    const PdImgFilter flt = pd_img_filter(side, S);
    const int D = flt.D;
    for (int i = tid; i < S; i += PD_IMG_THREADS) {
        int lo, hi;
        pd_img_window(flt, i, lo, hi);
        col_lo[i] = lo, col_hi[i] = hi;
        col_tot[i] = pd_img_window_total(flt, i, lo, hi);
    }
    if (tid < nrow) {
        int lo, hi;
        pd_img_window(flt, o0 + tid, lo, hi);
        row_lo[tid] = lo, row_hi[tid] = hi;
        row_tot[tid] = pd_img_window_total(flt, o0 + tid, lo, hi);
    }
    for (int e = tid; e < nrow * 3 * S; e += PD_IMG_THREADS) acc[e] = 0.0f;
    __syncthreads();

    // crop columns [jA, jB) lie inside the picture; their bytes are what a row stages
    const long long xl = -(long long)fr.x0, xr = (long long)fr.width - fr.x0;
    const int jA = (int)(xl < 0 ? 0 : (xl > side ? side : xl)), jB = (int)(xr < 0 ? 0 : (xr > side ? side : xr));
    const int span = jB > jA ? jB - jA : 0;
    const int pitch = ((3 * span + 15) / 16 + 1) * 16;            // head (<= 15 bytes) + 3 span bytes, whole 16-byte pieces
    int R = PD_IMG_STAGE_BYTES / pitch;
    R = R < a.hrows ? R : a.hrows;                                 // >= 1: pitch <= 3 PD_IMG_MAX_SIDE + 32
    const uintptr_t base = (uintptr_t)a.pixels + (uintptr_t)fr.offset;
    const int r_begin = row_lo[0], r_end = row_hi[nrow - 1];
    const float invS = 1.0f / (float)S;

    for (int rc = r_begin; rc < r_end; rc += R) {
        const int Rc = r_end - rc < R ? r_end - rc : R;
        // stage: wave w takes the chunk's rows w, w + 4, ...
        if (span > 0) {
            for (int r = wave; r < Rc; r += PD_IMG_WAVES) {
                const long long y = (long long)fr.y0 + rc + r;
                if (y < 0 || y >= fr.height) continue;
                const uintptr_t p0 = base + (uintptr_t)((y * fr.width + fr.x0 + jA) * 3), p1 = p0 + (uintptr_t)(3 * span);
                const uintptr_t al = p0 & ~(uintptr_t)15;
                const int pieces = (int)((p1 - al + 15) >> 4);     // <= pitch / 16
                unsigned char *dst = stage + (size_t)r * pitch;
                for (int k = lane; k < pieces; k += PD_WAVE) {
                    const uintptr_t A = al + ((uintptr_t)k << 4);
                    if (A >= p0 && A + 16 <= p1) {
                        *(uint4 *)(dst + 16 * k) = *(const uint4 *)A;
                    } else {
                        for (int t = 0; t < 16; ++t)
                            if (A + t >= p0 && A + t < p1) dst[16 * k + t] = *(const uint8_t *)(A + t);
                    }
                }
            }
        }
        __syncthreads();
        // horizontal: one (row of the chunk, output column) per thread turn, three channels at once
        for (int idx = tid; idx < Rc * S; idx += PD_IMG_THREADS) {
            const int r = (int)(((float)idx + 0.5f) * invS), i = idx - r * S;
            const long long y = (long long)fr.y0 + rc + r;
            const bool row_in = span > 0 && y >= 0 && y < fr.height;
            const int head = row_in ? (int)((base + (uintptr_t)((y * fr.width + fr.x0 + jA) * 3)) & 15) : 0;
            const unsigned char *src = stage + (size_t)r * pitch + head;
            const int lo = col_lo[i], hi = col_hi[i];
            int num = pd_img_num(flt, i, lo);
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int j = lo; j < hi; ++j, num += flt.step) {
                const float w = pd_img_weight(D, num);
                const bool in = row_in && j >= jA && j < jB;
                const int q = in ? 3 * (j - jA) : 0;
                const float p0 = in ? (float)src[q] : a.fill, p1 = in ? (float)src[q + 1] : a.fill, p2 = in ? (float)src[q + 2] : a.fill;
                s0 = fmaf(w, p0, s0), s1 = fmaf(w, p1, s1), s2 = fmaf(w, p2, s2);
            }
            float *h = hbuf + (size_t)r * 3 * S;     // un-normalised: whole numbers, exact while below 2^24
            h[i] = s0, h[S + i] = s1, h[2 * S + i] = s2;
        }
        __syncthreads();
        // vertical: every accumulator has one owner
        for (int o = 0; o < nrow; ++o) {
            const int lo = row_lo[o] > rc ? row_lo[o] : rc, hi = row_hi[o] < rc + Rc ? row_hi[o] : rc + Rc;
            if (lo >= hi) continue;
            const int num0 = pd_img_num(flt, o0 + o, lo);
            for (int k = tid; k < 3 * S; k += PD_IMG_THREADS) {
                float v = acc[(size_t)o * 3 * S + k];
                int num = num0;
                for (int r = lo; r < hi; ++r, num += flt.step) v = fmaf(pd_img_weight(D, num), hbuf[(size_t)(r - rc) * 3 * S + k], v);
                acc[(size_t)o * 3 * S + k] = v;
            }
        }
        __syncthreads();
    }

    // epilogue: normalise, divide by 255, store; grey sum of what precedes contrast
    const bool want_mean = fr.colour >= 0 && a.colours[fr.colour].jitter != 0;
    pd_img_colour col;
    int n_pre = 0;
    if (want_mean) {
        col = a.colours[fr.colour];
        n_pre = col.order[0] == 1 ? 0 : (col.order[1] == 1 ? 1 : (col.order[2] == 1 ? 2 : 3));   // a checked permutation: contrast is there
    }
    float gsum = 0.0f;
    for (int idx = tid; idx < nrow * S; idx += PD_IMG_THREADS) {
        const int o = (int)(((float)idx + 0.5f) * invS), i = idx - o * S;
        const double den = (double)col_tot[i] * (double)row_tot[o] * 255.0;   // both normalisations and the 255 in ONE true division
        float x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = (float)((double)acc[(size_t)o * 3 * S + c * S + i] / den);
            out[((size_t)c * S + o0 + o) * S + i] = x[c];
        }
        if (want_mean) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < n_pre) pd_img_op(x, col.order[k], col, 0.0f);
            gsum += pd_img_grey(x);
        }
    }
    double g = (double)gsum;
#pragma unroll
    for (int off = PD_WAVE / 2; off > 0; off >>= 1) g += __shfl_down(g, off, PD_WAVE);
    if (lane == 0) red[wave] = g;
    __syncthreads();
    if (tid == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < PD_IMG_WAVES; ++w) t += red[w];
        a.partials[(size_t)f * a.n_bands + bandi] = t;
        if (bandi == 0) a.status[f] = PD_IMG_OK;
    }
}

__global__ __launch_bounds__(PD_IMG_THREADS) void pd_img_colour_kernel(PdImgArgs a) {
    const int f = blockIdx.y, S = a.S;
    const pd_img_frame fr = a.frames[f];
    if (fr.colour < 0 || pd_img_status(fr, a.colours, a.n_colours, S) != PD_IMG_OK) return;
    const pd_img_colour col = a.colours[fr.colour];
    if (!col.jitter && !col.grayscale && col.erase_h == 0) return;
    float mean = 0.0f;
    if (col.jitter) {
        double t = 0.0;
        for (int b = 0; b < a.n_bands; ++b) t += a.partials[(size_t)f * a.n_bands + b];
        mean = (float)(t / ((double)S * (double)S));
    }
    float *out = a.out + (size_t)f * 3 * S * S;
    const float invS = 1.0f / (float)S;
    for (int idx = blockIdx.x * PD_IMG_THREADS + threadIdx.x; idx < S * S; idx += gridDim.x * PD_IMG_THREADS) {
        const int y = (int)(((float)idx + 0.5f) * invS), xcol = idx - y * S;
        float x[3];
        if (col.erase_h != 0 && y >= col.erase_top && y < col.erase_top + col.erase_h && xcol >= col.erase_left &&
            xcol < col.erase_left + col.erase_w) {
            x[0] = x[1] = x[2] = 0.0f;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = out[(size_t)c * S * S + idx];
            if (col.jitter) {
#pragma unroll
                for (int k = 0; k < 4; ++k) pd_img_op(x, col.order[k], col, mean);
            }
            if (col.grayscale) x[0] = x[1] = x[2] = pd_img_grey(x);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(size_t)c * S * S + idx] = x[c];
    }
}

extern "C" long long pd_train_images_workspace_bytes(int n_frames, int image_size) {
    PdImgPlan p;
    if (n_frames < 0 || n_frames > PD_IMG_MAX_FRAMES || image_size < 1 || image_size > PD_IMG_MAX_SIZE || !pd_img_plan(image_size, &p)) return 0;
    return (long long)n_frames * p.n_bands * (long long)sizeof(double);
}

extern "C" int pd_train_images(const uint8_t *pixels, const pd_img_frame *frames, int n_frames, const pd_img_colour *colours, int n_colours,
                               int image_size, int fill, float *out, int32_t *status_out, void *workspace, long long workspace_bytes,
                               void *stream) {
    const char *null_arg = !pixels ? "pixels" : !frames ? "frames" : !out ? "out" : !status_out ? "status_out" : !workspace ? "workspace"
                           : (!colours && n_colours > 0) ? "colours" : nullptr;
    if (null_arg) {
        pd_set_error("pd_train_images: %s is NULL", null_arg);
        return PD_ERR_INVALID_ARG;
    }
    if (n_frames < 0 || n_colours < 0) {
        pd_set_error("pd_train_images: n_frames = %d and n_colours = %d must be >= 0", n_frames, n_colours);
        return PD_ERR_INVALID_ARG;
    }
    PdImgPlan plan;
    if (image_size < 1 || image_size > PD_IMG_MAX_SIZE || !pd_img_plan(image_size, &plan)) {
        pd_set_error("pd_train_images: image_size = %d must lie in 1 .. %d", image_size, PD_IMG_MAX_SIZE);
        return PD_ERR_INVALID_ARG;
    }
    if (fill < 0 || fill > 255) {
        pd_set_error("pd_train_images: fill = %d must lie in 0 .. 255", fill);
        return PD_ERR_INVALID_ARG;
    }
    const long long need = pd_train_images_workspace_bytes(n_frames, image_size);
    if (workspace_bytes < need || ((uintptr_t)workspace & 7)) {
        pd_set_error("pd_train_images: workspace of %lld bytes at %p is too small or not 8-byte aligned (%lld bytes needed)", workspace_bytes,
                     workspace, need);
        return PD_ERR_INVALID_ARG;
    }
    if (n_frames == 0) return PD_OK;
    if (n_frames > PD_IMG_MAX_FRAMES) {
        pd_set_error("pd_train_images: n_frames = %d exceeds the %d frames of one call", n_frames, PD_IMG_MAX_FRAMES);
        return PD_ERR_INVALID_ARG;
    }
    PdImgArgs a;
    a.pixels = pixels, a.frames = frames, a.colours = colours, a.out = out, a.status = status_out, a.partials = (double *)workspace;
    a.n_colours = n_colours, a.S = image_size, a.band = plan.band, a.hrows = plan.hrows, a.n_bands = plan.n_bands;
    a.fill = (float)fill;
    hipLaunchKernelGGL(pd_img_resize_kernel, dim3(plan.n_bands, n_frames), dim3(PD_IMG_THREADS), 0, (hipStream_t)stream, a);
    PD_HIP_CHECK(hipGetLastError());
    if (n_colours > 0) {
        const int px_blocks = (image_size * image_size + PD_IMG_THREADS - 1) / PD_IMG_THREADS;
        hipLaunchKernelGGL(pd_img_colour_kernel, dim3(px_blocks < 64 ? px_blocks : 64, n_frames), dim3(PD_IMG_THREADS), 0,
                           (hipStream_t)stream, a);
        PD_HIP_CHECK(hipGetLastError());
    }
    return PD_OK;
}
