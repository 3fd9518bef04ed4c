/*
 * pd_engine_images.h -- the training images of a whole batch in one call: jittered square crop (which may stick out of the picture),
 * antialiased bilinear resize to image_size x image_size, and the sequence's colour draw (ColorJitter in any order, grayscale, erase),
 * i.e. what the reference's datasets/co3d_v2.py:get_data does per frame on CPU workers (crop :205-214, ToTensor + Resize(antialias)
 * :149, color_jitter / rand_erase :365-368), from decoded uint8 frames to the fp32 [F, 3, S, S] tensor the backbone reads
 * (csrc/pd_images.hip).
 *
 * An extension header like pd_engine_cameras.h: the function list of pd_engine.h is pinned.  Stateless: DEVICE pointers borrowed for the
 * call, `stream` a hipStream_t as void *, no allocation, no host synchronisation.  Conventions are those of pd_engine.h (return
 * codes, pd_last_error).
 *
 * Resize.  The crop is a side x side picture whose pixels outside the source read as `fill`; it is divided by 255 and resized with the
 * triangle filter of torch's _upsample_bilinear2d_aa (align_corners = False), the same rule on both axes.  With scale = side / S,
 * support = max(scale, 1), output index i has the centre c = scale (i + 0.5), the taps j in [max(0, floor(c - support + 0.5)),
 * min(side, floor(c + support + 0.5))) and the weights max(0, 1 - |j - c + 0.5| / support) normalised to sum 1.  The windows are clipped
 * at the CROP's border: padded pixels are taps of value `fill`.  With D = 2 max(side, S) every un-normalised weight is the INTEGER
 *     n(i, j) = max(0, D - |(2 j + 1) S - side (2 i + 1)|)   over D,
 * and the window bounds are integer floor divisions, so bounds and weights are exact.  The kernel divides every n by their common factor
 * (gcd(side, S), twice that where (S - side) / gcd is even), accumulates sum_j n(i, j) pixel_j (horizontal pass, bytes 0 .. 255) and then
 * sum_r n(o, r) (.)_r (vertical pass) by fp32 fused multiply-adds in ascending tap order -- whole numbers, exact while they stay below
 * 2^24 -- and applies both normalisations and the 255 in ONE true division at the end (the divisor formed exactly, in fp64).  A crop with
 * side == S inside the picture has the weights 1 and 0 and is bitwise uint8 -> float -> / 255.
 *
 * Colour stage, on the resized values, torchvision's float-tensor definitions:
 *   brightness  clamp(f x, 0, 1)
 *   contrast    clamp(f x + (1 - f) m, 0, 1),  m = mean over the frame's S S pixels of grey = 0.2989 r + 0.587 g + 0.114 b taken AFTER the
 *               operations that precede contrast in `order`, per frame
 *   saturation  clamp(f x + (1 - f) grey(x), 0, 1)
 *   hue         RGB -> HSV, h <- (h + f) mod 1, HSV -> RGB; the max channel is r first, then g; s = 0 where max == min
 *   grayscale   grey on all three channels;   erase (value 0) last.
 * The mean is a sum of fp64 partials, one per band of output rows, stored in `workspace` and added in ascending band order: no atomics,
 * an order that depends on S alone, so a frame's output is bitwise the same alone, in any batch, and from run to run.
 * A frame with colour == -1, or whose entry has jitter == 0, grayscale == 0 and erase_h == 0, keeps the bits of the resize.
 */
#ifndef PD_ENGINE_IMAGES_H
#define PD_ENGINE_IMAGES_H

#include "pd_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PD_IMG_MAX_SIDE 6144      /* longest crop side: one source row of the crop is staged in on-chip memory (status PD_IMG_BAD_SIDE above it) */
#define PD_IMG_MAX_SIZE 1024      /* largest image_size (PD_ERR_INVALID_ARG above it) */
#define PD_IMG_MAX_FRAMES 65535   /* most frames of one call: a frame is a grid row (PD_ERR_INVALID_ARG above it) */

typedef struct {
    int64_t offset;               /* byte offset of the frame in `pixels`, any alignment */
    int32_t height, width;        /* RGB, HWC, rows of 3 * width bytes, no padding */
    int32_t x0, y0, side;         /* square crop box in image pixels [x0, x0 + side) x [y0, y0 + side); may lie partly or wholly outside */
    int32_t colour;               /* index into `colours`, -1 = none */
} pd_img_frame;

typedef struct {
    int32_t jitter;               /* 0 / 1: apply the four operations below */
    int32_t order[4];             /* a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue */
    float brightness, contrast, saturation, hue;   /* the four factors */
    int32_t grayscale;            /* 0 / 1 */
    int32_t erase_top, erase_left, erase_h, erase_w;   /* rectangle in output pixels set to 0; erase_h == 0: none */
} pd_img_colour;

/* status_out values; under every non-zero one the frame's output is +0 */
#define PD_IMG_OK 0
#define PD_IMG_BAD_SIDE 1         /* side < 1 or side > PD_IMG_MAX_SIDE */
#define PD_IMG_BAD_SIZE 2         /* height < 1, width < 1 or offset < 0 */
#define PD_IMG_BAD_COLOUR 3       /* colour outside [-1, n_colours) */
#define PD_IMG_BAD_ORDER 4        /* jitter != 0 and order is no permutation of 0..3 */
#define PD_IMG_BAD_ERASE 5        /* erase_h != 0 and the rectangle is empty-negative or not inside [0, S) x [0, S) */

/* bytes of `workspace` a call with these arguments needs (0 for arguments the call itself refuses) */
long long pd_train_images_workspace_bytes(int n_frames, int image_size);

/* pixels: uint8, all frames; frames [n_frames]; colours [n_colours] (may be NULL when n_colours == 0); fill 0 .. 255;
 * out [n_frames, 3, S, S] fp32; status_out [n_frames] int32 (PD_IMG_*); workspace: pd_train_images_workspace_bytes(...) bytes, 8-byte
 * aligned, contents undefined before and after.  Nothing outside out, status_out and workspace is written.  The frame table lives on the
 * device, so a bad frame is never known on the host and is always reported through status_out.
 * PD_ERR_INVALID_ARG naming the argument, before anything is launched: NULL pixels, frames, out, status_out or workspace, NULL colours
 * with n_colours > 0, n_frames outside 0 .. PD_IMG_MAX_FRAMES, n_colours < 0, image_size outside 1 .. PD_IMG_MAX_SIZE, fill outside 0 .. 255, workspace_bytes too
 * small.  n_frames == 0 is a no-op. */
int pd_train_images(const uint8_t *pixels, const pd_img_frame *frames, int n_frames, const pd_img_colour *colours, int n_colours,
                    int image_size, int fill, float *out, int32_t *status_out, void *workspace, long long workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_ENGINE_IMAGES_H */
