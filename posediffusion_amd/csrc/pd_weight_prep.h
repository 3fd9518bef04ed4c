// pd_weight_prep.h -- creation-time weight preparation shared by the two denoiser paths (pd_denoiser.hip, pd_denoiser_generic.hip)
// and the ViT (pd_vit.hip): the device buffers of an engine and the kernels that turn caller weights into the layouts the hot
// kernels read (pd_weight_prep.hip).  Nothing here runs during a sampling step or a forward.
#pragma once
#include "pd_internal.h"

// Every device buffer of one engine, freed with it.  The helpers allocate into the list; `who` prefixes their error messages
// (pd_engine_create / pd_vit_create).  Weight pointers are device pointers of the caller; a NULL one is PD_ERR_INVALID_ARG.
struct PdDevAllocs {
    const char *who;
    std::vector<void *> ptrs;

    explicit PdDevAllocs(const char *caller) : who(caller) {}
    PdDevAllocs(const PdDevAllocs &) = delete;
    PdDevAllocs &operator=(const PdDevAllocs &) = delete;
    ~PdDevAllocs();

    // n elements of T, optionally zero-filled
    template <typename T>
    int alloc(T **p, size_t n, bool zero = false) { return alloc_bytes((void **)p, n * sizeof(T), zero); }
    int alloc_bytes(void **p, size_t bytes, bool zero);
    void release(void *p);   // frees one buffer of the list (null: nothing)

    // a copy of n floats
    int copy(float **dst, const float *src, size_t n);
    // W [Nout][K] (row stride ldw, default K; first column koff) -> MFMA-fragment order for tile width nt (32 or 16), zero padded to
    // Kpad columns and to whole tiles; gamma (nullable) folded in as a column scale.  first_perm: K is _first's 702 columns in the
    // small-batch kernel's order (pd_first_col_all)
    int pack(float **dst, const float *W, int Nout, int K, int Kpad, int nt, const float *gamma, int first_perm = 0, int ldw = 0,
             int koff = 0);
    // b' = b + W beta (the LayerNorm shift folded into the following bias), W [Nout][K]
    int fold_bias(float **dst, const float *W, const float *beta, const float *b, int Nout, int K);
    // row-major copy of W [Nout][K] with gamma (nullable) folded in as a column scale
    int rowmajor(float **dst, const float *W, int Nout, int K, const float *gamma);
    // W [Nout][K] split into hi / lo planes in MFMA-fragment order (pd_gemm_split.h): bf16 halves of w * gamma[k] (gamma nullable), or
    // with f16 fp16 halves of w * 2^ew
    int planes(unsigned **dst, const float *W, int Nout, int K, const float *gamma, bool f16 = false, int ew = 0);
};

template <typename KernelT>
inline int pd_set_lds(KernelT kern, size_t bytes) {
    PD_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PD_OK;
}

// The fp16-plane scale exponents of one encoder layer.
struct PdPlaneExps {
    int qkv, out, ff1, ff2;   // weights: w * 2^e is split into fp16 planes
    int ctx, hid;             // operands of out (the attention output) and ff2 (the hidden rows)
};
// floor(log2(cap / v)) clamped to [-60, 60]; 0 for v <= 0
int pd_floor_log2_ratio(double cap, double v);
// Reads one encoder layer's four row-major Linear weights (LayerNorm scale folded) back from the device, qkv [3 D, D], out [D, D],
// ff1 [F, D], ff2 [D, F], with the biases the operand bounds need.  *finite is false when one of them holds inf / NaN (the exponents are
// then meaningless).
int pd_plane_exponents(const float *qkv_w, const float *qkv_b, const float *out_w, const float *ff1_w, const float *ff1_b,
                       const float *ff2_w, int D, int F, PdPlaneExps *e, bool *finite);
