/*
 * sdod_hip.h -- kernel-level C ABI of the MI355X (gfx950) hot path.
 *
 * Every entry point takes plain device pointers, sizes and a HIP stream handle
 * (void* == hipStream_t); no torch / C++ types cross this boundary.  Return value
 * is 0 on success, otherwise a libsdod status code (include/libsdod.h) with a
 * message retrievable through sdod_hip_last_error().
 *
 * What each group replaces in the reference (vaenyr/stable-diffusion-on-device):
 *   - sdod_group_norm_*    : the `sdod::GroupNorm` / `sdod::ParameterlessGroupNorm` custom op whose
 *                            schema is csrc/sdod_ops/config/group_norm.{xml,json} and whose Python
 *                            surface is sdod/efficient_gn.py:9-30 (no kernel exists in the reference)
 *   - sdod_gemm_f16, sdod_attention_f16, sdod_layer_norm_f16, ... : the arithmetic inside the opaque
 *                            QNN graphs executed by QnnGraph::execute (csrc/libsdod/src/qnn_context.cpp:711-713)
 *   - sdod_cfg_* / sdod_dpm_update / sdod_plms_* : the host-side CFG combine
 *                            (qnn_context.cpp:1018-1081 via context.cpp:359-373) and DPMSolver::update
 *                            (dpm_solver.cpp:136-181), moved on-device
 *   - sdod_timestep_features: context.cpp:257-274
 *   - sdod_image_to_u8      : context.cpp:392-395
 *
 * Layouts: activations are NHWC fp16 ("[N][H*W][C]", C contiguous); weights are [Cout][K] fp16 with
 * K contiguous (conv3x3: K = (r*3+s)*Cin + c, i.e. KRSC); bias / norm parameters are fp32.
 */
#ifndef SDOD_HIP_H
#define SDOD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifndef SDOD_API
#define SDOD_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* SDOD_ACT_RELU: sdod_act_f16 only.  The GEMM epilogue's `act` is compiled into shared device code (apply_act), which stays as it
 * is: sdod_gemm_f16 refuses it. */
enum sdod_act { SDOD_ACT_NONE = 0, SDOD_ACT_SILU = 1, SDOD_ACT_GELU = 2, SDOD_ACT_QUICK_GELU = 3, SDOD_ACT_RELU = 4 };
/* SDOD_U8Q (graph parameters only): per-tensor affine uint8, the reference's QNN weight format (`quantize=8`, todlc.py:108;
 * qnn_context.cpp:1018-1033): payload = {float scale; int32 offset (<= 0); uint8 q[numel]}, real = (q + offset) * scale */
enum sdod_dtype { SDOD_F16 = 0, SDOD_F32 = 1, SDOD_U8Q = 2, SDOD_BF16 = 3 /* sdod_group_norm_nchw only */ };
enum sdod_a_mode { SDOD_A_ROWS = 0, SDOD_A_CONV3X3 = 1 /* NHWC gather: 3x3 pad 1 or 1x1 */ };

/* out[M][N] = act(alpha * A[M][K] . W[N][K]^T + bias + row_bias) + residual        (fp16 in/out, fp32 acc)
 * A is either a row-major matrix (SDOD_A_ROWS) or gathered on the fly from an NHWC image for a 3x3
 * pad-1 convolution (SDOD_A_CONV3X3): row m = (img, oy, ox), k = (r, s, c); the image may be the
 * channel-concatenation of two tensors (a, a2) and may be nearest-2x upsampled on the fly. */
typedef struct sdod_gemm_desc {
    const void* a;        /* fp16; rows: [M][lda]; conv: [n_img][h_in][w_in][c0] */
    const void* a2;       /* conv only: second concat source [n_img][h_in][w_in][c1], or NULL */
    const void* w;        /* fp16 [N][ldw] */
    const void* bias;     /* fp32 [N] (or [M] if bias_on_m), may be NULL */
    const void* row_bias; /* fp16 [M / rows_per_img][ld_row_bias] added per image (time embedding), may be NULL */
    const void* residual; /* fp16 [M][ldr], may be NULL */
    void* out;            /* fp16 [M][ldo]; out and residual 16-byte aligned when the output width, ldo and ldr are multiples of 8 */
    void* workspace;      /* fp32 split-K slabs, >= split_k*M*N*4 bytes when split_k > 1 */
    size_t workspace_bytes;
    int M, N, K;
    int lda, ldw, ldo, ldr;
    int a_mode;
    int n_img, h_in, w_in, c0, c1; /* conv geometry: input (pre-upsample) */
    int stride;                    /* conv: 1 or 2 */
    int upsample;                  /* conv: 1 = nearest 2x before the conv */
    int ksize;                     /* conv: 3 (default when 0) or 1 */
    int rows_per_img;              /* for row_bias */
    int ld_row_bias;               /* row stride of row_bias (0 = N) */
    int act;
    float alpha;
    int bias_on_m;
    int split_k;                   /* 0 = auto; 1 = none; >1 = number of K slices (needs workspace) */
    int tile;                      /* 0 = auto; else forces a tile config (see gemm.hip) */
    /* --- fusions (LDS-DMA kernel family only) ---
     * geglu: W has N rows laid out as interleaved 16-row blocks [a(16) | gate(16)]...; out gets N/2 columns:
     *        out = (acc_a + bias_a) * gelu(acc_gate + bias_gate)    (ldm GEGLU: x * gelu(gate), fused into ff.net.0.proj)
     * tail segment: K columns [k_tail, K) of W multiply a SECOND, 1x1-gathered NHWC source (t0 | t1 channel concat) at the
     *        output pixel: out = conv3x3(a|a2) + conv1x1(t0|t1)  (ResBlock out_layers.3 + skip_connection in one GEMM);
     *        bias2 is added like bias.
     * ln: the rows of A are LayerNorm-ed on the fly (rows mode, K = normalised width, no split-K): the kernel sums
     *        x and x^2 of every row while the slabs pass through LDS and the epilogue applies
     *        out = rstd_m * (acc - mean_m * ln_s[n]) + bias[n]; the LayerNorm weight is pre-multiplied into W, ln_s[n] =
     *        sum_k W'[n][k] and bias[n] = sum_k beta[k] W[n][k] (+ linear bias) come from sdod_ln_fold_f16.
     *        rstd_m = 1 / sqrt(var_m + ln_eps) with the ONE-PASS variance var_m = sum x^2 / K - mean_m^2 in fp32, clamped at 0
     *        (the row passes through LDS once).  Contract: the result is within the Linear kernels' tolerance (rel-L2 3e-3
     *        against fp64) for rows with |row mean| / row std <= 100; beyond that the cancellation in var_m grows with the
     *        square of the ratio and the output is only guaranteed finite.  sdod_layer_norm_f16 is two-pass and has no such
     *        limit: LayerNorm rows far from zero mean go through it (tests/test_row_kernels_gpu.py). */
    int geglu;
    int k_tail;                    /* 0 = no tail segment; else 9*(c0+c1) */
    const void* t0;
    const void* t1;
    int tc0, tc1;
    const void* bias2;
    int ln;
    const void* ln_s;              /* fp32 [N] */
    float ln_eps;                  /* added to the one-pass variance under the square root (see `ln` above for the contract) */
    int phase;                     /* split-K only: 0 = GEMM + reduce (default), 1 = GEMM slabs only, 2 = reduce + epilogue only
                                    * (lets a launch list time / profile the two kernels separately) */
    /* --- int8 weight streaming (LDS-DMA kernel family only; BASELINE config 5, the reference's `quantize=8` path,
     * todlc.py:105-108): w holds the affine-uint8 CODES of the reference's encoding real = (q + offset) * scale
     * (qnn_context.cpp:1018-1033), one byte per element, row stride ldw BYTES; the slab is streamed as bytes (half the
     * weight traffic of fp16) and expanded to the integer q + offset in fp16 (exact) on the fragment read.  Per output
     * column n: w_scale[n] = scale, w_off[n] = offset + 128 (fp32 holding an INTEGER, offset in [-1024, 0] -- the QNN
     * zero point of a uint8 tensor is in [-255, 0]), so fused parameter groups may mix tensors with different
     * encodings.  out = act(alpha * w_scale[n] * sum_k A (q + offset[n]) + bias ...).  Not with ln / k_tail. */
    int wq;
    const void* w_scale;           /* fp32 [N] */
    const void* w_off;             /* fp32 [N] */
    /* --- split-K without a reduce launch (halo-patch convolution tiles): a buffer of >= sdod_gemm_fixup_counters() 32-bit
     * words, ZEROED ONCE by its owner, used by one launch at a time (one per stream of concurrent callers) and left zeroed by
     * every launch.  With it, a phase-0 call of a split-K plan on such a tile is ONE launch: every K slice publishes its fp32
     * tile, the slice that arrives last at the tile's counter reduces (in slice order: bit-identical to the reduce kernel)
     * and runs the fused epilogue.  NULL: partial slabs + splitk_reduce_kernel as before. */
    void* fix_counters;
    /* XCD-aware tile order: 0 = chosen per shape (the number of n-tile panels in {1, 2, 4, 8} that minimises the bytes the
     * eight L2s fetch between them, panels * A + (8 / panels) * W); 1 / 2 / 4 / 8 force it (1 = m-major: every XCD reads all
     * of W; 8 = n-major: every XCD reads all of A).  Speed only. */
    int xcd_panels;
    /* --- per-image weights (rows mode, LDS-DMA ring tiles): the rows of image i = m / rows_per_img multiply the matrix at
     * w + i * w_img_stride (elements, a multiple of 8) and take bias / ln_s from + i * vec_img_stride floats (0: shared vectors).
     * rows_per_img must be a multiple of 32 dividing M; the plan only uses tiles whose rows divide rows_per_img.
     * softmax_cols = 80: the epilogue replaces every run of 80 output columns by its row softmax in the exp2 domain
     * (p = 2^(x - max) / sum; N a multiple of 160; columns to be ignored carry a bias of -30000).  Together they are the two
     * GEMMs of the FOLDED cross-attention (sdod_xattn_fold_f16): scores = LN(x) . (Wq^T K_h^T) with the softmax in the
     * epilogue, then out = P . (V_h Wo_h^T) + bias + residual. */
    int w_img_stride;
    int vec_img_stride;
    int softmax_cols;
    /* conv padding: 0 = symmetric ksize / 2 (zero-initialised descriptors); 1 = ldm's VAE-encoder Downsample, F.pad(x, (0, 1, 0, 1))
     * then a 3x3 stride-2 pad-0 convolution: nothing above / left of the image, one zero row / column below / right of it, so
     * h_out = (h_in + 1 - 3) / 2 + 1.  Only the im2col gather kernels honour it: halo-patch tiles decline it (sdod_gemm_halo_ok = 0),
     * a tail segment or upsampling refuses it, and it needs ksize 3 with stride 2.
     * 2 / 3 / 4 = seamless tiling: the symmetric pad-1 border of a 3x3 convolution is CIRCULAR on both axes (2), on x only (3:
     * columns wrap, zero rows above and below) or on y only (4: rows wrap, zero columns left and right).  A wrapped tap reads pixel
     * (y mod H, x mod W) of the same image, in output coordinates before the >> 1 of upsampling.  Output size, plan, workspace
     * and every fusion (stride 1 or 2, upsampling, concat, tail segment, row bias, residual, split-K, uint8 weights) are those of
     * pad_mode 0, and every kernel family honours it (halo-patch tiles take it wherever they take 0); ksize 1 refuses it. */
    int pad_mode;
} sdod_gemm_desc;

SDOD_API int sdod_gemm_f16(const sdod_gemm_desc* d, void* stream);
/* Regional prompts: the score GEMM of the folded cross-attention with its 80-column groups laid out as
 * [region][head][80].  Plans and computes exactly as sdod_gemm_f16; in the softmax epilogue the probabilities of group g of row m are
 * multiplied by region_w[(m % rows_per_img) * regions + g / (N / 80 / regions)] (fp32 [rows_per_img][regions], read by the kernel in
 * the launch: a captured graph picks up new values).  The weight goes into the reciprocal of the group's sum, so weight 1.0 leaves
 * every bit as sdod_gemm_f16 writes it and weight 0 gives exact zeros.  Needs softmax_cols == 80, w_img_stride != 0 (with it
 * rows_per_img % 32 == 0), N % (80 * regions) == 0 and regions in [1, 4]; anything else is INVALID_ARGUMENT with nothing written. */
SDOD_API int sdod_gemm_region_f16(const sdod_gemm_desc* d, const void* region_w, int regions, void* stream);
/* 1 when the call above reduces its split-K slices inside the GEMM launch (see fix_counters), else 0 */
SDOD_API int sdod_gemm_fixup(const sdod_gemm_desc* d);
/* counter words a fix_counters buffer must hold for any descriptor (one per output tile; 64 Ki covers M*N up to 2^28 at 64x64) */
SDOD_API size_t sdod_gemm_fixup_counters(void);
/* picks split_k / tile as the auto heuristic would; returns required workspace bytes */
SDOD_API size_t sdod_gemm_workspace_bytes(const sdod_gemm_desc* d);
/* which tile configuration (1: 128x128, 2: 128x64, 3: 64x64, 4: 256x16, 5: 64x128) and split-K factor the call would use */
SDOD_API int sdod_gemm_plan(const sdod_gemm_desc* d, int* tile, int* splits);
/* 1 when halo-patch convolution tile `tile` takes the descriptor (3x3, stride 1, tile rows divide the image, patch fits LDS);
 * 0 otherwise -- sdod_gemm_f16 refuses such a forced tile with LIBSDOD_INVALID_ARGUMENT.  Host-only. */
SDOD_API int sdod_gemm_halo_ok(const sdod_gemm_desc* d, int tile);
/* 1 when A-panel tile `tile` (gemm_apanel_kernel: a row panel x the whole K resident in LDS, n-tiles streamed past it) takes
 * the descriptor: rows mode, fp16 weights, K >= 192, panel + ring within 160 KiB of LDS, no split-K / row_bias / bias2 /
 * bias_on_m / tail segment.  Host-only. */
SDOD_API int sdod_gemm_panel_ok(const sdod_gemm_desc* d, int tile);
/* n-tile panels (1, 2, 4 or 8) of the XCD-aware tile order the call would use (see sdod_gemm_desc::xcd_panels).  Host-only. */
SDOD_API int sdod_gemm_xcd_panels(const sdod_gemm_desc* d);
/* number of tile configurations (valid `tile` values are 1..this); a tune table naming anything else is stale */
SDOD_API int sdod_gemm_num_tiles(void);
/* rows x columns of tile configuration `tile`; lds_dma = 1 for the LDS-DMA kernel family (tiles >= 6) */
SDOD_API int sdod_gemm_tile_shape(int tile, int* bm, int* bn, int* lds_dma);
/* template arguments of the kernel behind `tile`: {BM, BN, WM, WN, STAGES (0: register-staged gemm_kernel), SPEC, KSUB} */
SDOD_API int sdod_gemm_tile_info(int tile, int out[7]);
/* developer aid: average duration in ms of `iters` back-to-back launches (HIP events on `stream`) */
SDOD_API int sdod_gemm_time(const sdod_gemm_desc* d, void* stream, int iters, float* ms_avg);
/* Same, with cold caches: before every timed launch a sweep of `scratch` (>= 64 MiB; use >= 512 MiB to clear the 256 MiB
 * Infinity Cache) evicts the weights, then the activation operands are re-read so that they are cache-resident as they are
 * behind a producer launch.  This is what a GEMM meets inside a graph replay; the engine's tile autotuner ranks with it. */
SDOD_API int sdod_gemm_time_cold(const sdod_gemm_desc* d, void* stream, int iters, void* scratch, size_t scratch_bytes, float* ms_avg,
                                float* ms_min /* may be NULL */);

/* GroupNorm over NHWC [N][HW][C] (optionally the channel concat of x (c0) and x2 (c1)), G groups,
 * y = (x-mean)*rstd*w+b, optional SiLU.  dtype applies to x and y; weight/bias fp32 or NULL.
 * workspace: >= sdod_group_norm_workspace_bytes(N, G) bytes of fp32 scratch, 128-byte aligned, ZEROED ONCE by its owner before
 * the first call and never shared by two calls that may run concurrently (different streams: one workspace each): the
 * one-launch kernel for big maps (>= 5 MB) keeps the words of its grid barrier in the FIRST 4 KiB of it (a fixed offset, so
 * that one workspace may serve calls of different (N, G): no layout's partial sums reach them) and leaves them re-armed.
 * A grid barrier that cannot meet (barrier words clobbered; two such launches sharing one workspace or starving each other of
 * CUs) gives up after ~1 s instead of hanging the device, and its output is INVALID.  It is never silent: the kernel sets a
 * sticky per-device error word, after which sdod_group_norm_status() -- read it behind a host synchronisation -- and every
 * later sdod_group_norm_nhwc / sdod_graph_execute on that device return LIBSDOD_RUNTIME_ERROR until the owner has re-zeroed
 * the workspace and called sdod_group_norm_clear_error(). */
SDOD_API size_t sdod_group_norm_workspace_bytes(int n, int groups);
/* byte offsets of the workspace's parts for (n, groups): barrier lines, partial statistics, collapsed statistics, a reserved
 * [n][groups] float region (unused), end */
SDOD_API int sdod_group_norm_layout(int n, int groups, size_t* sync_off, size_t* partial_off, size_t* stats_off, size_t* shift_off,
                                    size_t* end_off);
/* 0, or LIBSDOD_RUNTIME_ERROR once a one-launch GroupNorm on the current device has timed out at its grid barrier (sticky) */
SDOD_API int sdod_group_norm_status(void);
SDOD_API int sdod_group_norm_clear_error(void);
/* 1 = a single-launch kernel handles this shape, 2 = statistics + apply launches, 0 = no NHWC kernel takes it */
SDOD_API int sdod_group_norm_launches(int hw, int c, int groups, int dtype);
/* which kernel the call below launches for this shape: 0 = one-launch grid-barrier kernel (maps >= 5 MB), 1 = one launch, a
 * workgroup per (image, group), 2 = one launch, small-map LDS kernel, 3 = statistics + apply launches; -1 = no kernel takes it
 * (a bad shape, or channels too many for the kernels' tables): the call below then returns LIBSDOD_INVALID_ARGUMENT before any
 * launch, and sdod_group_norm_nchw takes the operator (it has no channel limit) */
SDOD_API int sdod_group_norm_path(int n, int hw, int c0, int c1, int groups, int dtype);
SDOD_API int sdod_group_norm_nhwc(const void* x, const void* x2, void* y, const float* weight, const float* bias,
                                  int n, int hw, int c0, int c1, int groups, float eps, int silu, int dtype,
                                  void* workspace, void* stream);

/* The same operator on torch's default layout, NCHW "[N][C][spatial]" (what sdod.EfficientGN receives from a model that was
 * not converted to channels_last, efficient_gn.py:61-86): a group is one contiguous slab of (C / G) * spatial elements, so
 * there is no transpose and no constraint on C; fp16 / bf16 / fp32, y may be x.  Slabs up to 32 Ki elements take one launch
 * (read once); bigger ones a statistics + an apply launch and `workspace` (>= sdod_group_norm_nchw_workspace_bytes(n,
 * groups) bytes, no initialisation needed, one per stream). */
SDOD_API size_t sdod_group_norm_nchw_workspace_bytes(int n, int groups);
SDOD_API int sdod_group_norm_nchw(const void* x, void* y, const float* weight, const float* bias, int n, int c, long long spatial,
                                  int groups, float eps, int silu, int dtype, void* workspace, void* stream);

/* GroupNorm whose source-0 tensor is still in split-K form: the producing GEMM ran with phase = 1 (fp32 partial slabs only),
 * and this call does what its phase 2 (splitk_reduce + fused epilogue) would have done -- x = fp16(act(alpha * sum_s partial
 * + bias + bias2 + row_bias[image])) + residual, same arithmetic and rounding points -- while loading the group: x is
 * written to x_out ([n*hw][c0], dense) for its later readers and GroupNorm(+SiLU) of (x | x2) goes to y, in ONE launch.
 * sdod_gemm_reduce_info fills the descriptor from the GEMM's; sdod_group_norm_reduce_ok tells whether the one-launch
 * (image, group) kernel takes the shape (otherwise run phase 2 and the plain GroupNorm). */
typedef struct sdod_gn_reduce {
    const void* partial;   /* fp32 [splits][M][N] */
    int splits;
    size_t slab_floats;    /* M * N */
    const void* bias;      /* fp32 [N] or NULL */
    const void* bias2;     /* fp32 [N] or NULL */
    const void* row_bias;  /* fp16 [n_img][ld_row_bias] or NULL (rows_per_img must equal hw) */
    int ld_row_bias;
    const void* residual;  /* fp16 [M][ldr] or NULL */
    int ldr;
    void* x_out;           /* fp16 [M][N] */
    float alpha;
    int act;
    int M, N;
} sdod_gn_reduce;
SDOD_API int sdod_gemm_reduce_info(const sdod_gemm_desc* d, sdod_gn_reduce* out);
SDOD_API int sdod_group_norm_reduce_ok(int hw, int c0, int c1, int groups);
SDOD_API int sdod_group_norm_reduce_nhwc(const sdod_gn_reduce* red, const void* x2, void* y, const float* weight,
                                         const float* bias, int n, int hw, int c0, int c1, int groups, float eps, int silu,
                                         void* stream);

/* Folds a LayerNorm (gamma, beta over K) into the Linear that consumes it, in place: t_out[n] = sum_k beta[k]*W[n][k]
 * (+ bias_in[n]); W[n][k] <- fp16(W[n][k]*gamma[k]); s_out[n] = sum_k W'[n][k].  Used once per weight at graph build. */
SDOD_API int sdod_ln_fold_f16(void* w, int n, int k, int ldw, const float* gamma, const float* beta, const float* bias_in,
                              float* s_out, float* t_out, void* stream);
/* Composes two Linear layers that follow each other with nothing in between, y = P (W x + bw) + bp, into one (one-time, at
 * graph build): c[o][k] = sum_j p[o][j] w[j][k] (fp32 accumulate, rounded to fp16 once), bias_out[o] = sum_j p[o][j] bw[j]
 * + bp[o].  p: fp16 [n_out][ldp] (n_mid columns), w: fp16 [n_mid][ldw] (k columns), c: fp16 [n_out][ldc]; c must not alias
 * p or w.  The UNet uses it for transformer_blocks.0.ff.net.2 -> proj_out (analyze_results.py:69-79 lists them as two ops). */
SDOD_API int sdod_compose_linear_f16(const void* p, int ldp, const void* w, int ldw, void* c, int ldc, int n_out, int n_mid, int k,
                                     const float* bias_w, const float* bias_p, float* bias_out, void* stream);
/* Low-rank (LoRA) update of a packed fp16 weight matrix, in place:
 *   W'[row(o)][col(j)] = fp16(float(W[row(o)][col(j)]) + scale * sum_r up[o][r] * down[r][j])     (fp32 accumulate, one rounding)
 * w: fp16 [n][ldw], k <= ldw columns of it (a column block of a wider row: nothing outside the k columns is written); up: fp16
 * [n][rank], down: fp16 [rank][k], both in CANONICAL PyTorch order (a 3x3 convolution: down = [rank][cin][3][3] flattened, up the
 * [n][rank][1][1] factor).  row() is the identity or, with geglu != 0, the 16-row value / gate interleave of a fused-GEGLU
 * projection (n % 32 == 0); col() is the identity or, with conv_cin > 0 (k = 9 conv_cin, conv_cin % 8 == 0), the KRSC order
 * j = c * 9 + t -> t * conv_cin + c: the packings of the graph engine (sdod_graph_param_device).  rank in [1, 128] (any value:
 * staged zero-padded to the MFMA K step), n >= 1, k % 8 == 0, ldw % 8 == 0, w 16-byte aligned, scale finite (it already holds
 * strength * alpha / rank); anything else is INVALID_ARGUMENT before any device call.  Deterministic (no atomics, fixed
 * summation order); scale = 0 leaves W bit-identical. */
SDOD_API int sdod_lora_merge_f16(void* w, int n, int k, int ldw, const void* up, const void* down, int rank, float scale,
                                 int conv_cin, int geglu, void* stream);
/* The LyCORIS families on the same packed matrix, with the same maps, column block, alignment rules, determinism and scale = 0
 * behaviour as sdod_lora_merge_f16; every argument error is INVALID_ARGUMENT before any device call.
 * LoHa (Hadamard product of two low-rank products):
 *   W'[row(o)][col(j)] = fp16(fma(scale, (sum_r w1a[o][r] w1b[r][j]) * (sum_r w2a[o][r] w2b[r][j]), float(W)))
 * each sum accumulated in fp32 on the matrix cores, the two multiplied in fp32, one rounding.  w1a, w2a: fp16 [n][rank]; w1b, w2b:
 * fp16 [rank][k] (a 3x3 convolution: [rank][cin][3][3]), canonical order; rank in [1, 128]. */
SDOD_API int sdod_loha_merge_f16(void* w, int n, int k, int ldw, const void* w1a, const void* w1b, const void* w2a, const void* w2b,
                                 int rank, float scale, int conv_cin, int geglu, void* stream);
/* LoKr (Kronecker product):
 *   W'[row(o)][col(i, t)] = fp16(fma(scale, float(w1[o / c][i / d]) * float(w2[o % c][i % d][t]), float(W)))
 * with c = n / a, d = cin / b; cin = k and one tap (t = 0) for a Linear or 1x1 weight, cin = conv_cin and nine taps for a 3x3 one.
 * w1: fp16 [a][b]; w2: fp16 [c][d] or [c][d][3][3], canonical.  o and i are CANONICAL indices (with geglu the row split applies to
 * the canonical row).  Any a >= 1 dividing n and b >= 1 dividing cin; a = b = 1 adds the full canonical delta w2. */
SDOD_API int sdod_lokr_merge_f16(void* w, int n, int k, int ldw, const void* w1, int a, int b, const void* w2, float scale,
                                 int conv_cin, int geglu, void* stream);
/* LayerNorm over the last dim of fp16 [M][C] rows, fp32 weight/bias (either may be NULL); C % 8 == 0, C <= 3072. */
SDOD_API int sdod_layer_norm_f16(const void* x, void* y, const float* weight, const float* bias, int m, int c,
                                 float eps, void* stream);

/* Fused attention: out[b][q][h*D..] = softmax(scale * Q K^T (+causal mask)) V, never materialising scores.
 * q: [B][Lq][ldq], k/v: [B][Lk][ldk]/[ldv], head h at column offset h*D.  D in {40, 64, 80, 160}.
 * Row strides in halves: ldq, ldk, ldv multiples of 8, ldo a multiple of 4, all >= heads * D; q, k, v 16-byte and out 8-byte
 * aligned (q / k / v / out may be column offsets into wider rows).  scale must be finite and > 0: anything else is an error. */
SDOD_API int sdod_attention_f16(const void* q, const void* k, const void* v, void* out, int batch, int heads,
                                int lq, int lk, int d, int ldq, int ldk, int ldv, int ldo, float scale, int causal,
                                void* stream);
/* 1 when the call above takes head dim d, else 0: the one statement of the set, which the graph engine asks when a graph is
 * created (sdod_model_config.num_heads / head_dim, include/sdod_engine.h).  Host-only. */
SDOD_API int sdod_attention_head_dim_ok(int d);

/* Folded cross-attention, the once-per-prompt part.  The text context is constant over the sampler run, so to_q and to_out can
 * be multiplied into K and V: scores_h = LN(x) . W1_h with W1_h = Wq_h^T K_h^T, out = [P_1 | .. | P_H] . [W2_1 ; .. ; W2_H] with
 * W2_h = V_h Wo_h^T -- two GEMMs per evaluation (sdod_gemm_desc: w_img_stride / vec_img_stride / softmax_cols) instead of
 * Linear + attention + Linear (the reference's /attn2/to_q, /attn2/MatMul, /attn2/to_out.0 ops, analyze_results.py:69-79).
 * kv: fp16 [n_img * L][ld_kv], K at column k_off, V at v_off (heads * d columns each), L <= 80 keys; wq: [C][ldq] with the
 * LayerNorm weight folded in, sq / tq its fold vectors (sdod_ln_fold_f16); wo: [C][ldwo]; scale = the softmax scale.
 * Writes w1 fp16 [n_img][heads*80][C] (scaled by scale * log2 e), s1 / t1 fp32 [n_img][heads*80] (padding columns: s = 0,
 * t = -30000), w2 fp16 [n_img][C][heads*80] (padding columns zero). */
SDOD_API int sdod_xattn_fold_f16(const void* kv, int ld_kv, int k_off, int v_off, int n_img, int L, const void* wq, int ldq,
                                 const void* sq, const void* tq, const void* wo, int ldwo, int heads, int d, float scale, void* w1,
                                 void* s1, void* t1, void* w2, void* stream);
/* The folded form's whole contract, 1 or 0.  Host-only; the three fold entry points REQUIRE through it and the graph builder
 * decides through it (0: Linear + attention + Linear), so a shape that passes never fails at execute.
 *   the launch:     heads >= 1; 8 <= d <= 160 with d % 8 == 0; 1 <= l_keys <= 80 (for sdod_xattn_fold_ip_f16 the text keys; its
 *                   image tokens are 1 .. 16); heads * d a multiple of 80 (W1 / W2 are built as 80-channel tiles)
 *   the two GEMMs:  heads a multiple of 4 (heads * 80 columns in 64-deep K slabs and whole 160-column softmax tiles); heads * d a
 *                   multiple of 64 (the score GEMM's K); rows_per_image (the pixels of one image) a multiple of 32
 * rows_per_image = 0 asks for the launch alone, which is what a caller that runs the GEMMs itself on other terms needs. */
SDOD_API int sdod_xattn_fold_ok(int heads, int d, int l_keys, int rows_per_image);

/* The same for regional prompts: kv holds n_img * regions segments of L rows (image-major), one per (image, region prompt).  w1 /
 * s1 / t1 are what the call above writes for n_img * regions images, bit for bit: for image b, [regions][heads*80] rows.  w2 for
 * image b is [C][regions * heads*80] -- region r's columns at r * heads*80, each slice what the call above writes -- so the
 * second GEMM sums over regions through its K axis.  regions in [1, 4]; 1 is the call above. */
SDOD_API int sdod_xattn_fold_regions_f16(const void* kv, int ld_kv, int k_off, int v_off, int n_img, int regions, int L, const void* wq,
                                         int ldq, const void* sq, const void* tq, const void* wo, int ldwo, int heads, int d, float scale,
                                         void* w1, void* s1, void* t1, void* w2, void* stream);

/* The same for an image prompt (IP-Adapter's decoupled cross-attention): two segments per image from two sources.
 * Segment 0 of image b is rows [b L, b L + L) of kv (the text keys, as in sdod_xattn_fold_f16); segment 1 is rows [b T, b T + T) of
 * kv_ip (the image tokens), which has a row stride and K / V offsets of its own.  w1 / s1 / t1 / w2 have the layout
 * sdod_xattn_fold_regions_f16 writes for regions = 2, and each slice is bit for bit what sdod_xattn_fold_f16 writes for that source
 * alone, padding columns included (s = 0, t = -30000, w2 zero).  1 <= T <= 16; k_off_ip / v_off_ip + heads * d <= ld_ip. */
SDOD_API int sdod_xattn_fold_ip_f16(const void* kv, int ld_kv, int k_off, int v_off, const void* kv_ip, int ld_ip, int k_off_ip, int v_off_ip,
                                    int n_img, int L, int T, const void* wq, int ldq, const void* sq, const void* tq, const void* wo, int ldwo,
                                    int heads, int d, float scale, void* w1, void* s1, void* t1, void* w2, void* stream);

/* Row softmax on fp16 [M][N] in place semantics allowed (y may equal x); fp32 math. */
SDOD_API int sdod_softmax_rows_f16(const void* x, void* y, int m, int n, void* stream);

/* Elementwise / glue (fp16 unless stated).
 * The 16-byte-lane entry points -- sdod_geglu_f16, sdod_act_f16, sdod_add_f16, sdod_concat_channels_f16, sdod_embedding_f16 (table,
 * pos, y) and, further down, sdod_avg_pool2_f16, sdod_adapter_stage_f16, sdod_add_feature_f16 -- move every fp16 operand as 8 halves
 * at a time: counts and channel widths are multiples of 8 and every fp16 pointer is 16-byte aligned (16-byte aligned pointers).  A
 * pointer that is not is refused with INVALID_ARGUMENT ("misaligned pointer") before any launch, the destination untouched.  y may
 * be x (or a, or b) itself; any other overlap is undefined. */
SDOD_API int sdod_geglu_f16(const void* x, void* y, int m, int c, void* stream); /* x:[M][2c] -> y = x[:, :c]*gelu(x[:, c:]); c % 8 == 0 */
SDOD_API int sdod_act_f16(const void* x, void* y, size_t n, int act, void* stream); /* n % 8 == 0 */
SDOD_API int sdod_add_f16(const void* a, const void* b, void* y, size_t n, void* stream); /* y = fp16((float)a + (float)b); n % 8 == 0 */
/* ---- Regional prompts.  Region masks -> per-pixel blend weights of the four UNet levels, one launch.
 * masks: uint8 [regions][8 h][8 w] at image resolution (255 = fully inside; soft and overlapping masks allowed), h x w the latent
 * size, both multiples of 8.  For ds = 1, 2, 4, 8: s_r = the integer sum of mask r over the (8 ds)^2 image pixels of a level pixel,
 * w_r = (float)s_r / (float)sum_r s_r (one correctly rounded division); where no region covers the pixel w_0 = 1, the others 0.
 * w1 / w2 / w4 / w8: fp32 [h / ds * w / ds][regions], row-major in pixels.  regions in [1, 4], masks 16-byte aligned. */
SDOD_API int sdod_region_weights_f32(const uint8_t* masks, int regions, int h, int w, float* w1, float* w2, float* w4, float* w8, void* stream);
/* out[m][j] = fp16(sum_r w[m % rows_per_img][r] * (float)a[r * region_stride + m * c + j]) for regions in [1, 4]: acc = w_0 a_0, then
 * acc = acc + w_r a_r for r = 1 .., every product and every sum rounded on its own in fp32 (no FMA).  a: fp16, `regions` tensors of
 * [rows][c] region_stride elements apart (>= rows * c, a multiple of 8); w: fp32 [rows_per_img][regions]; c % 8 == 0, rows_per_img
 * divides rows, a and out 16-byte aligned.  out may be a's first tensor. */
SDOD_API int sdod_region_blend_f16(const void* a, size_t region_stride, const float* w, void* out, int rows, int rows_per_img, int c, int regions,
                                   void* stream);
/* ---- Image prompts.  The per-pixel weights of the two cross-attention segments (text, image tokens) at the four
 * UNet levels, one launch: w1 / w2 / w4 / w8 fp32 [h / ds * w / ds][2] for ds = 1, 2, 4, 8.  Column 0 is 1.0f; column 1 is
 * scale * ((float)S / (float)(255 * (8 ds)^2)), S the integer sum of mask (uint8 [8 h][8 w], 255 = the image prompt fully applies)
 * over the level pixel, the division and the multiply each rounded once in fp32.  mask == NULL: scale everywhere.  h, w multiples of
 * 8 in [8, 1024]; scale finite and >= 0; mask 16-byte aligned. */
SDOD_API int sdod_ip_weights_f32(const uint8_t* mask, float scale, int h, int w, float* w1, float* w2, float* w4, float* w8, void* stream);
/* The CLIP vision tower's input side (graph kind SDOD_GRAPH_IMAGE_ENCODER).
 * sdod_patch_embed_u8_f16: img uint8 HWC [n][S][S][3], S a multiple of patch -> out fp16 [n * (S / patch)^2][kpad], the rows of the
 * patch-embedding GEMM, patches row-major.  Column c * p * p + dy * p + dx (the conv weight's flattening) is
 * fp16(((float)u / 255 - mean3[c]) / std3[c]), every operation rounded on its own in fp32; columns from 3 p * p up to kpad, which
 * must be 3 p * p rounded up to a multiple of 64, are zero.  mean3 / std3 are host pointers (CLIP's constants), std > 0.
 * sdod_vit_tokens_f16: patches fp16 [n][P][W] (the GEMM's output), class_embedding fp16 [W], position_embedding fp16 [P + 1][W],
 * LayerNorm weight / bias fp32 [W] -> out fp16 [n][P + 1][W]: row 0 = LN(class + pos_0), row 1 + i = LN(patch_i + pos_{1 + i}); fp32
 * math, one fp16 rounding. */
SDOD_API int sdod_patch_embed_u8_f16(const uint8_t* img, void* out, int n, int image_size, int patch, int kpad, const float* mean3, const float* std3,
                                     void* stream);
SDOD_API int sdod_vit_tokens_f16(const void* patches, const void* class_embedding, const void* position_embedding, const float* ln_weight,
                                 const float* ln_bias, void* out, int n, int num_patches, int width, float eps, void* stream);
/* y[r] = (a[r] | b[r]): a fp16 [rows][c0], b fp16 [rows][c1] -> y fp16 [rows][c0 + c1], a copy of the bits.  c0 % 8 == 0, c1 % 8 == 0,
 * 16-byte aligned pointers (see "Elementwise / glue" above). */
SDOD_API int sdod_concat_channels_f16(const void* a, const void* b, void* y, size_t rows, int c0, int c1, void* stream);
/* ---- T2I-Adapter structural control (graph kind SDOD_GRAPH_ADAPTER of include/sdod_engine.h).  Each of the four
 * checks its arguments and returns INVALID_ARGUMENT before any launch, the destination untouched; fp32 arithmetic, every operation
 * rounded on its own, one fp16 rounding of the result.
 * Input of the adapter: img uint8 HWC [n][h * factor][w * factor][ch] -> y fp16 NHWC [n][h][w][ch * factor * factor],
 *   y[b][i][j][c * factor * factor + dy * factor + dx] = fp16((float)img[b][i * factor + dy][j * factor + dx][c] / 255.0f)
 * (torch.nn.PixelUnshuffle's channel order).  factor must be 8, ch 1 or 3, y 16-byte aligned. */
SDOD_API int sdod_pixel_unshuffle_u8_f16(const uint8_t* img, void* y, int n, int h, int w, int ch, int factor, void* stream);
/* AvgPool2d(2) on NHWC fp16 [n][h][w][c] -> [n][h / 2][w / 2][c]: y = fp16(((a + b) + (c + d)) * 0.25f) with a = (2i, 2j),
 * b = (2i, 2j + 1), c = (2i + 1, 2j), d = (2i + 1, 2j + 1).  h and w even, c % 8 == 0, 16-byte aligned pointers. */
SDOD_API int sdod_avg_pool2_f16(const void* x, void* y, int n, int h, int w, int c, void* stream);
/* dst[i] = fp16(weight * (float)src[i]): an adapter output copied into a feature slot of the UNET graph with the conditioning weight
 * folded in.  count % 8 == 0, weight finite, 16-byte aligned pointers. */
SDOD_API int sdod_adapter_stage_f16(const void* src, void* dst, size_t count, float weight, void* stream);
/* The per-step launch: h fp16 [reps][per_copy] += f fp16 [per_copy] in place, h[r][i] = fp16((float)h[r][i] + (float)f[i]); one
 * thread loads its 16 bytes of f once and updates every copy.  reps 1 or 2 (the guidance copies, laid out as sdod_stage_unet_inputs
 * writes them), per_copy % 8 == 0, 16-byte aligned pointers. */
SDOD_API int sdod_add_feature_f16(void* h, const void* f, size_t per_copy, int reps, void* stream);
/* ---- ControlNet: the additions of cldm's ControlledUnetModel, hs[k] + control[k] for the twelve skip tensors and
 * h + control[12] for the middle output, as ONE launch over a by-value table of up to SDOD_CONTROL_MAX_SEGS segments:
 *   seg[k].h[i] = fp16((float)seg[k].h[i] + scales[k] * (float)seg[k].r[i]),  i < seg[k].count
 * in place, the product and the sum each rounded to fp32 on its own (no FMA).  16-byte lanes; every workgroup lies inside one
 * segment (up to 8192 halves of it).  scales is DEVICE memory, fp32 [count], read by the kernel: a captured launch picks up a new
 * weight.  A segment whose scale is exactly 0 is neither read nor written (its r may hold anything, its h keeps its bits).
 * count in [1, SDOD_CONTROL_MAX_SEGS]; every h and r non-null and 16-byte aligned, every seg count > 0 and % 8 == 0, scales 4-byte
 * aligned; otherwise INVALID_ARGUMENT before any launch, the destinations untouched.  Segments must not overlap (not checked). */
#define SDOD_CONTROL_MAX_SEGS 16
typedef struct sdod_control_seg {
    void* h;       /* fp16, updated in place */
    const void* r; /* fp16 residual, same length */
    size_t count;  /* halves */
} sdod_control_seg;
SDOD_API int sdod_add_control_f16(const sdod_control_seg* segs, int count, const float* scales, void* stream);
/* ---- FreeU (Si et al., CVPR 2024): what the method does at one decoder site, in place on the two fp16 NHWC tensors
 * the decoder is about to concatenate, h and skip, both [n][height][width][c].  params is DEVICE memory, fp32
 * [SDOD_FREEU_PARAMS] = {b1, s1, b2, s2, version (1 or 2), 0, 0, 0}, read by the kernels: a captured launch picks up new values.
 * stage 1 selects (b, s) = (b1, s1), stage 2 (b2, s2).
 *   skip: every channel plane v keeps all of its spectrum but the frequency set {0, -1 mod height} x {0, -1 mod width} (the box
 *         [H/2-1 : H/2+1, W/2-1 : W/2+1] of the published fftshift-ed mask, threshold 1), which is multiplied by s:
 *           out = fp16(v + (s - 1) / (H W) * Re sum_{(ky,kx) in the set} X[ky,kx] e^{+2 pi i (ky y / H + kx x / W)}),
 *         X the plane's DFT; fp32 sums in a fixed order, twiddles from sincospi, one rounding to fp16.
 *   h:    channels [0, c / 2) are multiplied by a factor, channels [c / 2, c) keep their bits.  version 1: factor = b, the result
 *         fp16((float)h * b).  version 2, per image: m[p] = fp32 mean over all c channels of pixel p, factor[p] =
 *         (b - 1) (m[p] - min m) / (max m - min m) + 1 -- and factor = 1 where max m == min m (a 1 x 1 map, a constant mean), the
 *         one departure from the published code, which divides 0 by 0 there.
 * Two launches, no atomics, the same bits every run: phases bit 0 = launch A (the filter, and the means of h into scratch, fp32
 * [n][height * width], which version 2 needs), bit 1 = launch B (min / max of the means and the scaling); 3 = both, in that order.
 * With s == 1 the filter's workgroups, with b == 1 the means' and launch B's, read params and end: nothing is read or written.
 * c % 128 == 0, height and width in [1, 1024], n in [1, 65535], h and skip 16-byte and params and scratch 4-byte aligned, all
 * non-null, stage 1 or 2; otherwise INVALID_ARGUMENT before any launch, the tensors untouched.  h, skip and scratch must not overlap. */
#define SDOD_FREEU_PARAMS 8
SDOD_API int sdod_freeu_f16(void* h, void* skip, int n, int height, int width, int c, const float* params, int stage, float* scratch,
                            int phases, void* stream);
SDOD_API int sdod_im2col3x3_small_f16(const void* x, void* y, int n_img, int h, int w, int c, int kpad, void* stream);
/* the same kernel with a circular border: wrap bit 0 = columns (x) wrap, bit 1 = rows (y) wrap; a wrapped tap reads pixel
 * (y mod h, x mod w) of its own image.  wrap = 0 is sdod_im2col3x3_small_f16, bit for bit. */
SDOD_API int sdod_im2col3x3_small_wrap_f16(const void* x, void* y, int n_img, int h, int w, int c, int kpad, int wrap, void* stream);
/* sdod_latent_prep_f16 (w = NULL) followed by sdod_im2col3x3_small_f16 in one launch: x NCHW fp32 [n][c][h][w] -> the im2col matrix
 * [n*h*w][kpad] fp16 of a 3x3 pad-1 convolution (k = tap * c + channel, zero beyond 9c), values (fp16)(x * scale); kpad % 8 == 0 */
SDOD_API int sdod_latent_im2col_f16(const float* x, void* y, int n_img, int h, int w, int c, int kpad, float scale, void* stream);

/* The UNet's input convolution in one launch (the reference's /input_blocks.0/Conv, analyze_results.py:69-79): x NCHW fp32
 * [n][c][h][w] (scaled by `scale`, rounded to fp16 as sdod_latent_im2col_f16 does) -> 3x3 pad-1 convolution with w fp16 [cout][64]
 * (k = tap * c + channel, zero beyond 9 c: the PK_CONV3_SMALL packing) + bias fp32 [cout] -> y NHWC fp16 [n*h*w][cout].
 * 9 * c <= 64; cout in {64, 128, 256, 320}.  Equals sdod_latent_im2col_f16 followed by the K = 64 sdod_gemm_f16. */
SDOD_API int sdod_conv_in_f16(const float* x, const void* w, const float* bias, void* y, int n_img, int h, int wd, int c, int cout,
                              float scale, void* stream);
/* sdod_conv_in_f16 with a circular border (seamless tiling): wrap bit 0 = x, bit 1 = y, as in sdod_im2col3x3_small_wrap_f16.
 * wrap = 0 is sdod_conv_in_f16, bit for bit (the old entry point forwards here). */
SDOD_API int sdod_conv_in_wrap_f16(const float* x, const void* w, const float* bias, void* y, int n_img, int h, int wd, int c, int cout,
                                   float scale, int wrap, void* stream);
/* The VAE encoder's input convolution in one launch: img uint8 HWC RGB [n][h][wd][3] -> x = fp16(2 * (u / 255) - 1) -> 3x3 pad-1
 * convolution with w fp16 [cout][64] (k = tap * 3 + channel, zero beyond 27: the PK_CONV3_SMALL packing) + bias fp32 [cout] -> y NHWC
 * fp16 [n*h*wd][cout].  cout in {64, 128, 256, 320}.  The same core as sdod_conv_in_f16: equals normalising, then
 * sdod_im2col3x3_small_f16 and the K = 64 sdod_gemm_f16, bit for bit. */
SDOD_API int sdod_image_conv_in_f16(const uint8_t* img, const void* w, const float* bias, void* y, int n_img, int h, int wd, int cout,
                                    void* stream);
/* The input convolution of a 9-channel inpainting UNet (ldm `conditioning_key: hybrid`) in one launch: sdod_conv_in_f16 on the channel
 * concatenation of x NCHW fp32 [n][c][h][w] and cond NCHW fp32 [n][c_cond][h][w], which is never written.  64 < 9 (c + c_cond) <= 96;
 * w fp16 [cout][128] (k = tap * (c + c_cond) + channel, zero from 9 (c + c_cond): the PK_CONV3_SMALL packing of such a Cin), of which
 * only the first 96 columns of a row are read (three K steps of 32); cout in {64, 128, 256, 320}.  The same products as
 * sdod_latent_im2col_f16 (kpad = 128) of the concatenated tensor followed by the K = 128 sdod_gemm_f16 on the same w. */
SDOD_API int sdod_conv_in_cat_f16(const float* x, const float* cond, const void* w, const float* bias, void* y, int n_img, int h, int wd,
                                  int c, int c_cond, int cout, void* stream);
/* sdod_image_conv_in_f16 on the masked image of inpainting, in the encoder's normalised space: a pixel is 0.0 where
 * mask uint8 [n][h][wd] >= 128 and fp16(2 * (u / 255) - 1) elsewhere (0.0 is not the image of any uint8 value, so the masked image
 * cannot be prepared as bytes).  With an all-zero mask the result is sdod_image_conv_in_f16's, bit for bit. */
SDOD_API int sdod_masked_image_conv_in_f16(const uint8_t* img, const uint8_t* mask, const void* w, const float* bias, void* y, int n_img,
                                           int h, int wd, int cout, void* stream);
/* sdod_image_conv_in_f16 in the [0, 1] space: x = fp16(u / 255), zero padding in THAT space (RRDBNet's conv_first; graph kind
 * SDOD_GRAPH_UPSCALER).  Not a re-parametrisation of the encoder's entry point: there the border taps see 0 where this space has
 * -1 -> 0.5, so folding the affine map into weights and bias is wrong on the border pixels.  Same kernel, arguments and checks.
 * y2 (may be NULL): a second copy of the result with pixel stride ld2 halves (ld2 % 8 == 0, ld2 >= cout, 16-byte aligned) -- the
 * upscaler keeps y for the trunk's skip while the first dense block updates the copy inside its wide buffer in place. */
SDOD_API int sdod_image_conv_in_unit_f16(const uint8_t* img, const void* w, const float* bias, void* y, void* y2, int ld2, int n_img, int h,
                                         int wd, int cout, void* stream);

/* ---- ESRGAN upscaler: the 3x3, stride 1, zero-pad-1 convolution of RRDBNet's residual dense block, NHWC fp16 with
 * fp32 accumulation, reading a channel prefix of a wide pixel row and writing a column slice of a (possibly the same) wide row:
 *   acc[pixel][o] = sum_{tap, c < cin} in[pixel + tap][c] * w[o][tap * cin + c]          (w: the KRSC packing [cout][9 cin])
 *   y = alpha * (acc + bias[o]);  if slope != 0: y = y < 0 ? slope * y : y;  if res1: y += c1 * res1[pixel][o];
 *   if res2: y += res2[pixel][o];  out[pixel][out_col + o] = fp16(y)                       (fp32 throughout, one rounding)
 * in: [n][h][w_in] pixels of ld_in halves, of which channels [0, cin) are read and NOTHING else (K is walked in 32-channel chunks;
 * the other channels may hold Inf or NaN).  cin in {64, 96, 128, 160, 192}, cout in {32, 64}.  upsample = 1: nearest-2x in front of
 * the convolution, output [n][2h][2w_in] (conv_up1 / conv_up2).  res1 / res2 point at channel 0 of the residual slice of pixel 0
 * and are read at the output pixel only, by the thread that writes it: either may be the written slice itself (the last
 * convolution of an RRDB adds the block input it overwrites).  out may be the input buffer when the written columns are disjoint
 * from [0, cin) (convolutions 1 to 4 of a dense block: ld_out = ld_in, out_col >= cin).  Any n, h, w_in >= 1 with fewer than 2^31
 * output pixels: tiles are clipped at the image edge.
 * Errors (INVALID_ARGUMENT before any launch, destination untouched): a null in / w / out; a pointer that is not 16-byte aligned;
 * another cin or cout; ld_in < cin, or a stride or out_col that is not a multiple of 8; out_col + cout > ld_out; a geometry outside
 * the above; a non-finite coefficient; a written slice that overlaps the channels read (with upsample: the input at all); a
 * residual that overlaps the written slice without being that slice or other columns of the same pixel rows. */
typedef struct sdod_dense_conv_desc {
    const void* in;     /* fp16 [n][h][w_in][ld_in] */
    const void* w;      /* fp16 [cout][9 * cin] */
    const float* bias;  /* fp32 [cout] or NULL */
    void* out;          /* fp16 [n][h_out][w_out][ld_out]; columns [out_col, out_col + cout) are written */
    const void* res1;   /* fp16, pixel stride ld_res1, or NULL */
    const void* res2;   /* fp16, pixel stride ld_res2, or NULL */
    int ld_in, ld_out, ld_res1, ld_res2;
    int out_col;
    int cin, cout;
    int n, h, w_in;
    int upsample;
    float alpha, slope, c1;
} sdod_dense_conv_desc;
SDOD_API int sdod_dense_conv3x3_f16(const sdod_dense_conv_desc* d, void* stream);
/* 1 when the call above takes the descriptor, 0 when it would refuse it.  Host-only. */
SDOD_API int sdod_dense_conv3x3_ok(const sdod_dense_conv_desc* d);

/* The conditioning input of a 9-channel inpainting UNet in one launch: cond fp32 [reps][n][1 + c][h_lat][w_lat] with
 *   channel 0      = mask_u8[i][8 y][8 x] >= 128 ? 1 : 0   (F.interpolate(mask, size=(h_lat, w_lat)), nearest, of the binarised mask;
 *                                                           mask_u8 uint8 [n][8 h_lat][8 w_lat])
 *   channels 1..c  = 0.18215 * (mean + exp(0.5 * clamp(logvar, -30, 20)) * n1) from moments fp32 NCHW [n][2c][h_lat][w_lat] (the VAE
 *                    encoder's output for the masked image): sdod_encode_latent_f32's z0, bit for bit.
 * n1 fp32 [n][c][h_lat][w_lat], or NULL: drawn in the kernel, image i's values those of sdod_randn_f32(c * h_lat * w_lat, seed,
 * (1 << 32) | (image_index0 + i)).  `reps` identical copies back to back (the two classifier-free-guidance halves).
 * Errors (nothing written): NULL moments / mask / cond, factor != 8, h_lat * w_lat % 4 != 0, cond or n1 not 16-byte aligned. */
SDOD_API int sdod_inpaint_cond_f32(const float* moments, const uint8_t* mask_u8, const float* n1, float* cond, int n, int c, int h_lat,
                                   int w_lat, int factor, int reps, uint64_t seed, uint64_t image_index0, void* stream);
/* ldm img2img's latent start in one launch.  moments fp32 NCHW [n][2c][h][w] (mean = channels [0, c), logvar = [c, 2c)):
 *   std = exp(0.5 * clamp(logvar, -30, 20)); z0 = 0.18215 * (mean + std * n1)      (DiagonalGaussianDistribution.sample,
 *   x = sqrt_at * z0 + sqrt_one_minus_at * n2                                          get_first_stage_encoding, stochastic_encode)
 * x, z0, n1, n2: fp32 NCHW [n][c][h][w]; z0 may be NULL.  n1 / n2 NULL: drawn in the kernel, image i's values exactly those of
 * sdod_randn_f32(count = c*h*w, seed, stream_id = (1 << 32) | (image_index0 + i)) for n1 and (2 << 32) | (image_index0 + i) for n2. */
SDOD_API int sdod_encode_latent_f32(const float* moments, const float* n1, const float* n2, float* x, float* z0, int n, int c, int hw,
                                    float sqrt_at, float sqrt_one_minus_at, uint64_t seed, uint64_t image_index0, void* stream);
/* The latent resize between the two sampler trajectories of the hires pass, with img2img's start-latent formula, in one launch:
 *   dst = a * R(src) + b * nu          src fp32 NCHW [n][c][h_in][w_in], dst fp32 NCHW [n][c][h_out][w_out]
 * R = torch.nn.functional.interpolate(size=(h_out, w_out), align_corners=False, antialias=False).  Per axis, output coordinate d:
 *   mode 0 nearest-exact: index min(floor((2 d + 1) n_in / (2 n_out)), n_in - 1), integer arithmetic
 *   mode 1 bilinear:      s = max(((2 d + 1) n_in - n_out) / (2 n_out), 0), i0 = floor(s), i1 = min(i0 + 1, n_in - 1), t = s - i0,
 *                         weights 1 - t, t
 *   mode 2 bicubic:       s without the clamp, i = floor(s), t = s - i, taps i - 1 .. i + 2 clamped to [0, n_in - 1], weights
 *                         c2(t + 1), c1(t), c1(1 - t), c2(2 - t) with c1(x) = ((A + 2) x - (A + 3)) x^2 + 1,
 *                         c2(x) = ((A x - 5 A) x + 8 A) x - 4 A, A = -0.75
 * floor(s) and the remainder come from an integer division, so t is an exact rational rounded once; the weights are evaluated in
 * fp64 and rounded once to fp32 (one function for host and device), the sums run in fp32, x first, then y.  The error does not grow
 * with the coordinate.  n_in == n_out copies the source bit for bit in every mode.
 * Taps of weight 0 are neither read nor added (that is what makes the copy exact), so a non-finite source value does not propagate
 * through a zero-weight tap: where torch gives NaN from 0 * inf or 0 * NaN (bilinear with t == 0, the integer ratios), this gives the
 * finite sum of the other taps.
 * nu: none is read or drawn when b == 0; else `noise` fp32 [n][c][h_out][w_out], or when NULL drawn in the kernel, image i's values
 * exactly those of sdod_randn_f32(c * h_out * w_out, seed, (2 << 32) | (image_index0 + i)) (sdod_encode_latent_f32's n2 family).
 * No alignment or divisibility assumption on any size.  Errors, returned before any device call (dst untouched): NULL src or dst, a
 * size below 1, an unknown mode, a non-finite a or b, dst overlapping src. */
SDOD_API int sdod_latent_resize_f32(const float* src, float* dst, int n, int c, int h_in, int w_in, int h_out, int w_out, int mode, float a,
                                    float b, const float* noise, uint64_t seed, uint64_t image_index0, void* stream);
/* Host only: the per-axis table sdod_latent_resize_f32 uses, idx int32 [n_out][4] and w fp32 [n_out][4]; unused slots hold index 0
 * and weight 0. */
SDOD_API int sdod_latent_resize_taps(int mode, int n_in, int n_out, int32_t* idx, float* w);
/* y(NHWC fp16)[img][pix][ch] = fp16(fp32(x(NCHW fp32)[img][ch][pix] * scale)): the fp32 product, rounded, is what is rounded to fp16
 * (nearest even; beyond 65519.99 the infinity of its sign, fp16 subnormals kept) -- two roundings, not one rounding of the exact
 * product.  No alignment or divisibility requirement. */
SDOD_API int sdod_nchw_f32_to_nhwc_f16(const float* x, void* y, int n, int c, int hw, float scale, void* stream);
/* y(NHWC fp16)[img][pix][o] = sum_c w[o][c]*(scale*x(NCHW fp32)[img][c][pix]) + b[o]; w/b fp32 [c][c]/[c] or NULL
 * (identity).  Folds ldm's z/0.18215 and first_stage_model.post_quant_conv into the layout change.  fp32 accumulation from b[o] (or
 * 0) through the channels in order, one fp16 rounding; c <= 16.  With w and b both NULL the result is sdod_nchw_f32_to_nhwc_f16's
 * bit for bit, the sign of a zero included. */
SDOD_API int sdod_latent_prep_f16(const float* x, const float* w, const float* b, void* y, int n, int c, int hw,
                                  float scale, void* stream);
SDOD_API int sdod_nhwc_f16_to_nchw_f32(const void* x, float* y, int n, int c, int hw, void* stream);
/* y[r][j] = fp16((float)table[ids[r]][j] + (float)pos[r % seq][j]): table fp16 [vocab][c], pos fp16 [seq][c], ids int32 [rows] (each in
 * [0, vocab): not checked) -> y fp16 [rows][c].  c % 8 == 0; table, pos and y 16-byte aligned pointers, ids 4-byte. */
SDOD_API int sdod_embedding_f16(const int32_t* ids, const void* table, const void* pos, void* y, int rows, int seq,
                                int c, void* stream);
/* Long, weighted prompts: the cross-attention context of P prompts from their K text-encoder chunks, in one launch.
 * enc fp16 [P][K][T][D] (the text encoder's rows, chunk after chunk) -> out fp16 [P][K*T][D]: the same memory order, so the
 * concatenation along the key axis is the layout itself and the kernel only applies the per-token emphasis w fp32 [P][K][T].
 * Per (prompt, chunk), in fp32 on the fp16 values:  s0 = sum x,  s1 = sum fl(x * w[t])  over the chunk's T * D values,
 * r = s0 / s1,  out = fp16(fl(fl(x * w[t]) * r)) -- scale the token rows, then restore the chunk's mean (the rule of the common
 * web front ends, applied per chunk).  Guard: r = 1 when s1 == 0 or r is not finite (a chunk whose weights are all zero comes out
 * as zeros, a weighted sum that cancels leaves the weighted rows unrestored) -- never NaN or inf from finite input.
 * Deterministic: both sums are taken in one fixed order, so all-ones weights give s0 == s1 and out == enc bit for bit.
 * w == NULL: a plain copy, no sums.  One workgroup per (prompt, chunk), 16-byte lanes.
 * Errors, returned before any device call: NULL enc / out; P, K or T < 1; D % 8 != 0; enc or out not 16-byte aligned; out
 * overlapping enc. */
SDOD_API int sdod_context_assemble_f16(const void* enc, const float* w, void* out, int P, int K, int T, int D, void* stream);
/* context.cpp:257-274: out[i][j]=cos(t_i*f_j), out[i][half+j]=sin(t_i*f_j), f_j=exp(-ln(1e4)*j/half); fp16 out */
SDOD_API int sdod_timestep_features_f16(const float* t, void* y, int n, int dim, void* stream);
/* The guidance-scale embedding of a full LCM checkpoint (diffusers get_guidance_scale_embedding; host form: sdod/amd/samplers.py,
 * guidance_embedding): v = (w_i - 1) * 1000, f_j = exp(-ln(1e4) * j / (half - 1)), out[i][j] = sin(v * f_j), out[i][half + j] =
 * cos(v * f_j) with half = dim / 2 -- sine first and the divisor half - 1, both unlike sdod_timestep_features_f16.  w fp32 [n], out
 * fp16 [n][dim].  The argument reaches 14 000 rad at w = 15 and goes through the range-reduced sinf / cosf; f_j is rounded once
 * from fp64, v and the product are fp32.  dim must be even and at least 4. */
SDOD_API int sdod_guidance_features_f16(const float* w, void* y, int n, int dim, void* stream);

/* Inputs of one guided UNet evaluation in one launch (host loop: context.cpp:348-349): x (fp32, lat_count values = n
 * images) -> x_dst written `reps` times back to back; temb_row (fp16, temb_width) -> temb_dst, `temb_reps` rows. */
SDOD_API int sdod_stage_unet_inputs(const float* x, float* x_dst, size_t lat_count, int reps, const void* temb_row,
                                    void* temb_dst, size_t temb_width, int temb_reps, void* stream);
/* x_T ~ N(0, I) on the device (replaces the host generator of context.cpp:333-334 for throughput runs): Philox4x32-10
 * keyed by `seed`, counter (i / 4, stream_id), Box-Muller on the word pairs (0,1), (2,3) with u = ((w >> 8) + 0.5) / 2^24.
 * words_out (optional, uint32[count]) receives the raw Philox words for bit-exact checks. */
SDOD_API int sdod_randn_f32(float* out, uint32_t* words_out, size_t count, uint64_t seed, uint64_t stream_id, void* stream);

/* Classifier-free guidance on the batched UNet output.  eps_nhwc: fp16 NHWC [2n][hw][c]; rows [0,n) are the
 * unconditional half when uncond_first != 0 (ldm ordering), else the conditional half.  e_out: fp32 NCHW [n][c][hw].
 *   mode 0: e = g*e_cond + (1-g)*e_uncond         -- the reference driver (context.cpp:359-373, libsdod.h:88)
 *   mode 1: e = e_uncond + g*(e_cond - e_uncond)  -- ldm's PLMS/DDIM samplers (config 1's CPU reference) */
SDOD_API int sdod_cfg_combine(const void* eps_nhwc, float* e_out, int n, int c, int hw, float guidance,
                              int uncond_first, int mode, void* stream);
/* DPM-Solver++(2M) update, dpm_solver.cpp:136-181, on fp32 device vectors of `count` elements, same operation
 * order and no FMA contraction (bit-identical to the host loop for identical inputs):
 *   y = (x - sigma_s*eps)/alpha_s ; x = sigma_ratio*x (+ c_prev*y_prev if order==2) + c_cur*y ; y_prev = y
 * with sigma_ratio = sigma[s+1]/sigma[s], c_prev = alpha[s+1]*phi[s+1]*i2r[s+1],
 * c_cur = -alpha[s+1]*phi[s+1] (order 1) or -alpha[s+1]*phi[s+1]*(1+i2r[s+1]) (order 2), all from the host tables. */
SDOD_API int sdod_dpm_update(float* x, const float* eps, float* y_prev, size_t count, int order, float sigma_s,
                             float alpha_s, float sigma_ratio, float c_prev, float c_cur, void* stream);
/* ldm DDIM/PLMS step (eta=0): x0 = (x - sqrt(1-abar_t)*e)/sqrt(abar_t); x = sqrt(abar_prev)*x0 + dir_coef*e */
SDOD_API int sdod_ddim_step_f32(float* x, const float* e, size_t count, float sqrt_one_minus_at, float sqrt_at,
                                float sqrt_a_prev, float dir_coef, void* stream);
/* out = (c0*e0 + c1*e1 + c2*e2 + c3*e3)/div, left to right (PLMS Adams-Bashforth combinations); e1..e3 may be NULL, each on its
 * own (a NULL term is left out whatever its coefficient; e2 may be given without e1).  Every product, sum and the quotient is
 * rounded on its own in fp32.  div == 0 is refused with INVALID_ARGUMENT, out untouched.  out may be any of the inputs. */
SDOD_API int sdod_lincomb4_f32(float* out, const float* e0, const float* e1, const float* e2, const float* e3,
                               float c0, float c1, float c2, float c3, float div, size_t count, void* stream);

/* One PLMS step behind a UNet evaluation in one launch (Python host loop, sdod/amd/pipeline.py: sample_plms; the reference's
 * sampler is ldm's PLMSSampler.p_sample_plms): e_t = CFG(eps) [sdod_cfg_combine; optional v -> eps conversion
 * e_t = vc0 * e + vc1 * x], e' = (c0 e_t + c1 old1 + c2 old2 + c3 old3) / div [sdod_lincomb4_f32], x <- DDIM step with e'
 * [sdod_ddim_step_f32], then the next evaluation's inputs [sdod_stage_unet_inputs: x into x_stage[stage_reps][..], temb_row into
 * temb_dst[temb_reps][..]]; the same fp32 operations in the same order as those four calls, bit for bit.  old1..3, x_stage,
 * temb_row may be NULL. */
typedef struct sdod_plms_update_args {
    const void* eps_nhwc;   /* fp16 [2n][hw][c] */
    float* e_out;           /* fp32 [n][c][hw]: e_t, kept by the caller as history */
    float* x;               /* fp32 [n][c][hw], updated in place */
    const float* old1; const float* old2; const float* old3;
    float* x_stage;         /* fp32 [stage_reps][n][c][hw] or NULL */
    const void* temb_row;   /* fp16 [temb_width] or NULL */
    void* temb_dst;         /* fp16 [temb_reps][temb_width] */
    int n, c, hw, uncond_first, mode, v_pred, stage_reps, temb_width, temb_reps;
    float guidance, vc0, vc1, c0, c1, c2, c3, div, sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef;
} sdod_plms_update_args;
SDOD_API int sdod_plms_update(const sdod_plms_update_args* a, void* stream);

/* The reference driver's per-step arithmetic behind a UNet evaluation in one launch (src/context.cpp:359-373: CFG; src/dpm_solver.cpp:
 * 139-180: DPM-Solver++(2M) update; :348-352: staging of the next step's inputs): sdod_cfg_combine + sdod_dpm_update +
 * sdod_stage_unet_inputs, the same fp32 operations in the same order, bit for bit.  e_out, x_stage, temb_row may be NULL. */
typedef struct sdod_dpm_step_args {
    const void* eps_nhwc;   /* fp16 [2n][hw][c] */
    float* e_out;           /* fp32 [n][c][hw] or NULL */
    float* x;               /* fp32 [n][c][hw], updated in place */
    float* y_prev;          /* fp32 [n][c][hw], read (order 2) and replaced */
    float* x_stage;         /* fp32 [stage_reps][n][c][hw] or NULL */
    const void* temb_row;   /* fp16 [temb_width] or NULL */
    void* temb_dst;         /* fp16 [temb_reps][temb_width] */
    int n, c, hw, uncond_first, mode, order, stage_reps, temb_width, temb_reps;
    float guidance, sigma_s, alpha_s, sigma_ratio, c_prev, c_cur;
} sdod_dpm_step_args;
SDOD_API int sdod_dpm_step(const sdod_dpm_step_args* a, void* stream);

/* One DDIM step (eta = 0) behind a UNet evaluation in one launch, with inpainting's latent blend (ldm DDIMSampler.ddim_sampling
 * (mask=, x0=); Python host loop: sdod/amd/pipeline.py, sample_ddim_inpaint):
 *   e  = CFG(eps) [sdod_cfg_combine; optional v -> eps conversion e = vc0 * e + vc1 * x, sdod_lincomb4_f32]
 *   x' = DDIM step of x with e [sdod_ddim_step_f32]
 *   known = known_sa * z0 + known_s1a * nu  (ldm q_sample of the clean latent z0 to the level x' has reached), or z0 when last != 0
 *   x  = keep * known + (1 - keep) * x'     (ldm: img_orig * mask + (1. - mask) * img; keep broadcast over the c channels)
 * then the next evaluation's inputs [sdod_stage_unet_inputs: x into x_stage[stage_reps][..], temb_row into temb_dst[temb_reps][..]].
 * Every product, sum and difference is rounded on its own in fp32 (no FMA contraction): the bits of the separate launches
 * followed by an elementwise fp32 blend.  nu: `noise` fp32 [n][c][hw], or when NULL drawn in the kernel, image i's values exactly
 * those of sdod_randn_f32(count = c * hw, seed, stream_id = ((3 + noise_level) << 32) | (image_index0 + i)) (streams 1 and 2 belong
 * to sdod_encode_latent_f32); with last != 0 no noise is drawn or read.  keep == NULL: a plain fused DDIM step, x = x' (z0, noise,
 * known_* and last are ignored).  c * hw must be a multiple of 4; x, z0, noise and x_stage 16-byte aligned (they move as 16-byte
 * lanes).  x_stage, temb_row may be NULL. */
typedef struct sdod_ddim_inpaint_step_args {
    const void* eps_nhwc;   /* fp16 [2n][hw][c] */
    float* x;               /* fp32 [n][c][hw], updated in place */
    const float* z0;        /* fp32 [n][c][hw]: the clean latent of the init image (needed when keep is given) */
    const float* keep;      /* fp32 [n][hw]: 1 = keep the init image, 0 = repaint; NULL = no blend */
    const float* noise;     /* fp32 [n][c][hw] or NULL (drawn in the kernel) */
    float* x_stage;         /* fp32 [stage_reps][n][c][hw] or NULL */
    const void* temb_row;   /* fp16 [temb_width] or NULL */
    void* temb_dst;         /* fp16 [temb_reps][temb_width] */
    uint64_t seed, image_index0;
    int n, c, hw, uncond_first, mode, v_pred, last, noise_level, stage_reps, temb_width, temb_reps;
    float guidance, vc0, vc1, sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef, known_sa, known_s1a;
} sdod_ddim_inpaint_step_args;
SDOD_API int sdod_ddim_inpaint_step(const sdod_ddim_inpaint_step_args* a, void* stream);

/* One step of a k-diffusion sampler (Euler, Euler ancestral, DPM++ 2M; host tables: sdod/amd/samplers.py, KSchedule.coef) behind a
 * UNet evaluation in one launch.  The three published algorithms reduce to one linear form in the unscaled latent x:
 *   e   = CFG(eps)                                              [sdod_cfg_combine]
 *   den = d0 * x + d1 * e                                       [sdod_lincomb4_f32([x, e], [d0, d1], 1)]
 *   x'  = a * x + b * den (+ cprev * den_prev) (+ u * nu)       [sdod_lincomb4_f32, left to right; the den_prev term only when
 *                                                                cprev != 0, the nu term only when u != 0]
 *   den_prev <- den (when den_prev is given);  x <- x'
 * then the next evaluation's inputs: x_stage[r] = stage_scale * x' (one fp32 multiply: the model sees c_in * x) and temb_row into
 * temb_dst[temb_reps][..] as sdod_stage_unet_inputs does.  Every product and sum is rounded on its own in fp32 (no FMA contraction):
 * the bits of those separate launches.  nu: `noise` fp32 [n][c][hw], or when NULL drawn in the kernel, image i's values exactly those
 * of sdod_randn_f32(count = c * hw, seed, stream_id = ((3 + noise_level) << 32) | (image_index0 + i)); with u == 0 no noise is drawn or
 * read.  eps_nhwc == NULL is the start form in front of the loop: x <- a * x, then the staging (b, cprev and u must be 0).
 * c * hw must be a multiple of 4; x, den_prev, noise and x_stage 16-byte aligned (they move as 16-byte lanes); every scalar finite.
 * den_prev, noise, x_stage, temb_row may be NULL. */
typedef struct sdod_k_step_args {
    const void* eps_nhwc;   /* fp16 [2n][hw][c], or NULL: the start form */
    float* x;               /* fp32 [n][c][hw], updated in place */
    float* den_prev;        /* fp32 [n][c][hw] or NULL: read when cprev != 0, then replaced by this step's den */
    const float* noise;     /* fp32 [n][c][hw] or NULL (drawn in the kernel); touched only when u != 0 */
    float* x_stage;         /* fp32 [stage_reps][n][c][hw] or NULL */
    const void* temb_row;   /* fp16 [temb_width] or NULL */
    void* temb_dst;         /* fp16 [temb_reps][temb_width] */
    uint64_t seed, image_index0;
    int n, c, hw, uncond_first, mode, noise_level, stage_reps, temb_width, temb_reps;
    float guidance, d0, d1, a, b, cprev, u, stage_scale;
} sdod_k_step_args;
SDOD_API int sdod_k_step(const sdod_k_step_args* a, void* stream);

/* One step of a Latent Consistency Model (Luo et al. 2023; host tables: sdod/amd/samplers.py, LcmSchedule.coef; host loop:
 * sdod/amd/pipeline.py, sample_lcm) behind a UNet evaluation in one launch.  In the unscaled latent x:
 *   e   = CFG(eps) when guided != 0                             [sdod_cfg_combine]
 *         float(eps[img]) when guided == 0: one row per image   [sdod_nhwc_f16_to_nchw_f32; guidance, mode, uncond_first are ignored]
 *   den = d0 * x + d1 * e                                       [sdod_lincomb4_f32([x, e], [d0, d1], 1): the x0 prediction]
 *   x'  = a * x + b * den (+ u * nu)                            [sdod_lincomb4_f32, left to right; the x term is left out when a == 0, the
 *                                                                nu term when u == 0]
 *   den_out <- den (when den_out is given);  x <- x'
 * then the next evaluation's inputs: x_stage[r] = x' UNSCALED (the model sees x itself) and temb_row into temb_dst[temb_reps][..] as
 * sdod_stage_unet_inputs does.  Every product and sum is rounded on its own in fp32 (no FMA contraction): the bits of those separate
 * launches.  nu: `noise` fp32 [n][c][hw], or when NULL drawn in the kernel, image i's values exactly those of sdod_randn_f32(count =
 * c * hw, seed, stream_id = ((3 + noise_level) << 32) | (image_index0 + i)); with u == 0 no noise is drawn or read.
 * Refused with INVALID_ARGUMENT before any launch: a NULL eps_nhwc or x; n, c or hw below 1; c * hw not a multiple of 4; x, den_out,
 * noise or x_stage not 16-byte aligned; a non-finite scalar; guided with a mode other than 0 or 1; temb_row without temb_dst; x_stage
 * without stage_reps.  den_out, noise, x_stage, temb_row may be NULL. */
typedef struct sdod_lcm_step_args {
    const void* eps_nhwc;   /* fp16 [guided ? 2n : n][hw][c] */
    float* x;               /* fp32 [n][c][hw], updated in place */
    float* den_out;         /* fp32 [n][c][hw] or NULL: this step's x0 prediction */
    const float* noise;     /* fp32 [n][c][hw] or NULL (drawn in the kernel); touched only when u != 0 */
    float* x_stage;         /* fp32 [stage_reps][n][c][hw] or NULL */
    const void* temb_row;   /* fp16 [temb_width] or NULL */
    void* temb_dst;         /* fp16 [temb_reps][temb_width] */
    uint64_t seed, image_index0;
    int n, c, hw, guided, uncond_first, mode, noise_level, stage_reps, temb_width, temb_reps;
    float guidance, d0, d1, a, b, u;
} sdod_lcm_step_args;
SDOD_API int sdod_lcm_step(const sdod_lcm_step_args* a, void* stream);

/* sdod_k_step on a MultiDiffusion canvas (Bar-Tal et al. 2023; host loop: sdod/amd/pipeline.py, sample_panorama; host tables:
 * sdod/amd/panorama.py): the UNet ran on ny * nx overlapping windows [wh][ww] of ONE canvas latent x [c][H][W]; window w = iy * nx + ix
 * covers rows oy[iy] .. + wh and columns ox[ix] .. + ww (with wrap_x the columns modulo W) and lies in chunk w / n of the predictions,
 * unconditional row w % n, conditional row n + w % n.  Per canvas element, with the covering windows taken in ascending w:
 *   acc = 0 ;  acc = acc + wgt[window pixel] * CFG_w     [CFG_w: sdod_cfg_combine of window w's pair at that window pixel]
 *   e   = acc / wsum[canvas pixel]                        [one IEEE-correct fp32 division]
 *   den = d0 * x + d1 * e ;  x' = a * x + b * den (+ cprev * den_prev) (+ u * nu) ;  den_prev <- den ;  x <- x'     [as sdod_k_step]
 * then x_stage (window w, both of its rows) = stage_scale * x' at every window pixel that covers the element, and temb_row into
 * temb_dst[temb_reps][..].  Every product, sum and quotient is rounded on its own in fp32 (no FMA contraction).  The rows of a partly
 * filled last chunk (ny * nx < chunks * n) are neither read nor written.  nu: `noise` fp32 [c][H][W], or when NULL drawn in the kernel,
 * exactly the values of sdod_randn_f32(count = c * H * W, seed, stream_id = ((3 + noise_level) << 32) | image_index0); with u == 0 no
 * noise is drawn or read.  eps == NULL is the start form: x <- a * x, then the staging (b, cprev and u must be 0).
 * wsum is the host's sum of wgt over the covering windows in the same order (panorama.weight_sum); a pixel no window covers has
 * wsum 0 and gets 0 / 0.  Refused with INVALID_ARGUMENT before any launch: a NULL x / wgt / wsum; x, den_prev, noise or x_stage not
 * 16-byte aligned, wgt or wsum not 4-byte, eps not 2-byte aligned; a non-finite scalar; c * wh * ww or c * H * W not a multiple of 4;
 * wh, ww, W or an origin not a multiple of 4; ny or nx outside [1, SDOD_PANO_MAX_AXIS]; an origin outside the canvas (oy + wh > H;
 * ox + ww > W without wrap, ox >= W with it); ww > W with wrap; ny * nx > chunks * n; cprev != 0 without den_prev.  den_prev, noise,
 * x_stage, temb_row may be NULL. */
#define SDOD_PANO_MAX_AXIS 32
typedef struct sdod_k_step_windows_args {
    const void* eps;        /* fp16 [chunks][2n][wh * ww][c], or NULL: the start form */
    float* x;               /* fp32 [c][H][W], updated in place */
    float* den_prev;        /* fp32 [c][H][W] or NULL: read when cprev != 0, then replaced by this step's den */
    const float* noise;     /* fp32 [c][H][W] or NULL (drawn in the kernel); touched only when u != 0 */
    const float* wgt;       /* fp32 [wh * ww]: the weight of a window pixel */
    const float* wsum;      /* fp32 [H * W]: the sum of the covering windows' weights */
    float* x_stage;         /* fp32 [chunks][2n][c][wh * ww] or NULL */
    const void* temb_row;   /* fp16 [temb_width] or NULL */
    void* temb_dst;         /* fp16 [temb_reps][temb_width] */
    uint64_t seed, image_index0;
    int c, H, W, wh, ww, ny, nx, wrap_x, n, chunks, mode, noise_level, temb_width, temb_reps;
    int oy[SDOD_PANO_MAX_AXIS], ox[SDOD_PANO_MAX_AXIS];
    float guidance, d0, d1, a, b, cprev, u, stage_scale;
} sdod_k_step_windows_args;
SDOD_API int sdod_k_step_windows(const sdod_k_step_windows_args* a, void* stream);
/* Inpainting's latent keep-mask: mask_u8 uint8 [n][factor * h_lat][factor * w_lat] (255 = repaint, 0 = keep) -> keep fp32
 * [n][h_lat][w_lat] = float(16320 - S) / 16320.0f with S the integer sum of the latent pixel's 8 x 8 block (16320 = 64 * 255; one
 * correctly rounded fp32 division).  factor must be 8 (the VAE's scale); mask_u8 8-byte aligned. */
SDOD_API int sdod_mask_to_latent_f32(const uint8_t* mask_u8, float* keep, int n, int h_lat, int w_lat, int factor, void* stream);
/* Inpainting's pixel composite: img fp16 NHWC [n][hw][3], init_u8 / out_u8 uint8 [n][hw][3], mask_u8 uint8 [n][hw].  Per byte, with
 * d = the value sdod_image_to_u8(a, b, mode) gives (the same device function), u the init byte, k the pixel's mask byte:
 * out = (d * k + u * (255 - k) + 127) / 255 in integer arithmetic; k = 0 returns u, k = 255 returns d. */
SDOD_API int sdod_image_composite_u8(const void* img, const uint8_t* init_u8, const uint8_t* mask_u8, uint8_t* out_u8, int n, size_t hw,
                                     float a, float b, int mode, void* stream);
/* img: fp16 NHWC [n][hw][3] -> uint8 HWC per image, f = a*v+b, truncating cast:
 *   mode 0: clamp(255*f, 0, 255)   (context.cpp:392-395; a=1,b=0 is the reference's already-[0,1] convention)
 *   mode 1: 255*clamp(f, 0, 1)     (ldm txt2img with a=0.5, b=0.5)
 * fp32 throughout, the product a*v, the sum with b and the product with 255 each rounded on its own; clamp(f, lo, hi) is
 * fminf(fmaxf(f, lo), hi), which returns the bound when f is NaN.  So in both modes a NaN pixel (or a NaN f, as from a = 0 on an
 * infinite pixel) gives 0, f = +inf gives 255, f = -inf gives 0, and -0 gives 0: every fp16 bit pattern has a defined byte. */
SDOD_API int sdod_image_to_u8(const void* img, uint8_t* out, size_t count, float a, float b, int mode, void* stream);

SDOD_API const char* sdod_hip_last_error(void);
SDOD_API int sdod_hip_device_info(int* cu_count, size_t* hbm_bytes, char* arch, int arch_len);

/* touch every 128-byte line of [ptr, ptr + bytes) once (a few workgroups on `stream`): the engine pulls the weights of the
 * deep, weight-heavy GEMMs towards the Infinity Cache a few launches ahead of their consumer (engine.hip: Graph::run_ops) */
SDOD_API int sdod_l2_prefetch(const void* ptr, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDOD_HIP_H */
