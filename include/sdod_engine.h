/*
 * sdod_engine.h -- graph-level C ABI of the MI355X txt2img engine.
 *
 * A "graph" here plays the role the serialized QNN graphs play in the reference: the reference's
 * Context loads four graphs -- "unet.serialized", "text_encoder.serialized", "vae_decoder.serialized",
 * "temb" (csrc/libsdod/src/context.cpp:105) -- allocates their I/O tensors (context.cpp:201-218) and
 * calls QnnGraph::execute() on them (qnn_context.cpp:711-713).  Here each graph is a static launch list
 * of the hand-written gfx950 kernels of include/sdod_hip.h over a weight arena and an activation arena
 * in HBM, optionally replayed as one hipGraph.
 *
 * I/O slots (device memory owned by the graph; sdod_graph_io() returns pointer + size):
 *   UNET          in0 x    fp32 NCHW [B][4][H][W]        (context.cpp:214  x = unet.allocate_input(0))
 *                 in1 temb fp16 [B][E]                   (context.cpp:215  t = unet.allocate_input(1)); E = width of the
 *                                                        TEMB graph's output: the time-MLP output pushed through every
 *                                                        ResBlock's emb_layers projection (all of it depends on t only,
 *                                                        so it is computed once per step and cached like context.cpp:276-278)
 *                 in2 ctx  fp16 [B][context_len][ctx_dim]  (context.cpp:216  p_cond / p_uncond = input(2)); context_len = 77 k
 *                                                        for a prompt of k text-encoder chunks concatenated along the key axis
 *                                                        (sdod_context_assemble_f16)
 *                 in3 cond fp32 NCHW [B][concat_channels][H][W]  only with sdod_model_config.concat_channels > 0 (an inpainting
 *                                                        checkpoint, ldm `c_concat`): mask (1) | latent of the masked image (4),
 *                                                        read by the input convolution next to in0; constant over a sampler run
 *                 in3..6 (in4..7 with concat_channels) feat fp16 NHWC [B / r][H / s][W / s][C], (s, C) = (1, MC), (2, 2 MC), (4, 4 MC),
 *                                                        (8, 4 MC): only with sdod_adapter_config.adapter_reps = r > 0 (T2I-Adapter
 *                                                        features): added in place behind ldm's input_blocks.2, .5,
 *                                                        .8 and .11, before the tensor becomes a skip, to each of the r guidance
 *                                                        copies of the batch.  Zero after finalize; constant over a sampler run
 *                 out0 e   fp16 NHWC [B][H][W][4]        (context.cpp:218  e = unet.allocate_output(0))
 *   TEMB          in0 t    fp32 [B]                      (model time, dpm_solver.cpp:115)
 *                 out0     fp16 [B][E]                   (context.cpp:257-278: sinusoid + temb graph, + emb_layers)
 *   TEXT_ENCODER  in0 ids  int32 [B][77]                 (context.cpp:207 tokens)
 *                 out0     fp16 [B][77][ctx_dim]         (context.cpp:208 p)
 *   VAE_DECODER   in0 z    fp32 NCHW [B][4][H][W]        (context.cpp:220 y)
 *                 out0 img fp16 NHWC [B][8H][8W][3] in [-1,1]  (context.cpp:221 img)
 *   VAE_ENCODER   in0 img  uint8 HWC [B][8H][8W][3]      (ldm img2img: x = 2 u / 255 - 1)
 *                 out0     fp32 NCHW [B][8][H][W]        moments = quant_conv(encoder(x)): mean | logvar (not part of the
 *                                                        reference, which has no img2img)
 *   VAE_ENCODER_MASKED  in0 img uint8 HWC [B][8H][8W][3], in1 mask uint8 [B][8H][8W]: the same graph and parameters on the masked
 *                 image of inpainting, x = mask >= 128 ? 0 : 2 u / 255 - 1 (only the first launch differs); out0 as VAE_ENCODER
 *   ADAPTER       in0 hint uint8 HWC [B][8H][8W][adapter_hint_channels]   (an edge map, depth map, sketch or pose skeleton)
 *                 out0..3  fp16 NHWC [B][H / s][W / s][C], the four feature maps above: TencentARC's "full" T2I-Adapter,
 *                 Adapter(channels=[MC, 2 MC, 4 MC, 4 MC], nums_rb=adapter_res_blocks, ksize=1, sk=True, use_conv=False) on
 *                 pixel_unshuffle8(hint / 255), parameters by the checkpoint's names (conv_in.*, body.K.{in_conv,block1,block2}.*);
 *                 always fp16 weights.  Runs once per hint, not once per step (not part of the reference)
 *   UPSCALER      in0 img  uint8 HWC [B][H][W][3]        (the pipeline's uint8 image, or any other)
 *                 out0     fp16 NHWC [B][4H][4W][3], the network's output, nominally in [0, 1], not clamped: ESRGAN's RRDBNet
 *                 (64 features, growth 32, scale 4, sdod_upscaler_config.num_blocks blocks) on u / 255, parameters by basicsr's names
 *                 (conv_first, body.N.rdbK.convJ, conv_body, conv_up1, conv_up2, conv_hr, conv_last); always fp16 weights;
 *                 15 num_blocks + 6 launches (not part of the reference)
 *   UNET with sdod_control_config.control_inputs (ControlNet): behind every other input, 13 residual inputs
 *                 fp16 NHWC [B][H / s][W / s][C] in skip order -- (s, C) = (1, MC) x3, (2, MC), (2, 2 MC) x2, (4, 2 MC), (4, 4 MC) x2,
 *                 (8, 4 MC) x3, and (8, 4 MC) for the middle block's output -- and one input control_scale fp32 [13]; all zero after
 *                 finalize.  One launch behind the middle block (sdod_add_control_f16) does cldm's ControlledUnetModel additions in
 *                 place: hs[k] += control_scale[k] * residual[k], h += control_scale[12] * residual[12]
 *   CONTROLNET    in0 x fp32 NCHW [B][4][H][W], in1 temb fp16 [B][E_c] (the control TEMB graph's output), in2 ctx fp16
 *                 [B][context_len][ctx_dim], in3 guided hint fp16 NHWC [B / 2][H][W][MC] (the CONTROL_HINT graph's output, shared by
 *                 the two guidance halves of the batch; zero after finalize); out0..12 the 13 residuals above.  ldm's cldm.ControlNet
 *                 for SD 1.x: input_blocks.0.0, + guided hint, the UNet's input blocks and middle block on the checkpoint's own
 *                 weights, then zero_convs.k.0 (k = 0..11) on the twelve skip tensors and middle_block_out.0 on the middle output.
 *                 Parameters by the checkpoint's names without `control_model.`; always fp16 weights; batch must be even
 *   CONTROL_HINT  in0 hint uint8 HWC [B][8H][8W][3]; out0 fp16 NHWC [B][H][W][MC]: cldm's input_hint_block on u / 255, eight 3x3
 *                 convolutions 3 -> 16 -> 16 -> 32 (stride 2) -> 32 -> 96 (stride 2) -> 96 -> 256 (stride 2) -> MC with SiLU behind
 *                 all but the last (input_hint_block.0, .2, .., .14).  The 16 / 32 / 96 channel widths are built zero-padded to 64 /
 *                 64 / 128 (the GEMM needs K % 64 == 0), which is exact: zero weights, zero bias and SiLU(0) = 0 keep the padded
 *                 channels zero.  The parameter table lists the PADDED shapes; whoever sets the parameters pads (sdod.amd.engine's
 *                 ControlHint does).  Runs once per hint, not once per step
 *   UNET with sdod_ip_config.ip_tokens = T (image prompts): behind every other input, ip_ctx fp16 [B][T][ctx_dim] (static
 *                 over a sampler run, like in2) and four inputs ip_w fp32 [H / ds * W / ds][2], ds = 1, 2, 4, 8; (1, 0) after finalize
 *   IMAGE_ENCODER in0 img uint8 HWC [B][S][S][3] (resized and cropped by the caller); out0 fp16 [B][proj_dim]: HF
 *                 CLIPVisionModelWithProjection's image_embeds -- CLIP's mean / std normalisation, patch embedding, class token and
 *                 position embedding, pre_layrnorm, the encoder layers, post_layernorm and visual_projection on the class token.
 *                 Parameters by HF's names (vision_model.embeddings.*, vision_model.pre_layrnorm.*, vision_model.encoder.layers.N.*,
 *                 vision_model.post_layernorm.*, visual_projection.weight).  The table lists patch_embedding.weight as the matrix
 *                 [width][Kpad] (the conv weight flattened, zero-padded from 3 p^2 to the next multiple of 64) and class_embedding as
 *                 [1][width]; whoever sets the parameters reshapes and pads (sdod.amd.engine's ImageEncoder does)
 *   IMAGE_PROJ    in0 fp16 [B][proj_dim] (image_embeds); out0 fp16 [B][T][ctx_dim] = LayerNorm(Linear(in0).reshape(T, ctx_dim)):
 *                 IP-Adapter's ImageProjModel, parameters proj.weight / proj.bias / norm.weight / norm.bias
 *   TEMB with sdod_control_config.control_temb: the time conditioning of a CONTROLNET graph, out0 fp16 [B][E_c]: the checkpoint's own
 *                 time_embed.* and the emb_layers of its ten ResBlocks (8 input blocks, 2 middle), E_c = 30 MC
 *
 * Parameters are addressed by their CompVis-ldm / HF-CLIP state-dict names (without the
 * `model.diffusion_model.` / `first_stage_model.` / `cond_stage_model.transformer.` prefixes) and are
 * given in their canonical PyTorch layouts (conv [Cout][Cin][kh][kw], linear [out][in]); the engine
 * repacks them to KRSC fp16 in HBM.  All functions return 0 or a libsdod status code; the message is
 * available from sdod_hip_last_error().
 */
#ifndef SDOD_ENGINE_H
#define SDOD_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifndef SDOD_API
#define SDOD_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum sdod_graph_kind { SDOD_GRAPH_UNET = 0, SDOD_GRAPH_VAE_DECODER = 1, SDOD_GRAPH_TEXT_ENCODER = 2, SDOD_GRAPH_TEMB = 3,
                       SDOD_GRAPH_VAE_ENCODER = 4, SDOD_GRAPH_VAE_ENCODER_MASKED = 5, SDOD_GRAPH_ADAPTER = 6, SDOD_GRAPH_UPSCALER = 7,
                       SDOD_GRAPH_CONTROLNET = 8, SDOD_GRAPH_CONTROL_HINT = 9, SDOD_GRAPH_IMAGE_ENCODER = 10, SDOD_GRAPH_IMAGE_PROJ = 11 };

typedef struct sdod_model_config {
    int latent_channels; /* 4 */
    int latent_h;        /* 64 (SD1.x 512px), 96 (SD2.1 768px) */
    int latent_w;
    int model_channels;  /* 320 */
    int context_dim;     /* 768 (SD1.x), 1024 (SD2.x) */
    int context_len;     /* 77: the text encoder's positions (its position table is [context_len][ctx_dim]) and the UNet's
                          * cross-attention keys.  A UNET graph takes any length >= 1 (77 k for k prompt chunks); above 80 keys
                          * its transformer blocks run the three-launch cross-attention instead of the folded form */
    int num_heads;       /* 8 (SD1.x: head dim = C/8); 0 = use head_dim; negative is an error */
    int head_dim;        /* 64 (SD2.x); ignored when num_heads > 0.
                          * One of the two decides the head geometry of every transformer of a UNET / CONTROLNET graph, whose widths
                          * are C = model_channels, 2 model_channels and 4 model_channels.  Creating such a graph is
                          * LIBSDOD_INVALID_ARGUMENT, with a message that names the field, unless at every C
                          *   num_heads > 0:                 C % num_heads == 0 and C / num_heads is a head dim the attention kernel takes;
                          *   num_heads == 0, head_dim > 0:  C % head_dim == 0 and head_dim is one the attention kernel takes
                          * (sdod_attention_head_dim_ok, include/sdod_hip.h: 40, 64, 80, 160).  So num_heads = 8 needs model_channels
                          * 320; head_dim 64 takes every model_channels (a multiple of 64); head_dim 40, 80 or 160 takes the multiples
                          * of 320.  Every accepted geometry runs: where the folded cross-attention does not take a level
                          * (sdod_xattn_fold_ok) the builder uses Linear + attention + Linear.  The other kinds do not read the fields */
    int vocab_size;      /* 49408 */
    int text_layers;     /* 12 */
    int text_heads;      /* 12; TEXT_ENCODER: positive, and context_dim / text_heads must be 64 (anything else is INVALID_ARGUMENT) */
    int vae_channels;    /* 128 */
    int linear_proj;     /* 0: transformer proj_in / proj_out are 1x1 convs [C,C,1,1] (SD1.x); 1: Linear [C,C] (SD2.x
                          * `use_linear_in_transformer`) -- same arithmetic, different checkpoint shapes */
    int text_arch;       /* TEXT_ENCODER graph: 0 = CLIP ViT-L/14 as HF `CLIPTextModel` names it (quick-GELU, text_layers
                          * blocks, last_hidden_state); 1 = OpenCLIP text tower as open_clip names it (`transformer.resblocks.N.*`,
                          * fused `attn.in_proj_*`, erf GELU) stopped after text_layers blocks + ln_final: SD2.x conditions on the
                          * PENULTIMATE block of ViT-H/14 (24 blocks in the checkpoint, text_layers = 23) */
    int weight_quant;    /* 0: GEMM weights live in HBM as fp16 (an SDOD_U8Q checkpoint tensor is dequantised once at load);
                          * 1 (UNET / TEMB graphs): every conv / linear weight must be given as SDOD_U8Q and STAYS affine uint8 in
                          * HBM (half the weight footprint and stream, BASELINE config 5 "int8 weight quant (mirrors QNN quant
                          * path)"): the GEMM expands the codes on the fragment read (sdod_gemm_desc.wq).  Costs two fusions the
                          * fp16 build has: LayerNorm is a launch again (its gamma cannot be folded into integer codes) and the
                          * ResBlock skip 1x1 conv is its own GEMM (its tensor has its own scale / offset).
                          * 2 ("where it pays"): same checkpoint format, but the codes are streamed only by the blocks whose GEMMs
                          * have <= 128 rows; every other block's tensors are dequantised once at load and the block is built
                          * exactly as with weight_quant = 0.  On MI355X no GEMM of the UNet is weight-bandwidth bound at batch 2,
                          * so the uint8 kernels lose wherever there are >= 288 rows and tie at 72
                          * (profiles/r03_config5_op_tables.txt): this is the setting that is never slower than fp16. */
    int concat_channels; /* 0; 5 for an inpainting checkpoint (sd-v1-5-inpainting, 512-inpainting-ema): the UNet's input convolution
                          * takes latent_channels + concat_channels channels (`input_blocks.0.0.weight` [320][9][3][3]), the extra ones
                          * from the UNET graph's in3; its output keeps latent_channels.  9 * (latent_channels + concat_channels) <= 96,
                          * and with concat_channels > 0 model_channels must be 64, 128, 256 or 320 (the one-launch input convolution;
                          * the im2col + GEMM form of other widths has no second source). */
} sdod_model_config;

SDOD_API void sdod_model_config_sd14(sdod_model_config* cfg);
/* SD v2.1-768 UNet / VAE shapes (BASELINE config 5): 96x96 latent, context 1024, 64-wide heads (5/10/20/20 of them),
 * linear transformer projections, OpenCLIP ViT-H/14 text tower (width 1024, 16 heads, 23 of its 24 blocks). */
SDOD_API void sdod_model_config_sd21(sdod_model_config* cfg);

SDOD_API int sdod_graph_create(void** graph, int kind, const sdod_model_config* cfg, int batch);
/* T2I-Adapter structural control.  The three values travel next to sdod_model_config, not inside it: the struct's size and field
 * list are part of the ABI that existing callers (and their checks) were built against, and all-zero means "no adapter anywhere". */
typedef struct sdod_adapter_config {
    int adapter_reps;          /* UNET graph: 0 = no adapter inputs (the graph is exactly the one sdod_graph_create builds: launch list,
                                * arena and op table); 1 or 2 = it has the four feature inputs, each shared by that many guidance
                                * copies of the batch; must divide the batch */
    int adapter_hint_channels; /* ADAPTER graph: 1 or 3 (conv_in takes 64 * adapter_hint_channels channels) */
    int adapter_res_blocks;    /* ADAPTER graph: residual blocks per stage (nums_rb), 1 .. 8; 0 = 2 */
} sdod_adapter_config;
/* sdod_graph_create with an adapter configuration (NULL = all zero).  SDOD_GRAPH_ADAPTER can only be created here; latent_h and
 * latent_w follow the UNet's rule (multiples of 8, at least 8).  Anything else is INVALID_ARGUMENT. */
SDOD_API int sdod_graph_create_ex(void** graph, int kind, const sdod_model_config* cfg, const sdod_adapter_config* adapter, int batch);
/* Seamless tiling.  sdod_graph_create_ex with a graph-wide `wrap`: bit 0 = the x axis wraps (left / right edges join), bit 1 = the
 * y axis wraps.  Every 3x3 symmetric-pad convolution of the graph -- ResBlocks, downsample and upsample convolutions, input and
 * output convolutions -- takes a circular border on the wrapped axes (sdod_gemm_desc::pad_mode 2 / 3 / 4, sdod_conv_in_wrap_f16,
 * sdod_im2col3x3_small_wrap_f16); GroupNorm, attention and nearest-2x upsampling do not know where the border is.  Like the adapter
 * configuration, the flag travels next to sdod_model_config, whose size is part of the ABI.  wrap = 0 builds exactly the graph of
 * sdod_graph_create_ex, and a wrapped graph has the plain graph's launch list, tiles and arena.  Honoured by SDOD_GRAPH_UNET (with
 * concat_channels == 0) and SDOD_GRAPH_VAE_DECODER; a non-zero wrap for any other kind is INVALID_ARGUMENT.  Latent shifts of a
 * wrapped UNet commute with it for multiples of 8 (three stride-2 levels); the wrapped decoder commutes with any shift. */
SDOD_API int sdod_graph_create_wrap(void** graph, int kind, const sdod_model_config* cfg, const sdod_adapter_config* adapter, int wrap,
                                    int batch);
/* ESRGAN upscaler (SDOD_GRAPH_UPSCALER).  Its three values travel next to sdod_model_config for the same reason, and the kind has
 * its own create entry because no field of sdod_model_config applies to it: the existing create functions refuse the kind.  Fixed:
 * 64 features, growth 32, scale 4.  num_blocks in [1, 23]; in_h and in_w multiples of 8 in [8, 1024] (the largest tensor then stays
 * below 2^31 elements).  NULL or anything else is INVALID_ARGUMENT. */
typedef struct sdod_upscaler_config {
    int num_blocks; /* RRDB blocks: 23 (ESRGAN_4x, R-ESRGAN 4x+), 6 (the anime model) */
    int in_h;       /* input image height */
    int in_w;       /* input image width */
} sdod_upscaler_config;
SDOD_API int sdod_graph_create_upscaler(void** graph, const sdod_upscaler_config* cfg, int batch);
/* ControlNet.  Like the adapter's, its switches travel next to sdod_model_config; all zero = nothing changes.  The
 * kinds SDOD_GRAPH_CONTROLNET and SDOD_GRAPH_CONTROL_HINT can only be created here (control may then be NULL); the other create
 * functions refuse them.  For the remaining kinds this is sdod_graph_create plus the two switches; a switch on a kind it does not
 * apply to, a CONTROLNET graph with an odd batch, concat_channels or weight_quant on a control graph: INVALID_ARGUMENT. */
typedef struct sdod_control_config {
    int control_inputs; /* UNET graph: 1 = it has the 13 residual inputs and control_scale, and one more launch; 0 = the plain graph */
    int control_temb;   /* TEMB graph: 1 = the time conditioning of a CONTROLNET graph ([B][30 MC]); 0 = the UNet's */
} sdod_control_config;
SDOD_API int sdod_graph_create_control(void** graph, int kind, const sdod_model_config* cfg, const sdod_control_config* control, int batch);
/* Latent Consistency Models: the guidance-scale embedding of a full LCM checkpoint, TEMB graph only.  With
 * time_cond_proj_dim = D > 0 the graph gets a second input, in1 = w fp32 [B] (the guidance scale of each row), and the parameter
 * `time_embed.cond_proj.weight` [model_channels][D] (no bias; diffusers: time_embedding.cond_proj.weight), and computes
 *   feat = timestep_features(t) + guidance_features(w) @ cond_proj^T      [sdod_guidance_features_f16, then one GEMM whose residual
 *                                                                          epilogue adds the timestep features]
 * in front of the time MLP; the rest of the graph is unchanged, and a zero cond_proj gives the plain graph's output bit for bit.
 * D must be a positive multiple of 16 (at most 4096; with uint8 weights a multiple of 64); on any other kind, or with
 * sdod_control_config.control_temb, it is refused.  lcm == NULL or D == 0 builds exactly what sdod_graph_create builds. */
typedef struct sdod_lcm_config {
    int time_cond_proj_dim; /* width of the guidance-scale features: 256 for LCM_Dreamshaper_v7; 0 = none */
} sdod_lcm_config;
SDOD_API int sdod_graph_create_lcm(void** graph, int kind, const sdod_model_config* cfg, const sdod_lcm_config* lcm, int batch);
/* Regional prompts, UNET graph only.  cfg->context_len must be 77 * regions: in2 holds, per image, the encodings of
 * `regions` prompts one behind the other.  Behind every other input the graph gets four inputs region_w[level], fp32
 * [H / ds * W / ds][regions] for ds = 1, 2, 4, 8 (what sdod_region_weights_f32 writes), shared by all images of the batch and
 * "region 0 everywhere" after finalize.  Every cross-attention computes sum_r w_r(pixel) attn(x, ctx[:, 77 r : 77 r + 77]); the
 * weights are read by the kernels in the launch, so a captured graph picks up new ones.  regions in [2, 4]; no weight_quant and no
 * concat_channels.  The other create functions build exactly what they built before. */
typedef struct sdod_region_config {
    int regions; /* prompts per image */
} sdod_region_config;
SDOD_API int sdod_graph_create_regions(void** graph, int kind, const sdod_model_config* cfg, const sdod_region_config* regions, int batch);
/* Image prompts (IP-Adapter's decoupled cross-attention), UNET graph only.  ip_tokens = T > 0: behind every other
 * input the graph gets ip_ctx fp16 [B][T][ctx_dim] (the projected image tokens; static over a sampler run like the text context) and
 * four inputs ip_w[level], fp32 [H / ds * W / ds][2] for ds = 1, 2, 4, 8 (what sdod_ip_weights_f32 writes), shared by all images
 * of the batch and (1, 0) after finalize.  Every transformer block has two more parameters, `...attn2.to_k_ip.weight` and
 * `...attn2.to_v_ip.weight` [C][ctx_dim], and every cross-attention computes
 *   to_out(w_0(pixel) attn(q, K_text, V_text) + w_1(pixel) attn(q, to_k_ip(ip_ctx), to_v_ip(ip_ctx))) + bias.
 * The weights are read by the kernels in the launch, so a captured graph picks up new ones; with w_1 = 0 the image segment
 * contributes exact zeros.  T in [1, 16]; context_len <= 80; no weight_quant and no concat_channels.  ip == NULL or all zero builds
 * exactly what sdod_graph_create builds. */
typedef struct sdod_ip_config {
    int ip_tokens; /* image tokens per image: 4 for ip-adapter_sd15 */
} sdod_ip_config;
SDOD_API int sdod_graph_create_ip(void** graph, int kind, const sdod_model_config* cfg, const sdod_ip_config* ip, int batch);
/* The image side of an image prompt: the kinds SDOD_GRAPH_IMAGE_ENCODER and SDOD_GRAPH_IMAGE_PROJ can only be created
 * here; every other create function refuses them.  IMAGE_ENCODER reads `vision` alone (cfg and ip may be NULL); IMAGE_PROJ reads
 * vision->proj_dim, cfg->context_dim and ip->ip_tokens.  Both always keep fp16 weights and run once per image prompt, not per step.
 * ViT-H/14, the encoder of ip-adapter_sd15: {224, 14, 1280, 32, 16, 5120, 1024, 0}. */
typedef struct sdod_vision_config {
    int image_size; /* S: the input is [B][S][S][3]; a multiple of patch */
    int patch;      /* patch size p; the patch-embedding rows are 3 p^2 long, zero-padded to the next multiple of 64 */
    int width;      /* hidden size, a multiple of 64 */
    int layers;     /* encoder layers */
    int heads;      /* width / heads must be 64 or 80 */
    int mlp_dim;    /* intermediate size, a multiple of 64 */
    int proj_dim;   /* width of image_embeds, a multiple of 64 */
    int quick_gelu; /* 1: x sigmoid(1.702 x) (OpenAI CLIP); 0: erf GELU (OpenCLIP ViT-H / bigG) */
} sdod_vision_config;
SDOD_API int sdod_graph_create_vision(void** graph, int kind, const sdod_model_config* cfg, const sdod_vision_config* vision, const sdod_ip_config* ip,
                                      int batch);
/* Before sdod_graph_finalize: output `index` of the graph is written to device_ptr (memory the caller owns, typically an input slot
 * of another graph, so that nothing is copied between the two per run) instead of a slot the graph allocates.  bytes must equal the
 * output's size and device_ptr be 256-byte aligned, else INVALID_ARGUMENT.  sdod_graph_io then reports device_ptr.  Unbound outputs
 * stay owned by the graph.  The last GEMM of the path writes there directly (no extra launch). */
SDOD_API int sdod_graph_bind_output(void* graph, int index, void* device_ptr, size_t bytes);
SDOD_API int sdod_graph_destroy(void* graph);

/* parameter table (fixed by kind + config) */
SDOD_API int sdod_graph_num_params(void* graph);
SDOD_API int sdod_graph_param_info(void* graph, int index, const char** name, int* ndim, int64_t shape[4]);
/* data: host pointer in canonical layout, dtype SDOD_F32 or SDOD_F16 (include/sdod_hip.h), numel from shape */
SDOD_API int sdod_graph_set_param(void* graph, const char* name, const void* data, int dtype, const int64_t* shape, int ndim);
/* where a set parameter lives in the weight arena, in its PACKED form (conv [Cout][tap * Cin + c] fp16, a tiny-Cin 3x3 convolution
 * zero-padded to rows of 64 halves while 9 Cin <= 64 and of 128 up to 9 Cin <= 96; vectors fp32), and its size there: for tests and tools
 * that check the packing or run a kernel on a graph's own weights.  A parameter that aliases columns of a wider matrix reports 0 bytes. */
SDOD_API int sdod_graph_param_device(void* graph, const char* name, void** device_ptr, size_t* bytes);
/* load every parameter from a .sdodw container (see DESIGN.md "weight file"); prefix is prepended to graph names */
SDOD_API int sdod_graph_load_file(void* graph, const char* path, const char* prefix);
/* checks that every parameter is set, sizes and allocates the activation arena, builds the launch list */
SDOD_API int sdod_graph_finalize(void* graph);
SDOD_API int sdod_graph_io(void* graph, int is_output, int index, void** device_ptr, size_t* bytes);
/* run once on `stream`.  flags bit 0 (SDOD_EXEC_HIP_GRAPH): the launch list is captured on first use and replayed as one
 * hipGraph; bit 1 (SDOD_EXEC_STATIC_UNCHANGED): the graph's static inputs (UNET in2, the text context, which is constant
 * over a sampler run) have not changed since the previous execute, so the launches depending only on them are skipped */
enum sdod_exec_flags { SDOD_EXEC_HIP_GRAPH = 1, SDOD_EXEC_STATIC_UNCHANGED = 2 };
SDOD_API int sdod_graph_execute(void* graph, void* stream, int flags);
/* Device-side failures a launch cannot report itself: LIBSDOD_RUNTIME_ERROR once a one-launch GroupNorm of any graph on this
 * device has timed out at its grid barrier (sdod_group_norm_status, include/sdod_hip.h) -- call it behind a host
 * synchronisation of the stream the graph ran on; sdod_graph_execute makes the same check on entry. */
SDOD_API int sdod_graph_check(void* graph);
/* launch list introspection + per-launch timing (HIP events on `stream`, eager, averaged over iters runs after one
 * warm-up): label = kernel family/variant ("gemm_t2", "gemm_t3_splitk", "attn_d40", "group_norm", ...), flops/bytes =
 * algorithmic work of that launch.  bench.py derives its roofline block from these. */
SDOD_API int sdod_graph_num_ops(void* graph);
SDOD_API int sdod_graph_op_info(void* graph, int index, const char** label, double* flops, double* bytes);
SDOD_API int sdod_graph_op_detail(void* graph, int index, const char** detail); /* shape string of launch `index` */
SDOD_API int sdod_graph_profile(void* graph, void* stream, int iters, float* ms_out, int n);
SDOD_API int sdod_graph_stats(void* graph, size_t* weight_bytes, size_t* arena_bytes, int* num_launches, double* flops);
/* provenance of the launch list: how many distinct GEMM shapes took their tile from the tune table(s) (the shipped
 * tune/gfx950.tune, then $SDOD_TUNE_CACHE) and how many were timed in this process (0 = the list is reproducible across
 * processes); table_path receives the path(s) consulted */
SDOD_API int sdod_graph_tune_info(void* graph, int* from_table, int* tuned_in_process, char* table_path, int cap);

/* ---- LoRA adapters: low-rank updates W + scale * up . down merged into the weight arena in place.
 * sdod_graph_keep_base (before sdod_graph_finalize): finalize keeps a second device copy of the weight arena as it is after every
 * parameter is set and BEFORE LayerNorm weights are folded in and Linear pairs composed -- what a delta has to be added to.
 * sdod_graph_base_bytes reports its size, 0 when the base was not kept (such a graph allocates nothing more than before). */
SDOD_API int sdod_graph_keep_base(void* graph);
SDOD_API int sdod_graph_base_bytes(void* graph, size_t* bytes);
typedef struct {
    const char* name; /* a conv / Linear weight of the graph (3x3 convolutions, 1x1 convolutions, Linear, the GEGLU projection) */
    const void* up;   /* host, canonical layout: [out][rank] (a convolution's [out][rank][1][1]) */
    const void* down; /* host, canonical layout: [rank][in] (a 3x3 convolution's [rank][cin][3][3]) */
    int dtype;        /* SDOD_F16 or SDOD_F32 (rounded to fp16 on the host) */
    int rank;         /* 1 .. 128 */
    float scale;      /* strength * alpha / rank */
} sdod_lora_entry;
/* Restores the arena from the kept base, merges every entry on the device (sdod_lora_merge_f16 on the parameter's packed location;
 * entries naming the same parameter accumulate in the order given), re-runs the folds and compositions of finalize and marks the
 * static launches stale: the next sdod_graph_execute ignores SDOD_EXEC_STATIC_UNCHANGED once.  No address changes: the launch list
 * and a captured hipGraph stay valid.  count = 0 restores the base model bit for bit.  Every entry is validated first (finalized
 * graph with a kept base and weight_quant = 0, known parameter of a supported kind, rank, finite scale): on a failure the arena is
 * untouched.  Synchronises `stream` before it returns. */
SDOD_API int sdod_graph_set_loras(void* graph, const sdod_lora_entry* entries, int count, void* stream);
/* The same for every adapter family: an entry is a plain LoRA pair, a LoHa quadruple (sdod_loha_merge_f16) or a LoKr
 * pair (sdod_lokr_merge_f16; a = b = 1 adds a full canonical delta), host factors in canonical layout.  Same contract as
 * sdod_graph_set_loras, which is this call with kind = SDOD_NET_LORA: everything validated before the arena is touched, one upload of
 * all factors, one merge launch per entry, entries naming the same parameter accumulate in the order given whatever their kinds,
 * folds re-run, static launches marked stale, no address moves.  LoKr: a must divide the weight's rows and b its input channels. */
enum { SDOD_NET_LORA = 0, SDOD_NET_LOHA = 1, SDOD_NET_LOKR = 2 };
typedef struct {
    const char* name;
    int kind;         /* SDOD_NET_* */
    int dtype;        /* SDOD_F16 or SDOD_F32 host factors (rounded to fp16 on the host) */
    const void* f[4]; /* LORA: up, down | LOHA: w1a, w1b, w2a, w2b | LOKR: w1 [a][b], w2 [n / a][cin / b](, [3][3]) */
    int rank;         /* LORA, LOHA: 1 .. 128 */
    int a, b;         /* LOKR */
    float scale;
} sdod_network_entry;
SDOD_API int sdod_graph_set_networks(void* graph, const sdod_network_entry* entries, int count, void* stream);

/* ---- FreeU (Si et al., CVPR 2024): a switch, not a configuration -- it adds no parameter and composes with every
 * UNET graph the create functions make (control inputs, adapter inputs, regions, image prompts, wrap, concat_channels, weight_quant).
 * sdod_graph_enable_freeu (kind UNET, before sdod_graph_finalize; anything else is INVALID_ARGUMENT): in ldm's UNetModel.forward, where
 * the decoder is about to concatenate h and the popped skip tensor hs_ and both have 4 MC channels (stage 1: b1, s1) or both 2 MC
 * (stage 2: b2, s2), the graph runs sdod_freeu_f16 (include/sdod_hip.h) on the two: two launches per site, labels freeu_filter and
 * freeu_scale, six sites for the SD 1.x / 2.x shape (output_blocks 0 .. 4 and 7), behind the control additions where there are any.
 * The graph gets one more input behind every other one, slot sdod_graph_freeu_input: fp32 [SDOD_FREEU_PARAMS] = {b1, s1, b2, s2,
 * version, 0, 0, 0}, {1, 1, 1, 1, 2, ...} after finalize -- the identity, at which the launches end without reading or writing a
 * tensor and out0 has the bits of the graph without the switch.  The kernels read it on the device: a captured hipGraph follows new
 * values.  A graph without the switch is what it was: same launch list, arena and inputs; its sdod_graph_freeu_input is -1. */
SDOD_API int sdod_graph_enable_freeu(void* graph);
SDOD_API int sdod_graph_freeu_input(void* graph, int* index);

#ifdef __cplusplus
}
#endif
#endif /* SDOD_ENGINE_H */
