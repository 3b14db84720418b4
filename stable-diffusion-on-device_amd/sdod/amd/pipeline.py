"""txt2img on MI355X: Python host loop over the engine graphs (north_star: "Python host code on PyTorch-ROCm drives
the PLMS/DPM sampler loop while the UNet denoising step ... and the VAE decoder run as hand-written CDNA4 HIP kernels").

Mirrors the reference's Context (context.cpp:49-403) in structure: setup -> graphs + cached unconditional embedding +
cached time embeddings; generate -> tokenise, text-encode, sampler loop over the batched (uncond, cond) UNet
evaluation with CFG, decode, uint8.  Multi-GPU: one process per GPU, images sharded over ranks, the text conditioning
computed on rank 0 and sent with ONE RCCL broadcast."""
import os

import numpy as np
import torch

from . import engine as E
from . import ops
from . import prompts as PR
from . import regions as RG
from . import ip_adapter as IP
from . import freeu as FU
from . import upscale as UP
from . import panorama as PN
from .host import DpmSolver
from .samplers import K_SAMPLERS, K_SCHEDULES, PLMS_ORDERS, KSchedule, LcmSchedule, PlmsSchedule


class Txt2Img:
    # what an object made by Txt2Img.__new__ (no constructor: the argument checks run without a device) has of these
    inpaint_unet = False
    _cond_staged = False
    encoder = None
    masked_encoder = None
    _traj = None        # {key: (graph, static inputs, output)} of _graphed, created with its first entry
    prompt_chunks = 1
    model = 'sd14'
    tokenizer = None
    text = None
    _loras = False
    hires = None        # the second pipeline of the hires pass (Txt2Img(..., hires_hw=)), or None
    adapter = None      # the T2I-Adapter graph (Txt2Img(..., adapter=True)), or None
    controlnet = None   # the ControlNet graph (Txt2Img(..., controlnet=True)), or None; control_hint: its hint encoder
    control_hint = None
    _control_on = False         # a hint is set: every evaluation runs the control graph in front of the UNet
    _control_ctx_fresh = True   # the control graph's own static-unchanged state
    adapter_channels = 3
    upscaler = None     # the ESRGAN x4 upscaler (Txt2Img(..., upscaler=True): sdod.amd.upscale.Upscaler), or None
    tiling = 0          # seamless tiling: the wrap bits the UNet and the VAE decoder were built with (bit 0 = x, bit 1 = y)
    ip_tokens = 0       # image prompts: image tokens per image the UNet was built for (Txt2Img(..., ip_adapter=True)), 0 = none
    image_proj = None   # ... the IMAGE_PROJ graph, whose output IS unet.ip_ctx, and image_encoder, the CLIP vision tower (or None)
    image_encoder = None
    ip_proj_dim = 0
    ip_image_size = None
    regions = 0         # regional prompts: prompts per image the UNet was built for (Txt2Img(..., regions=k)), 0 = none
    canvas_hw = None    # MultiDiffusion panoramas: the canvas latent's (H, W) (Txt2Img(..., canvas_hw=)), or None; canvas_vae: its decoder
    canvas_wrap = False
    canvas_vae = None
    freeu = False       # FreeU: the UNet was built with the switch and has the unet.freeu parameter input (Txt2Img(..., freeu=True))
    _pano = None        # {(oy, ox, weights kind): the window plan and its device tables}, created with its first entry
    unguided = False    # LCM: the UNet has one row per image, the conditional one (Txt2Img(..., unguided=True)): only the *_lcm entry points run
    guidance_embed = False      # ... and the TEMB graphs take the guidance scale w (Txt2Img(..., guidance_embed=True))
    lora_time_modules = False   # set_loras also adapts the time conditioning: the TEMB graphs keep their base weights
    _time_networks = ()         # ... the 'temb' entries of the current set_loras, for the TEMB graphs made later

    def __init__(self, state_dicts=None, models_dir=None, images_per_gpu=1, latent_hw=64, device='cuda:0', use_hip_graph=True,
                 tokenizer=None, with_text_encoder=True, model='sd14', with_vae=True, cfg_split=False, weight_quant=None,
                 with_vae_encoder=False, inpaint_unet=False, prompt_chunks=1, *, loras=False, hires_hw=None, adapter=False,
                 adapter_channels=3, tiling=False, upscaler=False, controlnet=False, regions=False, ip_adapter=False, canvas_hw=None,
                 canvas_wrap=False, freeu=False, unguided=False, guidance_embed=False, lora_time_modules=False):
        """state_dicts: {'unet': sd, 'temb': sd, 'text': sd, 'vae': sd} in ldm/HF naming (canonical layouts; values may be
        weights.QuantU8 for an int8-weight checkpoint), or models_dir with the .sdodw containers libsdod_setup uses.
        model='sd21': SD v2.1-768 (BASELINE config 5): UNet with 64-wide heads / context 1024, v-prediction, OpenCLIP
        ViT-H/14 text tower (open_clip key names, penultimate block + ln_final, prompts padded with id 0 after EOT).
        with_vae_encoder=True: also build the VAE encoder (state_dicts['vae_enc'] or models_dir/vae_encoder.sdodw) for img2img();
        off, nothing of it is constructed or loaded.
        inpaint_unet=True: the UNet checkpoint is an inpainting one (`input_blocks.0.0.weight` [320, 9, 3, 3]): the UNet graph gets its
        conditioning input (unet.cond) and the masked VAE encoder is built (state_dicts['vae_enc'] or models_dir/vae_encoder.sdodw) for
        inpaint_concat(); off, nothing of either exists.
        prompt_chunks=k in [1, 4]: prompts of up to k chunks of 75 tokens (sdod/amd/prompts.py).  The UNet is built on a copy of the
        config with context_len = 77 k -- its transformer blocks then take the three-launch cross-attention, the folded form stops
        at 80 keys -- and the text encoder with batch 2 k, so one execute encodes every chunk of both prompts; every ctx2 of this
        pipeline is [2, 77 k, D].  At 1 nothing is constructed or sized differently.  Anything else raises ValueError before any
        device work.
        loras=True: the UNet and the text encoder keep a second device copy of their weights (Graph.keep_base: unet.base_bytes() +
        text.base_bytes() more device memory) so that set_loras() can re-weight them in place; off, nothing is constructed or sized
        differently.
        latent_hw: an integer (a square latent, as ever) or (h, w), each a multiple of 8 and at least 8 (64 px of image): latents are
        [n, 4, h, w], images [n, 8h, 8w, 3], inpainting masks [n, 8h, 8w] in every entry point.  Anything else raises ValueError
        before any device work (check_latent_hw).
        hires_hw=(H2, W2), the same size rule: also build self.hires, a second Txt2Img of the same model arguments at that size with a
        UNet and a VAE decoder (no text encoder, no VAE encoder), for generate_hires() / generate_hires_graphed() /
        hires_from_latent().  It loads the same state dicts or containers and owns its own weights: hires.unet.stats() +
        hires.vae.stats() more device memory ('weight_bytes' + 'arena_bytes' of each; with loras=True hires.unet.base_bytes() on top).
        Without it nothing is constructed or sized differently.  With cfg_split or inpaint_unet it raises ValueError.
        adapter=True: structural control by a T2I-Adapter (TencentARC's full SD 1.x adapters: canny, depth, sketch, seg, openpose,
        keypose).  The UNet graph gets four feature slots (unet.adapter_feat, zero until a hint is set) that it
        adds behind input_blocks.2 / .5 / .8 / .11 in both guidance halves, and self.adapter = E.Adapter(cfg, 1) is built from
        state_dicts['adapter'] or models_dir/adapter.sdodw, for hints of adapter_channels (1 or 3) channels: set_adapter_hint() /
        clear_adapter_hint().  Off, nothing is constructed or sized differently.  Not with cfg_split, hires_hw, inpaint_unet or
        model='sd21' (the released adapters are SD 1.x ones; the other three would each need the slots in a second place): ValueError
        before any device work, as for an adapter_channels other than 1 or 3.
        tiling=True or 'xy': seamless tiling -- the left / right and top / bottom edges of every image join without a seam (textures,
        backgrounds); 'x' / 'y': that axis only ('x': 360-degree panoramas).  The UNet and the VAE decoder are built with a circular
        border in every 3x3 convolution (E.UNet / E.VaeDecoder on a config copy with cfg.tiling set: sdod_graph_create_wrap); same
        launches, tiles and memory as the plain graphs, and every sampler, generate / generate_graphed / generate_pipelined,
        latent_hw, prompt_chunks, loras, model='sd21', weight_quant and cfg_split work as without it.  False: nothing is constructed
        or sized differently.  Not with with_vae_encoder, inpaint_unet (the encoder graphs are not wrapped: no img2img or inpainting
        under tiling), hires_hw (the latent resize clamps at the border) or adapter (the adapter graph is not wrapped), and no other
        value: ValueError before any device work (tiling_check_build).
        upscaler=True: ESRGAN x4 upscaling of the pipeline's images: self.upscaler, an
        sdod.amd.upscale.Upscaler built from state_dicts['upscaler'] or models_dir/upscaler.sdodw at this pipeline's image size -- with
        hires_hw at the hires image size -- for upscale(), generate_upscaled() and generate_upscaled_graphed().  Its memory:
        upscaler.graph.stats().  Off, nothing is constructed or sized differently.  Not with tiling (the upscaler's border is not
        circular) or an image side above 1024 px: ValueError before any device work (upscaler_check_build).

        controlnet=True: structural control by a ControlNet (the SD 1.x ControlNet 1.0 / 1.1 checkpoints: canny, depth, openpose,
        scribble, softedge, lineart, seg, normalbae, mlsd; INTEGRATION.md "Structural control (ControlNet)").  The UNet graph gets 13
        residual inputs and their scales (unet.control_res, unet.control_scale: zero until a hint is set) and one more launch;
        self.controlnet = E.ControlNet(cfg, 2 n) writes those inputs directly (its outputs are bound to them), self.control_hint =
        E.ControlHint(cfg, 1) encodes one hint image per run.  All three take their weights from state_dicts['controlnet'] (one dict,
        `control_model.` stripped) or models_dir/controlnet.sdodw: set_control_hint() / clear_control_hint().  Off, nothing is
        constructed or sized differently.  Not with cfg_split, hires_hw, inpaint_unet, adapter, tiling or model='sd21': ValueError
        before any device work (control_check_build).  LoRA adapters re-weight the UNet, not the ControlNet.
        regions=k in [2, 4]: regional prompts (sdod/amd/regions.py).  The UNet is built on a config copy with context_len =
        77 k and regions = k, the text encoder with batch 2 k; encode_regions(prompts, negative) gives the context [2, 77 k, D],
        set_regions(masks_u8) says where each prompt applies (uint8 [k, 8h, 8w]; region 0 everywhere until then, and after
        clear_regions()).  Every cross-attention computes sum_r w_r(pixel) attn(x, prompt r).  Works with rectangular latent_hw, loras,
        with_vae_encoder, upscaler, every sampler and the eager, graphed and pipelined entry points; a captured trajectory picks up new
        masks without a recapture.  With prompt_chunks > 1, cfg_split, hires_hw, controlnet, adapter, tiling, inpaint_unet, model='sd21'
        or uint8 weights: ValueError before any device work (regions.regions_check_build).  False: nothing is constructed or sized
        differently.
        ip_adapter=True: image prompts (IP-Adapter for SD 1.x; DESIGN.md 6l, sdod/amd/ip_adapter.py).  state_dicts['ip_adapter'] or
        models_dir/ip_adapter.sdodw holds the image projection and every block's to_k_ip / to_v_ip; state_dicts['image_encoder'] /
        models_dir/image_encoder.sdodw, when present, the CLIP vision tower.  The UNet is built on a config copy with ip_tokens;
        set_image_prompt(image_u8 | embeds=, weight, mask_u8) conditions every entry point and sampler until clear_image_prompt(), and
        a captured trajectory picks up a new image, weight or mask without a recapture.  Works with loras, with_vae_encoder, upscaler,
        rectangular latent_hw and images_per_gpu > 1 (one image prompt per image).  Not with regions, prompt_chunks > 1, cfg_split,
        hires_hw, controlnet, adapter, tiling, inpaint_unet, model='sd21' or uint8 weights: ValueError before any device work
        (ip_adapter.ip_check_build).  False: nothing is constructed or sized differently.
        canvas_hw=(H, W), latent_hw's size rule, each side at least the window's: MultiDiffusion panoramas (DESIGN.md 6n,
        sdod/amd/panorama.py).  latent_hw is then the window -- the UNet keeps its native size -- and images_per_gpu = n the number of
        windows per UNet evaluation; self.canvas_vae = E.VaeDecoder(cfg at the canvas size, 1) is built from the same 'vae' weights, for
        sample_panorama() / decode_canvas() / generate_panorama() / generate_panorama_graphed().  canvas_wrap=True: the windows wrap
        around the canvas in x and the canvas decoder takes the circular border in x (cfg.tiling = 1): a 360-degree panorama; the UNet's
        convolutions stay plain, a window is a crop.  Works with loras, prompt_chunks, model='sd21' and weight_quant.  Not with
        cfg_split, inpaint_unet, hires_hw, adapter, controlnet, regions, ip_adapter, tiling or upscaler: ValueError before any device
        work (panorama.panorama_check_build).  None: nothing is constructed or sized differently.
        freeu=True: FreeU (sdod/amd/freeu.py).  The UNet graph -- whichever one the other arguments select; the hires
        pipeline's too -- runs two more launches at each of its six decoder sites and gets one input, unet.freeu = (b1, s1, b2, s2,
        version, 0, 0, 0), the identity until set_freeu() and after clear_freeu(): at the identity the launches end without touching a
        tensor and the images are the plain pipeline's, bit for bit.  The kernels read the block on the device, so every entry point
        and sampler follows it and a captured trajectory picks up new values without a recapture.  It needs no weights and composes
        with every other argument.  Anything but True / False: ValueError before any device work (freeu.freeu_check_build).  False:
        nothing is constructed or sized differently.
        unguided=True: few-step sampling with a full Latent Consistency Model checkpoint (LCM_Dreamshaper_v7), which needs
        no classifier-free guidance: the UNet is built with images_per_gpu rows, one per image, and evaluates the conditional row of
        ctx2 alone (ctx2 keeps its [2, L, D] shape: encode_prompt is unchanged).  Only sample_lcm() / generate_lcm() /
        generate_lcm_graphed() / img2img_lcm() run on such a pipeline; every other sampling entry point needs the pair and raises.  Works
        with loras, prompt_chunks, rectangular latent_hw, with_vae_encoder, tiling, freeu, upscaler, model='sd21' and weight_quant.  Not
        with cfg_split, inpaint_unet, hires_hw, adapter, controlnet, regions, ip_adapter or canvas_hw: ValueError before any device
        work (lcm_check_build).  False: nothing is constructed or sized differently -- and the *_lcm entry points then run guided, in
        the LCM-LoRA form.
        guidance_embed=True (needs unguided=True): the checkpoint conditions on the guidance scale w through time_embedding.cond_proj
        -- the TEMB graphs are built with cond_proj_dim = 256 and read time_embed.cond_proj.weight from state_dicts['temb'] /
        temb.sdodw (convert(..., guidance_embed=True)), and `guidance` of the *_lcm entry points is w.
        lora_time_modules=True (needs loras=True): the TEMB graphs keep their base weights too, and set_loras() also adapts
        lora_unet_*_resnets_*_time_emb_proj and lora_unet_time_embedding_linear_1 / _2 -- what LCM-LoRA (lcm-lora-sdv1-5) holds next to
        the usual modules -- instead of refusing them.  Off, they are refused as ever."""
        lcm_check_build(unguided, guidance_embed, lora_time_modules, loras, cfg_split, inpaint_unet, hires_hw, adapter, controlnet, regions,
                        ip_adapter, canvas_hw)
        self.unguided, self.guidance_embed, self.lora_time_modules = bool(unguided), bool(guidance_embed), bool(lora_time_modules)
        self.freeu = FU.freeu_check_build(freeu)
        self.prompt_chunks = check_prompt_chunks(prompt_chunks)
        latent_h, latent_w = check_latent_hw(latent_hw)
        self.canvas_hw = PN.panorama_check_build(canvas_hw, canvas_wrap, (latent_h, latent_w), cfg_split, inpaint_unet, hires_hw, adapter,
                                                 controlnet, regions, ip_adapter, tiling, upscaler)
        self.canvas_wrap = bool(canvas_wrap)
        adapter_check_build(adapter, adapter_channels, cfg_split, hires_hw, inpaint_unet, model)
        control_check_build(controlnet, cfg_split, hires_hw, inpaint_unet, adapter, tiling, model)
        self.tiling = tiling_check_build(tiling, with_vae_encoder, inpaint_unet, hires_hw, adapter)
        quant_asked = bool(regions) and (weight_quant or (weight_quant is None and state_dicts is not None and any(
            hasattr(v, 'payload') and len(v.shape) >= 2 for v in state_dicts.get('unet', {}).values())))      # (uint8 codes decide it, as below)
        self.regions = RG.regions_check_build(regions, self.prompt_chunks, cfg_split, hires_hw, controlnet, adapter, tiling, inpaint_unet,
                                              model, quant_asked)
        quant_ip = bool(ip_adapter) and (weight_quant or (weight_quant is None and state_dicts is not None and any(
            hasattr(v, 'payload') and len(v.shape) >= 2 for v in state_dicts.get('unet', {}).values())))
        if IP.ip_check_build(ip_adapter, regions, self.prompt_chunks, cfg_split, hires_hw, controlnet, adapter, tiling, inpaint_unet, model, quant_ip):
            self.ip_tokens, self.ip_proj_dim, ip_vision = IP.ip_sources(state_dicts, models_dir)
        up_args = upscaler_check_build(upscaler, tiling, hires_hw if hires_hw is not None else latent_hw, state_dicts, models_dir)
        if hires_hw is not None:
            check_latent_hw(hires_hw, 'hires_hw')
            if cfg_split or inpaint_unet:
                raise ValueError('hires_hw cannot be combined with cfg_split or inpaint_unet')
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.n = images_per_gpu
        self.model = model
        self.v_prediction = model == 'sd21'
        self.cfg = E.sd21_config(latent_h, latent_w) if model == 'sd21' else E.sd14_config(latent_h, latent_w)
        # int8 weight streaming (BASELINE config 5): when the UNet checkpoint holds affine-uint8 tensors (weights.QuantU8, the
        # reference's QNN encoding) they stay uint8 in HBM and the GEMMs expand them on the fly; weight_quant=False keeps the
        # round-1 behaviour (dequantise once at load, fp16 in HBM)
        self.inpaint_unet = bool(inpaint_unet)
        if self.inpaint_unet:
            self.cfg.concat_channels = 5         # mask (1) | latent of the masked image (4), ldm's c_concat
        self._cond_staged = False
        if weight_quant is None:
            weight_quant = state_dicts is not None and any(hasattr(v, 'payload') and len(v.shape) >= 2 for v in state_dicts['unet'].values())
        # weight_quant='auto' (or 2): stream the codes only where that is not slower than fp16 (sdod_model_config.weight_quant = 2)
        self.cfg.weight_quant = 2 if weight_quant in ('auto', 2) else 1 if weight_quant else 0
        # latency mode: the two halves of the classifier-free-guidance batch run on TWO GPUs -- even rank =
        # unconditional, odd rank = conditional -- and exchange their [n,H,W,4] fp16 predictions once per UNet evaluation
        # (32 KB per image over xGMI); everything after the exchange is computed redundantly, so both ranks hold the image
        self.cfg_split = bool(cfg_split)
        self._pair = None
        if self.cfg_split:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() % 2 == 0):
                raise RuntimeError('cfg_split needs torch.distributed initialised with an even world size')
            rank = dist.get_rank()
            self._half = rank % 2
            for a in range(0, dist.get_world_size(), 2):           # every rank creates every pair group, in the same order
                grp = dist.new_group([a, a + 1])
                if a == rank - self._half:
                    self._pair = grp
            self._pair_staged = dist.get_backend() == 'gloo'         # gloo gathers on the host (rehearsals); RCCL on device
        self.use_hip_graph = use_hip_graph
        self.tokenizer = tokenizer
        unet_cfg = self.cfg
        if self.prompt_chunks > 1:       # the text encoder keeps 77 (its position table); only the UNet sees the longer context
            unet_cfg = E.copy_config(self.cfg)
            unet_cfg.context_len = PR.CHUNK_LEN * self.prompt_chunks
        if adapter:                      # only the UNet graph takes the feature slots: one per level, shared by the two guidance halves
            unet_cfg = E.copy_config(unet_cfg)
            unet_cfg.adapter_reps = 2
            self.adapter_channels = int(adapter_channels)
        if controlnet:                   # 13 residual slots and their scales, filled by the control graph built below
            unet_cfg = E.copy_config(unet_cfg)
            unet_cfg.control_inputs = 1
        if self.regions:                 # k prompts per image: only the UNet sees the k-fold context and has the weight inputs
            unet_cfg = E.copy_config(unet_cfg)
            unet_cfg.context_len = PR.CHUNK_LEN * self.regions
            unet_cfg.regions = self.regions
        if self.ip_tokens:               # the image tokens and the two segments' weights are inputs of the UNet alone
            unet_cfg = E.copy_config(unet_cfg)
            unet_cfg.ip_tokens = self.ip_tokens
        if self.freeu:                   # a switch on the UNet graph, whatever else it was configured with
            unet_cfg = E.copy_config(unet_cfg)
            unet_cfg.freeu = 1
        vae_cfg = self.cfg
        if self.tiling:                  # the UNet and the VAE decoder take the circular border; every other graph has no border to wrap
            unet_cfg, vae_cfg = E.copy_config(unet_cfg), E.copy_config(self.cfg)
            unet_cfg.tiling = vae_cfg.tiling = self.tiling
        self.unet = E.UNet(unet_cfg, self.n if cfg_split or self.unguided else 2 * self.n, device)
        self.vae = E.VaeDecoder(vae_cfg, 1, device) if with_vae else None
        self.text = E.TextEncoder(self.cfg, 2 * (self.regions or self.prompt_chunks), device) if with_text_encoder else None
        self.encoder = E.VaeEncoder(self.cfg, 1, device) if with_vae_encoder else None
        self.masked_encoder = E.MaskedVaeEncoder(self.cfg, 1, device) if self.inpaint_unet else None
        if adapter:
            acfg = E.copy_config(self.cfg)
            acfg.adapter_hint_channels = self.adapter_channels
            self.adapter = E.Adapter(acfg, 1, device)
        if self.canvas_hw is not None:   # the canvas decoder: the same model at the canvas size, its x border circular under canvas_wrap
            ccfg = E.sd21_config(*self.canvas_hw) if model == 'sd21' else E.sd14_config(*self.canvas_hw)
            if self.canvas_wrap:
                ccfg.tiling = 1
            self.canvas_vae = E.VaeDecoder(ccfg, 1, device) if with_vae else None
        self._temb_graphs = {}
        self._sd = state_dicts
        self._dir = models_dir
        for g, key, stem in ((self.unet, 'unet', 'unet'), (self.vae, 'vae', 'vae_decoder'), (self.text, 'text', 'text_encoder'),
                             (self.encoder, 'vae_enc', 'vae_encoder'), (self.masked_encoder, 'vae_enc', 'vae_encoder'),
                             (self.adapter, 'adapter', 'adapter'), (self.canvas_vae, 'vae', 'vae_decoder')):
            if g is None:
                continue
            self._load(g, key, stem)
            if loras and (g is self.unet or g is self.text):
                g.keep_base()
            g.finalize()
        if controlnet:
            # the control graph sees the UNet's context length; its 13 outputs ARE the UNet's residual inputs (no copy per step)
            ccfg = E.copy_config(unet_cfg)
            ccfg.control_inputs, ccfg.weight_quant = 0, 0       # (a ControlNet's weights are always fp16)
            self.controlnet = E.ControlNet(ccfg, 2 * self.n, device)
            self.control_hint = E.ControlHint(ccfg, 1, device)
            for g in (self.controlnet, self.control_hint):
                self._load(g, 'controlnet', 'controlnet')
            for k, slot in enumerate(self.unet.control_res):
                self.controlnet.bind_output(k, slot)
            self.controlnet.finalize()
            self.control_hint.finalize()
            self._temb_stage = torch.zeros((self.unet.batch, self.unet.temb_width + self.controlnet.temb_width), dtype=torch.float16,
                                           device=self.device)
        if self.ip_tokens:
            # the projection runs on the (unconditional = zeros ; conditional) rows of the UNet's batch and writes unet.ip_ctx itself
            self.image_proj = E.ImageProj(self.cfg, self.ip_proj_dim, self.ip_tokens, 2 * self.n, device)
            self._load(self.image_proj, 'ip_adapter', 'ip_adapter')
            self.image_proj.bind_output(0, self.unet.ip_ctx)
            self.image_proj.finalize()
            if ip_vision is not None:
                self.image_encoder = E.ImageEncoder(E.VisionConfig(*ip_vision), self.n, device)
                self._load(self.image_encoder, 'image_encoder', 'image_encoder')
                self.image_encoder.finalize()
                self.ip_image_size = int(ip_vision[0])
        if up_args is not None:
            self.upscaler = UP.Upscaler(device=device, use_hip_graph=use_hip_graph, **up_args)
        self._loras = bool(loras)
        self._temb_cache = {}
        self._ctx_fresh = True
        if hires_hw is not None:
            self.hires = Txt2Img(state_dicts=state_dicts, models_dir=models_dir, images_per_gpu=images_per_gpu, latent_hw=hires_hw,
                                 device=device, use_hip_graph=use_hip_graph, tokenizer=None, with_text_encoder=False, model=model,
                                 with_vae=with_vae, cfg_split=False, weight_quant=weight_quant, with_vae_encoder=False, inpaint_unet=False,
                                 prompt_chunks=prompt_chunks, loras=loras, freeu=freeu, lora_time_modules=lora_time_modules)

    def _load(self, g, key, stem):
        ip_unet = g is self.unet and self.ip_tokens      # its to_k_ip / to_v_ip come from the adapter's container, by the UNet's names
        if self._sd is not None:
            g.load_state_dict({**self._sd[key], **self._sd['ip_adapter']} if ip_unet else self._sd[key])
        else:
            g.load_file(f'{self._dir}/{stem}.sdodw')
            if ip_unet:
                g.load_file(f'{self._dir}/ip_adapter.sdodw')

    # ------------------------------------------------------------------ LoRA adapters
    def set_loras(self, adapters, strict=True):
        """adapters: [(path_or_dict, strength)] or [(path_or_dict, strength_unet, strength_text)] -- kohya-style LoRA files and
        LyCORIS files (LoHa, LoKr, Tucker-cored and full-diff modules, also mixed in one file: sdod/amd/lycoris.py: read_network; module
        names: lora.map_key).  All of them are applied together, summed, to the base weights of the UNet and the text
        encoder, in place on the device: every address, the launch lists and every captured graph (generate_graphed's trajectories
        included: their first evaluation re-derives the cross-attention operands inside the capture) stay valid.  [] restores the base
        model.  A context encoded BEFORE a text-encoder adapter was set or cleared is stale: encode the prompt again.
        strict=False skips the modules the engine cannot adapt; their keys are returned.  RuntimeError when the pipeline was built
        without loras=True; ValueError, before any device work, for a bad strength, uint8 weights, or text-encoder modules on a
        pipeline without a text encoder (a cfg_split rank built with with_text_encoder=False).  With hires_hw the UNet modules are
        applied to both UNets, the text-encoder modules to the base pipeline's alone (the hires pipeline has no text encoder)."""
        from . import lycoris as L
        if not self._loras:
            raise RuntimeError('this pipeline was built without loras=True: merge on the host (lora.merged_state_dict) and build a new one')
        parsed = []
        for a in adapters:
            if not isinstance(a, (tuple, list)) or len(a) not in (2, 3):
                raise ValueError('an adapter is (path_or_dict, strength) or (path_or_dict, strength_unet, strength_text)')
            strengths = [a[1], a[1] if len(a) == 2 else a[2]]
            for v in strengths:
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)):
                    raise ValueError(f'LoRA strength must be a finite number, got {v!r}')
            parsed.append((a[0], float(strengths[0]), float(strengths[1])))
        if self.cfg.weight_quant != 0:
            raise ValueError('LoRA adapters need fp16 weights: this pipeline keeps uint8 codes (weight_quant); merge on the host instead')
        lists, skipped = {'unet': [], 'text': [], 'temb': []}, []
        shapes = {'unet': dict(self.unet.param_table()), 'text': dict(self.text.param_table()) if self.text is not None else {}} if parsed else None
        if parsed and self.lora_time_modules:
            shapes['temb'] = self._temb_shapes()
        for src, s_unet, s_text in parsed:
            if self.lora_time_modules:
                ent, skip = L.entries_for(src, self.model, s_unet, s_text, strict=strict, shapes=shapes, time_modules=True)
                lists['temb'] += ent['temb']
            else:           # (the call, and what it refuses, of every build before lora_time_modules)
                ent, skip = L.entries_for(src, self.model, s_unet, s_text, strict=strict, shapes=shapes)
            lists['unet'] += ent['unet']
            lists['text'] += ent['text']
            skipped += skip
        if lists['text'] and self.text is None:
            raise ValueError('the adapters hold text-encoder modules and this pipeline has no text encoder')
        self.unet.set_networks(lists['unet'])
        if self.lora_time_modules:       # the time conditioning: every TEMB graph there is, the cached rows in place, and the list kept
            self._set_time_networks(lists['temb'])
        if self.hires is not None:       # the second pass runs the same model: its UNet takes the same adapters
            self.hires.unet.set_networks(lists['unet'])
            self.hires._ctx_fresh = True
            if self.lora_time_modules:
                self.hires._set_time_networks(lists['temb'])
        if self.text is not None:
            self.text.set_networks(lists['text'])
        self._ctx_fresh = True
        return skipped

    _temb_table = None          # {parameter name: shape} of this pipeline's TEMB graphs, read once (_temb_shapes)

    def _temb_shapes(self):
        """the parameter table of the TEMB graphs, which is the same at every row count: from one that exists, else from a declared
        graph (no device memory), and kept"""
        if self._temb_table is None:
            g = next((g for k, g in self._temb_graphs.items() if not isinstance(k, tuple)), None)
            if g is None:
                g = E.Temb(self.cfg, 1, self.device, cond_proj_dim=E.LCM_COND_PROJ_DIM if self.guidance_embed else 0)
            self._temb_table = dict(g.param_table())
        return self._temb_table

    def _set_time_networks(self, entries):
        """set_loras' part on the time conditioning (lora_time_modules): the entries go to every TEMB graph that exists, every cached
        time-embedding tensor is recomputed in the same memory, and the list is kept for the TEMB graphs a new schedule length makes"""
        self._time_networks = tuple(entries)
        for key, g in self._temb_graphs.items():
            if not (isinstance(key, tuple) and key[0] == 'control'):      # (the ControlNet's own TEMB graph is not adapted)
                g.set_networks(list(entries))
        self._refresh_time_embeddings()

    def clear_loras(self):
        """back to the base weights, bit for bit: set_loras([])"""
        return self.set_loras([])

    # ------------------------------------------------------------------ structural control (T2I-Adapter)
    def set_adapter_hint(self, hint_u8, weight=1.0):
        """hint_u8: uint8 [n, 8h, 8w, adapter_channels] ([n, 8h, 8w] is accepted for one channel) -- an edge map, depth map, sketch or
        pose skeleton, one per image of the pipeline's batch; the caller makes it (no preprocessor here).  The adapter runs once per
        image, then four launches write weight * feature into the UNet's slots (ops.adapter_stage).  The slots are memory of the UNet
        graph at fixed addresses that every evaluation reads: from here on EVERY entry point is conditioned -- generate,
        generate_graphed, img2img*, inpaint*, every sampler -- and a trajectory that was captured already picks up a new hint or
        weight without a new capture.  weight scales the features (TencentARC's cond_weight); 0.0 is clear_adapter_hint().
        ValueError for a wrong shape or dtype or a non-finite weight (adapter_check_args), before any device work; RuntimeError on a
        pipeline built without adapter=True."""
        if self.adapter is None:
            raise RuntimeError('this pipeline was built without adapter=True: Txt2Img(..., adapter=True) is needed for structural control')
        hint_u8 = adapter_check_args(hint_u8, weight, self._latent_shape, self.n, self.adapter_channels)
        hint_u8 = hint_u8.to(self.device).contiguous()
        for i in range(self.n):
            self.adapter.hint.copy_(hint_u8[i:i + 1])
            self.adapter.execute(self.use_hip_graph)
            for out, slot in zip(self.adapter.out, self.unet.adapter_feat):
                ops.adapter_stage(out, slot[i:i + 1], weight)

    # ------------------------------------------------------------------ ControlNet
    def _require_controlnet(self):
        if self.controlnet is None:
            raise RuntimeError('this pipeline was built without controlnet=True: Txt2Img(..., controlnet=True) is needed for ControlNet')

    def set_control_hint(self, hint_u8, weight=1.0):
        """hint_u8: uint8 [n, 8h, 8w, 3] ([n, 8h, 8w] is expanded to three equal channels) -- the preprocessed control image (edge
        map, depth map, pose skeleton, ...), one per image of the pipeline's batch; the caller makes it (no preprocessor here).
        weight: a finite float, or 13 finite floats, one per residual in skip order with the middle block's last (the front ends'
        control weight; cldm's control_scales).  Runs the hint encoder once per image into the control graph's guided-hint slot and
        writes the 13 scales; from then on every evaluation runs the control graph in front of the UNet, on both guidance halves,
        until clear_control_hint().  Slots and scales are fixed memory read by the launches: a captured trajectory picks up a new
        hint or weight without a new capture.  All scales 0.0 still runs the control graph and adds nothing.  ValueError for a wrong
        shape or dtype or a non-finite weight (control_check_args), before any device work; RuntimeError without controlnet=True."""
        self._require_controlnet()
        hint_u8, scales = control_check_args(hint_u8, weight, self._latent_shape, self.n)
        hint_u8 = hint_u8.to(self.device)
        for i in range(self.n):
            self.control_hint.hint.copy_(hint_u8[i:i + 1])
            self.control_hint.execute(self.use_hip_graph)
            self.controlnet.hint[i:i + 1].copy_(self.control_hint.out)
        self.unet.control_scale.copy_(torch.tensor(scales, dtype=torch.float32))
        self._control_on = True

    def clear_control_hint(self):
        """no control: the scales are zeroed (the UNet's one extra launch then reads and writes nothing) and the control graph is
        no longer executed, eager or captured -- the plain pipeline's images, bit for bit"""
        self._require_controlnet()
        self.unet.control_scale.zero_()
        self._control_on = False

    # ------------------------------------------------------------------ image prompts (IP-Adapter)
    def image_embeds(self, image_u8):
        """CLIP image_embeds fp16 [n, proj_dim] of uint8 images [n, S, S, 3] (resized and cropped by the caller): one execute of the
        image encoder.  What set_image_prompt(image_u8) conditions on; set_image_prompt(embeds=...) with them gives the same images."""
        image_u8, _, _, _ = IP.ip_check_args(self, image_u8, None, 1.0, None)
        self.image_encoder.img.copy_(image_u8.to(self.device))
        self.image_encoder.execute(self.use_hip_graph)
        return self.image_encoder.out.clone()

    def set_image_prompt(self, image_u8=None, weight=1.0, mask_u8=None, *, embeds=None):
        """image_u8: uint8 [n, S, S, 3], one image per image of the batch, resized and cropped by the caller to the encoder's size (224)
        -- or embeds: precomputed CLIP image_embeds, fp16 / fp32 [n, proj_dim].  weight: IP-Adapter's scale, a finite number >= 0.
        mask_u8: optional uint8 [8h, 8w] at image resolution, where the image prompt applies (255 = fully).  The encoder (for
        image_u8) and the image projection run once, here: the conditional rows of the UNet's image tokens take image_proj(embeds),
        the unconditional rows image_proj(zeros), as IP-Adapter's get_image_embeds does; one launch writes the four levels' weights
        (ops.ip_weights).  Tokens and weights are inputs of the UNet at fixed addresses: every entry point and sampler is conditioned
        from here on, and a captured trajectory picks the new ones up without a recapture.  ValueError for wrong shapes or dtypes,
        both or neither of image_u8 / embeds, a bad weight, or image_u8 without an image encoder (ip_adapter.ip_check_args), before
        any device work; RuntimeError without ip_adapter=True."""
        image_u8, embeds, weight, mask_u8 = IP.ip_check_args(self, image_u8, embeds, weight, mask_u8)
        n = self.n
        if image_u8 is not None:
            self.image_encoder.img.copy_(image_u8.to(self.device))
            self.image_encoder.execute(self.use_hip_graph)
            embeds = self.image_encoder.out
        self.image_proj.embeds[:n].zero_()
        self.image_proj.embeds[n:].copy_(embeds.to(self.device))
        self.image_proj.execute(self.use_hip_graph)
        h, w = self._latent_shape[-2:]
        ops.ip_weights(weight, h, w, None if mask_u8 is None else mask_u8.to(self.device), out=self.unet.ip_w, device=self.device)
        self._ctx_fresh = True     # the image tokens' K / V and the fold are static launches of the UNet, like the text's

    def clear_image_prompt(self):
        """no image prompt, the state after construction: weights (1, 0), the image segment contributes exact zeros"""
        if not self.ip_tokens:
            raise RuntimeError('this pipeline was built without ip_adapter=True: Txt2Img(..., ip_adapter=True) is needed for image prompts')
        for w in self.unet.ip_w:
            w.zero_()
            w[:, 0] = 1.0

    # ------------------------------------------------------------------ FreeU
    def set_freeu(self, b1, b2, s1, s2, version=2):
        """the four FreeU numbers in the published argument order -- b1, b2: backbone factors of stage 1 (the 4 MC sites: 1/8 and 1/4
        of the latent) and stage 2 (the 2 MC site at 1/2); s1, s2: the skip tensors' low-frequency scales there -- and the version:
        2 (the authors' current code and the front ends' default) modulates the factor by the per-pixel channel mean, 1 multiplies by b.
        freeu.preset(version, model) has the README's values, e.g. set_freeu(*freeu.preset(2, 'sd14')).  One copy into unet.freeu (and
        the hires pipeline's): every later evaluation uses them, eager or captured.  ValueError for a non-finite number, one outside
        [0, 10] or a version other than 1 or 2 (freeu.freeu_check_args), before any device work; RuntimeError without freeu=True."""
        FU.require(self)
        block = FU.freeu_check_args(b1, b2, s1, s2, version)
        self.unet.freeu.copy_(torch.tensor(block, dtype=torch.float32))
        if self.hires is not None:
            self.hires.set_freeu(b1, b2, s1, s2, version)

    def clear_freeu(self):
        """the identity, the state after construction: the FreeU launches end without reading or writing a tensor"""
        FU.require(self)
        self.unet.freeu.copy_(torch.tensor(FU.IDENTITY, dtype=torch.float32))
        if self.hires is not None:
            self.hires.clear_freeu()

    # ------------------------------------------------------------------ regional prompts
    def set_regions(self, masks_u8):
        """masks_u8: uint8 [regions, 8h, 8w] at image resolution (torch or numpy; 255 = inside, soft and overlapping masks allowed,
        regions.column_masks / row_masks / feather make the common ones): where each of encode_regions' prompts applies, for every image
        of the batch and both guidance halves.  One launch (ops.region_weights) writes the four levels' weights into the UNet's inputs,
        which its kernels read in every evaluation: captured trajectories pick them up without a recapture.  ValueError for a wrong
        dtype, shape or region count (regions.regions_check_args), before any device work; RuntimeError without regions."""
        masks = RG.regions_check_args(self, masks_u8)
        ops.region_weights(masks.to(self.device), out=self.unet.region_w)

    def clear_regions(self):
        """region 0 everywhere, the state after construction: every pixel takes the first prompt"""
        if not self.regions:
            raise RuntimeError('this pipeline was built without regions: Txt2Img(..., regions=k) is needed for regional prompts')
        for w in self.unet.region_w:
            w.zero_()
            w[:, 0] = 1.0

    def encode_regions(self, prompts, negative=''):
        """prompts: exactly `regions` literal texts (CLIP's one window each, no emphasis grammar), region 0 first.  Returns the context
        fp16 [2, 77 regions, D]: the unconditional row holds the negative prompt's encoding once per region, the conditional row the
        prompts' encodings in order.  ONE text-encoder execute (the encode_chunks path)."""
        prompts = RG.regions_check_prompts(self, prompts)
        if not isinstance(negative, str):
            raise ValueError('negative must be a string: per-region negative prompts are not supported')
        if self.tokenizer is None:
            raise ValueError('encode_regions needs the pipeline\'s tokenizer (Txt2Img(..., tokenizer=host.Tokenizer(path)))')
        neg = np.asarray(self._ids(negative))
        return self.encode_chunks(np.stack([neg] * self.regions), np.stack([np.asarray(self._ids(p)) for p in prompts]))

    def clear_adapter_hint(self):
        """zero the UNet's feature slots: the unconditioned model again (its additions of zero change no bit)"""
        if self.adapter is None:
            raise RuntimeError('this pipeline was built without adapter=True: Txt2Img(..., adapter=True) is needed for structural control')
        for slot in self.unet.adapter_feat:
            slot.zero_()

    # ------------------------------------------------------------------ conditioning
    def encode_tokens(self, ids_uncond, ids_cond):
        """ids: int arrays [77]; returns fp16 [2, 77 * prompt_chunks, D] = (uncond, cond), computed on this GPU.  With prompt_chunks
        > 1 both are padded with empty chunks (SOT, EOT, the model's padding) through encode_chunks."""
        if self.prompt_chunks > 1:
            return self.encode_chunks(self._pad_ids(ids_uncond), self._pad_ids(ids_cond))
        ids = torch.from_numpy(np.stack([np.asarray(ids_uncond), np.asarray(ids_cond)]).astype(np.int32))
        self.text.ids.copy_(ids)
        self.text.execute(self.use_hip_graph)
        return self.text.out.clone()

    def encode_prompt(self, prompt, negative=''):
        """the prompt as CLIP's one window: cut at 75 tokens and read literally (no emphasis grammar); encode_prompt_weighted is the
        long, weighted form"""
        return self.encode_tokens(self._ids(negative), self._ids(prompt))

    @property
    def _pad(self):
        """prompts.chunk_prompt's padding rule for this model (see _ids)"""
        return 'zero' if self.model == 'sd21' else 'eot'

    def _pad_ids(self, ids):
        """ids [77] -> [prompt_chunks, 77]: the empty chunks are SOT (the ids' first), EOT (their largest: EOT is the largest id of the
        vocabulary and every window holds one), then the model's padding"""
        ids = np.asarray(ids).astype(np.int64).reshape(1, -1)
        if ids.shape[1] != PR.CHUNK_LEN:
            raise ValueError(f'ids must be [{PR.CHUNK_LEN}], got {ids.shape[1:]}')
        empty = np.full((1, PR.CHUNK_LEN), 0 if self._pad == 'zero' else ids.max(), np.int64)
        empty[0, 0], empty[0, 1] = ids[0, 0], ids.max()
        return np.concatenate([ids] + [empty] * (self.prompt_chunks - 1))

    def encode_chunks(self, ids_uncond, ids_cond, weights=None):
        """ids_uncond, ids_cond: integer arrays [prompt_chunks, 77] (prompts.chunk_prompt / pad_chunks); weights: fp32
        [2, prompt_chunks, 77] (numpy or torch), uncond first, or None.  Returns the context fp16 [2, 77 * prompt_chunks, D].  ONE
        text-encoder execute on the ids laid out as (uncond chunks ; cond chunks): its output [2 k, 77, D] already is the
        concatenation along the key axis.  With weights one more launch, ops.context_assemble (token rows scaled, each chunk's mean
        restored); without, none.  Shape or dtype errors raise ValueError before any device work."""
        k = self.regions or self.prompt_chunks     # (regional prompts: one window per region in the place of the chunks)
        both = []
        for name, ids in (('ids_uncond', ids_uncond), ('ids_cond', ids_cond)):
            ids = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
            if ids.dtype.kind not in 'iu':
                raise ValueError(f'{name} must be an integer array, got {ids.dtype}')
            if ids.shape != (k, PR.CHUNK_LEN):
                built = f'regions={k}' if self.regions else f'prompt_chunks={k}'
                raise ValueError(f'{name} must be {(k, PR.CHUNK_LEN)} (this pipeline was built with {built}), got {ids.shape}')
            vocab = getattr(getattr(self, 'cfg', None), 'vocab_size', None)
            if ids.min() < 0 or (vocab is not None and ids.max() >= vocab):
                raise ValueError(f'{name} holds ids outside the vocabulary [0, {vocab})')
            both.append(ids.astype(np.int32))
        if weights is not None:
            if isinstance(weights, np.ndarray):
                weights = torch.from_numpy(weights)
            _want_tensor('weights', weights, (2, k, PR.CHUNK_LEN), torch.float32, ' (uncond first)')
            if not bool(torch.isfinite(weights).all()):
                raise ValueError('weights must be finite')
        if self.text is None:
            raise RuntimeError('Txt2Img(..., with_text_encoder=True) is needed to encode prompts')
        self.text.ids.copy_(torch.from_numpy(np.concatenate(both)))
        self.text.execute(self.use_hip_graph)
        d = self.text.out.shape[-1]
        if weights is None:
            return self.text.out.reshape(2, k * PR.CHUNK_LEN, d).clone()
        return ops.context_assemble(self.text.out.view(2, k, PR.CHUNK_LEN, d), weights.to(self.device).contiguous())

    def encode_prompt_weighted(self, prompt, negative='', emphasis=True):
        """prompt and negative through prompts.chunk_prompt (emphasis grammar, 75-token chunks, this model's padding rule), both padded
        to prompt_chunks with empty chunks, then encode_chunks with the weights.  emphasis=False: the texts are literal, all weights 1
        (still chunked).  ValueError when either text needs more chunks than the pipeline was built with."""
        if self.tokenizer is None:
            raise ValueError('encode_prompt_weighted needs the pipeline\'s tokenizer (Txt2Img(..., tokenizer=host.Tokenizer(path)))')
        ids, ws = [], []
        for text in (negative, prompt):
            i, w = PR.pad_chunks(*PR.chunk_prompt(self.tokenizer, text, self._pad, emphasis), self.prompt_chunks, self.tokenizer, self._pad)
            ids.append(i); ws.append(w)
        return self.encode_chunks(ids[0], ids[1], np.stack(ws))

    def _ids(self, text):
        """token ids [77]: SOT, tokens, EOT, padding.  CLIP (SD1.x) pads with EOT, as the reference's tokenizer does
        (tokenizer.cpp:274-275); open_clip's tokenizer (SD2.x) pads with 0 -- the padded positions are part of the context"""
        ids = np.array(self.tokenizer.encode(text), dtype=np.int64)
        if self.model == 'sd21':
            eot = int(ids.max())                       # EOT is the largest id of the vocabulary
            first = int(np.argmax(ids == eot))
            ids[first + 1:] = 0
        return ids

    def _temb_graph(self, rows):
        """the TEMB graph of `rows` rows, made on first use: with guidance_embed it has the w input and cond_proj, with
        lora_time_modules it keeps its base weights and starts from the adapters set_loras() holds"""
        g = self._temb_graphs.get(rows)
        if g is None:
            g = E.Temb(self.cfg, rows, self.device, cond_proj_dim=E.LCM_COND_PROJ_DIM) if self.guidance_embed else E.Temb(self.cfg, rows, self.device)
            self._load(g, 'temb', 'temb')
            if self.lora_time_modules:
                g.keep_base()
            g.finalize()
            if self._time_networks:
                g.set_networks(list(self._time_networks))
            self._temb_graphs[rows] = g
        return g

    def _time_embeddings_w(self, key, w, out=None):
        """time_embeddings on a guidance_embed pipeline: every row at guidance scale w; out: recompute into this cached tensor"""
        if w is None:
            raise ValueError('this pipeline was built with guidance_embed=True: its time conditioning needs the guidance scale w')
        ckey = (key, float(w))
        if out is None and ckey in self._temb_cache:
            return self._temb_cache[ckey]
        g = self._temb_graph(len(key))
        g.t.copy_(torch.tensor(key, dtype=torch.float32))
        g.w.fill_(float(w))
        g.execute()
        if out is None:
            out = self._temb_cache[ckey] = g.out.clone()
        else:
            out.copy_(g.out)
        return out

    def _refresh_time_embeddings(self):
        """after the TEMB graphs' weights changed (set_loras with lora_time_modules): every cached tensor recomputed in place, in the
        same memory, so that what already points at its rows -- a captured trajectory -- follows"""
        for ckey, out in self._temb_cache.items():
            if self.guidance_embed:
                self._time_embeddings_w(ckey[0], ckey[1], out)
                continue
            g = self._temb_graph(len(ckey))
            g.t.copy_(torch.tensor(ckey, dtype=torch.float32))
            g.execute()
            out[:, :g.width].copy_(g.out)       # (a ControlNet's own columns ride behind: they are not adapted)

    def time_embeddings(self, times, w=None):
        """[len(times), E] fp16: time-MLP output projected for every ResBlock, for model times `times` (cached per
        schedule, as context.cpp:257-278 does).  w: the guidance scale, for a pipeline built with guidance_embed (and only there)."""
        key = tuple(float(t) for t in times)
        if self.guidance_embed:         # these pipelines' rows depend on the guidance scale too: the key is (times, w)
            return self._time_embeddings_w(key, w)
        if key not in self._temb_cache:
            g = self._temb_graph(len(key))
            g.t.copy_(torch.tensor(key, dtype=torch.float32))
            g.execute()
            if self.controlnet is None:
                self._temb_cache[key] = g.out.clone()
            else:
                # a ControlNet has a time MLP of its own: its columns ride behind the UNet's in the same row, so that every sampler
                # keeps its indexing and its one staging launch (_temb_dst); _unet_eps hands each graph its part
                cg = self._temb_graphs.get(('control', len(key)))
                if cg is None:
                    ccfg = E.copy_config(self.cfg)
                    ccfg.control_temb, ccfg.weight_quant = 1, 0
                    cg = E.Temb(ccfg, len(key), self.device)
                    self._load(cg, 'controlnet', 'controlnet')
                    cg.finalize()
                    self._temb_graphs[('control', len(key))] = cg
                cg.t.copy_(g.t)
                cg.execute()
                self._temb_cache[key] = torch.cat([g.out, cg.out], dim=1)
        return self._temb_cache[key]

    @property
    def _temb_dst(self):
        """where the samplers stage an evaluation's time row: the UNet's slot, or -- with a ControlNet, whose columns ride in the same
        row -- the pipeline's wider buffer that _unet_eps splits between the two graphs"""
        return self.unet.temb if self.controlnet is None else self._temb_stage

    # ------------------------------------------------------------------ one guided eps evaluation
    def _require_cond(self):
        """an inpainting UNet reads unet.cond in every evaluation: refuse to sample before inpaint_concat() has staged it"""
        if self.inpaint_unet and not self._cond_staged:
            raise RuntimeError('this pipeline was built with inpaint_unet=True: its UNet needs the conditioning channels that '
                               'inpaint_concat() stages; nothing has been staged yet')

    def _require_pairs(self, name):
        """every sampling entry point but the LCM ones reads (uncond, cond) pairs: refuse on a pipeline whose UNet has one row per image"""
        if self.unguided:
            raise ValueError(f'{name} needs the classifier-free-guidance pair, and this pipeline was built with unguided=True (one UNet row per '
                             f'image): use sample_lcm / generate_lcm / generate_lcm_graphed / img2img_lcm')

    def _set_context(self, ctx2, lcm=False):
        self._require_cond()
        n = self.n
        if self.unguided:
            if not lcm:
                self._require_pairs('this sampler')
            self.unet.ctx.copy_(ctx2[1:2].expand(n, -1, -1))          # the conditional row alone
        elif self.cfg_split:
            self.unet.ctx.copy_(ctx2[self._half:self._half + 1].expand(n, -1, -1))
        else:
            self.unet.ctx[:n].copy_(ctx2[0:1].expand(n, -1, -1))
            self.unet.ctx[n:].copy_(ctx2[1:2].expand(n, -1, -1))
        if self.controlnet is not None:
            self.controlnet.ctx.copy_(self.unet.ctx)
            self._control_ctx_fresh = True
        self._ctx_fresh = True     # the next UNet execute must redo the cross-attention K/V projections

    def _exchange_halves(self, mine):
        """[n,H,W,4] fp16 of this rank -> [2n,H,W,4] = (uncond rows ; cond rows), identical on both ranks of the pair"""
        import torch.distributed as dist
        both = torch.empty((2 * self.n,) + tuple(mine.shape[1:]), dtype=mine.dtype, device=mine.device)
        if self._pair_staged:
            host = torch.empty(both.shape, dtype=mine.dtype)
            dist.all_gather_into_tensor(host, mine.cpu().contiguous(), group=self._pair)
            both.copy_(host)
        else:
            dist.all_gather_into_tensor(both, mine.contiguous(), group=self._pair)
        return both

    def _unet_eps(self):
        """one UNet evaluation of the staged inputs: the fp16 prediction [2n, H, W, 4] = (uncond rows ; cond rows)"""
        if self.controlnet is not None:
            w = self.unet.temb_width
            self.unet.temb.copy_(self._temb_stage[:, :w])
            if self._control_on:         # control first: its 13 outputs are the UNet's residual inputs
                cn = self.controlnet
                cn.x.copy_(self.unet.x)
                cn.temb.copy_(self._temb_stage[:, w:])
                cn.execute(self.use_hip_graph, static_unchanged=not self._control_ctx_fresh)
                self._control_ctx_fresh = False
        self.unet.execute(self.use_hip_graph, static_unchanged=not self._ctx_fresh)
        self._ctx_fresh = False
        return self._exchange_halves(self.unet.eps) if self.cfg_split else self.unet.eps

    def _eps(self, x, temb_row, guidance, mode, v_coef=None):
        """x: fp32 [n,4,H,W]; returns guided eps fp32 [n,4,H,W].  Batch rows: [uncond x n ; cond x n] (ldm order).
        v_coef = (sqrt(abar_t), sqrt(1 - abar_t)) for a v-prediction model: the guided output is v, eps follows from it."""
        # one in-tree launch stages the graph inputs: x repeated for the (uncond, cond) halves, the time row for every batch row
        ops.stage_unet_inputs(x, self.unet.x, temb_row, self._temb_dst)
        out = ops.cfg_combine(self._unet_eps(), guidance, uncond_first=True, mode=mode)
        if v_coef is not None:
            out = ops.lincomb4([out, x], [v_coef[0], v_coef[1]], 1.0)
        return out

    # ------------------------------------------------------------------ samplers
    def sample_plms(self, ctx2, x_T, steps=20, guidance=7.5, trace=None):
        self._require_pairs('sample_plms')
        sch = PlmsSchedule(steps)
        temb = self.time_embeddings(sch.timesteps.astype(np.float32))     # row k <-> timestep index k
        self._set_context(ctx2)
        x = x_T.to(self.device, torch.float32).clone()
        old = []
        staged = False   # the previous step's fused update already staged this evaluation's inputs
        n_steps = len(sch.time_range)
        for i, step in enumerate(sch.time_range):
            index = sch.steps - i - 1
            vc = sch.v_to_eps_coef(index) if self.v_prediction else None
            if len(old) > 0:
                # steps 2..: stage (unless done) -> UNet -> ONE launch for guidance, the multistep combination, the DDIM update
                # and the staging of the next evaluation's inputs (ops.plms_update = the four separate launches, bit for bit)
                if not staged:
                    ops.stage_unet_inputs(x, self.unet.x, temb[index], self._temb_dst)
                eps = self._unet_eps()
                k = min(len(old), 3)
                coefs, div = PLMS_ORDERS[k]
                nxt_stage = (self.unet.x, temb[index - 1], self._temb_dst) if i + 1 < n_steps else None
                e_t = ops.plms_update(eps, x, old[::-1][:k], coefs, div, sch.coef(index), guidance, mode=1, v_coef=vc, stage=nxt_stage)
                staged = nxt_stage is not None
                old.append(e_t)
                old = old[-3:]
                if trace is not None:
                    trace.append((int(step), index))
                continue
            # first step (pseudo improved Euler, two evaluations): the separate launches
            e_t = self._eps(x, temb[index], guidance, mode=1, v_coef=vc)
            x_pred = x.clone()
            ops.ddim_step(x_pred, e_t, **sch.coef(index))
            nxt = max(index - 1, 0)
            e_next = self._eps(x_pred, temb[nxt], guidance, mode=1, v_coef=sch.v_to_eps_coef(nxt) if self.v_prediction else None)
            e_prime = ops.lincomb4([e_t, e_next], [1.0, 1.0], 2.0)
            ops.ddim_step(x, e_prime, **sch.coef(index))
            old.append(e_t)
            old = old[-3:]
            if trace is not None:
                trace.append((int(step), index))
        return x

    def sample_dpm(self, ctx2, x_T, steps=20, guidance=7.5):
        """the reference driver's sampler: DPM-Solver++(2M), CFG as g*e_c + (1-g)*e_u (context.cpp:342-382)"""
        self._require_pairs('sample_dpm')
        solver = DpmSolver()
        model_ts = solver.prepare(steps)
        temb = self.time_embeddings(model_ts[:steps])
        self._set_context(ctx2)
        x = x_T.to(self.device, torch.float32).clone()
        y_prev = torch.zeros_like(x)
        # one staging launch in front of the loop; every step is then the UNet replay + ONE launch (guidance, solver update and the
        # staging of the next step's inputs: ops.dpm_step = cfg_combine + dpm_update + stage_unet_inputs, bit for bit)
        ops.stage_unet_inputs(x, self.unet.x, temb[0], self._temb_dst)
        for s in range(steps):
            ops.dpm_step(self._unet_eps(), x, y_prev, solver.coef(s), guidance, mode=0,
                         stage=(self.unet.x, temb[s + 1], self._temb_dst) if s + 1 < steps else None)
        return x

    def sample_k(self, ctx2, x, sampler, steps=20, guidance=7.5, schedule='discrete', eta=1.0, first=0, seed=0, image_index=0,
                 step_noise=None):
        """k-diffusion's sample_euler / sample_euler_ancestral / sample_dpmpp_2m ('euler', 'euler_a', 'dpmpp_2m') over KSchedule(steps,
        schedule), steps first .. steps - 1, CFG mode 1, eps or v models.  first = 0: x is unit-variance noise x_T and the trajectory
        starts from sigmas[0] * x_T; first > 0 (img2img): x already lies at level sigmas[first] (z0 + sigmas[first] * noise) and the
        first executed step has no history.  One start launch in front of the loop (the scaling and the first staging), then per step
        the UNet replay and ONE launch (ops.k_step = cfg_combine + lincomb4 + lincomb4 + the c_in multiply + stage_unet_inputs, bit
        for bit): the model sees c_in(i) * x at the fractional time times[i].  euler_a's fresh noise of step i: step_noise[i - first]
        (fp32 [steps - first - 1, n, 4, H, W]; the last step draws none) or Philox on the device, stream ((3 + i) << 32) |
        (image_index + k) of `seed` for image k.  Under cfg_split the step runs redundantly on both ranks behind the exchange."""
        self._require_pairs('sample_k')
        k_check_args(sampler, steps, schedule, eta, step_noise, self._latent_shape, x.shape[0], first)
        sch = KSchedule(steps, schedule)
        temb = self.time_embeddings(sch.times)                             # row i <-> step i
        self._set_context(ctx2)
        x = x.to(self.device, torch.float32).clone()
        if step_noise is not None:
            step_noise = step_noise.to(self.device, torch.float32).contiguous()
        den_prev = torch.empty_like(x) if sampler == 'dpmpp_2m' else None
        ops.k_step(None, x, dict(a=float(sch.sigmas[0]) if first == 0 else 1.0, stage_scale=sch.c_in(first)),
                   stage=(self.unet.x, temb[first], self._temb_dst))
        for i in range(first, steps):
            cf = sch.coef(sampler, i, eta, self.v_prediction, first)
            ops.k_step(self._unet_eps(), x, cf, guidance, den_prev=den_prev,
                       noise=step_noise[i - first] if step_noise is not None and cf['u'] != 0.0 else None,
                       seed=seed, noise_level=i, image_index=image_index, mode=1,
                       stage=(self.unet.x, temb[i + 1], self._temb_dst) if i + 1 < steps else None)
        return x

    # ------------------------------------------------------------------ few-step sampling (Latent Consistency Models)
    def sample_lcm(self, ctx2, x, steps=4, guidance=None, *, original_steps=50, strength=1.0, seed=0, image_index=0, step_noise=None,
                   return_denoised=False):
        """Multistep consistency sampling (Luo et al. 2023; diffusers' LCMScheduler) over LcmSchedule(steps, original_steps, strength),
        eps or v models.  x: unit-variance noise x_T, used as it is (the model sees x itself; strength < 1: x already lies at
        timesteps[0], LcmSchedule.start).  guidance: on a pipeline with the pair, the CFG scale in mode 1 -- the LCM-LoRA form, typically
        1 to 2, None = 1; on an unguided pipeline with guidance_embed the scale w the checkpoint conditions on (required); on an
        unguided pipeline without it, None.  One staging launch in front of the loop, then per step the UNet replay and ONE launch
        (ops.lcm_step = cfg_combine or nhwc_f16_to_nchw_f32 + lincomb4 + lincomb4 + stage_unet_inputs, bit for bit).  The fresh noise
        behind step i: step_noise[i] (fp32 [steps - 1, n, 4, H, W]; the last step draws none) or Philox on the device, stream
        ((3 + i) << 32) | (image_index + k) of `seed` for image k.  return_denoised=True: (x, den) with den the last step's x0
        prediction.  Argument errors raise ValueError before any device work (lcm_check_args)."""
        g, w = lcm_check_args(self, x, steps, guidance, original_steps, strength, step_noise)
        sch = LcmSchedule(int(steps), int(original_steps), float(strength))
        temb = self.time_embeddings(sch.timesteps.astype(np.float32), w)   # row i <-> step i
        self._set_context(ctx2, lcm=True)
        x = x.to(self.device, torch.float32).clone()
        if step_noise is not None:
            step_noise = step_noise.to(self.device, torch.float32).contiguous()
        den = torch.empty_like(x) if return_denoised else None
        ops.stage_unet_inputs(x, self.unet.x, temb[0], self._temb_dst)
        for i in range(sch.steps):
            cf = sch.coef(i, self.v_prediction)
            ops.lcm_step(self._unet_eps(), x, cf, g, den_out=den,
                         noise=step_noise[i] if step_noise is not None and cf['u'] != 0.0 else None,
                         seed=seed, noise_level=i, image_index=image_index, mode=1,
                         stage=(self.unet.x, temb[i + 1], self._temb_dst) if i + 1 < sch.steps else None)
        return (x, den) if return_denoised else x

    def generate_lcm(self, ctx2, x, steps=4, guidance=None, *, original_steps=50, strength=1.0, seed=0, image_index=0, step_noise=None):
        """decode(sample_lcm(...), mode 1): uint8 [n, 8H, 8W, 3]"""
        lcm_check_args(self, x, steps, guidance, original_steps, strength, step_noise)
        self._require_cond()
        z = self.sample_lcm(ctx2, x, steps, guidance, original_steps=original_steps, strength=strength, seed=seed, image_index=image_index,
                            step_noise=step_noise)
        return self.decode(z, mode=1)

    def generate_lcm_graphed(self, ctx2, x, steps=4, guidance=None, *, original_steps=50, strength=1.0, seed=0, image_index=0,
                             step_noise=None):
        """generate_lcm() with the whole trajectory and the decode replayed as ONE device graph, captured once per (steps, guidance,
        shape, original_steps, strength) from the eager path.  The step noise is a static input, the caller's or drawn on the eager
        path's streams (_replay): the result equals generate_lcm() with the same arguments, bit for bit, and the graph bakes no seed."""
        lcm_check_args(self, x, steps, guidance, original_steps, strength, step_noise)
        self._require_cond()
        kw = dict(steps=steps, guidance=guidance, original_steps=original_steps, strength=strength)
        if self.cfg_split:                 # a collective per evaluation cannot live inside one captured graph
            return self.generate_lcm(ctx2, x, seed=seed, image_index=image_index, step_noise=step_noise, **kw)
        key = ('lcm', int(steps), None if guidance is None else float(guidance), tuple(x.shape), int(original_steps), float(strength))
        inputs = dict(ctx2=_copied(ctx2), x=_copied(x, torch.float32))
        if int(steps) > 1:
            inputs['step_noise'] = _step_noise(step_noise, (int(steps) - 1,) + tuple(x.shape), seed, 0, image_index)
        return self._replay(key, lambda **s: self.generate_lcm(**s, **kw), inputs)

    def img2img_lcm(self, ctx2, init_u8, strength=0.5, steps=4, guidance=None, *, original_steps=50, seed=0, noise=None, image_index=0,
                    step_noise=None):
        """img2img in few steps: encode the init image as img2img() does (noise = (n1, n2) or Philox streams 1 and 2), noise its
        clean latent to LcmSchedule(steps, original_steps, strength).timesteps[0] with LcmSchedule.start(), sample_lcm from there,
        decode to uint8.  Needs with_vae_encoder.  Argument errors raise ValueError before any device work."""
        if self.encoder is None:
            raise RuntimeError('Txt2Img(..., with_vae_encoder=True) is needed for img2img')
        lat = (init_u8.shape[0],) + self._latent_shape
        lcm_check_args(self, None, steps, guidance, original_steps, strength, step_noise, shape=lat)
        sch = LcmSchedule(int(steps), int(original_steps), float(strength))
        x = self.encode(init_u8, seed, image_index, noise=noise, coef=sch.start())
        z = self.sample_lcm(ctx2, x, steps, guidance, original_steps=original_steps, strength=strength, seed=seed, image_index=image_index,
                            step_noise=step_noise)
        return self.decode(z, mode=1)

    # ------------------------------------------------------------------ MultiDiffusion panoramas
    def _panorama_plan(self, x_T, sampler, steps, schedule, eta, stride, weights, step_noise):
        """the argument checks of the panorama entry points (no device work before them), then the window plan of (stride, weights):
        origins, chunk count and -- made once per plan -- the device tables wgt [wh, ww] and wsum [H, W] and, for more than one chunk,
        the zero-filled staging buffer [chunks, 2n, 4, wh, ww] and the prediction buffer [chunks, 2n, wh, ww, 4]"""
        c, wh, ww = self._latent_shape
        oy, ox, chunks = PN.panorama_check_args(self.canvas_hw, (wh, ww), self.canvas_wrap, self.n, x_T, sampler, stride, weights)
        k_check_args(sampler, steps, schedule, eta, step_noise, (c,) + tuple(self.canvas_hw), 1)
        key = (tuple(oy), tuple(ox), weights)
        if self._pano is None:
            self._pano = {}
        if key not in self._pano:
            wgt = PN.window_weights((wh, ww), weights)
            plan = dict(oy=oy, ox=ox, chunks=chunks, wgt=torch.from_numpy(wgt).to(self.device),
                        wsum=torch.from_numpy(PN.weight_sum(self.canvas_hw, (wh, ww), oy, ox, wgt, self.canvas_wrap)).to(self.device))
            if chunks > 1:       # zero-filled: the spare rows of a partly filled last chunk evaluate zeros, step after step
                plan['stage'] = torch.zeros((chunks,) + tuple(self.unet.x.shape), dtype=torch.float32, device=self.device)
                plan['eps'] = torch.zeros((chunks,) + tuple(self.unet.eps.shape), dtype=torch.float16, device=self.device)
            self._pano[key] = plan
        return self._pano[key]

    def _panorama_eps(self, plan):
        """the windows' predictions [chunks, 2n, wh, ww, 4]: one chunk -- the staged inputs are unet.x, the result unet.eps; more --
        per chunk its staged rows into unet.x, the UNet, unet.eps out (the time row and the context are the same for every chunk)"""
        if plan['chunks'] == 1:
            return self._unet_eps()
        for k in range(plan['chunks']):
            self.unet.x.copy_(plan['stage'][k])
            plan['eps'][k].copy_(self._unet_eps())
        return plan['eps']

    def sample_panorama(self, ctx2, x_T, sampler='dpmpp_2m', steps=20, guidance=7.5, *, schedule='discrete', eta=1.0, stride=None,
                        weights='uniform', seed=0, image_index=0, step_noise=None):
        """MultiDiffusion on the canvas of Txt2Img(canvas_hw=): x_T fp32 [1, 4, H, W] unit-variance noise -> the canvas latent [1, 4, H, W].
        sample_k's loop with ops.k_step_windows in the place of ops.k_step: the UNet evaluates the overlapping windows of the canvas
        (latent_hw each, `stride` apart -- an int or (sy, sx), default half the window; panorama.plan_windows), n = images_per_gpu per
        evaluation; per step ONE launch averages the windows' guided predictions per canvas pixel with `weights` ('uniform' or
        'gaussian': panorama.window_weights), applies the sampler step on the canvas and scatters c_in * x' into the windows.  One
        history and one noise stream for the whole canvas: euler_a's noise of step i is step_noise[i] (fp32 [steps - 1, 1, 4, H, W]) or
        Philox stream ((3 + i) << 32) | image_index of `seed` over the canvas.  With all windows in one evaluation a step is the UNet
        replay plus that launch; with more, two device copies per further evaluation.  Only the k-samplers: 'plms' and 'dpm' raise
        ValueError, as every other argument error does before any device work."""
        self._require_pairs('sample_panorama')
        plan = self._panorama_plan(x_T, sampler, steps, schedule, eta, stride, weights, step_noise)
        sch = KSchedule(steps, schedule)
        temb = self.time_embeddings(sch.times)                             # row i <-> step i
        self._set_context(ctx2)
        x = x_T.to(self.device, torch.float32).clone()
        if step_noise is not None:
            step_noise = step_noise.to(self.device, torch.float32).contiguous()
        den_prev = torch.empty_like(x) if sampler == 'dpmpp_2m' else None
        x_stage = self.unet.x if plan['chunks'] == 1 else plan['stage']
        grid = dict(wgt=plan['wgt'], wsum=plan['wsum'], window_hw=self._latent_shape[1:], oy=plan['oy'], ox=plan['ox'], n=self.n,
                    chunks=plan['chunks'], wrap_x=self.canvas_wrap)
        ops.k_step_windows(None, x, dict(a=float(sch.sigmas[0]), stage_scale=sch.c_in(0)), stage=(x_stage, temb[0], self._temb_dst), **grid)
        for i in range(steps):
            cf = sch.coef(sampler, i, eta, self.v_prediction, 0)
            ops.k_step_windows(self._panorama_eps(plan), x, cf, guidance=guidance, den_prev=den_prev,
                               noise=step_noise[i] if step_noise is not None and cf['u'] != 0.0 else None,
                               seed=seed, noise_level=i, image_index=image_index, mode=1,
                               stage=(x_stage, temb[i + 1], self._temb_dst) if i + 1 < steps else None, **grid)
        return x

    def decode_canvas(self, latent):
        """the canvas latent fp32 [1, 4, H, W] -> uint8 [1, 8H, 8W, 3] through self.canvas_vae (its x border circular under canvas_wrap),
        ldm's 255 * clamp((x + 1) / 2, 0, 1)"""
        self.canvas_vae.z.copy_(latent)
        self.canvas_vae.execute(self.use_hip_graph)
        return ops.image_to_u8(self.canvas_vae.img, 0.5, 0.5, 1)

    def generate_panorama(self, ctx2, x_T, sampler='dpmpp_2m', steps=20, guidance=7.5, *, schedule='discrete', eta=1.0, stride=None,
                          weights='uniform', seed=0, image_index=0, step_noise=None):
        """decode_canvas(sample_panorama(...)): uint8 [1, 8H, 8W, 3]"""
        self._require_pairs('generate_panorama')
        z = self.sample_panorama(ctx2, x_T, sampler, steps, guidance, schedule=schedule, eta=eta, stride=stride, weights=weights, seed=seed,
                                 image_index=image_index, step_noise=step_noise)
        return self.decode_canvas(z)

    def generate_panorama_graphed(self, ctx2, x_T, sampler='dpmpp_2m', steps=20, guidance=7.5, *, schedule='discrete', eta=1.0, stride=None,
                                  weights='uniform', seed=0, image_index=0, step_noise=None):
        """generate_panorama() with the whole trajectory -- every chunk's UNet evaluation and copies, the canvas steps, the canvas
        decode -- replayed as ONE device graph (_replay), captured once per (sampler, steps, guidance, schedule, eta, stride, weights).
        euler_a's step noise is a static input, the caller's or drawn on the eager path's streams: the result equals
        generate_panorama() with the same arguments, bit for bit."""
        self._require_pairs('generate_panorama_graphed')
        plan = self._panorama_plan(x_T, sampler, steps, schedule, eta, stride, weights, step_noise)
        kw = dict(sampler=sampler, steps=steps, guidance=guidance, schedule=schedule, eta=eta, stride=stride, weights=weights)
        key = ('panorama', sampler, int(steps), float(guidance), schedule, float(eta), tuple(plan['oy']), tuple(plan['ox']), weights)
        inputs = dict(ctx2=_copied(ctx2), x_T=_copied(x_T, torch.float32))
        if sampler == 'euler_a':
            inputs['step_noise'] = _step_noise(step_noise, (int(steps) - 1,) + tuple(x_T.shape), seed, 0, image_index)
        return self._replay(key, lambda **s: self.generate_panorama(**s, **kw), inputs)

    def _sample(self, sampler, ctx2, x_T, steps, guidance, *, schedule='discrete', eta=1.0, seed=0, image_index=0, step_noise=None):
        """a whole trajectory from unit-variance noise x_T: 'plms', 'dpm' (the keyword arguments play no part) or a k-sampler from its
        first step"""
        if sampler in K_SAMPLERS:
            return self.sample_k(ctx2, x_T, sampler, steps, guidance, schedule, eta, 0, seed, image_index, step_noise)
        return self.sample_plms(ctx2, x_T, steps, guidance) if sampler == 'plms' else self.sample_dpm(ctx2, x_T, steps, guidance)

    def _sample_from(self, k_sampler, ctx2, start, t_enc, steps, guidance, schedule, eta, seed, image_index, step_noise, trace=None):
        """start at a noise level and finish (img2img, the hires pass): the last t_enc of `steps` evaluations.  start(a, b) makes the
        start latent a * z0 + b * noise from the clean latent.  k_sampler None: ldm's DDIM, (a, b) = (sqrt_alphas[t_enc],
        sqrt_one_minus_alphas[t_enc]), then sample_ddim_from(t_enc).  A k-sampler: first = steps - t_enc, (a, b) = (1, sigmas[first]),
        then sample_k(first=first)."""
        if k_sampler is None:
            sch = PlmsSchedule(steps)
            x = start(float(sch.sqrt_alphas[t_enc]), float(sch.sqrt_one_minus_alphas[t_enc]))
            return self.sample_ddim_from(ctx2, x, t_enc, steps, guidance, trace)
        first = int(steps) - t_enc
        x = start(1.0, float(KSchedule(steps, schedule).sigmas[first]))
        return self.sample_k(ctx2, x, k_sampler, steps, guidance, schedule, eta, first, seed, image_index, step_noise)

    @property
    def _latent_shape(self):
        return (self.cfg.latent_channels, self.cfg.latent_h, self.cfg.latent_w)

    # ------------------------------------------------------------------ decode
    def decode(self, latents, mode=1, composite=None):
        """latents fp32 [n,4,H,W] -> uint8 [n, 8H, 8W, 3] (mode 1 = ldm's 255*clamp((x+1)/2,0,1); mode 0 = reference driver).
        composite = (init_u8, mask_u8): inpainting's pixel composite in the place of image_to_u8, (d k + u (255 - k) + 127) / 255 per
        byte (d decoded, u init, k mask byte)"""
        outs = []
        for i in range(latents.shape[0]):
            self.vae.z.copy_(latents[i:i + 1])
            self.vae.execute(self.use_hip_graph)
            if composite is None:
                outs.append(ops.image_to_u8(self.vae.img, 0.5, 0.5, mode))
            else:
                outs.append(ops.image_composite(self.vae.img, composite[0][i:i + 1], composite[1][i:i + 1], 0.5, 0.5, mode))
        return torch.cat(outs, 0)

    def generate(self, ctx2, x_T, steps=20, guidance=7.5, sampler='plms', *, schedule='discrete', eta=1.0, seed=0, image_index=0,
                 step_noise=None):
        """sampler 'plms' / 'dpm': as ever (schedule, eta, seed, image_index play no part; a non-default schedule or a step_noise
        raises).  'euler' / 'euler_a' / 'dpmpp_2m': sample_k from sigmas[0] * x_T (x_T stays unit-variance noise) on schedule
        'discrete' or 'karras', decode mode 1; eta, seed, image_index, step_noise (fp32 [steps - 1, n, 4, H, W]) are euler_a's noise.
        Argument errors raise ValueError before any device work."""
        self._require_pairs('generate')
        k_check_args(sampler, steps, schedule, eta, step_noise, self._latent_shape, x_T.shape[0], old_samplers=True)
        self._require_cond()
        z = self._sample(sampler, ctx2, x_T, steps, guidance, schedule=schedule, eta=eta, seed=seed, image_index=image_index,
                         step_noise=step_noise)
        return self.decode(z, mode=0 if sampler == 'dpm' else 1)

    # ------------------------------------------------------------------ whole trajectories as one device graph
    def _graphed(self, key, inputs, run):
        """The capture behind every *_graphed method.  On the first use of `key`: allocates the graph's static inputs (`inputs`:
        [(shape, dtype)], zeroed), calls run(*statics) -- the eager method -- once as warm-up (kernel attributes, time embeddings,
        tuning) and captures a second call as ONE device graph, so a replay is the same kernels on the same buffers, bit for bit.
        Returns the cached (graph, statics, out); the caller (_replay) fills the statics, then replays."""
        if self._traj is None:
            self._traj = {}
        if self._control_on:                    # a capture made with the control graph in it is another trajectory than one without
            key = (key, 'control')
        if key not in self._traj:
            statics = [torch.zeros(tuple(shape), dtype=dtype, device=self.device) for shape, dtype in inputs]
            pipes = [self] if self.hires is None else [self, self.hires]
            keep = [p.use_hip_graph for p in pipes]
            for p in pipes:                     # inside a capture the engine graphs run their launch lists, not graphs of their own
                p.use_hip_graph = False
            try:
                run(*statics)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                # thread_local: another thread of the process (a collective backend's watchdog) may touch the runtime meanwhile
                with torch.cuda.graph(g, capture_error_mode='thread_local'):
                    out = run(*statics)
            finally:
                for p, k in zip(pipes, keep):
                    p.use_hip_graph = k
            self._traj[key] = (g, statics, out)
        return self._traj[key]

    def _fill_noise(self, dst, seed, family, image_index):
        """dst fp32 [n, 4, H, W] (a static noise input of a graph): image i from Philox stream (family << 32) | (image_index + i) of
        `seed` by sdod_randn_f32, which is what the eager path's kernels draw for it, bit for bit"""
        for i in range(dst.shape[0]):
            ops.randn(tuple(dst[i:i + 1].shape), seed, (family << 32) | (image_index + i), self.device, out=dst[i:i + 1])

    def _fill(self, static, desc):
        """one static input of a graph from its description (_copied, _noise, _step_noise): the caller's tensor copied into it, or --
        a noise input the caller did not pass -- drawn into it, row r of step noise [rows, n, 4, H, W] from family `family + r`"""
        _, _, value, draw = desc
        if value is not None:
            static.copy_(value)
            return
        seed, family, image_index = draw
        rows = static[None] if static.dim() == 4 else static
        for r in range(rows.shape[0]):
            self._fill_noise(rows[r], seed, family + r, image_index)

    def _replay(self, key, run, inputs):
        """Everything a *_graphed method does after its checks.  inputs: {keyword argument of `run`: description}, in the order the
        static inputs are allocated; run(**statics) is the eager method on them.  Captures on the first use of `key` (_graphed), fills
        every static from its description (_fill), replays, returns the graph's output buffer.  The noise descriptions name the Philox
        streams the eager path's kernels draw from -- (family << 32) | (image_index + i) for image i: family 1 = n1, 2 = n2 (of
        hires_seed: hires_noise), 3 + step = a k-sampler's or inpaint's step noise -- so graphed equals eager bit for bit and the graph
        bakes no seed."""
        names = list(inputs)
        g, statics, out = self._graphed(key, [d[:2] for d in inputs.values()], lambda *s: run(**dict(zip(names, s))))
        for static, desc in zip(statics, inputs.values()):
            self._fill(static, desc)
        g.replay()
        return out

    def generate_graphed(self, ctx2, x_T, steps=20, guidance=7.5, sampler='plms', *, schedule='discrete', eta=1.0, seed=0, image_index=0,
                         step_noise=None):
        """generate() with the WHOLE trajectory -- context upload, every UNet evaluation, CFG, sampler updates, VAE decode,
        uint8 -- replayed as ONE device graph: the host enqueues a single launch per image instead of ~9 small launches per
        step, so the GPU never waits for Python between steps (2-3 ms per image at 20 steps).  The sequence is static for a
        given (sampler, steps, guidance, batch, schedule, eta): it is captured once from the ordinary eager code path (so it is the
        same kernels on the same buffers, bit for bit) and cached; ctx2 / x_T are copied into the graph's static inputs.  euler_a's
        step noise is a static input too, the caller's or drawn on the eager path's streams (_replay): the result equals generate() with
        the same arguments."""
        self._require_pairs('generate_graphed')
        k_check_args(sampler, steps, schedule, eta, step_noise, self._latent_shape, x_T.shape[0], old_samplers=True)
        self._require_cond()
        kw = dict(steps=steps, guidance=guidance, sampler=sampler, schedule=schedule, eta=eta)
        if self.cfg_split:                 # a collective per evaluation cannot live inside one captured graph
            return self.generate(ctx2, x_T, seed=seed, image_index=image_index, step_noise=step_noise, **kw)
        key = (sampler, int(steps), float(guidance), tuple(x_T.shape), schedule, float(eta))
        inputs = dict(ctx2=_copied(ctx2), x_T=_copied(x_T, torch.float32))
        if sampler == 'euler_a':
            inputs['step_noise'] = _step_noise(step_noise, (int(steps) - 1,) + tuple(x_T.shape), seed, 0, image_index)
        return self._replay(key, lambda **s: self.generate(**s, **kw), inputs)

    # ------------------------------------------------------------------ ESRGAN x4 upscaling of the pipeline's images
    def upscale(self, img_u8):
        """uint8 [n, 8H, 8W, 3] (this pipeline's images; with hires_hw the hires pipeline's) -> uint8 [n, 32H, 32W, 3] through
        self.upscaler (Txt2Img(upscaler=True)).  Argument errors raise ValueError before any device work."""
        upscale_check_args(self, img_u8)
        return self.upscaler.upscale(img_u8.to(self.device))

    def generate_upscaled(self, ctx2, x_T, steps=20, guidance=7.5, sampler='plms', *, schedule='discrete', eta=1.0, seed=0, image_index=0,
                          step_noise=None):
        """upscale(generate(...)) -- with hires_hw: upscale(generate_hires(...)) with the hires pass's defaults.  generate()'s arguments."""
        self._require_pairs('generate_upscaled')
        upscale_check_args(self, None)
        kw = dict(steps=steps, guidance=guidance, sampler=sampler, schedule=schedule, eta=eta, seed=seed, image_index=image_index,
                  step_noise=step_noise)
        k_check_args(sampler, steps, schedule, eta, step_noise, self._latent_shape, x_T.shape[0], old_samplers=True)
        img = self.generate(ctx2, x_T, **kw) if self.hires is None else self.generate_hires(ctx2, x_T, **kw)
        return self.upscaler.upscale(img)

    def generate_upscaled_graphed(self, ctx2, x_T, steps=20, guidance=7.5, sampler='plms', *, schedule='discrete', eta=1.0, seed=0,
                                  image_index=0, step_noise=None):
        """generate_upscaled() with the trajectory, the decode and the upscale replayed as ONE device graph (captured once per
        generate_graphed key from the eager path, so it is the same kernels on the same buffers: the result equals
        generate_upscaled() with the same arguments).  generate_graphed()'s arguments; not with hires_hw (generate_hires_graphed has
        its own noise inputs) or cfg_split: ValueError."""
        self._require_pairs('generate_upscaled_graphed')
        upscale_check_args(self, None)
        if self.hires is not None or getattr(self, 'cfg_split', False):
            raise ValueError('generate_upscaled_graphed cannot be combined with hires_hw or cfg_split: use generate_upscaled')
        k_check_args(sampler, steps, schedule, eta, step_noise, self._latent_shape, x_T.shape[0], old_samplers=True)
        self._require_cond()
        kw = dict(steps=steps, guidance=guidance, sampler=sampler, schedule=schedule, eta=eta)
        key = ('upscaled', sampler, int(steps), float(guidance), tuple(x_T.shape), schedule, float(eta))
        inputs = dict(ctx2=_copied(ctx2), x_T=_copied(x_T, torch.float32))
        if sampler == 'euler_a':
            inputs['step_noise'] = _step_noise(step_noise, (int(steps) - 1,) + tuple(x_T.shape), seed, 0, image_index)
        up = self.upscaler
        keep = up.use_hip_graph

        def run(**s):
            up.use_hip_graph = False       # inside the capture the upscaler runs its launch list, like the other engine graphs
            try:
                return self.generate_upscaled(**s, **kw)
            finally:
                up.use_hip_graph = keep
        return self._replay(key, run, inputs)

    # ------------------------------------------------------------------ img2img (ldm scripts/img2img.py, DDIM eta = 0)
    def encode(self, init_u8, seed=0, image_index=0, strength=0.75, steps=50, noise=None, return_z0=False, coef=None):
        """uint8 [n, 8H, 8W, 3] -> x fp32 [n, 4, H, W]: the VAE encoder, a posterior sample scaled by 0.18215, and ldm's
        stochastic_encode to ddim index t_enc = int(strength * steps).  noise = (n1, n2), fp32 [n, 4, H, W] each, or None: drawn
        on the device (Philox, seed, streams (1 << 32) | index and (2 << 32) | index with index = image_index + i).
        return_z0=True: returns (x, z0) with z0 fp32 [n, 4, H, W] the clean latent (the scaled posterior sample) from the same launch.
        coef = (c_z0, c_noise): x = c_z0 * z0 + c_noise * n2 with these in the place of ldm's (sqrt(abar), sqrt(1 - abar)) at t_enc --
        (1, sigmas[first]) is the k-samplers' start latent."""
        if self.encoder is None:
            raise RuntimeError('Txt2Img(..., with_vae_encoder=True) is needed for img2img')
        sch, t_enc = img2img_schedule(strength, steps)
        c_z0, c_noise = (float(sch.sqrt_alphas[t_enc]), float(sch.sqrt_one_minus_alphas[t_enc])) if coef is None else coef
        init_u8 = init_u8.to(self.device)
        xs = []
        z0 = None
        if return_z0:
            z0 = torch.empty((init_u8.shape[0],) + self._latent_shape, dtype=torch.float32, device=self.device)
        for i in range(init_u8.shape[0]):
            self.encoder.img.copy_(init_u8[i:i + 1])
            self.encoder.execute(self.use_hip_graph)
            n1, n2 = (None, None) if noise is None else (noise[0][i:i + 1].to(self.device, torch.float32).contiguous(),
                                                         noise[1][i:i + 1].to(self.device, torch.float32).contiguous())
            xs.append(ops.encode_latent(self.encoder.moments, float(c_z0), float(c_noise),
                                        seed, image_index + i, n1, n2, z0=None if z0 is None else z0[i:i + 1]))
        x = torch.cat(xs, 0)
        return (x, z0) if return_z0 else x

    def sample_ddim_from(self, ctx2, x, t_enc, steps=50, guidance=7.5, trace=None):
        """ldm DDIMSampler.decode: t_enc DDIM steps (eta = 0, CFG mode 1) from ddim index t_enc - 1 down to 0"""
        self._require_pairs('sample_ddim_from')
        sch = PlmsSchedule(steps)
        temb = self.time_embeddings(sch.timesteps.astype(np.float32))     # row k <-> timestep index k
        self._set_context(ctx2)
        x = x.to(self.device, torch.float32).clone()
        for i in range(t_enc):
            index = t_enc - i - 1
            e_t = self._eps(x, temb[index], guidance, mode=1)
            ops.ddim_step(x, e_t, **sch.coef(index))
            if trace is not None:
                trace.append((int(sch.timesteps[index]), index))
        return x

    def img2img(self, ctx2, init_u8, strength=0.75, steps=50, guidance=7.5, seed=0, noise=None, image_index=0, trace=None, sampler=None,
                schedule='discrete', eta=1.0, step_noise=None):
        """ldm scripts/img2img.py: encode the init image, noise it to ddim index int(strength * steps), denoise, decode to uint8.
        sampler None: ldm's DDIM, as ever.  'euler' / 'euler_a' / 'dpmpp_2m': with t_enc = int(strength * steps) and first = steps -
        t_enc the start latent is z0 + sigmas[first] * n2 and sample_k(first=first) makes the t_enc evaluations; step_noise fp32
        [t_enc - 1, n, 4, H, W], row r = step first + r (euler_a); `trace` is not filled."""
        self._require_pairs('img2img')
        t_enc = img2img_k_check_args(strength, steps, sampler, schedule, eta, step_noise, self._latent_shape, init_u8.shape[0])
        z = self._sample_from(sampler, ctx2, lambda a, b: self.encode(init_u8, seed, image_index, strength, steps, noise, coef=(a, b)),
                              t_enc, steps, guidance, schedule, eta, seed, image_index, step_noise, trace)
        return self.decode(z, mode=1)

    def img2img_graphed(self, ctx2, init_u8, strength=0.75, steps=50, guidance=7.5, seed=0, noise=None, image_index=0, sampler=None,
                        schedule='discrete', eta=1.0, step_noise=None):
        """img2img() as ONE device graph replay (encoder, start latent, every UNet evaluation, DDIM updates, decoder, uint8), captured
        once per (t_enc, steps, guidance, shape) from the eager path.  The noise is always an input of the graph, the caller's or drawn
        on the streams encode() uses (_replay), so the result equals img2img() with the same arguments.  With a k-sampler the key adds
        (sampler, schedule, eta), and euler_a's step noise is one more input of the graph."""
        self._require_pairs('img2img_graphed')
        t_enc = img2img_k_check_args(strength, steps, sampler, schedule, eta, step_noise, self._latent_shape, init_u8.shape[0])
        kw = dict(strength=strength, steps=steps, guidance=guidance, sampler=sampler, schedule=schedule, eta=eta)
        if self.cfg_split:
            return self.img2img(ctx2, init_u8, seed=seed, noise=noise, image_index=image_index, step_noise=step_noise, **kw)
        lat = (init_u8.shape[0],) + self._latent_shape
        key = ('img2img', t_enc, int(steps), float(guidance), tuple(init_u8.shape))
        if sampler is not None:
            key += (sampler, schedule, float(eta))
        inputs = dict(ctx2=_copied(ctx2), init_u8=_copied(init_u8, torch.uint8), **_noise_pair(noise, lat, seed, image_index))
        if sampler == 'euler_a':
            inputs['step_noise'] = _step_noise(step_noise, (t_enc - 1,) + lat, seed, int(steps) - t_enc, image_index)
        return self._replay(key, lambda n1, n2, **s: self.img2img(noise=(n1, n2), **s, **kw), inputs)

    # ------------------------------------------------------------------ inpainting (ldm DDIMSampler.ddim_sampling(mask=, x0=) on img2img's start)
    def sample_ddim_inpaint(self, ctx2, x, z0, keep, t_enc, steps=50, guidance=7.5, seed=0, image_index=0, step_noise=None, trace=None):
        """t_enc DDIM steps (eta = 0, CFG mode 1) from ddim index t_enc - 1 down to 0 with ldm's latent blend after every step:
        x' = DDIM step(x, e) has reached the level of ddim index j = index - 1, and x = keep * known + (1 - keep) * x' with
        known = sqrt_alphas[j] * z0 + sqrt_one_minus_alphas[j] * nu_j (ldm q_sample of the clean latent z0 at timesteps[j]), or
        known = z0 after the last step (index 0: nothing is drawn).  keep: fp32 [n, H, W], 1 = keep the init image, or None (a plain
        DDIM decode on the fused step).  nu_j: step_noise[j] (fp32 [t_enc - 1, n, 4, H, W]) or Philox on the device, stream
        ((3 + j) << 32) | (image_index + i) of `seed` for image i.
        Against ldm's masked ddim_sampling, which blends BEFORE each evaluation, this blends AFTER each step for the next
        evaluation: the same sequence, except that the start latent is not blended (it is the noised init image everywhere
        already) and that there is a final noise-free blend, so the kept region of the result is z0 itself.
        One staging launch in front of the loop, then per step the UNet replay and ONE launch (ops.ddim_inpaint_step = cfg_combine
        + ddim_step + the blend + stage_unet_inputs, bit for bit)."""
        self._require_pairs('sample_ddim_inpaint')
        sch = PlmsSchedule(steps)
        temb = self.time_embeddings(sch.timesteps.astype(np.float32))     # row k <-> timestep index k
        self._set_context(ctx2)
        x = x.to(self.device, torch.float32).clone()
        ops.stage_unet_inputs(x, self.unet.x, temb[t_enc - 1], self._temb_dst)
        for index, j, sa, s1a in inpaint_levels(sch, t_enc):
            ops.ddim_inpaint_step(self._unet_eps(), x, sch.coef(index), guidance, z0=z0, keep=keep, known=None if j is None else (sa, s1a),
                                  noise=None if j is None or step_noise is None else step_noise[j],
                                  seed=seed, noise_level=j or 0, image_index=image_index, mode=1,
                                  v_coef=sch.v_to_eps_coef(index) if self.v_prediction else None,
                                  stage=None if j is None else (self.unet.x, temb[j], self._temb_dst))
            if trace is not None:
                trace.append((int(sch.timesteps[index]), index))
        return x

    def _inpaint_args(self, init_u8, mask_u8, strength, steps, step_noise):
        """the host-side checks of inpaint() / inpaint_graphed(), in one order for both: argument errors (ValueError), then the
        missing encoder; returns t_enc"""
        _, t_enc = inpaint_check_args(init_u8, mask_u8, strength, steps, step_noise, self._latent_shape, self.n)
        if self.encoder is None:
            raise RuntimeError('Txt2Img(..., with_vae_encoder=True) is needed for inpainting')
        return t_enc

    def inpaint(self, ctx2, init_u8, mask_u8, strength=0.75, steps=50, guidance=7.5, seed=0, noise=None, step_noise=None,
                image_index=0, composite=True, trace=None):
        """Inpainting with the 4-channel UNet (latent blending): init_u8 uint8 [n, 8H, 8W, 3], mask_u8 uint8 [n, 8H, 8W] (255 =
        repaint, 0 = keep, values between blend).  keep = (16320 - 8 x 8 block sum of the mask) / 16320 per latent pixel; img2img's
        start latent at ddim index int(strength * steps) and the clean latent z0 from one launch; sample_ddim_inpaint; VAE decode;
        then per byte out = (d k + u (255 - k) + 127) / 255 (d decoded, u init, k mask byte), so the pixels with k = 0 are the init
        image's bit for bit.  composite=False returns the plain decode.  noise = (n1, n2) as encode(); step_noise fp32
        [t_enc - 1, n, 4, H, W] or None (device Philox, see sample_ddim_inpaint).  Argument errors raise ValueError before any
        device work."""
        self._require_pairs('inpaint')
        t_enc = self._inpaint_args(init_u8, mask_u8, strength, steps, step_noise)
        init_u8 = init_u8.to(self.device).contiguous()
        mask_u8 = mask_u8.to(self.device).contiguous()
        if step_noise is not None:
            step_noise = step_noise.to(self.device, torch.float32).contiguous()
        keep = ops.mask_to_latent(mask_u8)
        x, z0 = self.encode(init_u8, seed, image_index, strength, steps, noise, return_z0=True)
        z = self.sample_ddim_inpaint(ctx2, x, z0, keep, t_enc, steps, guidance, seed, image_index, step_noise, trace)
        return self.decode(z, mode=1, composite=(init_u8, mask_u8) if composite else None)

    def inpaint_graphed(self, ctx2, init_u8, mask_u8, strength=0.75, steps=50, guidance=7.5, seed=0, noise=None, step_noise=None,
                        image_index=0, composite=True):
        """inpaint() as ONE device graph replay (mask reduction, encoder, start latent, every UNet evaluation and fused step, decoder,
        composite), captured once per (t_enc, steps, guidance, composite, shape) from the eager path.  Image, mask and all noise are
        inputs of the graph, the caller's or drawn on the eager path's streams (_replay), so the result equals inpaint() with the same
        arguments.  Eager under cfg_split."""
        self._require_pairs('inpaint_graphed')
        t_enc = self._inpaint_args(init_u8, mask_u8, strength, steps, step_noise)
        kw = dict(strength=strength, steps=steps, guidance=guidance, composite=composite)
        if self.cfg_split:
            return self.inpaint(ctx2, init_u8, mask_u8, seed=seed, noise=noise, step_noise=step_noise, image_index=image_index, **kw)
        lat = (init_u8.shape[0],) + self._latent_shape
        key = ('inpaint', t_enc, int(steps), float(guidance), bool(composite), tuple(init_u8.shape))
        inputs = dict(ctx2=_copied(ctx2), init_u8=_copied(init_u8), mask_u8=_copied(mask_u8), **_noise_pair(noise, lat, seed, image_index),
                      step_noise=_step_noise(step_noise, (t_enc - 1,) + lat, seed, 0, image_index))
        return self._replay(key, lambda n1, n2, **s: self.inpaint(noise=(n1, n2), **s, **kw), inputs)

    # ------------------------------------------------------------------ inpainting with a 9-channel UNet (runwayml inpaint_st.py, ldm `hybrid`)
    def _inpaint_concat_args(self, init_u8, mask_u8, x_T, steps, sampler, noise):
        """the host-side checks of inpaint_concat() / inpaint_concat_graphed(), in one order for both: argument errors (ValueError),
        then the missing 9-channel UNet (RuntimeError)"""
        inpaint_concat_check_args(init_u8, mask_u8, x_T, steps, sampler, noise, self._latent_shape, self.n)
        if self.masked_encoder is None:
            raise RuntimeError('Txt2Img(..., inpaint_unet=True) and a 9-channel inpainting checkpoint are needed for inpaint_concat')

    def stage_inpaint_cond(self, init_u8, mask_u8, seed=0, image_index=0, noise=None):
        """the UNet's conditioning input from the image and the mask: the masked encoder per image, then ONE launch into unet.cond
        (ops.inpaint_cond: nearest-downsampled binarised mask | 0.18215 * posterior sample of the masked image, for both guidance
        halves).  It is written once per image, no sampler launch touches it."""
        moments = []
        for i in range(init_u8.shape[0]):
            self.masked_encoder.img.copy_(init_u8[i:i + 1])
            self.masked_encoder.mask.copy_(mask_u8[i:i + 1])
            self.masked_encoder.execute(self.use_hip_graph)
            moments.append(self.masked_encoder.moments if init_u8.shape[0] == 1 else self.masked_encoder.moments.clone())
        mom = moments[0] if len(moments) == 1 else torch.cat(moments, 0)
        n1 = None if noise is None else noise.to(self.device, torch.float32).contiguous()
        ops.inpaint_cond(mom, mask_u8, seed, image_index, n1, out=self.unet.cond, reps=self.unet.batch // self.n)
        self._cond_staged = True

    def inpaint_concat(self, ctx2, init_u8, mask_u8, x_T, steps=20, guidance=7.5, sampler='plms', seed=0, noise=None, image_index=0,
                       composite=True):
        """Inpainting with a 9-channel UNet: init_u8 uint8 [n, 8H, 8W, 3], mask_u8 uint8 [n, 8H, 8W] (255 = repaint).  m = mask >= 128;
        the VAE encoder runs on (2 u / 255 - 1) * (1 - m); c_lat = 0.18215 * posterior sample with noise n1 (`noise`, fp32 [n, 4, H, W], or
        None: Philox on the device, stream (1 << 32) | (image_index + i) of `seed`); c_mask = m[:, ::8, ::8]; the UNet sees
        cat(x, c_mask, c_lat) in both guidance halves.  From pure noise x_T the ordinary sampler ('plms' or 'dpm', all steps), decode, and
        with composite=True the integer pixel composite of inpaint() with the unbinarised mask bytes (pixels with mask byte 0 are
        the init image's).  Argument errors raise ValueError before any device work."""
        self._require_pairs('inpaint_concat')
        self._inpaint_concat_args(init_u8, mask_u8, x_T, steps, sampler, noise)
        init_u8 = init_u8.to(self.device).contiguous()
        mask_u8 = mask_u8.to(self.device).contiguous()
        self.stage_inpaint_cond(init_u8, mask_u8, seed, image_index, noise)
        z = self._sample(sampler, ctx2, x_T, steps, guidance)
        return self.decode(z, mode=1, composite=(init_u8, mask_u8) if composite else None)

    def inpaint_concat_graphed(self, ctx2, init_u8, mask_u8, x_T, steps=20, guidance=7.5, sampler='plms', seed=0, noise=None,
                               image_index=0, composite=True):
        """inpaint_concat() as ONE device graph replay (masked encoder, conditioning, every UNet evaluation and sampler update, decoder,
        composite), captured once per (sampler, steps, guidance, composite, shape) from the eager path.  Image, mask, x_T and the noise
        are inputs of the graph, the noise the caller's or drawn on the eager path's stream (_replay), so the result equals
        inpaint_concat() with the same arguments.  Eager under cfg_split."""
        self._require_pairs('inpaint_concat_graphed')
        self._inpaint_concat_args(init_u8, mask_u8, x_T, steps, sampler, noise)
        kw = dict(steps=steps, guidance=guidance, sampler=sampler, composite=composite)
        if self.cfg_split:
            return self.inpaint_concat(ctx2, init_u8, mask_u8, x_T, seed=seed, noise=noise, image_index=image_index, **kw)
        lat = (init_u8.shape[0],) + self._latent_shape
        key = ('inpaint_concat', sampler, int(steps), float(guidance), bool(composite), tuple(init_u8.shape))
        inputs = dict(ctx2=_copied(ctx2), init_u8=_copied(init_u8), mask_u8=_copied(mask_u8), x_T=_copied(x_T, torch.float32),
                      noise=_noise(noise, lat, seed, 1, image_index))
        return self._replay(key, lambda **s: self.inpaint_concat(**s, **kw), inputs)

    # ------------------------------------------------------------------ hires: sample small, resize the latent, img2img at the target size
    def hires_from_latent(self, ctx2, z_lo, sampler='dpmpp_2m', guidance=7.5, *, hires_steps, hires_seed, denoise=0.7, upscaler='bilinear',
                          schedule='karras', eta=1.0, image_index=0, hires_noise=None, hires_step_noise=None):
        """The second pass alone: z_lo fp32 [n, 4, h, w] (a clean latent of the base size) -> uint8 [n, 8 H2, 8 W2, 3].  The hires
        pipeline's img2img loop with strength = denoise and steps = hires_steps, started from the resized latent instead of an encoded
        image: t_enc = int(denoise * hires_steps) (img2img_schedule's domain).
        sampler 'plms' / 'dpm' (schedule plays no part): x = sqrt_alphas[t_enc] * R(z_lo) + sqrt_one_minus_alphas[t_enc] * nu from ONE
        ops.latent_resize launch, then hires.sample_ddim_from(ctx2, x, t_enc, hires_steps, guidance); ValueError with model='sd21' (the
        DDIM img2img loop has no v-conversion).  A k-sampler: first = hires_steps - t_enc, x = R(z_lo) + sigmas[first] * nu, then
        hires.sample_k(..., first=first) with the same sampler, schedule and eta.  Then hires.decode(z, mode=1).
        R: upscaler 'nearest-exact', 'bilinear' or 'bicubic' (F.interpolate, align_corners=False, no antialiasing).  nu: hires_noise
        (fp32 [n, 4, H2, W2]) or Philox family 2 of hires_seed; euler_a's step noise: hires_step_noise (fp32 [t_enc - 1, n, 4, H2, W2],
        row r = step first + r) or families 3 + step of hires_seed.  hires_steps and hires_seed have no defaults here: generate_hires
        owns them (steps and seed + 1).  Argument errors raise ValueError before any device work."""
        self._require_pairs('hires_from_latent')
        if not isinstance(z_lo, torch.Tensor) or z_lo.dim() != 4 or tuple(z_lo.shape[1:]) != self._latent_shape:
            raise ValueError(f'z_lo must be a tensor [n, {", ".join(str(v) for v in self._latent_shape)}], got {tuple(getattr(z_lo, "shape", ()))}')
        t_enc = hires_check_args(self, z_lo.shape[0], sampler, hires_steps, denoise, upscaler, schedule, eta, hires_noise, hires_step_noise)
        hires_steps = int(hires_steps)
        hi = self.hires
        z_lo = z_lo.to(self.device, torch.float32).contiguous()
        if hires_noise is not None:
            hires_noise = hires_noise.to(self.device, torch.float32).contiguous()
        z = hi._sample_from(sampler if sampler in K_SAMPLERS else None, ctx2,
                            lambda a, b: ops.latent_resize(z_lo, hi._latent_shape[1:], upscaler, a, b, hires_noise, hires_seed, image_index),
                            t_enc, hires_steps, guidance, schedule, eta, hires_seed, image_index, hires_step_noise)
        return hi.decode(z, mode=1)

    def generate_hires(self, ctx2, x_T, steps=20, guidance=7.5, sampler='dpmpp_2m', *, hires_steps=None, denoise=0.7, upscaler='bilinear',
                       schedule='karras', eta=1.0, seed=0, image_index=0, step_noise=None, hires_seed=None, hires_noise=None,
                       hires_step_noise=None):
        """The two-pass hires fix: pass 1 is generate()'s sampling at the base size without the decode (sampler 'plms' / 'dpm', which
        take no schedule, or a k-sampler on `schedule`; seed, step_noise are euler_a's first-pass noise), pass 2 is hires_from_latent()
        on its result with hires_steps (default: steps) and denoise.  hires_seed defaults to seed + 1: with the same seed pass 2's
        step-noise streams would coincide with pass 1's.  Returns uint8 [n, 8 H2, 8 W2, 3].  Argument errors raise ValueError before
        any device work."""
        self._require_pairs('generate_hires')
        sched1 = schedule if sampler in K_SAMPLERS else 'discrete'
        hires_steps = steps if hires_steps is None else hires_steps
        k_check_args(sampler, steps, sched1, eta, step_noise, self._latent_shape, x_T.shape[0], old_samplers=True)
        hires_check_args(self, x_T.shape[0], sampler, hires_steps, denoise, upscaler, schedule, eta, hires_noise, hires_step_noise)
        hires_seed = int(seed) + 1 if hires_seed is None else hires_seed
        z_lo = self._sample(sampler, ctx2, x_T, steps, guidance, schedule=schedule, eta=eta, seed=seed, image_index=image_index,
                            step_noise=step_noise)
        return self.hires_from_latent(ctx2, z_lo, sampler, guidance, hires_steps=hires_steps, denoise=denoise, upscaler=upscaler,
                                      schedule=schedule, eta=eta, hires_seed=hires_seed, image_index=image_index, hires_noise=hires_noise,
                                      hires_step_noise=hires_step_noise)

    def generate_hires_graphed(self, ctx2, x_T, steps=20, guidance=7.5, sampler='dpmpp_2m', *, hires_steps=None, denoise=0.7,
                               upscaler='bilinear', schedule='karras', eta=1.0, seed=0, image_index=0, step_noise=None, hires_seed=None,
                               hires_noise=None, hires_step_noise=None):
        """generate_hires() as ONE device graph replay (both trajectories, the resize, the decode), captured once per (sampler, steps,
        hires_steps, t_enc, guidance, upscaler, schedule, eta, shape) from the eager path.  ctx2, x_T and all noise are inputs of the
        graph, the caller's or drawn on the eager path's streams (_replay), so the result equals generate_hires() with the same
        arguments."""
        self._require_pairs('generate_hires_graphed')
        sched1 = schedule if sampler in K_SAMPLERS else 'discrete'
        hires_steps = steps if hires_steps is None else hires_steps
        k_check_args(sampler, steps, sched1, eta, step_noise, self._latent_shape, x_T.shape[0], old_samplers=True)
        t_enc = hires_check_args(self, x_T.shape[0], sampler, hires_steps, denoise, upscaler, schedule, eta, hires_noise, hires_step_noise)
        hires_steps = int(hires_steps)
        hires_seed = int(seed) + 1 if hires_seed is None else hires_seed
        kw = dict(steps=steps, guidance=guidance, sampler=sampler, hires_steps=hires_steps, denoise=denoise, upscaler=upscaler,
                  schedule=schedule, eta=eta)
        lat_hi = (x_T.shape[0],) + self.hires._latent_shape
        key = ('hires', sampler, int(steps), hires_steps, t_enc, float(guidance), upscaler, schedule, float(eta), tuple(x_T.shape))
        inputs = dict(ctx2=_copied(ctx2), x_T=_copied(x_T, torch.float32), hires_noise=_noise(hires_noise, lat_hi, hires_seed, 2, image_index))
        if sampler == 'euler_a':
            inputs['step_noise'] = _step_noise(step_noise, (int(steps) - 1,) + tuple(x_T.shape), seed, 0, image_index)
            inputs['hires_step_noise'] = _step_noise(hires_step_noise, (t_enc - 1,) + lat_hi, hires_seed, hires_steps - t_enc, image_index)
        return self._replay(key, lambda **s: self.generate_hires(**s, **kw), inputs)

    def generate_pipelined(self, ctx2, x_T, steps=20, guidance=7.5, sampler='plms'):
        """generate_graphed() as TWO device graphs -- sampling (context upload, every UNet evaluation, CFG, sampler updates) on
        the current stream and decoding (VAE + uint8) on a side stream -- so that the decode of image i runs while image i+1 is
        being sampled.  EXPERIMENT, not the default: the guided UNet chain is latency-bound (batch 1 takes 82 % of the time of
        batch 2, tools/two_chain_probe.py), but on MI355X the decode's big grids take more from that chain than the overlap
        gives back (bench.py --overlap-decode: 8.97 vs 9.29 images/s serial, same box).  Returns (uint8 images, event): the
        images are valid once the event has completed and until the decode of the NEXT call starts.  'plms' and 'dpm' only: its
        sampling graph has no noise input."""
        self._require_pairs('generate_pipelined')
        if sampler not in ('plms', 'dpm'):
            raise ValueError(f"generate_pipelined samples with 'plms' or 'dpm', got {sampler!r}")
        if self.cfg_split:
            out = self.generate(ctx2, x_T, steps, guidance, sampler)
            ev = torch.cuda.Event(); ev.record()
            return out, ev
        key = ('pipelined', sampler, int(steps), float(guidance), tuple(x_T.shape))
        mode = 1 if sampler == 'plms' else 0
        g_s, (s_ctx, s_x), z_s = self._graphed(key + ('sample',), [(ctx2.shape, ctx2.dtype), (x_T.shape, torch.float32)],
                                               lambda c, x: self._sample(sampler, c, x, steps, guidance))
        g_d, (z_in,), out = self._graphed(key + ('decode',), [(z_s.shape, z_s.dtype)], lambda z: self.decode(z, mode=mode))
        if key not in self._traj:
            self._traj[key] = dict(side=torch.cuda.Stream(device=self.device), copied=None, decoded=None)
        c = self._traj[key]
        main = torch.cuda.current_stream(self.device)
        if c['copied'] is not None:
            main.wait_event(c['copied'])        # the previous latent has left z_s
        s_ctx.copy_(ctx2); s_x.copy_(x_T)
        g_s.replay()
        sampled = torch.cuda.Event(); sampled.record(main)
        with torch.cuda.stream(c['side']):
            c['side'].wait_event(sampled)
            z_in.copy_(z_s)
            c['copied'] = torch.cuda.Event(); c['copied'].record(c['side'])
            g_d.replay()
            c['decoded'] = torch.cuda.Event(); c['decoded'].record(c['side'])
        return out, c['decoded']


# the descriptions of a graph's static inputs (Txt2Img._replay): (shape, dtype, value, draw) -- `value` the caller's tensor to copy, or
# None for noise to be drawn as draw = (seed, family, image_index) says (Txt2Img._fill)
def _copied(value, dtype=None):
    """a tensor the caller always passes; the static takes its shape and `dtype` (default: its own)"""
    return (tuple(value.shape), value.dtype if dtype is None else dtype, value, None)


def _noise(value, shape, seed, family, image_index):
    """one fp32 noise tensor [n, 4, H, W]: the caller's, or None = Philox family `family` of `seed`"""
    return (tuple(shape), torch.float32, value, (seed, family, image_index))


def _step_noise(value, shape, seed, first, image_index):
    """fp32 step-noise rows [rows, n, 4, H, W], row r = the noise of step first + r: the caller's, or None = family 3 + first + r"""
    return _noise(value, shape, seed, 3 + first, image_index)


def _noise_pair(noise, lat, seed, image_index):
    """encode()'s noise=(n1, n2) as the two statics n1, n2 (families 1 and 2); `run` puts the pair together again"""
    n1, n2 = (None, None) if noise is None else noise
    return dict(n1=_noise(n1, lat, seed, 1, image_index), n2=_noise(n2, lat, seed, 2, image_index))


def _want_tensor(name, t, shape, dtype=None, note=''):
    """ValueError unless t is a tensor of exactly `shape` (and of `dtype`, when one is given); the message names both"""
    if not isinstance(t, torch.Tensor) or (dtype is not None and t.dtype != dtype) or tuple(t.shape) != tuple(shape):
        kind = 'a tensor' if dtype is None else f'a {str(dtype).replace("torch.", "")} tensor'
        raise ValueError(f'{name} must be {kind} {tuple(shape)}{note}, got {tuple(getattr(t, "shape", ()))} {getattr(t, "dtype", type(t))}')


def _want_steps(name, steps):
    """ValueError unless steps is a positive integer (an integral float passes, a bool does not)"""
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f'{name} must be a positive integer, got {steps!r}')


def img2img_schedule(strength, steps):
    """(PlmsSchedule(steps), t_enc) of ldm img2img: t_enc = int(strength * steps), noise added at ddim index t_enc, the first
    denoising step at timesteps[t_enc - 1].  ldm fails at t_enc == steps (index out of range) and does nothing at 0, so the
    domain is 1 <= t_enc <= steps - 1; anything else raises ValueError before any device work."""
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f'strength must be in [0, 1], got {strength}')
    steps = int(steps)
    t_enc = int(strength * steps)
    if not 1 <= t_enc <= steps - 1:
        raise ValueError(f'int(strength * steps) = {t_enc} is outside [1, steps - 1] = [1, {steps - 1}]')
    return PlmsSchedule(steps), t_enc


def check_prompt_chunks(prompt_chunks):
    """Txt2Img's prompt_chunks: an integer in [1, 4] (77 to 308 keys in the UNet's cross-attention); returns it, raises ValueError"""
    if isinstance(prompt_chunks, bool) or not isinstance(prompt_chunks, (int, np.integer)) or not 1 <= prompt_chunks <= 4:
        raise ValueError(f'prompt_chunks must be an integer in [1, 4], got {prompt_chunks!r}')
    return int(prompt_chunks)


def check_latent_hw(latent_hw, name='latent_hw'):
    """Txt2Img's latent_hw / hires_hw: an integer (square) or (h, w), each a multiple of 8 and at least 8 -- 64 px of image: the UNet's
    three stride-2 levels and the nearest-2x upsampling back must land on the skip tensors' sizes.  Returns (h, w); raises ValueError."""
    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    hw = (latent_hw, latent_hw) if is_int(latent_hw) else latent_hw
    if not isinstance(hw, (tuple, list)) or len(hw) != 2 or not all(is_int(v) for v in hw):
        raise ValueError(f'{name} must be an integer or (h, w), got {latent_hw!r}')
    if any(v < 8 or v % 8 for v in hw):
        raise ValueError(f'{name}: height and width must be multiples of 8, at least 8 (64 px of image), got {latent_hw!r}')
    return int(hw[0]), int(hw[1])


def adapter_check_build(adapter, adapter_channels, cfg_split, hires_hw, inpaint_unet, model):
    """Txt2Img's adapter=True: adapter_channels 1 or 3, and none of cfg_split, hires_hw, inpaint_unet, model='sd21'.  Raises ValueError."""
    if not adapter:
        return
    if isinstance(adapter_channels, bool) or not isinstance(adapter_channels, (int, np.integer)) or adapter_channels not in (1, 3):
        raise ValueError(f'adapter_channels must be 1 or 3, got {adapter_channels!r}')
    for name, on in (('cfg_split', cfg_split), ('hires_hw', hires_hw is not None), ('inpaint_unet', inpaint_unet), ("model='sd21'", model == 'sd21')):
        if on:
            raise ValueError(f'adapter=True cannot be combined with {name}')


def control_check_build(controlnet, cfg_split, hires_hw, inpaint_unet, adapter, tiling, model):
    """Txt2Img's controlnet=True: none of cfg_split, hires_hw, inpaint_unet, adapter, tiling, model='sd21' (each would need the
    residual slots or the control graph in a second place, or a checkpoint family that does not exist for it).  Raises ValueError;
    needs no device."""
    if not controlnet:
        return
    for name, on in (('cfg_split', cfg_split), ('hires_hw', hires_hw is not None), ('inpaint_unet', inpaint_unet), ('adapter', adapter),
                     ('tiling', tiling not in (False, None, 0)), ("model='sd21'", model == 'sd21')):
        if on:
            raise ValueError(f'controlnet=True cannot be combined with {name}')


def control_check_args(hint_u8, weight, latent, n_images):
    """the argument contract of Txt2Img.set_control_hint, checked on the host before any device work.  Returns (hint uint8
    [n, 8h, 8w, 3] contiguous, the 13 scales as floats); raises ValueError."""
    _, h, w = latent
    if not torch.is_tensor(hint_u8) or hint_u8.dtype != torch.uint8:
        raise ValueError('hint_u8 must be a uint8 tensor')
    if hint_u8.dim() == 3:
        hint_u8 = hint_u8[..., None].expand(-1, -1, -1, 3)
    if tuple(hint_u8.shape) != (n_images, 8 * h, 8 * w, 3):
        raise ValueError(f'hint_u8 must be [{n_images}, {8 * h}, {8 * w}, 3] (or without the channel axis), got {tuple(hint_u8.shape)}')
    if isinstance(weight, (bool, str)):
        raise ValueError(f'weight must be a finite number or 13 of them, got {weight!r}')
    try:
        scales = [float(weight)] * 13 if np.isscalar(weight) else [float(v) for v in weight]
    except (TypeError, ValueError):
        raise ValueError(f'weight must be a finite number or 13 of them, got {weight!r}') from None
    if len(scales) != 13 or not all(np.isfinite(v) for v in scales):
        raise ValueError(f'weight must be a finite number or 13 of them (one per residual), got {weight!r}')
    return hint_u8.contiguous(), scales


def upscaler_check_build(upscaler, tiling, latent_hw, state_dicts, models_dir):
    """Txt2Img's upscaler=True: not with tiling; the image (8 x the latent, the hires one with hires_hw) at most 1024 px a side; the
    parameters in state_dicts['upscaler'] or models_dir/upscaler.sdodw.  Returns the keyword arguments of sdod.amd.upscale.Upscaler, or
    None when off; raises ValueError."""
    if not upscaler:
        return None
    if E.tiling_wrap(tiling):
        raise ValueError("upscaler=True cannot be combined with tiling: the upscaler's border is not circular")
    h, w = check_latent_hw(latent_hw)
    if state_dicts is not None:
        if 'upscaler' not in state_dicts:
            raise ValueError("upscaler=True needs state_dicts['upscaler']")
        src = dict(state_dict=state_dicts['upscaler'])
    elif models_dir is not None:
        src = dict(path=os.path.join(models_dir, 'upscaler.sdodw'))
        if not os.path.exists(src['path']):
            raise ValueError(f"upscaler=True needs {src['path']} (python -m sdod.amd.convert --upscaler FILE --out DIR)")
    else:
        raise ValueError('upscaler=True needs state_dicts or models_dir')
    UP.upscaler_check_build(src.get('state_dict'), src.get('path'), (8 * h, 8 * w), None)
    return dict(src, image_hw=(8 * h, 8 * w))


def upscale_check_args(pipe, img_u8):
    """Txt2Img.upscale / generate_upscaled*: a pipeline built with upscaler=True and (when given) a uint8 image [n, H, W, 3] of the size
    the upscaler was built for; raises ValueError"""
    if pipe.upscaler is None:
        raise ValueError('this pipeline was built without upscaler=True')
    if img_u8 is not None:
        UP.upscale_check_args(img_u8, pipe.upscaler.image_hw)


def tiling_check_build(tiling, with_vae_encoder, inpaint_unet, hires_hw, adapter):
    """Txt2Img's tiling: False, True / 'xy', 'x' or 'y', and for anything but False none of with_vae_encoder, inpaint_unet, hires_hw,
    adapter.  Returns the engine's wrap bits (0 = off, bit 0 = x, bit 1 = y); raises ValueError."""
    wrap = E.tiling_wrap(tiling)
    if not wrap:
        return 0
    for name, on, why in (('with_vae_encoder', with_vae_encoder, 'the VAE encoder graph is not wrapped (no img2img under tiling)'),
                          ('inpaint_unet', inpaint_unet, 'the encoder graphs and the 9-channel input convolution are not wrapped'),
                          ('hires_hw', hires_hw is not None, 'the latent resize of the hires pass clamps at the border'),
                          ('adapter', adapter, 'the adapter graph is not wrapped')):
        if on:
            raise ValueError(f'tiling cannot be combined with {name}: {why}')
    return wrap


def adapter_check_args(hint_u8, weight, latent, n_images, channels):
    """the argument contract of Txt2Img.set_adapter_hint, checked on the host before any device work: hint_u8 a uint8 tensor
    [n_images, 8H, 8W, channels] with (4, H, W) = latent -- [n_images, 8H, 8W] is accepted when channels == 1 -- and weight a finite
    number.  Returns the hint as [n_images, 8H, 8W, channels]; raises ValueError."""
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not np.isfinite(float(weight)):
        raise ValueError(f'weight must be a finite number, got {weight!r}')
    if not isinstance(hint_u8, torch.Tensor) or hint_u8.dtype != torch.uint8:
        raise ValueError(f'hint_u8 must be a uint8 tensor, got {getattr(hint_u8, "dtype", type(hint_u8))}')
    want = (n_images, 8 * latent[1], 8 * latent[2], channels)
    if channels == 1 and tuple(hint_u8.shape) == want[:3]:
        hint_u8 = hint_u8[..., None]
    if tuple(hint_u8.shape) != want:
        raise ValueError(f'hint_u8 must be {want}' + (f' or {want[:3]}' if channels == 1 else '') + f', got {tuple(hint_u8.shape)}')
    return hint_u8


HIRES_UPSCALERS = ('nearest-exact', 'bilinear', 'bicubic')


def hires_check_args(pipe, n_images, sampler, hires_steps, denoise, upscaler, schedule, eta, hires_noise, hires_step_noise):
    """the argument contract of the second pass (Txt2Img.hires_from_latent, generate_hires, generate_hires_graphed), checked on the host
    before any device work: a pipeline built with hires_hw; sampler 'plms' / 'dpm' (not with model='sd21') or one of K_SAMPLERS;
    upscaler one of HIRES_UPSCALERS; denoise and hires_steps in img2img_schedule's domain; hires_noise None or an fp32 tensor
    [n_images, 4, H2, W2]; hires_step_noise None or -- euler_a only -- an fp32 tensor [t_enc - 1, n_images, 4, H2, W2].  Returns t_enc;
    raises ValueError."""
    if pipe.hires is None:
        raise ValueError('this pipeline was built without hires_hw: Txt2Img(..., hires_hw=(H2, W2)) is needed for the hires pass')
    if upscaler not in HIRES_UPSCALERS:
        raise ValueError(f'upscaler must be one of {HIRES_UPSCALERS}, got {upscaler!r}')
    if sampler not in ('plms', 'dpm') + K_SAMPLERS:
        raise ValueError(f"sampler must be one of {('plms', 'dpm') + K_SAMPLERS}, got {sampler!r}")
    _want_steps('hires_steps', hires_steps)
    _, t_enc = img2img_schedule(denoise, hires_steps)
    latent = pipe.hires._latent_shape
    if sampler in K_SAMPLERS:
        k_check_args(sampler, hires_steps, schedule, eta, hires_step_noise, latent, n_images, first=int(hires_steps) - t_enc)
    else:
        if pipe.model == 'sd21':
            raise ValueError(f"sampler {sampler!r}'s second pass is ldm's DDIM img2img loop, which has no v-conversion: use a k-sampler with model='sd21'")
        if hires_step_noise is not None:
            raise ValueError(f"hires_step_noise is euler_a's fresh noise; the DDIM second pass of sampler {sampler!r} draws none")
    if hires_noise is not None:
        _want_tensor('hires_noise', hires_noise, (n_images,) + tuple(latent), torch.float32)
    return t_enc


def k_check_args(sampler, steps, schedule, eta, step_noise, latent, n_images, first=0, old_samplers=False):
    """the argument contract of the k-diffusion samplers (Txt2Img.sample_k, generate, generate_graphed), checked on the host before any
    device work: sampler one of K_SAMPLERS (old_samplers=True: or 'plms' / 'dpm', which take schedule 'discrete' and no step_noise);
    steps a positive integer; 0 <= first < steps; schedule 'discrete' or 'karras'; eta >= 0; step_noise None or -- euler_a only -- an
    fp32 tensor [steps - first - 1, n_images, *latent].  Raises ValueError."""
    old = ('plms', 'dpm') if old_samplers else ()
    if sampler not in K_SAMPLERS + old:
        raise ValueError(f'sampler must be one of {old + K_SAMPLERS}, got {sampler!r}')
    _want_steps('steps', steps)
    if int(first) != first or not 0 <= first < steps:
        raise ValueError(f'first must be an integer in [0, steps - 1] = [0, {int(steps) - 1}], got {first!r}')
    if schedule not in K_SCHEDULES:
        raise ValueError(f'schedule must be one of {K_SCHEDULES}, got {schedule!r}')
    if not float(eta) >= 0.0 or float(eta) == float('inf'):
        raise ValueError(f'eta must be a finite number >= 0, got {eta!r}')
    if sampler in old:
        if schedule != 'discrete' or step_noise is not None:
            raise ValueError(f"sampler {sampler!r} runs on its own time grid without per-step noise: schedule must be 'discrete' and "
                             f'step_noise None')
        return
    if step_noise is not None:
        if sampler != 'euler_a':
            raise ValueError(f"step_noise is euler_a's fresh noise; sampler {sampler!r} draws none")
        _want_tensor('step_noise', step_noise, (int(steps) - int(first) - 1, n_images) + tuple(latent), torch.float32,
                     ' (one row per step but the last)')


def lcm_check_build(unguided, guidance_embed, lora_time_modules, loras, cfg_split, inpaint_unet, hires_hw, adapter, controlnet, regions,
                    ip_adapter, canvas_hw):
    """Txt2Img's unguided / guidance_embed / lora_time_modules: each True or False; unguided with none of cfg_split, inpaint_unet,
    hires_hw, adapter, controlnet, regions, ip_adapter, canvas_hw (each of them is built on the guidance pair); guidance_embed needs
    unguided, lora_time_modules needs loras.  Raises ValueError."""
    for name, v in (('unguided', unguided), ('guidance_embed', guidance_embed), ('lora_time_modules', lora_time_modules)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f'{name} must be True or False, got {v!r}')
    if unguided:
        for name, on in (('cfg_split', cfg_split), ('inpaint_unet', inpaint_unet), ('hires_hw', hires_hw is not None), ('adapter', adapter),
                         ('controlnet', controlnet), ('regions', regions), ('ip_adapter', ip_adapter), ('canvas_hw', canvas_hw is not None)):
            if on:
                raise ValueError(f'unguided cannot be combined with {name}: it is built on the (uncond, cond) pair of rows')
    if guidance_embed and not unguided:
        raise ValueError('guidance_embed needs unguided=True: a checkpoint with a guidance-scale embedding evaluates one row per image')
    if lora_time_modules and not loras:
        raise ValueError('lora_time_modules needs loras=True')


def lcm_check_args(pipe, x, steps, guidance, original_steps, strength, step_noise, shape=None):
    """the argument contract of the LCM entry points (Txt2Img.sample_lcm, generate_lcm, generate_lcm_graphed, img2img_lcm), checked on
    the host before any device work: steps and original_steps positive integers, strength in (0, 1] and steps no more than the
    int(original_steps * strength) levels they leave (LcmSchedule); x a tensor [n, *latent] with n the pipeline's images_per_gpu
    (shape: that shape where there is no x yet, img2img_lcm); step_noise None or an fp32 tensor [steps - 1, n, *latent]; guidance a
    finite number or None on a pipeline with the guidance pair (None = 1), a finite number on an unguided pipeline with
    guidance_embed, None on one without.  Returns (CFG scale or None, w or None); raises ValueError."""
    _want_steps('steps', steps)
    _want_steps('original_steps', original_steps)
    if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) or not 0.0 < float(strength) <= 1.0:
        raise ValueError(f'strength must be in (0, 1], got {strength!r}')
    LcmSchedule(int(steps), int(original_steps), float(strength))
    want = (pipe.n,) + tuple(pipe._latent_shape)
    if shape is None:
        _want_tensor('x', x, want)
    elif tuple(shape) != want:
        raise ValueError(f'this pipeline samples {want[0]} image(s) of latent {want[1:]} at a time, got {tuple(shape)}')
    if step_noise is not None:
        _want_tensor('step_noise', step_noise, (int(steps) - 1,) + want, torch.float32, ' (one row per step but the last)')
    number = guidance is not None and not isinstance(guidance, bool) and isinstance(guidance, (int, float, np.integer, np.floating)) \
        and bool(np.isfinite(float(guidance)))
    if guidance is not None and not number:
        raise ValueError(f'guidance must be a finite number, got {guidance!r}')
    if not pipe.unguided:
        return (float(guidance) if number else 1.0), None
    if pipe.guidance_embed:
        if not number:
            raise ValueError('this pipeline was built with guidance_embed=True: guidance is the scale w its checkpoint conditions on, a finite number')
        return None, float(guidance)
    if guidance is not None:
        raise ValueError('this pipeline was built with unguided=True and without guidance_embed: nothing takes a guidance scale, guidance must be None')
    return None, None


def img2img_k_check_args(strength, steps, sampler, schedule, eta, step_noise, latent, n_images):
    """the argument contract of Txt2Img.img2img / img2img_graphed: strength and steps in img2img_schedule's domain; sampler None (ldm's
    DDIM: schedule 'discrete', no step_noise) or one of K_SAMPLERS with k_check_args' contract at first = steps - t_enc.  Returns t_enc;
    raises ValueError."""
    _, t_enc = img2img_schedule(strength, steps)
    if sampler is None:
        if schedule != 'discrete' or step_noise is not None:
            raise ValueError("sampler None is ldm's DDIM (eta = 0): schedule must be 'discrete' and step_noise None")
        return t_enc
    k_check_args(sampler, steps, schedule, eta, step_noise, latent, n_images, first=int(steps) - t_enc)
    return t_enc


def inpaint_levels(sch, t_enc):
    """the steps of sample_ddim_inpaint: [(index, j, sa, s1a)] for ddim index t_enc - 1 .. 0, with j = index - 1 the ddim index of the
    level the step reaches and (sa, s1a) = (sqrt_alphas[j], sqrt_one_minus_alphas[j]) the q_sample coefficients of the known region
    there (ldm q_sample at timesteps[j]); the last step (index 0) reaches the clean level: j, sa, s1a are None, no noise is drawn"""
    out = []
    for index in range(t_enc - 1, -1, -1):
        j = index - 1
        out.append((index, j, float(sch.sqrt_alphas[j]), float(sch.sqrt_one_minus_alphas[j])) if index >= 1 else (0, None, None, None))
    return out


def inpaint_check_images(init_u8, mask_u8, latent, n_images):
    """the image half of inpainting's argument contract: init_u8 uint8 [n, 8H, 8W, 3] with n = n_images and (4, H, W) = latent, the
    pipeline's batch and latent shape; mask_u8 uint8 [n, 8H, 8W].  Returns n; raises ValueError."""
    for t, name in ((init_u8, 'init_u8'), (mask_u8, 'mask_u8')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f'{name} must be a uint8 tensor, got {getattr(t, "dtype", type(t))}')
    if init_u8.dim() != 4 or init_u8.shape[-1] != 3:
        raise ValueError(f'init_u8 must be [n, 8H, 8W, 3], got {tuple(init_u8.shape)}')
    n, h, w = (int(v) for v in init_u8.shape[:3])
    if n < 1 or h % 8 or w % 8 or h == 0 or w == 0:
        raise ValueError(f'init_u8 height and width must be positive multiples of 8, got {tuple(init_u8.shape)}')
    if tuple(mask_u8.shape) != (n, h, w):
        raise ValueError(f'mask_u8 must be {(n, h, w)} (the image without its channel axis), got {tuple(mask_u8.shape)}')
    if n != n_images:
        raise ValueError(f'the pipeline was built for {n_images} image(s) per call, got {n}')
    if (h // 8, w // 8) != tuple(latent[1:]):
        raise ValueError(f'the pipeline was built for {8 * latent[1]} x {8 * latent[2]} images, got {h} x {w}')
    return n


def inpaint_check_args(init_u8, mask_u8, strength, steps, step_noise, latent, n_images):
    """the argument contract of Txt2Img.inpaint, checked on the host before any device work: init_u8 uint8 [n, 8H, 8W, 3] with n =
    n_images and (4, H, W) = latent, the pipeline's batch and latent shape; mask_u8 uint8 [n, 8H, 8W]; strength in img2img_schedule's
    domain; step_noise None or [t_enc - 1, n, 4, H, W].  Returns (schedule, t_enc); raises ValueError."""
    n = inpaint_check_images(init_u8, mask_u8, latent, n_images)
    sch, t_enc = img2img_schedule(strength, steps)
    if step_noise is not None:
        _want_tensor('step_noise', step_noise, (t_enc - 1, n) + tuple(latent), note=f' (t_enc - 1 = {t_enc - 1} noise levels)')
    return sch, t_enc


def inpaint_concat_check_args(init_u8, mask_u8, x_T, steps, sampler, noise, latent, n_images):
    """the argument contract of Txt2Img.inpaint_concat, checked on the host before any device work: image and mask as
    inpaint_check_images; x_T a floating-point tensor [n, 4, H, W]; steps >= 1; sampler 'plms' or 'dpm'; noise None or a tensor
    [n, 4, H, W].  Raises ValueError."""
    n = inpaint_check_images(init_u8, mask_u8, latent, n_images)
    want = (n,) + tuple(latent)
    if not isinstance(x_T, torch.Tensor) or not x_T.is_floating_point() or tuple(x_T.shape) != want:
        raise ValueError(f'x_T must be a floating-point tensor {want}, got {tuple(getattr(x_T, "shape", ()))} {getattr(x_T, "dtype", type(x_T))}')
    if sampler not in ('plms', 'dpm'):
        raise ValueError(f"sampler must be 'plms' or 'dpm', got {sampler!r}")
    if int(steps) != steps or int(steps) < 1:
        raise ValueError(f'steps must be a positive integer, got {steps!r}')
    if noise is not None:
        _want_tensor('noise', noise, want, note=" (the posterior sample's normal draw)")


def broadcast_conditioning(ctx2, src=0):
    """the one collective of the path: the conditioning ctx2 fp16 [2, 77 * prompt_chunks, D] (236,544 B at one chunk of SD 1.x) from
    rank `src` to every rank over RCCL"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.broadcast(ctx2, src=src)
    return ctx2


def shard_images(total, rank, world):
    """block distribution of image indices over ranks"""
    per = (total + world - 1) // world
    lo = min(total, rank * per)
    return list(range(lo, min(total, lo + per)))


def initial_latent(seed, image_index, shape=(4, 64, 64)):
    """x_T for image `image_index`: CPU generator seeded with (seed, index) so any sharding yields the same images"""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(image_index))
    return torch.randn((1,) + tuple(shape), generator=g)


def device_latent(seed, image_index, shape=(4, 64, 64), device='cuda:0'):
    """x_T drawn ON the device for throughput runs (SURVEY 7.2 "RNG"; the reference draws on the host, context.cpp:333-334):
    in-tree Philox4x32-10 + Box-Muller, stream = image index, so the latent depends on (seed, image index) only -- any
    sharding of the images over ranks, and any batch slot, yields the same image.  Parity runs inject x_T instead."""
    return ops.randn((1,) + tuple(shape), seed, image_index, torch.device(device))
