"""ctypes wrapper of the graph-level C ABI (include/sdod_engine.h): the MI355X stand-in for the reference's
QnnGraph objects (context.cpp:105 loads unet / text_encoder / vae_decoder / temb; :201-221 wires their I/O)."""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check

UNET, VAE_DECODER, TEXT_ENCODER, TEMB, VAE_ENCODER, VAE_ENCODER_MASKED, ADAPTER, UPSCALER, CONTROLNET, CONTROL_HINT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
IMAGE_ENCODER, IMAGE_PROJ = 10, 11


class ModelConfig(ctypes.Structure):
    """mirror of `struct sdod_model_config`"""
    _fields_ = [(n, ctypes.c_int) for n in (
        'latent_channels', 'latent_h', 'latent_w', 'model_channels', 'context_dim', 'context_len', 'num_heads',
        'head_dim', 'vocab_size', 'text_layers', 'text_heads', 'vae_channels', 'linear_proj', 'text_arch', 'weight_quant',
        'concat_channels')]
    # T2I-Adapter (`struct sdod_adapter_config`, which travels NEXT to the model config: the struct above keeps its size): plain
    # attributes of the instance, 0 = no adapter.  Every copy made from a ModelConfig carries them: from_buffer_copy() and copy_config().
    adapter_reps = 0
    adapter_hint_channels = 0
    adapter_res_blocks = 0
    # Seamless tiling (the `wrap` argument of sdod_graph_create_wrap, which also travels next to the struct): bit 0 = the x axis wraps,
    # bit 1 = the y axis wraps; read by UNet and VaeDecoder only, 0 = the plain graphs through the old creation entry points.
    tiling = 0
    # ControlNet (`struct sdod_control_config`, next to the struct like the others): control_inputs = 1 gives a UNet the 13 residual
    # inputs and control_scale, control_temb = 1 makes a Temb the time conditioning of a ControlNet graph; 0 = the plain graphs.
    control_inputs = 0
    control_temb = 0
    # Regional prompts (`struct sdod_region_config`, next to the struct like the others): prompts per image of a UNet, whose context_len
    # is then 77 * regions and which gets the four UNet.region_w inputs; 0 = the plain graph through the old creation entry points.
    regions = 0
    # Image prompts (`struct sdod_ip_config`, next to the struct like the others): image tokens per image of a UNet, which then has the
    # to_k_ip / to_v_ip parameters and the UNet.ip_ctx / UNet.ip_w inputs; 0 = the plain graph through the old creation entry points.
    ip_tokens = 0
    # FreeU (sdod_graph_enable_freeu, a switch on the created graph, not a configuration struct): 1 makes a UNet run the FreeU launches at
    # its decoder sites and gives it the UNet.freeu parameter input; composes with every attribute above; 0 = the graph as it was.
    freeu = 0
    _ADAPTER_FIELDS = ('adapter_reps', 'adapter_hint_channels', 'adapter_res_blocks', 'tiling', 'control_inputs', 'control_temb', 'regions',
                       'ip_tokens', 'freeu')

    @classmethod
    def from_buffer_copy(cls, source, offset=0):
        out = type(ctypes.Structure).from_buffer_copy(cls, source, offset)   # (a method of the ctypes metaclass: no super() reaches it)
        for n in cls._ADAPTER_FIELDS:          # (a raw buffer has none: the class defaults, 0, stay)
            v = int(getattr(source, n, 0))
            if v:
                setattr(out, n, v)
        return out


class AdapterConfig(ctypes.Structure):
    """mirror of `struct sdod_adapter_config`"""
    _fields_ = [(n, ctypes.c_int) for n in ('adapter_reps', 'adapter_hint_channels', 'adapter_res_blocks')]


class ControlConfig(ctypes.Structure):
    """mirror of `struct sdod_control_config`"""
    _fields_ = [(n, ctypes.c_int) for n in ('control_inputs', 'control_temb')]


class RegionConfig(ctypes.Structure):
    """mirror of `struct sdod_region_config`"""
    _fields_ = [('regions', ctypes.c_int)]


class IpConfig(ctypes.Structure):
    """mirror of `struct sdod_ip_config`"""
    _fields_ = [('ip_tokens', ctypes.c_int)]


LCM_COND_PROJ_DIM = 256     # time_cond_proj_dim of the released full LCM checkpoints (LCM_Dreamshaper_v7): what the converter and
#                             Txt2Img(guidance_embed=True) build the TEMB graphs with


class LcmConfig(ctypes.Structure):
    """mirror of `struct sdod_lcm_config`"""
    _fields_ = [('time_cond_proj_dim', ctypes.c_int)]


class VisionConfig(ctypes.Structure):
    """mirror of `struct sdod_vision_config`"""
    _fields_ = [(n, ctypes.c_int) for n in ('image_size', 'patch', 'width', 'layers', 'heads', 'mlp_dim', 'proj_dim', 'quick_gelu')]


def vit_h14_config():
    """OpenCLIP ViT-H/14 as HF CLIPVisionModelWithProjection holds it: the image encoder of ip-adapter_sd15"""
    return VisionConfig(224, 14, 1280, 32, 16, 5120, 1024, 0)


class UpscalerConfig(ctypes.Structure):
    """mirror of `struct sdod_upscaler_config`"""
    _fields_ = [(n, ctypes.c_int) for n in ('num_blocks', 'in_h', 'in_w')]


TILING_WRAP = {False: 0, True: 3, 'xy': 3, 'x': 1, 'y': 2}


def tiling_wrap(tiling):
    """Txt2Img's `tiling` argument -> the engine's wrap bits (bit 0 = x, bit 1 = y); anything else is a ValueError"""
    if isinstance(tiling, (bool, str)) and tiling in TILING_WRAP:
        return TILING_WRAP[tiling]
    raise ValueError(f"tiling must be False, True, 'xy', 'x' or 'y', not {tiling!r}")


def copy_config(cfg):
    """an independent copy of a ModelConfig, its adapter and tiling attributes included"""
    return ModelConfig.from_buffer_copy(cfg)


class LoraEntry(ctypes.Structure):
    """mirror of `sdod_lora_entry`"""
    _fields_ = [('name', ctypes.c_char_p), ('up', ctypes.c_void_p), ('down', ctypes.c_void_p), ('dtype', ctypes.c_int),
                ('rank', ctypes.c_int), ('scale', ctypes.c_float)]


class NetworkEntry(ctypes.Structure):
    """mirror of `sdod_network_entry`"""
    _fields_ = [('name', ctypes.c_char_p), ('kind', ctypes.c_int), ('dtype', ctypes.c_int), ('f', ctypes.c_void_p * 4),
                ('rank', ctypes.c_int), ('a', ctypes.c_int), ('b', ctypes.c_int), ('scale', ctypes.c_float)]


NET_LORA, NET_LOHA, NET_LOKR = 0, 1, 2


ENGINE_SYMBOLS = [
    'sdod_model_config_sd14', 'sdod_model_config_sd21', 'sdod_graph_create', 'sdod_graph_create_ex', 'sdod_graph_create_wrap', 'sdod_graph_destroy', 'sdod_graph_num_params', 'sdod_graph_param_info',
    'sdod_graph_set_param', 'sdod_graph_param_device', 'sdod_graph_load_file', 'sdod_graph_finalize', 'sdod_graph_io', 'sdod_graph_execute', 'sdod_graph_check',
    'sdod_graph_stats', 'sdod_graph_tune_info', 'sdod_graph_num_ops', 'sdod_graph_op_info', 'sdod_graph_op_detail', 'sdod_graph_profile',
    'sdod_graph_keep_base', 'sdod_graph_base_bytes', 'sdod_graph_set_loras', 'sdod_graph_create_upscaler',
    'sdod_graph_create_control', 'sdod_graph_bind_output', 'sdod_graph_create_regions',
    'sdod_graph_create_ip', 'sdod_graph_create_vision',
    'sdod_graph_enable_freeu', 'sdod_graph_freeu_input',
    'sdod_graph_set_networks',
    'sdod_graph_create_lcm',
]


def _engine():
    lib = _lib.hip()
    if not getattr(lib, '_sdod_engine_typed', False):
        P, I = ctypes.c_void_p, ctypes.c_int
        lib.sdod_model_config_sd14.argtypes = [ctypes.POINTER(ModelConfig)]
        lib.sdod_model_config_sd14.restype = None
        lib.sdod_model_config_sd21.argtypes = [ctypes.POINTER(ModelConfig)]
        lib.sdod_model_config_sd21.restype = None
        lib.sdod_graph_create.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), I]
        lib.sdod_graph_create_ex.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), ctypes.POINTER(AdapterConfig), I]
        lib.sdod_graph_create_wrap.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), ctypes.POINTER(AdapterConfig), I, I]
        lib.sdod_graph_create_upscaler.argtypes = [ctypes.POINTER(P), ctypes.POINTER(UpscalerConfig), I]
        lib.sdod_graph_create_control.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), ctypes.POINTER(ControlConfig), I]
        lib.sdod_graph_create_regions.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), ctypes.POINTER(RegionConfig), I]
        lib.sdod_graph_create_ip.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), ctypes.POINTER(IpConfig), I]
        lib.sdod_graph_create_vision.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), ctypes.POINTER(VisionConfig), ctypes.POINTER(IpConfig), I]
        lib.sdod_graph_create_lcm.argtypes = [ctypes.POINTER(P), I, ctypes.POINTER(ModelConfig), ctypes.POINTER(LcmConfig), I]
        lib.sdod_graph_bind_output.argtypes = [P, I, P, ctypes.c_size_t]
        lib.sdod_graph_destroy.argtypes = [P]
        lib.sdod_graph_num_params.argtypes = [P]
        lib.sdod_graph_param_info.argtypes = [P, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(I), ctypes.POINTER(ctypes.c_int64)]
        lib.sdod_graph_set_param.argtypes = [P, ctypes.c_char_p, P, I, ctypes.POINTER(ctypes.c_int64), I]
        lib.sdod_graph_load_file.argtypes = [P, ctypes.c_char_p, ctypes.c_char_p]
        lib.sdod_graph_param_device.argtypes = [P, ctypes.c_char_p, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]
        lib.sdod_graph_finalize.argtypes = [P]
        lib.sdod_graph_io.argtypes = [P, I, I, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)]
        lib.sdod_graph_execute.argtypes = [P, P, I]
        lib.sdod_graph_check.argtypes = [P]
        lib.sdod_graph_stats.argtypes = [P, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(I),
                                         ctypes.POINTER(ctypes.c_double)]
        lib.sdod_graph_tune_info.argtypes = [P, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.c_char_p, I]
        lib.sdod_graph_num_ops.argtypes = [P]
        lib.sdod_graph_op_info.argtypes = [P, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        lib.sdod_graph_profile.argtypes = [P, P, I, P, I]
        lib.sdod_graph_op_detail.argtypes = [P, I, ctypes.POINTER(ctypes.c_char_p)]
        lib.sdod_graph_keep_base.argtypes = [P]
        lib.sdod_graph_base_bytes.argtypes = [P, ctypes.POINTER(ctypes.c_size_t)]
        lib.sdod_graph_set_loras.argtypes = [P, ctypes.POINTER(LoraEntry), I, P]
        lib.sdod_graph_set_networks.argtypes = [P, ctypes.POINTER(NetworkEntry), I, P]
        lib.sdod_graph_enable_freeu.argtypes = [P]
        lib.sdod_graph_freeu_input.argtypes = [P, ctypes.POINTER(I)]
        lib._sdod_engine_typed = True
    return lib


def sd14_config(latent_h=64, latent_w=64, concat_channels=0, adapter_reps=0, adapter_hint_channels=0, adapter_res_blocks=0):
    """concat_channels=5: an inpainting checkpoint (sd-v1-5-inpainting), whose UNet input convolution takes 4 + 5 channels.
    adapter_reps=1 or 2: a UNet built on this config has the four T2I-Adapter feature inputs (UNet.adapter_feat), each shared by that
    many guidance copies of its batch; adapter_hint_channels=1 or 3 (and adapter_res_blocks, 0 = 2): what an Adapter graph needs."""
    cfg = ModelConfig()
    _engine().sdod_model_config_sd14(ctypes.byref(cfg))
    cfg.latent_h, cfg.latent_w, cfg.concat_channels = latent_h, latent_w, concat_channels
    cfg.adapter_reps, cfg.adapter_hint_channels, cfg.adapter_res_blocks = int(adapter_reps), int(adapter_hint_channels), int(adapter_res_blocks)
    return cfg


def sd21_config(latent_h=96, latent_w=96, concat_channels=0):
    """SD v2.1-768 shapes (BASELINE config 5): UNet with 64-wide heads / context 1024, OpenCLIP ViT-H/14 text tower;
    concat_channels=5: an SD 2 inpainting checkpoint (512-inpainting-ema)"""
    cfg = ModelConfig()
    _engine().sdod_model_config_sd21(ctypes.byref(cfg))
    cfg.latent_h, cfg.latent_w, cfg.concat_channels = latent_h, latent_w, concat_channels
    return cfg


class _DevView:
    """exposes raw device memory through __cuda_array_interface__ so torch can alias it without a copy"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}


def device_view(ptr, shape, dtype, device):
    typestr = {torch.float16: '<f2', torch.float32: '<f4', torch.int32: '<i4', torch.uint8: '|u1'}[dtype]
    return torch.as_tensor(_DevView(ptr, shape, typestr), device=device)


class Graph:
    """One compiled graph: parameters in, I/O slots as torch views, execute() on the current stream.
    Without a GPU only the parameter table can be read (what the checkpoint converter needs); everything that touches
    device memory raises."""

    def __init__(self, kind, cfg, batch, device='cuda:0', wrap=None, cond_proj_dim=0):
        """wrap: None = the creation entry points of every build before seamless tiling; an int 0..3 goes through
        sdod_graph_create_wrap (0 builds the plain graph there).  cond_proj_dim: a TEMB graph with an LCM checkpoint's guidance-scale
        embedding goes through sdod_graph_create_lcm; 0 = the entry points as before"""
        self._lib = _engine()
        self._h = ctypes.c_void_p()
        self.kind, self.cfg, self.batch = kind, cfg, batch
        self.device = torch.device(device)
        acfg = AdapterConfig(*(int(getattr(cfg, n, 0)) for n, _ in AdapterConfig._fields_))
        ccfg = ControlConfig(int(getattr(cfg, 'control_inputs', 0)) if kind == UNET else 0, int(getattr(cfg, 'control_temb', 0)) if kind == TEMB else 0)
        control = kind in (CONTROLNET, CONTROL_HINT) or ccfg.control_inputs or ccfg.control_temb
        if control and (wrap or any(getattr(acfg, n) for n, _ in AdapterConfig._fields_)):
            raise ValueError('a ControlNet graph, or a UNet with control inputs, takes neither tiling nor a T2I-Adapter configuration')
        regions = int(getattr(cfg, 'regions', 0)) if kind == UNET else 0
        if regions and (control or wrap or any(getattr(acfg, n) for n, _ in AdapterConfig._fields_)):
            raise ValueError('a UNet with regions takes no control inputs, no tiling and no T2I-Adapter configuration')
        ip_tokens = int(getattr(cfg, 'ip_tokens', 0)) if kind == UNET else 0
        if ip_tokens and (regions or control or wrap or any(getattr(acfg, n) for n, _ in AdapterConfig._fields_)):
            raise ValueError('a UNet with an image prompt takes no regions, no control inputs, no tiling and no T2I-Adapter configuration')
        cond_proj_dim = int(cond_proj_dim)
        if cond_proj_dim and (kind != TEMB or control):
            raise ValueError("cond_proj_dim applies to the UNet's TEMB graph only, not to a ControlNet's time conditioning (control_temb)")
        with self._on_device():
            if cond_proj_dim:       # the guidance embedding has an entry point of its own; without it nothing changes
                check(self._lib.sdod_graph_create_lcm(ctypes.byref(self._h), kind, ctypes.byref(cfg), ctypes.byref(LcmConfig(cond_proj_dim)), batch))
            elif kind in (IMAGE_ENCODER, IMAGE_PROJ):   # the image side of an image prompt: cfg.vision, and cfg.ip_tokens for the projection
                icfg = IpConfig(int(getattr(cfg, 'ip_tokens', 0)))
                check(self._lib.sdod_graph_create_vision(ctypes.byref(self._h), kind, ctypes.byref(cfg), ctypes.byref(cfg.vision), ctypes.byref(icfg), batch))
            elif ip_tokens:         # image prompts have an entry point of their own; without them nothing changes
                icfg = IpConfig(ip_tokens)
                check(self._lib.sdod_graph_create_ip(ctypes.byref(self._h), kind, ctypes.byref(cfg), ctypes.byref(icfg), batch))
            elif regions:           # regional prompts have an entry point of their own; without them nothing changes
                rcfg = RegionConfig(regions)
                check(self._lib.sdod_graph_create_regions(ctypes.byref(self._h), kind, ctypes.byref(cfg), ctypes.byref(rcfg), batch))
            elif control:             # the ControlNet kinds and switches have an entry point of their own; without them nothing changes
                check(self._lib.sdod_graph_create_control(ctypes.byref(self._h), kind, ctypes.byref(cfg), ctypes.byref(ccfg), batch))
            elif kind == UPSCALER:    # its configuration is the UpscalerConfig itself; no ModelConfig field applies
                check(self._lib.sdod_graph_create_upscaler(ctypes.byref(self._h), ctypes.byref(cfg), batch))
            elif wrap is not None:
                check(self._lib.sdod_graph_create_wrap(ctypes.byref(self._h), kind, ctypes.byref(cfg), ctypes.byref(acfg), int(wrap), batch))
            elif kind == ADAPTER or any(getattr(acfg, n) for n, _ in AdapterConfig._fields_):
                check(self._lib.sdod_graph_create_ex(ctypes.byref(self._h), kind, ctypes.byref(cfg), ctypes.byref(acfg), batch))
            else:       # no adapter anywhere: the entry point, and the graph, of every build before it
                check(self._lib.sdod_graph_create(ctypes.byref(self._h), kind, ctypes.byref(cfg), batch))
            if kind == UNET and int(getattr(cfg, 'freeu', 0)):   # a switch on whichever graph was created above
                self.enable_freeu()
        self.finalized = False

    def _on_device(self):
        return torch.cuda.device(self.device) if torch.cuda.is_available() else contextlib.nullcontext()

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self._lib.sdod_graph_destroy(h)
            self._h = None

    def param_table(self):
        out = []
        n = self._lib.sdod_graph_num_params(self._h)
        name = ctypes.c_char_p(); nd = ctypes.c_int(); shape = (ctypes.c_int64 * 4)()
        for i in range(n):
            check(self._lib.sdod_graph_param_info(self._h, i, ctypes.byref(name), ctypes.byref(nd), shape))
            out.append((name.value.decode(), tuple(shape[:nd.value])))
        return out

    def set_param(self, name, tensor):
        if hasattr(tensor, 'payload'):     # weights.QuantU8: the library dequantises with the reference's arithmetic
            buf = tensor.payload()
            shape = (ctypes.c_int64 * max(len(tensor.shape), 1))(*tensor.shape)
            check(self._lib.sdod_graph_set_param(self._h, name.encode(), ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p), 2, shape,
                                                 len(tensor.shape)))
            return
        t = tensor.detach().cpu().contiguous()
        if t.dtype not in (torch.float32, torch.float16):
            t = t.float()
        shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
        check(self._lib.sdod_graph_set_param(self._h, name.encode(), ctypes.c_void_p(t.data_ptr()),
                                             1 if t.dtype == torch.float32 else 0, shape, t.dim()))

    def packed_param(self, name, dtype=torch.float16):
        """a set parameter as it lives in the weight arena (its packed form), as a flat torch view of `dtype`"""
        p = ctypes.c_void_p(); n = ctypes.c_size_t()
        check(self._lib.sdod_graph_param_device(self._h, name.encode(), ctypes.byref(p), ctypes.byref(n)))
        return device_view(p.value, (n.value // torch.empty((), dtype=dtype).element_size(),), dtype, self.device)

    def load_state_dict(self, sd, prefix=''):
        """sd: mapping of (prefix+)ldm/HF names to tensors in canonical layout; every graph parameter must be present."""
        with torch.cuda.device(self.device):
            for name, _ in self.param_table():
                key = prefix + name
                if key not in sd:
                    raise KeyError(f'missing parameter {key}')
                self.set_param(name, sd[key])

    def load_file(self, path, prefix=''):
        with self._on_device():
            check(self._lib.sdod_graph_load_file(self._h, path.encode(), prefix.encode()))

    def finalize(self):
        with torch.cuda.device(self.device):
            check(self._lib.sdod_graph_finalize(self._h))
        self.finalized = True
        return self

    def keep_base(self):
        """before finalize(): keep a second device copy of the weights as set, so that set_loras() can re-weight the graph in place
        (costs base_bytes() of device memory)"""
        check(self._lib.sdod_graph_keep_base(self._h))
        return self

    def enable_freeu(self):
        """before finalize(), UNET graphs only: the graph runs FreeU at its decoder sites and gets the parameter input UNet.freeu"""
        check(self._lib.sdod_graph_enable_freeu(self._h))
        return self

    def freeu_input(self):
        """index of the FreeU parameter input, -1 for a graph without the switch"""
        i = ctypes.c_int()
        check(self._lib.sdod_graph_freeu_input(self._h, ctypes.byref(i)))
        return i.value

    def base_bytes(self):
        n = ctypes.c_size_t()
        check(self._lib.sdod_graph_base_bytes(self._h, ctypes.byref(n)))
        return n.value

    def set_loras(self, entries):
        """entries: [(param_name, up, down, scale)] with torch CPU tensors in canonical layout (up [out, rank] or [out, rank, 1, 1];
        down [rank, in] or [rank, cin, kh, kw]).  The graph then computes with W + sum scale * up @ down for every named weight;
        [] restores the base weights.  Pointers do not move: views, launch list and captured replays stay valid."""
        shapes = None
        keep, arr = [], (LoraEntry * max(len(entries), 1))()
        for i, (name, up, down, scale) in enumerate(entries):
            if not (torch.is_tensor(up) and torch.is_tensor(down)) or up.dim() < 2 or down.dim() < 2:
                raise ValueError(f'{name}: up and down must be tensors of at least two dimensions')
            if shapes is None:
                shapes = dict(self.param_table())
            dt = torch.float16 if up.dtype == torch.float16 and down.dtype == torch.float16 else torch.float32
            up = up.detach().cpu().to(dt).contiguous()
            down = down.detach().cpu().to(dt).contiguous()
            rank = down.shape[0]
            if len(shapes.get(name, ())) >= 2:   # (an unknown name or a vector is the library's to refuse)
                shape = shapes[name]
                fan_in = int(np.prod(shape[1:]))
                if up.numel() != shape[0] * rank or up.shape[0] != shape[0] or down.numel() != rank * fan_in:
                    raise ValueError(f'{name}: factors {tuple(up.shape)} x {tuple(down.shape)} do not give a {tuple(shape)} weight')
            keep += [up, down]
            arr[i] = LoraEntry(name.encode(), up.data_ptr(), down.data_ptr(), 1 if dt == torch.float32 else 0, rank, float(scale))
        with self._on_device():
            check(self._lib.sdod_graph_set_loras(self._h, arr, len(entries),
                                                 ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if torch.cuda.is_available() else None)))

    def set_networks(self, entries):
        """set_loras for every adapter family (sdod/amd/lycoris.py).  An entry is one of
            (param_name, up, down, scale)                          plain LoRA, as set_loras takes it
            ('loha', param_name, w1a, w1b, w2a, w2b, scale)        W + scale * (w1a @ w1b) * (w2a @ w2b);  w*a [out, rank], w*b [rank, in]
                                                                   or [rank, cin, kh, kw]
            ('lokr', param_name, w1, w2, scale)                    W + scale * kron(w1, w2);  w1 [a, b], w2 [out / a, in / b] or
                                                                   [out / a, cin / b, kh, kw]; a = b = 1 adds the full delta w2
        with torch CPU tensors in canonical layout.  Entries naming the same weight accumulate in the order given; [] restores the base
        weights.  ValueError for factors that do not give the weight's shape, before the library is called."""
        shapes = None
        keep, arr = [], (NetworkEntry * max(len(entries), 1))()
        for i, e in enumerate(entries):
            if len(e) == 4:
                kind, name, factors, scale = NET_LORA, e[0], e[1:3], e[3]
            elif len(e) == 7 and e[0] == 'loha':
                kind, name, factors, scale = NET_LOHA, e[1], e[2:6], e[6]
            elif len(e) == 5 and e[0] == 'lokr':
                kind, name, factors, scale = NET_LOKR, e[1], e[2:4], e[4]
            else:
                raise ValueError("an entry is (name, up, down, scale), ('loha', name, w1a, w1b, w2a, w2b, scale) or ('lokr', name, w1, w2, scale)")
            if not all(torch.is_tensor(t) and t.dim() >= 2 for t in factors):
                raise ValueError(f'{name}: the factors must be tensors of at least two dimensions')
            if shapes is None:
                shapes = dict(self.param_table())
            dt = torch.float16 if all(t.dtype == torch.float16 for t in factors) else torch.float32
            factors = [t.detach().cpu().to(dt).contiguous() for t in factors]
            rank = a = b = 0
            shape = shapes.get(name, ())
            known = len(shape) >= 2                      # (an unknown name or a vector is the library's to refuse)
            fan_in = int(np.prod(shape[1:])) if known else 0
            what = ' x '.join(str(tuple(t.shape)) for t in factors)
            if kind == NET_LOKR:
                w1, w2 = factors
                a, b = (int(v) for v in w1.shape[:2])
                if w1.dim() != 2 or a < 1 or b < 1:
                    raise ValueError(f'{name}: w1 must be a non-empty [a, b] matrix, got {tuple(w1.shape)}')
                if known and (shape[0] % a or shape[1] % b or w2.shape[0] * a != shape[0] or w2.numel() * a * b != shape[0] * fan_in):
                    raise ValueError(f'{name}: the Kronecker factors {what} do not give a {tuple(shape)} weight')
            else:
                rank = int(factors[1].shape[0])
                for up, down in zip(factors[0::2], factors[1::2]):
                    if down.shape[0] != rank or (known and (up.numel() != shape[0] * rank or up.shape[0] != shape[0] or down.numel() != rank * fan_in)):
                        raise ValueError(f'{name}: factors {what} do not give a {tuple(shape)} weight')
            keep += factors
            ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in factors])
            arr[i] = NetworkEntry(name.encode(), kind, 1 if dt == torch.float32 else 0, ptrs, rank, a, b, float(scale))
        with self._on_device():
            check(self._lib.sdod_graph_set_networks(self._h, arr, len(entries),
                                                    ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if torch.cuda.is_available() else None)))

    def bind_output(self, index, tensor):
        """before finalize(): output `index` is written straight into `tensor` (device memory of the same size that outlives the
        graph, typically an input slot of another graph) instead of a slot of this graph's own"""
        if not tensor.is_cuda or not tensor.is_contiguous():
            raise ValueError('a bound output must be a contiguous device tensor')
        self._bound = getattr(self, '_bound', []) + [tensor]      # keep it alive as long as the graph
        check(self._lib.sdod_graph_bind_output(self._h, int(index), ctypes.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))

    def _io(self, is_out, idx):
        p = ctypes.c_void_p(); n = ctypes.c_size_t()
        check(self._lib.sdod_graph_io(self._h, 1 if is_out else 0, idx, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def io_tensor(self, is_out, idx, shape, dtype):
        ptr, nbytes = self._io(is_out, idx)
        numel = int(np.prod(shape))
        assert numel * torch.empty((), dtype=dtype).element_size() == nbytes, (shape, dtype, nbytes)
        return device_view(ptr, shape, dtype, self.device)

    def execute(self, use_hip_graph=False, static_unchanged=False):
        """static_unchanged: the static inputs (UNet: text context) are the same as in the previous execute()"""
        flags = (1 if use_hip_graph else 0) | (2 if static_unchanged else 0)
        check(self._lib.sdod_graph_execute(self._h, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), flags))

    def check(self):
        """raises once a launch of this device has failed in a way it could not report itself (a GroupNorm grid barrier that
        timed out): call it after synchronising; execute() makes the same check on entry"""
        check(self._lib.sdod_graph_check(self._h))

    def op_table(self):
        """[(label, flops, bytes)] for every launch of the graph"""
        out = []
        lab = ctypes.c_char_p(); fl = ctypes.c_double(); by = ctypes.c_double()
        for i in range(self._lib.sdod_graph_num_ops(self._h)):
            check(self._lib.sdod_graph_op_info(self._h, i, ctypes.byref(lab), ctypes.byref(fl), ctypes.byref(by)))
            out.append((lab.value.decode(), fl.value, by.value))
        return out

    def op_details(self):
        out = []
        det = ctypes.c_char_p()
        for i in range(self._lib.sdod_graph_num_ops(self._h)):
            check(self._lib.sdod_graph_op_detail(self._h, i, ctypes.byref(det)))
            out.append(det.value.decode())
        return out

    def profile(self, iters=3):
        """per-launch durations in ms (HIP events on the current stream, eager); same order as op_table()"""
        n = self._lib.sdod_graph_num_ops(self._h)
        ms = (ctypes.c_float * n)()
        check(self._lib.sdod_graph_profile(self._h, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), iters, ms, n))
        return list(ms)

    def tune_source(self):
        """where this graph's GEMM tiles came from: table file(s), shapes found there, shapes timed in this process"""
        a = ctypes.c_int(); b = ctypes.c_int(); buf = ctypes.create_string_buffer(1024)
        check(self._lib.sdod_graph_tune_info(self._h, ctypes.byref(a), ctypes.byref(b), buf, 1024))
        import os
        return {'table': ' + '.join(os.path.basename(p) for p in buf.value.decode().split(' + ') if p), 'shapes_from_table': a.value,
                'shapes_tuned_in_process': b.value}

    def stats(self):
        w = ctypes.c_size_t(); a = ctypes.c_size_t(); n = ctypes.c_int(); f = ctypes.c_double()
        check(self._lib.sdod_graph_stats(self._h, ctypes.byref(w), ctypes.byref(a), ctypes.byref(n), ctypes.byref(f)))
        return {'weight_bytes': w.value, 'arena_bytes': a.value, 'launches': n.value, 'flops': f.value}


class UNet(Graph):
    def __init__(self, cfg, batch, device='cuda:0', wrap=None):
        super().__init__(UNET, cfg, batch, device, wrap if wrap is not None else (int(getattr(cfg, 'tiling', 0)) or None))

    def finalize(self):
        super().finalize()
        c, b = self.cfg, self.batch
        self.x = self.io_tensor(False, 0, (b, c.latent_channels, c.latent_h, c.latent_w), torch.float32)
        self.temb_width = self._io(False, 1)[1] // (2 * b)       # projected time conditioning (TEMB graph output width)
        self.temb = self.io_tensor(False, 1, (b, self.temb_width), torch.float16)
        self.ctx = self.io_tensor(False, 2, (b, c.context_len, c.context_dim), torch.float16)
        self.eps = self.io_tensor(True, 0, (b, c.latent_h, c.latent_w, c.latent_channels), torch.float16)
        if c.concat_channels > 0:   # inpainting checkpoint: mask | latent of the masked image, read by the input convolution next to x
            self.cond = self.io_tensor(False, 3, (b, c.concat_channels, c.latent_h, c.latent_w), torch.float32)
        reps = int(getattr(c, 'adapter_reps', 0))
        if reps > 0:                # T2I-Adapter: four feature slots behind the other inputs, zero until something is staged into them
            first = 4 if c.concat_channels > 0 else 3
            self.adapter_feat = [self.io_tensor(False, first + k, shape, torch.float16) for k, shape in enumerate(adapter_feature_shapes(c, b // reps))]
        if int(getattr(c, 'control_inputs', 0)):   # ControlNet: 13 residual slots and their scales, zero until a ControlNet graph fills them
            first = 4 if c.concat_channels > 0 else 3
            self.control_res = [self.io_tensor(False, first + k, shape, torch.float16) for k, shape in enumerate(control_residual_shapes(c, b))]
            self.control_scale = self.io_tensor(False, first + 13, (13,), torch.float32)
        k = int(getattr(c, 'regions', 0))
        if k:                       # regional prompts: the blend weights of the four levels, "region 0 everywhere" until set (ops.region_weights)
            self.region_w = [self.io_tensor(False, 3 + lvl, ((c.latent_h >> lvl) * (c.latent_w >> lvl), k), torch.float32) for lvl in range(4)]
        t = int(getattr(c, 'ip_tokens', 0))
        if t:                       # image prompt: the projected image tokens and the two segments' weights, (1, 0) until set (ops.ip_weights)
            self.ip_ctx = self.io_tensor(False, 3, (b, t, c.context_dim), torch.float16)
            self.ip_w = [self.io_tensor(False, 4 + lvl, ((c.latent_h >> lvl) * (c.latent_w >> lvl), 2), torch.float32) for lvl in range(4)]
        fi = self.freeu_input()
        if fi >= 0:                 # FreeU: (b1, s1, b2, s2, version, 0, 0, 0) behind every other input, the identity until set (freeu.params)
            self.freeu = self.io_tensor(False, fi, (8,), torch.float32)
        return self


def control_residual_shapes(cfg, batch):
    """the 13 ControlNet residuals of `batch` UNet rows, NHWC, in skip order: (H / s, W / s, m MC) for (s, m) = (1, 1) x3, (2, 1),
    (2, 2) x2, (4, 2), (4, 4) x2, (8, 4) x3, and (8, 4) for the middle block's output"""
    mc = cfg.model_channels
    sm = [(1, 1)] * 3 + [(2, 1)] + [(2, 2)] * 2 + [(4, 2)] + [(4, 4)] * 2 + [(8, 4)] * 4
    return [(batch, cfg.latent_h // s, cfg.latent_w // s, m * mc) for s, m in sm]


def control_hint_checkpoint_table(model_channels=320):
    """(name, shape) of input_hint_block.* as a ControlNet CHECKPOINT holds them (the ControlHint graph's own table lists the padded
    shapes): eight 3x3 convolutions 3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 -> model_channels at indices 0, 2, .., 14"""
    widths = [3, 16, 16, 32, 32, 96, 96, 256, model_channels]
    out = []
    for j in range(8):
        out += [(f'input_hint_block.{2 * j}.weight', (widths[j + 1], widths[j], 3, 3)), (f'input_hint_block.{2 * j}.bias', (widths[j + 1],))]
    return out


class ControlNet(Graph):
    """ldm's cldm.ControlNet for SD 1.x (ControlNet 1.0 / 1.1 checkpoints, `control_model.` stripped): x, temb (a control Temb's
    output), ctx and the guided hint (a ControlHint's output, one per image, shared by the two guidance halves of the batch) -> the 13
    residuals of control_residual_shapes.  bind_output(k, unet.control_res[k]) before finalize() makes it write a UNet's slots."""

    def __init__(self, cfg, batch, device='cuda:0'):
        super().__init__(CONTROLNET, cfg, batch, device)

    def finalize(self):
        super().finalize()
        c, b = self.cfg, self.batch
        self.x = self.io_tensor(False, 0, (b, c.latent_channels, c.latent_h, c.latent_w), torch.float32)
        self.temb_width = self._io(False, 1)[1] // (2 * b)
        self.temb = self.io_tensor(False, 1, (b, self.temb_width), torch.float16)
        self.ctx = self.io_tensor(False, 2, (b, c.context_len, c.context_dim), torch.float16)
        self.hint = self.io_tensor(False, 3, (b // 2, c.latent_h, c.latent_w, c.model_channels), torch.float16)
        self.out = [self.io_tensor(True, k, shape, torch.float16) for k, shape in enumerate(control_residual_shapes(c, b))]
        return self


class ControlHint(Graph):
    """cldm's input_hint_block: uint8 hint [B, 8H, 8W, 3] -> the guided hint, fp16 NHWC [B, H, W, MC].  The graph is built with the
    16 / 32 / 96 channel widths zero-padded to 64 / 64 / 128 and its parameter table lists those shapes; set_param pads a checkpoint
    tensor of the original shape with zeros (exact: the padded channels stay zero).  One execute per hint image."""

    def __init__(self, cfg, batch, device='cuda:0'):
        super().__init__(CONTROL_HINT, cfg, batch, device)
        self._shapes = dict(self.param_table())

    def set_param(self, name, tensor):
        want = self._shapes.get(name)
        if want is not None and torch.is_tensor(tensor) and tuple(tensor.shape) != want and tensor.dim() == len(want) \
                and all(a <= b for a, b in zip(tensor.shape, want)):
            padded = torch.zeros(want, dtype=tensor.dtype)
            padded[tuple(slice(0, n) for n in tensor.shape)] = tensor.detach().cpu()
            tensor = padded
        super().set_param(name, tensor)

    def finalize(self):
        super().finalize()
        c, b = self.cfg, self.batch
        self.hint = self.io_tensor(False, 0, (b, 8 * c.latent_h, 8 * c.latent_w, 3), torch.uint8)
        self.out = self.io_tensor(True, 0, (b, c.latent_h, c.latent_w, c.model_channels), torch.float16)
        return self


class ImageEncoder(Graph):
    """HF CLIPVisionModelWithProjection: uint8 [B, S, S, 3], resized and cropped by the caller -> image_embeds fp16
    [B, proj_dim].  Parameters by HF's names; set_param flattens `patch_embedding.weight` [W, 3, p, p] to [W, 3 p p] and pads it with
    zeros to the row length the table lists, and gives `class_embedding` [W] its table shape [1, W].  One execute per image prompt."""

    def __init__(self, vision, batch, device='cuda:0'):
        cfg = sd14_config()
        cfg.vision = self.vision = VisionConfig.from_buffer_copy(vision)
        super().__init__(IMAGE_ENCODER, cfg, batch, device)
        self._shapes = dict(self.param_table())

    def checkpoint_table(self):
        """(name, shape) as a checkpoint holds them"""
        v = self.vision
        fix = {'vision_model.embeddings.patch_embedding.weight': (v.width, 3, v.patch, v.patch), 'vision_model.embeddings.class_embedding': (v.width,)}
        return [(n, fix.get(n, s)) for n, s in self.param_table()]

    def set_param(self, name, tensor):
        want = self._shapes.get(name)
        if want is not None and torch.is_tensor(tensor) and tuple(tensor.shape) != want:
            t = tensor.detach().cpu()
            if name.endswith('patch_embedding.weight') and t.dim() == 4 and t.shape[0] == want[0] and t[0].numel() <= want[1]:
                padded = torch.zeros(want, dtype=t.dtype)
                padded[:, :t[0].numel()] = t.reshape(t.shape[0], -1)
                tensor = padded
            elif name.endswith('class_embedding') and t.numel() == want[1]:
                tensor = t.reshape(want)
        super().set_param(name, tensor)

    def finalize(self):
        super().finalize()
        v, b = self.vision, self.batch
        self.img = self.io_tensor(False, 0, (b, v.image_size, v.image_size, 3), torch.uint8)
        self.out = self.io_tensor(True, 0, (b, v.proj_dim), torch.float16)
        return self


class ImageProj(Graph):
    """IP-Adapter's ImageProjModel: image_embeds fp16 [B, proj_dim] -> fp16 [B, T, ctx_dim] = LayerNorm(Linear(e).reshape(T, ctx_dim)).
    bind_output(0, unet.ip_ctx) before finalize() makes it write a UNet's slot (same batch)."""

    def __init__(self, cfg, proj_dim, ip_tokens, batch, device='cuda:0'):
        c = copy_config(cfg)
        c.ip_tokens = int(ip_tokens)
        c.vision = VisionConfig(0, 0, 0, 0, 0, 0, int(proj_dim), 0)
        self.proj_dim, self.ip_tokens = int(proj_dim), int(ip_tokens)
        super().__init__(IMAGE_PROJ, c, batch, device)

    def finalize(self):
        super().finalize()
        self.embeds = self.io_tensor(False, 0, (self.batch, self.proj_dim), torch.float16)
        self.out = self.io_tensor(True, 0, (self.batch, self.ip_tokens, self.cfg.context_dim), torch.float16)
        return self


def adapter_feature_shapes(cfg, n):
    """the four T2I-Adapter feature maps of n images, NHWC: [n, H / s, W / s, C] for (s, C) = (1, MC), (2, 2 MC), (4, 4 MC), (8, 4 MC)"""
    mc = cfg.model_channels
    return [(n, cfg.latent_h // s, cfg.latent_w // s, m * mc) for s, m in ((1, 1), (2, 2), (4, 4), (8, 4))]


class Adapter(Graph):
    """TencentARC's full T2I-Adapter (SD 1.x canny / depth / sketch / seg / openpose / keypose checkpoints): uint8 hint
    [B, 8H, 8W, cfg.adapter_hint_channels] -> four fp16 NHWC feature maps (adapter_feature_shapes).  One execute per hint image."""

    def __init__(self, cfg, batch, device='cuda:0'):
        super().__init__(ADAPTER, cfg, batch, device)

    def finalize(self):
        super().finalize()
        c, b = self.cfg, self.batch
        self.hint = self.io_tensor(False, 0, (b, 8 * c.latent_h, 8 * c.latent_w, c.adapter_hint_channels), torch.uint8)
        self.out = [self.io_tensor(True, k, shape, torch.float16) for k, shape in enumerate(adapter_feature_shapes(c, b))]
        return self


def upscaler_check_config(num_blocks, image_hw):
    """the UPSCALER graph's own limits, as a ValueError before anything is created"""
    if not isinstance(num_blocks, int) or isinstance(num_blocks, bool) or not 1 <= num_blocks <= 23:
        raise ValueError(f'upscaler: num_blocks must be an integer in [1, 23], not {num_blocks!r}')
    try:
        h, w = (int(v) for v in image_hw)
    except (TypeError, ValueError):
        raise ValueError(f'upscaler: image_hw must be a (height, width) pair, not {image_hw!r}') from None
    for v in (h, w):
        if v < 8 or v > 1024 or v % 8:
            raise ValueError(f'upscaler: image height and width must be multiples of 8 in [8, 1024], not {(h, w)}')
    return h, w


class Upscaler(Graph):
    """ESRGAN's RRDBNet (64 features, growth 32, scale 4; the front ends' "ESRGAN_4x" and "R-ESRGAN 4x+"): uint8 image [B, H, W, 3] ->
    fp16 NHWC [B, 4H, 4W, 3], the network's output, nominally in [0, 1], not clamped.  Parameters by basicsr's names."""

    SCALE = 4

    def __init__(self, num_blocks=23, image_hw=(512, 512), batch=1, device='cuda:0'):
        h, w = upscaler_check_config(num_blocks, image_hw)
        self.num_blocks, self.image_hw = num_blocks, (h, w)
        super().__init__(UPSCALER, UpscalerConfig(num_blocks, h, w), batch, device)

    def finalize(self):
        super().finalize()
        (h, w), b = self.image_hw, self.batch
        self.img = self.io_tensor(False, 0, (b, h, w, 3), torch.uint8)
        self.out = self.io_tensor(True, 0, (b, 4 * h, 4 * w, 3), torch.float16)
        return self


class Temb(Graph):
    def __init__(self, cfg, batch, device='cuda:0', cond_proj_dim=0):
        """cond_proj_dim = D > 0: a full LCM checkpoint's time conditioning -- the graph has the input Temb.w (the guidance scale of each
        row) and the parameter time_embed.cond_proj.weight [model_channels, D]; 0: the graph as ever"""
        super().__init__(TEMB, cfg, batch, device, cond_proj_dim=cond_proj_dim)
        self.cond_proj_dim = int(cond_proj_dim)

    def finalize(self):
        super().finalize()
        self.t = self.io_tensor(False, 0, (self.batch,), torch.float32)
        if self.cond_proj_dim:
            self.w = self.io_tensor(False, 1, (self.batch,), torch.float32)
        self.width = self._io(True, 0)[1] // (2 * self.batch)
        self.out = self.io_tensor(True, 0, (self.batch, self.width), torch.float16)
        return self


class TextEncoder(Graph):
    def __init__(self, cfg, batch, device='cuda:0'):
        super().__init__(TEXT_ENCODER, cfg, batch, device)

    def finalize(self):
        super().finalize()
        c = self.cfg
        self.ids = self.io_tensor(False, 0, (self.batch, c.context_len), torch.int32)
        self.out = self.io_tensor(True, 0, (self.batch, c.context_len, c.context_dim), torch.float16)
        return self


class VaeDecoder(Graph):
    def __init__(self, cfg, batch, device='cuda:0', wrap=None):
        super().__init__(VAE_DECODER, cfg, batch, device, wrap if wrap is not None else (int(getattr(cfg, 'tiling', 0)) or None))

    def finalize(self):
        super().finalize()
        c, b = self.cfg, self.batch
        self.z = self.io_tensor(False, 0, (b, c.latent_channels, c.latent_h, c.latent_w), torch.float32)
        self.img = self.io_tensor(True, 0, (b, 8 * c.latent_h, 8 * c.latent_w, 3), torch.float16)
        return self


class VaeEncoder(Graph):
    """first_stage_model.encoder + quant_conv: uint8 image [B, 8H, 8W, 3] -> fp32 moments [B, 8, H, W] (mean | logvar)"""

    def __init__(self, cfg, batch, device='cuda:0'):
        super().__init__(VAE_ENCODER, cfg, batch, device)

    def finalize(self):
        super().finalize()
        c, b = self.cfg, self.batch
        self.img = self.io_tensor(False, 0, (b, 8 * c.latent_h, 8 * c.latent_w, 3), torch.uint8)
        self.moments = self.io_tensor(True, 0, (b, 2 * c.latent_channels, c.latent_h, c.latent_w), torch.float32)
        return self


class MaskedVaeEncoder(Graph):
    """VaeEncoder on inpainting's masked image: uint8 image [B, 8H, 8W, 3] and uint8 mask [B, 8H, 8W] -> fp32 moments [B, 8, H, W] of
    x = 0 where mask >= 128, 2 u / 255 - 1 elsewhere.  Same parameters (and weight files) as VaeEncoder."""

    def __init__(self, cfg, batch, device='cuda:0'):
        super().__init__(VAE_ENCODER_MASKED, cfg, batch, device)

    def finalize(self):
        super().finalize()
        c, b = self.cfg, self.batch
        self.img = self.io_tensor(False, 0, (b, 8 * c.latent_h, 8 * c.latent_w, 3), torch.uint8)
        self.mask = self.io_tensor(False, 1, (b, 8 * c.latent_h, 8 * c.latent_w), torch.uint8)
        self.moments = self.io_tensor(True, 0, (b, 2 * c.latent_channels, c.latent_h, c.latent_w), torch.float32)
        return self
