"""LyCORIS adapters on the host: reading a file that holds plain LoRA, LoHa, LoKr, Tucker-cored ("CP") and full-diff modules, reducing
each to the form the device merges (Graph.set_networks: a LoRA pair, a LoHa quadruple or a LoKr pair) and the fp64 host merge of all of
them.  Module keys are kohya's (lora.map_key); tensor names are the ones LyCORIS writes and A1111's network_lora / network_hada /
network_lokr / network_full read:

    family   tensors                                                                              delta (times strength * scale)
    lora     lora_up.weight [out, r(,1,1)], lora_down.weight [r, in(,kh,kw)]                      up @ down
             + lora_mid.weight [r, r, kh, kw] (then down is [r, in(,1,1)])                        einsum('nmkl,in,mj->ijkl', mid, up, down)
    loha     hada_w1_a [out, r], hada_w1_b [r, in * taps], hada_w2_a, hada_w2_b                   (w1a @ w1b) * (w2a @ w2b)
             + hada_t1, hada_t2 [r, r, kh, kw] (then w*_a is [r, out], w*_b [r, in])              each side einsum('rskl,ro,si->oikl', t, wa, wb)
    lokr     lokr_w1 [a, b] or lokr_w1_a [a, r] @ lokr_w1_b [r, b];                               kron(w1, w2)
             lokr_w2 [c, d(,kh,kw)] or lokr_w2_a [c, r] @ lokr_w2_b [r, d * taps]
             or lokr_t2 [r, r, kh, kw] with lokr_w2_a [r, c], lokr_w2_b [r, d]                    w2 = einsum('rskl,rc,sd->cdkl', t2, w2a, w2b)
    full     diff [out, in(,kh,kw)]                                                               diff

scale = alpha / r for lora and loha (r = lora_down's / hada_w1_b's first size); for lokr alpha / r when either side is factored (r =
lokr_w1_b's first size, else lokr_w2_b's), else 1; for full 1; a module without `alpha` gets 1.

The reductions -- a Tucker core contracted into the flattened b factor, b'[r][i][t] = sum_s t[r][s][t] w_b[s][i], with a transposed;
a factored LoKr side multiplied out -- are made here in fp64 and rounded to fp16 once: the device sees the plain forms only.  A full
diff is a LoKr entry with w1 = [[1]].

Refused, with the reason in the error (skipped under strict=False): `dora_scale` (DoRA needs column norms of the merged matrix and a
norm-axis convention the files do not record), `diff_b` and the norm-layer tensors `w_norm` / `b_norm` (vectors are not adapter targets),
LoKr factors that do not divide the weight (when the weights' shapes are given), and everything lora.map_key refuses."""
import math

import torch

from . import lora as _lora

_FAMILY_TENSORS = {
    'lora': ('lora_up.weight', 'lora_down.weight', 'lora_mid.weight'),
    'loha': ('hada_w1_a', 'hada_w1_b', 'hada_w2_a', 'hada_w2_b', 'hada_t1', 'hada_t2'),
    'lokr': ('lokr_w1', 'lokr_w1_a', 'lokr_w1_b', 'lokr_w2', 'lokr_w2_a', 'lokr_w2_b', 'lokr_t2'),
    'full': ('diff',),
}
_REFUSED_TENSORS = {
    'dora_scale': 'dora_scale (DoRA) is not supported: it needs column norms of the merged matrix and a norm-axis convention the file does not record',
    'diff_b': 'diff_b (a bias difference) is not supported: vectors are not adapter targets',
    'w_norm': 'w_norm (a norm-layer weight) is not supported: vectors are not adapter targets',
    'b_norm': 'b_norm (a norm-layer bias) is not supported: vectors are not adapter targets',
}


class Module(dict):
    """one adapted module of a file: family ('lora' | 'loha' | 'lokr' | 'full'), tensors {suffix: tensor} as the file holds them,
    alpha (float or None), rank (the size alpha is divided by, or None) and scale (alpha / rank, or 1)"""


class NetworkFile(dict):
    """{module_key: Module}; `refused` maps the modules that hold unsupported tensors to the reason"""
    refused = {}


class NetEntry(tuple):
    """an entry for Graph.set_networks that remembers the file tensors it was reduced from (`raw`: family, tensors, scale), so that
    merged_state_dict can evaluate the unreduced definition"""
    def __new__(cls, items, raw=None):
        obj = super().__new__(cls, items)
        obj.raw = raw
        return obj


def _load(path):
    if isinstance(path, dict):
        return path
    if str(path).endswith('.safetensors'):
        from safetensors.torch import load_file
        return load_file(str(path))
    raw = torch.load(str(path), map_location='cpu')
    if not isinstance(raw, dict):
        raise ValueError(f'{path}: not a dict of tensors')
    return raw


def _need(module, t, *names):
    for n in names:
        if n not in t:
            raise ValueError(f'{module}: {n} is missing')


def _classify(module, t):
    """family, rank of one module's tensors {suffix: tensor}; ValueError for a set that is not one complete family"""
    fams = [f for f, names in _FAMILY_TENSORS.items() if any(n in t for n in names)]
    if len(fams) != 1:
        raise ValueError(f'{module}: tensors of {" and ".join(fams) if fams else "no known"} adapter family')
    fam = fams[0]
    if fam == 'lora':
        _need(module, t, 'lora_up.weight', 'lora_down.weight')
        up, down = t['lora_up.weight'], t['lora_down.weight']
        if down.dim() < 2 or up.dim() < 2 or up.shape[1] != down.shape[0] or up.numel() != up.shape[0] * up.shape[1]:
            raise ValueError(f'{module}: factors {tuple(up.shape)} x {tuple(down.shape)} are not a rank decomposition')
        if 'lora_mid.weight' in t:
            mid = t['lora_mid.weight']
            if mid.dim() != 4 or mid.shape[0] != up.shape[1] or mid.shape[1] != down.shape[0] or down.numel() != down.shape[0] * down.shape[1]:
                raise ValueError(f'{module}: lora_mid.weight {tuple(mid.shape)} does not fit factors {tuple(up.shape)} x {tuple(down.shape)}')
        return fam, int(down.shape[0])
    if fam == 'loha':
        _need(module, t, 'hada_w1_a', 'hada_w1_b', 'hada_w2_a', 'hada_w2_b')
        if ('hada_t1' in t) != ('hada_t2' in t):
            raise ValueError(f'{module}: hada_t1 and hada_t2 must both be present')
        for s in ('1', '2'):
            a, b = t[f'hada_w{s}_a'], t[f'hada_w{s}_b']
            if a.dim() != 2 or b.dim() != 2 or (a.shape[0] if 'hada_t1' in t else a.shape[1]) != b.shape[0]:
                raise ValueError(f'{module}: hada_w{s}_a {tuple(a.shape)} and hada_w{s}_b {tuple(b.shape)} are not a rank decomposition')
            if 'hada_t1' in t and (t[f'hada_t{s}'].dim() != 4 or tuple(t[f'hada_t{s}'].shape[:2]) != (a.shape[0], b.shape[0])):
                raise ValueError(f'{module}: hada_t{s} {tuple(t[f"hada_t{s}"].shape)} does not fit its factors')
        return fam, int(t['hada_w1_b'].shape[0])
    if fam == 'lokr':
        if 'lokr_w1' not in t:
            _need(module, t, 'lokr_w1_a', 'lokr_w1_b')
        if 'lokr_w2' not in t:
            _need(module, t, 'lokr_w2_a', 'lokr_w2_b')
        if 'lokr_w1_b' in t:
            return fam, int(t['lokr_w1_b'].shape[0])
        if 'lokr_w2_b' in t:
            return fam, int(t['lokr_w2_b'].shape[0])
        return fam, None
    if t['diff'].dim() < 2:
        raise ValueError(f'{module}: diff must be a matrix or a convolution weight')
    return fam, None


def read_network(path):
    """A .safetensors file, a torch.save'd dict, or such a dict itself -> NetworkFile {module_key: Module}.  Modules that hold a tensor
    this reader refuses (dora_scale, diff_b, w_norm, b_norm, an unknown name) are in `.refused` with the reason, for entries_for."""
    if isinstance(path, NetworkFile):
        return path
    if isinstance(path, dict) and path and all(isinstance(v, tuple) and len(v) == 3 for v in path.values()):
        out = NetworkFile()                          # what lora.read_lora returns: {module: (down, up, alpha)}
        for module, (down, up, alpha) in path.items():
            out[module] = Module(family='lora', tensors={'lora_up.weight': up, 'lora_down.weight': down}, alpha=float(alpha),
                                 rank=int(down.shape[0]), scale=float(alpha) / down.shape[0])
        out.refused = {m: f'{m}: not a plain LoRA module (LoHa / LoKr / DoRA tensors)' for m in getattr(path, 'other', ())}
        return out
    mods = {}
    for key, t in _load(path).items():
        module, _, rest = key.partition('.')
        mods.setdefault(module, {})[rest] = t
    known = {n for names in _FAMILY_TENSORS.values() for n in names} | {'alpha'}
    out, refused = NetworkFile(), {}
    for module, t in mods.items():
        bad = [n for n in t if n in _REFUSED_TENSORS] or [n for n in t if n not in known]
        if bad:
            refused[module] = f'{module}: ' + _REFUSED_TENSORS.get(bad[0], f'unknown tensor {bad[0]!r}')
            continue
        alpha = float(t['alpha']) if 'alpha' in t else None
        tensors = {n: v for n, v in t.items() if n != 'alpha'}
        family, rank = _classify(module, tensors)
        scale = alpha / rank if alpha is not None and rank else 1.0
        out[module] = Module(family=family, tensors=tensors, alpha=alpha, rank=rank, scale=scale)
    out.refused = refused
    return out


def _d(t):
    return t.detach().double()


def _tucker(core, wa, wb):
    """[out, in, kh, kw] from a core [r, s, kh, kw] and factors wa [r, out], wb [s, in] (A1111's make_weight_cp)"""
    return torch.einsum('rskl,ro,si->oikl', _d(core), _d(wa), _d(wb))


def _lokr_sides(t):
    """the two Kronecker operands of the definition, fp64: w1 [a, b]; w2 [c, d], [c, d * taps] or [c, d, kh, kw]"""
    w1 = _d(t['lokr_w1']) if 'lokr_w1' in t else _d(t['lokr_w1_a']) @ _d(t['lokr_w1_b'])
    if 'lokr_w2' in t:
        w2 = _d(t['lokr_w2'])
    elif 'lokr_t2' in t:
        w2 = torch.einsum('rskl,rc,sd->cdkl', _d(t['lokr_t2']), _d(t['lokr_w2_a']), _d(t['lokr_w2_b']))
    else:
        w2 = _d(t['lokr_w2_a']) @ _d(t['lokr_w2_b'])
    return w1, w2


def delta(family, t):
    """the unreduced definition of one module's weight difference (before scale), fp64, from the file tensors"""
    if family == 'lora':
        up, down = _d(t['lora_up.weight']), _d(t['lora_down.weight'])
        up = up.reshape(up.shape[0], -1)
        if 'lora_mid.weight' in t:
            return torch.einsum('nmkl,in,mj->ijkl', _d(t['lora_mid.weight']), up, down.reshape(down.shape[0], -1))
        return up @ down.reshape(down.shape[0], -1)
    if family == 'loha':
        if 'hada_t1' in t:
            return _tucker(t['hada_t1'], t['hada_w1_a'], t['hada_w1_b']) * _tucker(t['hada_t2'], t['hada_w2_a'], t['hada_w2_b'])
        return (_d(t['hada_w1_a']) @ _d(t['hada_w1_b'])) * (_d(t['hada_w2_a']) @ _d(t['hada_w2_b']))
    if family == 'lokr':
        w1, w2 = _lokr_sides(t)
        if w2.dim() == 4:
            w1 = w1.unsqueeze(2).unsqueeze(2)
        return torch.kron(w1, w2.contiguous())
    if family == 'full':
        return _d(t['diff'])
    raise ValueError(f'unknown adapter family {family!r}')


def reduce_module(mod):
    """the plain form the device merges, without the parameter name and scale: ('lora', up, down), ('loha', w1a, w1b, w2a, w2b) or
    ('lokr', w1, w2).  Tensors the file already holds in that form pass through; what has to be contracted or multiplied out is
    computed in fp64 and rounded to fp16."""
    t = mod['tensors']
    fam = mod['family']
    if fam == 'lora':
        up, down = t['lora_up.weight'], t['lora_down.weight']
        if 'lora_mid.weight' in t:
            down = torch.einsum('nmkl,mj->njkl', _d(t['lora_mid.weight']), _d(down).reshape(down.shape[0], -1)).half()
        return ('lora', up, down)
    if fam == 'loha':
        if 'hada_t1' not in t:
            return ('loha', t['hada_w1_a'], t['hada_w1_b'], t['hada_w2_a'], t['hada_w2_b'])
        out = []
        for s in ('1', '2'):
            out.append(_d(t[f'hada_w{s}_a']).t().contiguous().half())
            out.append(torch.einsum('rskl,si->rikl', _d(t[f'hada_t{s}']), _d(t[f'hada_w{s}_b'])).half())
        return ('loha', *out)
    if fam == 'lokr':
        w1, w2 = _lokr_sides(t)
        return ('lokr', t['lokr_w1'] if 'lokr_w1' in t else w1.half(), t['lokr_w2'] if 'lokr_w2' in t else w2.half())
    return ('lokr', torch.ones(1, 1, dtype=torch.float16), t['diff'])


def entries_for(src, model='sd14', scale_unet=1.0, scale_text=1.0, strict=True, shapes=None, time_modules=False):
    """src: what read_network takes or returns.  Returns ({'unet': [entry], 'text': [entry]}, skipped): the entry lists
    Graph.set_networks takes -- (name, up, down, scale), ('loha', name, w1a, w1b, w2a, w2b, scale), ('lokr', name, w1, w2, scale), each a
    NetEntry that keeps the file tensors for merged_state_dict -- with scale = strength * the module's scale, and the module keys that
    were skipped.  shapes: {'unet': {param_name: shape}, 'text': {...}} of the graphs, when known: a LoKr module whose factors do not
    divide its weight is then refused here.  strict=True raises ValueError listing every unsupported module instead of skipping it.
    time_modules=True: the modules of the time conditioning (lora.map_key: time_emb_proj, time_embedding_linear_1 / _2) come back under
    a third list, 'temb', at the UNet's strength, instead of being refused; shapes may then hold a 'temb' table too."""
    net = read_network(src)
    out, skipped, why = {'unet': [], 'text': []}, [], []
    if time_modules:
        out['temb'] = []
    for module, reason in net.refused.items():
        skipped.append(module)
        why.append(reason)
    for module, mod in net.items():
        try:
            graph, name = _lora.map_key(module, model, time_modules)
            reduced = reduce_module(mod)
            shape = (shapes or {}).get(graph, {}).get(name)
            if reduced[0] == 'lokr' and shape is not None:
                (a, b), w2 = reduced[1].shape, reduced[2]
                fan = math.prod(shape)
                if shape[0] % a or shape[1] % b or w2.shape[0] * a != shape[0] or w2.numel() * a * b != fan:
                    raise ValueError(f'{module}: LoKr factors {tuple(reduced[1].shape)} (x) {tuple(w2.shape)} do not divide the '
                                     f'{tuple(shape)} weight {name}')
        except ValueError as e:
            skipped.append(module)
            why.append(str(e))
            continue
        scale = float(scale_text if graph == 'text' else scale_unet) * float(mod['scale'])
        raw = dict(family=mod['family'], tensors=mod['tensors'], scale=scale)
        items = (name, *reduced[1:], scale) if reduced[0] == 'lora' else (reduced[0], name, *reduced[1:], scale)
        out[graph].append(NetEntry(items, raw))
    if strict and skipped:
        raise ValueError('unsupported adapter modules:\n  ' + '\n  '.join(why))
    return out, skipped


def _plain(entry):
    """(name, family, tensors, scale) of a bare Graph.set_networks entry: the plain definition on the factors it carries"""
    if len(entry) == 4:
        return entry[0], 'lora', {'lora_up.weight': entry[1], 'lora_down.weight': entry[2]}, entry[3]
    if len(entry) == 7 and entry[0] == 'loha':
        a1, b1, a2, b2 = entry[2:6]
        return entry[1], 'loha', {'hada_w1_a': a1.reshape(a1.shape[0], -1), 'hada_w1_b': b1.reshape(b1.shape[0], -1),
                                  'hada_w2_a': a2.reshape(a2.shape[0], -1), 'hada_w2_b': b2.reshape(b2.shape[0], -1)}, entry[6]
    if len(entry) == 5 and entry[0] == 'lokr':
        return entry[1], 'lokr', {'lokr_w1': entry[2], 'lokr_w2': entry[3]}, entry[4]
    raise ValueError("an entry is (name, up, down, scale), ('loha', name, w1a, w1b, w2a, w2b, scale) or ('lokr', name, w1, w2, scale)")


def merged_state_dict(sd, entries):
    """The fp64 host merge of every family from its definition: a copy of `sd` with W + sum scale * delta (cast back to W's dtype once,
    canonical layout) for every entry of the kinds Graph.set_networks takes.  A NetEntry from entries_for is evaluated on the UNREDUCED
    file tensors (torch.kron for LoKr, einsum for a Tucker core); a bare tuple on the factors it carries.  The fallback for graphs built
    without keep_base() or with uint8 weights -- load the result into a new graph -- and what the tests feed the oracle."""
    acc = {}
    for e in entries:
        raw = getattr(e, 'raw', None)
        if raw is not None:
            name, family, tensors, scale = (e[0] if len(e) == 4 else e[1]), raw['family'], raw['tensors'], raw['scale']
        else:
            name, family, tensors, scale = _plain(e)
        if name not in sd:
            raise KeyError(name)
        w = sd[name]
        if not torch.is_tensor(w):
            raise ValueError(f'{name}: a quantised tensor cannot take a delta')
        dw = delta(family, tensors)
        if dw.numel() != w.numel() or dw.shape[0] != w.shape[0]:
            raise ValueError(f'{name}: the {family} factors give a {tuple(dw.shape)} difference, not a {tuple(w.shape)} weight')
        if not math.isfinite(scale):
            raise ValueError(f'{name}: scale must be finite')
        if name not in acc:
            acc[name] = w.double().clone()
        acc[name].add_(dw.reshape(w.shape), alpha=float(scale))
    out = dict(sd)
    for name, w in acc.items():
        out[name] = w.to(sd[name].dtype)
    return out
