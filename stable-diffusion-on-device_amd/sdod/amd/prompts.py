"""Long, weighted prompts on the host: the emphasis grammar `(word)`, `[word]`, `(word:1.3)` and the 75-token chunks that let a
prompt exceed CLIP's 77 positions.  Pure Python and numpy, no device: Txt2Img.encode_prompt_weighted feeds the (ids, weights)
built here to the text encoder (one execute for every chunk of both prompts) and to sdod_context_assemble_f16.

The grammar and the chunk layout are those of the common Stable Diffusion web front ends, so prompts written for them mean the
same here, with two differences ("Long and weighted prompts"): a full chunk is closed where it is full (no
back-tracking to the last comma), and textual-inversion embeddings are not part of it."""
import math
import re

import numpy as np

CHUNK_TOKENS = 75          # tokens per chunk; with SOT and EOT a chunk is the text encoder's 77 positions
CHUNK_LEN = CHUNK_TOKENS + 2
BREAK = ('BREAK', -1.0)    # parse_emphasis' entry for the word BREAK: close the current chunk

_ROUND, _SQUARE = 1.1, 1.0 / 1.1
# one lexeme per match: an escaped character, a lone backslash, an opening bracket, `:number)`, a closing bracket, plain text, a colon
_LEX = re.compile(r'\\[()\[\]\\]|\\|\(|\[|:\s*([+-]?[.\d]+)\s*\)|\)|\]|[^\\()\[\]:]+|:')
_BREAK = re.compile(r'\s*\bBREAK\b\s*')


def _weight(value, what):
    try:
        w = float(value)
    except ValueError:
        raise ValueError(f'{what!r} does not hold an emphasis weight') from None
    if not math.isfinite(w):
        raise ValueError(f'emphasis weights must be finite, got {value!r} in {what!r}')
    return w


def parse_emphasis(text):
    """text -> [(fragment, multiplier)].  `(x)` multiplies the weight of x by 1.1, `[x]` divides it by 1.1, `(x:1.3)` multiplies it
    by the number ([+-]?[.\\d]+, spaces allowed around it, directly before the `)`); groups nest and their multipliers multiply;
    `\\(`, `\\)`, `\\[`, `\\]`, `\\\\` are the literal characters; a group still open at the end of the text is closed there; a
    closing bracket or `:number)` without an open group is literal text.  The word BREAK (upper case, on word boundaries, its
    surrounding whitespace removed) gives the entry ('BREAK', -1.0); no multiplier applies to it.  Adjacent fragments of equal weight
    are merged; an empty text gives [('', 1.0)].  A number that is not a finite float raises ValueError."""
    res = []                     # [fragment, weight]
    opened = {'(': [], '[': []}  # index into res at which each open group starts

    def scale(start, m):
        for item in res[start:]:
            if item[1] != BREAK[1]:
                item[1] *= m

    for m in _LEX.finditer(text):
        tok, num = m.group(0), m.group(1)
        if tok[0] == '\\' and len(tok) == 2:
            res.append([tok[1], 1.0])
        elif tok == '(' or tok == '[':
            opened[tok].append(len(res))
        elif num is not None and opened['(']:
            scale(opened['('].pop(), _weight(num, tok))
        elif tok == ')' and opened['(']:
            scale(opened['('].pop(), _ROUND)
        elif tok == ']' and opened['[']:
            scale(opened['['].pop(), _SQUARE)
        else:
            for i, part in enumerate(_BREAK.split(tok)):
                if i > 0:
                    res.append(list(BREAK))
                res.append([part, 1.0])
    for start in opened['(']:
        scale(start, _ROUND)
    for start in opened['[']:
        scale(start, _SQUARE)
    out = []
    for frag, w in res:
        if frag == '' and w != BREAK[1]:
            continue
        if out and w != BREAK[1] and out[-1][1] == w:
            out[-1] = (out[-1][0] + frag, w)
        else:
            out.append((frag, w))
    for _, w in out:
        _weight(w, text)
    return out or [('', 1.0)]


def _raw_ids(tokenizer, fragment):
    """the BPE ids of `fragment` alone: no SOT, no EOT, nothing cut.  A token covers at least one byte of the text, so a window of
    len(bytes) + 2 positions holds SOT, every token and an EOT."""
    if not fragment:
        return []
    n = len(fragment.encode('utf-8')) + 2
    ids = np.asarray(tokenizer.encode(fragment, context_len=n), dtype=np.int64)
    end = 1 + int(np.argmax(ids[1:] == tokenizer.end_token))
    return ids[1:end].tolist()


def _chunk(tokenizer, tokens, weights, pad):
    fill = tokenizer.end_token if pad == 'eot' else 0
    ids = np.full(CHUNK_LEN, fill, np.int64)
    w = np.ones(CHUNK_LEN, np.float32)
    ids[0] = tokenizer.start_token
    ids[1:1 + len(tokens)] = tokens
    ids[1 + len(tokens)] = tokenizer.end_token
    w[1:1 + len(tokens)] = weights
    return ids, w


def _check_pad(pad):
    if pad not in ('eot', 'zero'):
        raise ValueError(f"pad must be 'eot' (SD 1.x: padding repeats EOT) or 'zero' (SD 2.x: id 0 after EOT), got {pad!r}")


def empty_chunk(tokenizer, pad='eot'):
    """(ids int64 [77], weights float32 [77]) of a chunk without tokens: SOT, EOT, padding; all weights 1"""
    _check_pad(pad)
    return _chunk(tokenizer, [], [], pad)


def chunk_prompt(tokenizer, text, pad='eot', emphasis=True):
    """text -> (ids int64 [k, 77], weights float32 [k, 77]).  Every fragment of parse_emphasis(text) is tokenised on its own (raw BPE
    ids) and each token carries its fragment's weight.  Tokens fill chunks of 75: a full chunk is closed where it is full and the
    next begins (no back-tracking to a comma); BREAK closes the current chunk unconditionally.  A chunk is SOT, tokens, EOT, padded
    to 77 with EOT (pad='eot', SD 1.x) or with id 0 (pad='zero', SD 2.x); SOT, EOT and padding have weight 1.  A text without
    tokens gives one empty chunk.  emphasis=False: the text is literal and all weights are 1."""
    _check_pad(pad)
    fragments = parse_emphasis(text) if emphasis else [(text, 1.0)]
    for _, w in fragments:           # (finite as a float is not yet finite as the fp32 the device reads)
        if abs(w) > float(np.finfo(np.float32).max):
            raise ValueError(f'emphasis weights must be finite in fp32, got {w!r}')
    chunks, tokens, weights = [], [], []

    def close():
        chunks.append(_chunk(tokenizer, tokens, weights, pad))
        tokens.clear(); weights.clear()

    for frag, w in fragments:
        if emphasis and (frag, w) == BREAK:
            close()
            continue
        for t in _raw_ids(tokenizer, frag):
            if len(tokens) == CHUNK_TOKENS:
                close()
            tokens.append(t); weights.append(w)
    if tokens or not chunks:
        close()
    return np.stack([c[0] for c in chunks]), np.stack([c[1] for c in chunks])


def pad_chunks(ids, weights, k, tokenizer, pad='eot'):
    """(ids [j, 77], weights [j, 77]) -> ([k, 77], [k, 77]) by appending empty chunks; ValueError naming the needed count when j > k"""
    ids = np.asarray(ids, dtype=np.int64)
    weights = np.asarray(weights, dtype=np.float32)
    if ids.ndim != 2 or ids.shape[1] != CHUNK_LEN or weights.shape != ids.shape:
        raise ValueError(f'ids and weights must both be [chunks, {CHUNK_LEN}], got {ids.shape} and {weights.shape}')
    if not np.isfinite(weights).all():
        raise ValueError('emphasis weights must be finite')
    j = ids.shape[0]
    if j > k:
        raise ValueError(f'the prompt needs {j} chunks of {CHUNK_TOKENS} tokens, {k} are available (prompt_chunks={j} or more)')
    if j == k:
        return ids, weights
    e_ids, e_w = empty_chunk(tokenizer, pad)
    return (np.concatenate([ids, np.tile(e_ids, (k - j, 1))]), np.concatenate([weights, np.tile(e_w, (k - j, 1))]))
