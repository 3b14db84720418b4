"""Long, weighted prompts on the host (no GPU): the emphasis parser against its known answers, the 75-token chunker on the synthetic
tokenizer, the argument contract of the pipeline's entry points, and what of sdod_context_assemble_f16 and of the longer UNet
context can be checked without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from sdod.amd import prompts as PR

REL = 1e-12


def same(got, want):
    assert [g[0] for g in got] == [w[0] for w in want], got
    for (_, gw), (_, ww) in zip(got, want):
        assert gw == pytest.approx(ww, rel=REL), (got, want)


# ------------------------------------------------------------------ the parser
@pytest.mark.parametrize('text, want', [
    ('normal text', [('normal text', 1.0)]),
    ('an (important) word', [('an ', 1.0), ('important', 1.1), (' word', 1.0)]),
    ('(unbalanced', [('unbalanced', 1.1)]),
    ('\\(literal\\]', [('(literal]', 1.0)]),
    ('(unnecessary)(parens)', [('unnecessaryparens', 1.1)]),
    ('a (((house:1.3)) [on] a (hill:0.5), sun, (((sky))).',
     [('a ', 1.0), ('house', 1.5730000000000004), (' ', 1.1), ('on', 1.0), (' a ', 1.1), ('hill', 0.55), (', sun, ', 1.1),
      ('sky', 1.4641000000000006), ('.', 1.1)]),
    ('', [('', 1.0)]),
])
def test_parser_known_answers(text, want):
    same(PR.parse_emphasis(text), want)


def test_parser_nesting_multiplies():
    same(PR.parse_emphasis('((a) b)'), [('a', 1.1 * 1.1), (' b', 1.1)])
    same(PR.parse_emphasis('[[a]]'), [('a', 1 / 1.1 / 1.1)])
    same(PR.parse_emphasis('([a])'), [('a', 1.0)])
    same(PR.parse_emphasis('((a:2):3)'), [('a', 6.0)])
    same(PR.parse_emphasis('[(a:2)'), [('a', 2 / 1.1)])                # the square group is still open at the end
    same(PR.parse_emphasis('(a:-.5)(b: +2. )'), [('a', -0.5), ('b', 2.0)])


def test_parser_escapes_and_stray_brackets():
    same(PR.parse_emphasis('\\\\(a\\)'), [('\\', 1.0), ('a)', 1.1)])  # an escaped backslash, then a group holding an escaped ')'
    same(PR.parse_emphasis('a\\[b\\]'), [('a[b]', 1.0)])
    same(PR.parse_emphasis('x) y] :1.2)'), [('x) y] :1.2)', 1.0)])     # nothing is open: all of it is text
    same(PR.parse_emphasis('a:b (c:d)'), [('a:b ', 1.0), ('c:d', 1.1)])  # a colon without a number is text
    same(PR.parse_emphasis('back\\slash'), [('back\\slash', 1.0)])


def test_parser_break():
    same(PR.parse_emphasis('a BREAK b'), [('a', 1.0), ('BREAK', -1.0), ('b', 1.0)])
    same(PR.parse_emphasis('(a  BREAK\tb:1.2)'), [('a', 1.2), ('BREAK', -1.0), ('b', 1.2)])    # no multiplier touches the entry
    same(PR.parse_emphasis('BREAK'), [('BREAK', -1.0)])
    same(PR.parse_emphasis('a BREAK BREAK b'), [('a', 1.0), ('BREAK', -1.0), ('BREAK', -1.0), ('b', 1.0)])
    same(PR.parse_emphasis('BREAKFAST break Break'), [('BREAKFAST break Break', 1.0)])        # upper case, on word boundaries


def test_parser_refuses_numbers_that_are_no_weights():
    with pytest.raises(ValueError):
        PR.parse_emphasis('(a:1.2.3)')
    with pytest.raises(ValueError, match='finite'):
        PR.parse_emphasis('(a:1' + '0' * 400 + ')')


# ------------------------------------------------------------------ the chunker
@pytest.fixture(scope='module')
def tok(golden_dir):
    from sdod.amd import host
    return host.Tokenizer(os.path.join(golden_dir, 'ctokenizer_synthetic.txt'))


def test_raw_ids_are_what_the_tokenizer_puts_between_sot_and_eot(tok):
    text = 'a photograph of an astronaut riding a horse'
    ids = tok.encode(text)
    n = int(np.argmax(ids == tok.end_token))
    i, w = PR.chunk_prompt(tok, text)
    assert i.dtype == np.int64 and w.dtype == np.float32 and i.shape == w.shape == (1, 77)
    assert i[0].tolist() == ids.astype(np.int64).tolist() and n > 5       # a short literal prompt: encode()'s own window
    assert np.all(w == 1.0)


@pytest.mark.parametrize('n_tokens, n_chunks', [(0, 1), (75, 1), (76, 2), (151, 3)])
@pytest.mark.parametrize('pad', ['eot', 'zero'])
def test_chunk_counts_and_layout(tok, n_tokens, n_chunks, pad):
    a = int(tok.encode('a')[1])
    ids, w = PR.chunk_prompt(tok, 'a ' * n_tokens, pad=pad)
    assert ids.shape == w.shape == (n_chunks, 77)
    fill = tok.end_token if pad == 'eot' else 0
    left = n_tokens
    for c in range(n_chunks):
        n = min(left, 75)
        left -= n
        assert ids[c, 0] == tok.start_token
        assert ids[c, 1:1 + n].tolist() == [a] * n
        assert ids[c, 1 + n] == tok.end_token
        assert np.all(ids[c, 2 + n:] == fill)
    assert left == 0 and np.all(w == 1.0)


def test_token_weights_follow_their_fragments(tok):
    ids, w = PR.chunk_prompt(tok, 'a (abc:1.5) [a] \\(a')
    a, abc = int(tok.encode('a')[1]), int(tok.encode('abc')[1])
    par = int(tok.encode('(')[1])
    assert ids[0, :7].tolist() == [tok.start_token, a, abc, a, par, a, tok.end_token]
    assert w[0, :7].tolist() == pytest.approx([1.0, 1.0, 1.5, 1 / 1.1, 1.0, 1.0, 1.0], rel=1e-7)
    assert np.all(w[0, 7:] == 1.0)
    # a weight that spans a chunk boundary goes with its tokens
    ids, w = PR.chunk_prompt(tok, 'a ' * 74 + '(a a a:2)')
    assert ids.shape == (2, 77)
    assert w[0, 1:75].tolist() == [1.0] * 74 and w[0, 75] == 2.0 and w[0, 76] == 1.0      # token 75 weighted, EOT not
    assert w[1, :4].tolist() == [1.0, 2.0, 2.0, 1.0]


def test_break_closes_the_chunk(tok):
    a = int(tok.encode('a')[1])
    ids, w = PR.chunk_prompt(tok, 'a a BREAK (a:3)')
    assert ids.shape == (2, 77)
    assert ids[0, :4].tolist() == [tok.start_token, a, a, tok.end_token] and ids[1, :3].tolist() == [tok.start_token, a, tok.end_token]
    assert w[1, 1] == 3.0 and np.all(w[0] == 1.0)
    assert PR.chunk_prompt(tok, 'BREAK a')[0].shape == (2, 77)            # unconditionally: the first chunk is empty
    assert PR.chunk_prompt(tok, 'a BREAK')[0].shape == (1, 77)            # nothing follows: no further chunk


def test_emphasis_off_reads_the_text_literally(tok):
    text = 'a (abc:1.5) BREAK'
    ids, w = PR.chunk_prompt(tok, text, emphasis=False)
    assert ids.shape == (1, 77) and np.all(w == 1.0)
    assert ids[0].tolist() == tok.encode(text).astype(np.int64).tolist()   # parentheses, colon, digits and the word are tokens
    assert PR.chunk_prompt(tok, text)[0].shape == (1, 77) and not np.array_equal(PR.chunk_prompt(tok, text)[0], ids)


def test_bad_pad_and_weights_outside_fp32(tok):
    with pytest.raises(ValueError):
        PR.chunk_prompt(tok, 'a', pad='space')
    with pytest.raises(ValueError, match='finite'):
        PR.chunk_prompt(tok, '(a:1' + '0' * 39 + ')')                      # 1e39: a float, not an fp32


def test_pad_chunks(tok):
    ids, w = PR.chunk_prompt(tok, 'a ' * 80, pad='zero')
    i3, w3 = PR.pad_chunks(ids, w, 3, tok, pad='zero')
    assert i3.shape == w3.shape == (3, 77) and i3.dtype == np.int64 and w3.dtype == np.float32
    assert np.array_equal(i3[:2], ids) and np.array_equal(w3[:2], w)
    assert i3[2].tolist() == [tok.start_token, tok.end_token] + [0] * 75 and np.all(w3[2] == 1.0)
    e_ids, e_w = PR.empty_chunk(tok, 'eot')
    assert e_ids.tolist() == [tok.start_token] + [tok.end_token] * 76 and np.all(e_w == 1.0)
    assert np.array_equal(PR.chunk_prompt(tok, '')[0][0], e_ids)
    same_ids, same_w = PR.pad_chunks(ids, w, 2, tok)
    assert np.array_equal(same_ids, ids) and np.array_equal(same_w, w)
    with pytest.raises(ValueError, match='needs 2 chunks'):
        PR.pad_chunks(ids, w, 1, tok)
    bad = w.copy()
    bad[0, 3] = np.inf
    with pytest.raises(ValueError, match='finite'):
        PR.pad_chunks(ids, bad, 2, tok)
    with pytest.raises(ValueError):
        PR.pad_chunks(ids[:, :76], w[:, :76], 2, tok)


# ------------------------------------------------------------------ pipeline arguments (no constructor: no graphs, no device)
@pytest.mark.parametrize('k', [0, 5, -1, 2.0, '2', None, True])
def test_constructor_refuses_prompt_chunks_before_device_work(k):
    from sdod.amd.pipeline import Txt2Img, check_prompt_chunks
    with pytest.raises(ValueError, match='prompt_chunks'):
        check_prompt_chunks(k)
    with pytest.raises(ValueError, match='prompt_chunks'):             # (this host has no GPU: anything later would fail otherwise)
        Txt2Img(state_dicts={}, prompt_chunks=k, device='cuda:0')
    assert [check_prompt_chunks(v) for v in (1, 2, 3, 4, np.int64(2))] == [1, 2, 3, 4, 2]


def _pipe(k):
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)
    pipe.cfg = E.sd14_config(16, 16)
    pipe.prompt_chunks = k
    return pipe


def test_encode_chunks_argument_errors():
    pipe = _pipe(2)
    ids = np.zeros((2, 77), np.int64)
    w = np.ones((2, 2, 77), np.float32)
    bad = [
        (ids[:1], ids, None),                              # one chunk on a two-chunk pipeline
        (ids, ids[:, :76], None),
        (ids.astype(np.float32), ids, None),               # ids must be integers
        (ids, ids, w[:1]),
        (ids, ids, w[:, :, :76]),
        (ids, ids, w.astype(np.float64)),
        (ids, ids, torch.ones(2, 2, 77, dtype=torch.float16)),
        (ids, ids, [[1.0] * 77] * 4),                      # neither an array nor a tensor
        (ids, ids - 1, None),                              # ids outside the vocabulary
        (ids + pipe.cfg.vocab_size, ids, None),
    ]
    for iu, ic, ww in bad:
        with pytest.raises(ValueError):
            pipe.encode_chunks(iu, ic, ww)
    nan = w.copy()
    nan[1, 0, 5] = np.nan
    with pytest.raises(ValueError, match='finite'):
        pipe.encode_chunks(ids, ids, nan)
    # an object made by __new__ has the default: one chunk
    from sdod.amd.pipeline import Txt2Img
    with pytest.raises(ValueError, match='prompt_chunks=1'):
        Txt2Img.__new__(Txt2Img).encode_chunks(ids, ids)


def test_encode_prompt_weighted_refuses_a_prompt_that_needs_more_chunks(tok):
    pipe = _pipe(2)
    pipe.tokenizer = tok
    with pytest.raises(ValueError, match='needs 3 chunks'):
        pipe.encode_prompt_weighted('a ' * 151)
    with pytest.raises(ValueError, match='needs 3 chunks'):
        pipe.encode_prompt_weighted('a', negative='a BREAK a BREAK a')
    pipe.tokenizer = None
    with pytest.raises(ValueError, match='tokenizer'):
        pipe.encode_prompt_weighted('a')


def test_short_ids_are_padded_with_empty_chunks(tok):
    for model, pad in (('sd14', 'eot'), ('sd21', 'zero')):
        pipe = _pipe(3)
        pipe.model, pipe.tokenizer = model, tok
        ids = pipe._ids('a photograph')
        want, _ = PR.pad_chunks(*PR.chunk_prompt(tok, 'a photograph', pad, emphasis=False), 3, tok, pad)
        assert np.array_equal(pipe._pad_ids(ids), want)


# ------------------------------------------------------------------ the kernel's C ABI and the engine, without a device
def test_context_assemble_is_bound_and_checks_its_arguments_before_any_device_call():
    from sdod.amd import _lib
    assert 'sdod_context_assemble_f16' in _lib.HIP_SYMBOLS
    lib = _lib.hip()
    fn = lib.sdod_context_assemble_f16
    assert fn.argtypes is not None and len(fn.argtypes) == 8 and fn.restype == ctypes.c_int
    a, b = 0x10000, 0x900000         # never dereferenced: every call below is refused on the host
    bad = [
        (None, None, b, 1, 1, 77, 768),          # NULL enc
        (a, None, None, 1, 1, 77, 768),          # NULL out
        (a, None, b, 0, 1, 77, 768), (a, None, b, 1, 0, 77, 768), (a, None, b, 1, 1, 0, 768), (a, None, b, -1, 1, 77, 768),
        (a, None, b, 1, 1, 77, 772), (a, None, b, 1, 1, 77, 0),        # D % 8, D < 8
        (a + 8, None, b, 1, 1, 77, 768), (a, None, b + 2, 1, 1, 77, 768),  # alignment
        (a, None, a, 1, 1, 77, 768),             # in place
        (a, None, a + 16, 2, 2, 77, 768),        # overlapping
        (a + 768 * 2 * 77, None, a, 1, 2, 77, 768),
    ]
    for args in bad:
        assert fn(*args, None) != 0, args
        assert lib.sdod_hip_last_error()


def test_unet_parameters_do_not_depend_on_the_context_length():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    long = E.ModelConfig.from_buffer_copy(cfg)
    long.context_len = 154
    assert cfg.context_len == 77                     # the copy is a copy: the text encoder keeps its 77 positions
    assert E.UNet(long, 2).param_table() == E.UNet(cfg, 2).param_table()
    pos = dict(E.TextEncoder(cfg, 4).param_table())['text_model.embeddings.position_embedding.weight']
    assert pos == (77, 768)
    bad = E.ModelConfig.from_buffer_copy(cfg)
    bad.context_len = 0
    with pytest.raises(Exception, match='context_len'):
        E.UNet(bad, 2)
