"""CPU tests: the C-ABI library loads (no compute) and exports every symbol include/percival_hip.h declares,
and the ctypes signature table that percivaltts_amd/_hip.py parses from that header covers exactly that set."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'percival_hip.h')


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(ptts_\w+)\s*\(', src)))


def test_header_declares_the_hot_path_entry_points():
    syms = declared_symbols()
    for must in ('ptts_conv2d_fwd', 'ptts_conv2d_bwd', 'ptts_gemm', 'ptts_gp_interpolate', 'ptts_gp_sqnorm',
                 'ptts_gp_penalty', 'ptts_weight_clip', 'ptts_adam_keras_step', 'ptts_lstm_fwd', 'ptts_lstm_bwd',
                 'ptts_colstats', 'ptts_bn_finalize', 'ptts_version', 'ptts_device_arch', 'ptts_last_error'):
        assert must in syms


def test_library_exports_every_declared_symbol():
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(lib, s), 'missing export ' + s
    assert set(_hip.SIGNATURES) == set(declared_symbols())
    lib.ptts_device_arch.restype = ctypes.c_char_p
    assert lib.ptts_device_arch() == b'gfx950'


SNIPPET = """
/* every shape of declaration the real header has */
#ifndef SNIPPET_H
#define SNIPPET_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PTTS_X 1   /* a constant */
const char* ptts_name(void);      // a line comment; with (punctuation)
unsigned* ptts_word(void);
int ptts_message(unsigned word, char* buf, size_t n);
typedef struct ptts_desc {
    const float* partials;      /* a pointer */
    int a, b;
    long long ld;
    float* dw; float* dbias;
    float alpha;
} ptts_desc;
int ptts_grouped(const ptts_desc* descs, int n, void* stream);
size_t ptts_bytes(int B, long long rows);
long long ptts_elems(int B);
int ptts_fwd(const float* x, const float* bias /*[Cout] or NULL*/,
             const unsigned char* labels, unsigned* word_out, const float* const* w,
             double fs, unsigned long long seed, unsigned long long* state,
             const int offs[], float alpha, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SNIPPET_H */
"""


def test_parser_reads_every_shape_of_declaration():
    from percivaltts_amd._hip import parse_header
    c = ctypes
    P, I = c.c_void_p, c.c_int
    structs, functions = parse_header(SNIPPET)
    assert structs == {'ptts_desc': [('partials', P), ('a', I), ('b', I), ('ld', c.c_longlong), ('dw', P), ('dbias', P),
                                     ('alpha', c.c_float)]}
    assert functions == {
        'ptts_name': (c.c_char_p, []),
        'ptts_word': (P, []),
        'ptts_message': (I, [c.c_uint, c.c_char_p, c.c_size_t]),
        'ptts_grouped': (I, [P, I, P]),
        'ptts_bytes': (c.c_size_t, [I, c.c_longlong]),
        'ptts_elems': (c.c_longlong, [I]),
        'ptts_fwd': (I, [P, P, P, P, P, c.c_double, c.c_ulonglong, P, P, c.c_float, P]),
    }
    for res, args in functions.values():            # the classes themselves, not look-alikes: c_char_p == c_void_p is False anyway
        assert all(isinstance(t, type) and issubclass(t, c._SimpleCData) for t in [res] + args)


@pytest.mark.parametrize('text', ['int ptts_x(foo_t v);',                    # unknown type
                                  'foo_t ptts_x(int v);',                    # unknown return type
                                  'int ptts_x(int);',                        # a parameter without a name
                                  'int other_x(int v);',                     # not an entry point of this library
                                  'typedef struct s { foo_t a; } s; int ptts_x(void);',
                                  'typedef struct s { int a, *b; } s;',
                                  'struct s { int a; };'])
def test_parser_raises_on_what_it_cannot_read(text):
    from percivaltts_amd._hip import HipLibraryError, parse_header
    with pytest.raises(HipLibraryError, match='percival_hip.h: '):
        parse_header(text)


def test_descriptor_structures_follow_the_header():
    from percivaltts_amd import _hip
    for cls, fields, size in (
            (_hip.WGradDesc, 'A B C colsum_b in_scale in_shift mask_src M N K lda ldb ldc in_mode alpha', 104),
            (_hip.DenseWgradReduceDesc, 'partials split Kin N ldc C colsum_b', 48),
            (_hip.DenseSplitDesc, 'w planes ldw K N transposed reserved', 40),
            (_hip.Conv2dReduceDesc, 'partials nblocks npart nw cout dw dbias', 40)):
        assert issubclass(cls, ctypes.Structure)
        assert [f[0] for f in cls._fields_] == fields.split() and ctypes.sizeof(cls) == size, cls


def test_missing_header_fails_loudly(tmp_path):
    from percivaltts_amd import _hip
    with pytest.raises(_hip.HipLibraryError, match='absent.h'):
        _hip.read_header(str(tmp_path / 'absent.h'))
    assert _hip.read_header(HEADER)[1] == _hip.SIGNATURES


def test_device_status_word_is_sticky_and_decoded():
    """The host side of the device status word (include/percival_hip.h: ptts_device_status*): a code a kernel would store -- written
    here through the word's host address, no GPU involved -- makes ptts_device_status return PTTS_EDEVICE with a message naming the
    kernel family, stays until ptts_device_status_clear(), and _hip.check_status() raises."""
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = _hip.lib()
    word = ctypes.cast(lib.ptts_device_status_word(), ctypes.POINTER(ctypes.c_uint))
    _hip.clear_status()
    out = ctypes.c_uint(99)
    assert lib.ptts_device_status(ctypes.byref(out)) == 0 and out.value == 0
    _hip.check_status()
    for slot, code, text in ((0, 1, 'conv2d'), (1, 2, 'LSTM')):
        word[slot] = code
        assert lib.ptts_device_status(ctypes.byref(out)) == -4 and out.value == code        # PTTS_EDEVICE
        assert text in _hip.last_error()
        assert lib.ptts_device_status(None) == -4                                           # sticky
        with pytest.raises(_hip.HipLibraryError, match='hand-off|hidden state'):
            _hip.check_status()
        _hip.clear_status()
        assert lib.ptts_device_status(ctypes.byref(out)) == 0 and out.value == 0
    word[0] = 1; word[1] = 2
    assert lib.ptts_device_status(ctypes.byref(out)) == -4 and out.value == 3
    buf = ctypes.create_string_buffer(400)
    assert lib.ptts_device_status_message(3, buf, 400) == 0 and b'conv2d' in buf.value and b'LSTM' in buf.value
    assert lib.ptts_device_status_message(0, buf, 400) == 0 and buf.value == b'ok'
    _hip.clear_status()


def test_missing_library_or_cpu_tensor_fails_loudly(monkeypatch):
    import torch
    from percivaltts_amd import _hip, ops
    with pytest.raises(_hip.HipLibraryError):
        ops.gp_interpolate(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), torch.zeros(2))   # CPU tensors: no fallback
    monkeypatch.setattr(_hip, '_lib', None)
    monkeypatch.setattr(_hip, 'LIB_PATH', '/nonexistent/libpercival_hip.so')
    with pytest.raises(_hip.HipLibraryError):
        _hip.lib()


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, 'percivaltts_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                txt = open(os.path.join(dirpath, f)).read()
                assert 'import oracle' not in txt and 'from oracle' not in txt, f
