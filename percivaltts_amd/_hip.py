"""ctypes binding of libpercival_hip.so (the C ABI declared in include/percival_hip.h).

The header is the single source of the binding: SIGNATURES and the descriptor structures below are parsed from it once, at
import.  A new entry point or struct field is declared in the header only; a declaration the parser cannot read, or a type
it does not know, raises at import.

There is NO fallback: if the library is missing or a kernel reports an error the call raises.
The reference reaches its arithmetic through tf.keras (percivaltts/backend_tensorflow.py:38-39
opens the TF session); this module is the counterpart for the MI355X build.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PTTS_LIB_PATH') or os.path.join(_HERE, 'lib', 'libpercival_hip.so')      # (PTTS_LIB_PATH: an A/B build of the library, tools/ab_define.sh)
HEADER_PATH = os.environ.get('PTTS_HEADER_PATH') or os.path.join(_HERE, '..', 'include', 'percival_hip.h')   # as csrc/Makefile finds it


class HipLibraryError(RuntimeError):
    pass


_SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'size_t': ctypes.c_size_t, 'long long': ctypes.c_longlong, 'unsigned long long': ctypes.c_ulonglong}
_DECLARATOR = re.compile(r'(.*[\s*])(\w+)\s*(\[\s*\])?', re.S)      # type, name, [] of `const float* bias` / `int n` / `T name[]`


def _ctype(spelling, where):
    """The ctypes class of a C type as the header spells it: char* is c_char_p, any other pointer c_void_p."""
    t = ' '.join(w for w in spelling.replace('*', ' * ').split() if w != 'const')
    if t.endswith('*'):
        return ctypes.c_char_p if t == 'char *' else ctypes.c_void_p
    if t not in _SCALARS:
        raise HipLibraryError('percival_hip.h: unknown type {!r} in {!r}'.format(spelling.strip(), ' '.join(where.split())))
    return _SCALARS[t]


def _declaration(text, where):
    """`TYPE name` or `TYPE name[]` -> (name, ctypes class)."""
    m = _DECLARATOR.fullmatch(text.strip())
    if m is None:
        raise HipLibraryError('percival_hip.h: cannot read {!r} in {!r}'.format(text.strip(), ' '.join(where.split())))
    return m.group(2), _ctype(m.group(1) + ('*' if m.group(3) else ''), where)


def parse_header(text):
    """The declarations of a C header in the style of include/percival_hip.h -> (structs, functions): struct name ->
    [(field, ctypes class)] for every `typedef struct NAME { ... } NAME;`, function name -> (restype, [argtypes]) for every
    `RET ptts_xxx(ARGS);`.  Anything else left after comments and preprocessor lines raises HipLibraryError."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'#ifdef __cplusplus.*?#endif', '', text, flags=re.S)          # the extern "C" braces
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    structs, functions = {}, {}

    def struct(m):
        fields = structs[m.group(1)] = []
        for line in filter(str.strip, m.group(2).split(';')):                   # `int a, b` declares several fields of one type
            first, *more = line.split(',')
            name, ctype = _declaration(first, line)
            if not all(n.strip().isidentifier() for n in more):
                raise HipLibraryError('percival_hip.h: cannot read {!r}'.format(' '.join(line.split())))
            fields.extend((n.strip(), ctype) for n in [name] + more)
        return ''

    text = re.sub(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;', struct, text, flags=re.S)
    for decl in filter(str.strip, text.split(';')):
        m = re.fullmatch(r'\s*(.+?)\b(ptts_\w+)\s*\((.*)\)\s*', decl, flags=re.S)
        if m is None:
            raise HipLibraryError('percival_hip.h: cannot read {!r}'.format(' '.join(decl.split())))
        args = [] if m.group(3).strip() == 'void' else [_declaration(a, decl)[1] for a in m.group(3).split(',')]
        functions[m.group(2)] = (_ctype(m.group(1), decl), args)
    return structs, functions


def read_header(path):
    """parse_header of the file at `path`; like the library, a missing header is an error that names the path."""
    if not os.path.exists(path):
        raise HipLibraryError('percival_hip.h not found at {}: it lies in include/ beside the package (or set PTTS_HEADER_PATH). '
                              'The binding is read from it.'.format(path))
    with open(path) as f:
        return parse_header(f.read())


_STRUCTS, SIGNATURES = read_header(HEADER_PATH)          # SIGNATURES: name -> (restype, argtypes)


def _structure(name, cname):
    return type(name, (ctypes.Structure,), {'_fields_': _STRUCTS[cname], '__doc__': 'struct {} of include/percival_hip.h.'.format(cname)})


WGradDesc = _structure('WGradDesc', 'ptts_wgrad_desc')                                   # one weight-gradient product of a grouped launch
DenseWgradReduceDesc = _structure('DenseWgradReduceDesc', 'ptts_dense_wgrad_reduce_desc')   # the partial rows of one weight-gradient product
DenseSplitDesc = _structure('DenseSplitDesc', 'ptts_dense_split_desc')                   # one weight of a grouped plane split
Conv2dReduceDesc = _structure('Conv2dReduceDesc', 'ptts_conv2d_reduce_desc')             # one queued conv2d backward pass
DenseRowsDesc = _structure('DenseRowsDesc', 'ptts_dense_rows_desc')                      # the fp32-rows form of a batched product's right operand


def _define(name):
    """The integer value of `#define NAME value` in the header."""
    with open(HEADER_PATH) as f:
        m = re.search(r'^[ \t]*#[ \t]*define[ \t]+{}[ \t]+(\w+)'.format(name), f.read(), flags=re.M)
    if m is None:
        raise HipLibraryError('percival_hip.h: no #define {}'.format(name))
    return int(m.group(1), 0)


PLANES_ROWS = _define('PTTS_PLANES_ROWS')            # flag bit in planes_count of ptts_dense_bf16x6_batched: `planes` is a DenseRowsDesc

_lib = None


def lib():
    """Load the library once; raise loudly if it is absent (no CPU path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                'libpercival_hip.so not found at {}: run `python -c "import __graft_entry__ as g; g.build()"` '
                '(or `make -C percivaltts_amd/csrc`). There is no CPU fallback.'.format(LIB_PATH))
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)   # AttributeError if the symbol is missing -> loud
            fn.restype = res
            fn.argtypes = args
        if os.environ.get('PTTS_DETERMINISTIC', '0') == '1':
            l.ptts_set_deterministic(1)
        _lib = l
    return _lib


def last_error():
    return lib().ptts_last_error().decode('utf8', 'replace')


class KernelTimer(object):
    """HIP-event timing of every C-ABI call made while it is active (bench.py's roofline leg).  Events are recorded on
    the stream the kernels are launched on (torch's current stream).  Not usable during graph capture."""
    active = None

    def __init__(self):
        self.records = []   # (name, tag, start_event, end_event)

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def durations_ms(self):
        torch.cuda.synchronize()
        return [(n, t, s.elapsed_time(e)) for n, t, s, e in self.records]


def call(name, *args, **kw):
    """Invoke an int-returning entry point and raise on a non-zero status.  `tag` labels the call for KernelTimer."""
    timer = KernelTimer.active
    if timer is not None:
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
    rc = getattr(lib(), name)(*args)
    if timer is not None:
        e.record()
        timer.records.append((name, kw.get('tag'), s, e))
    if rc != 0:
        raise HipLibraryError('{} failed (rc={}): {}'.format(name, rc, last_error()))


def check_status():
    """Raise HipLibraryError if a kernel has reported a failed hand-off since the last clear_status() (the sticky device status
    word of include/percival_hip.h).  A host memory load, no synchronisation: the optimiser calls it at every step boundary."""
    rc = lib().ptts_device_status(None)
    if rc != 0:
        raise HipLibraryError('device status (rc={}): {}'.format(rc, last_error()))


def clear_status():
    lib().ptts_device_status_clear()


def stream_id():
    """Raw handle (an integer) of the current HIP stream of the current device.  torch.cuda.current_stream() builds a Stream object
    through several layers of Python (7 us a call, 150 calls per training step: a millisecond of a host-bound step); the raw getter
    is the same lookup without them."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def stream():
    return ctypes.c_void_p(stream_id())


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The tensor must be fp32/fp64/int32 CUDA memory."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError('percivaltts_amd kernels need device tensors (got a {} tensor); there is no CPU path'
                              .format(t.device))
    return ctypes.c_void_p(t.data_ptr())


def f32c(t, name='tensor'):
    """Validate: CUDA, float32, contiguous."""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise HipLibraryError('{}: expected a contiguous float32 device tensor, got {} {} contiguous={}'.format(
            name, t.device, t.dtype, t.is_contiguous()))
    return t


_ws_cache = {}


def _workspace(nbytes, device):
    """One growing scratch buffer per device and stream (kernels on one stream are ordered)."""
    key = (device.index, stream_id(), torch.cuda.is_current_stream_capturing())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf
