"""ctypes binding of libhoig_hip.so (the C ABI declared in include/hoig_kernels.h).

An entry point is declared ONCE, in the header: this module parses it at import and derives every function's argtypes / restype
and every HOIG_* constant from it.  There is NO fallback: if the shared library is missing, a symbol the header declares is
absent, or the header holds a declaration this module cannot read, importing it raises.  Every product op in ``hoig_amd.ops``
goes through here.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', '_build', 'libhoig_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'hoig_kernels.h')


class HoigKernelError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('B', 'Hi', 'Wi', 'Ci', 'Ho', 'Wo', 'Co', 'R', 'S', 'stride', 'pad',
                                              'transposed', 'act')] + \
               [('slope', ctypes.c_float), ('precision', ctypes.c_int32)]


def build(verbose=False):
    """Compile every HIP source for gfx950 into hoig_amd/csrc/_build/libhoig_hip.so."""
    script = os.path.join(_HERE, 'csrc', 'build.sh')
    out = subprocess.run(['bash', script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
    if out.returncode != 0:
        raise RuntimeError('hipcc build of libhoig_hip.so failed')
    return LIB_PATH


# ------------------------------------------------------------------------------------------------ the header, read once
# The type map is closed: a spelling that is not listed raises with the function's name, it never becomes c_void_p or c_int.
_CTYPES = {
    'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64,
    'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double,
    'hoig_stream_t': ctypes.c_void_p, 'hoig_stream_t *': ctypes.POINTER(ctypes.c_void_p),
    'const hoig_conv_desc *': ctypes.POINTER(ConvDesc), 'const char *': ctypes.c_char_p,
}
# what a data pointer (c_void_p) may point to, besides the structs the header defines
_POINTEES = {'void', 'float', 'double', 'int', 'int32_t', 'int64_t', 'uint8_t', 'uint16_t', 'uint32_t', 'uint64_t', 'unsigned char'}


def _ctype(spelling, pointees, where):
    spelling = ' '.join(spelling.replace('*', ' * ').split())
    if spelling in _CTYPES:
        return _CTYPES[spelling]
    m = re.fullmatch(r'(?:const )?([\w ]+?)(?: \*(?: const)?)+', spelling)      # a data pointer (or a table of them)
    if m and m.group(1) in pointees:
        return ctypes.c_void_p
    raise TypeError('%s: %s: no ctypes mapping for the type %r' % (os.path.basename(HEADER_PATH), where, spelling))


def parse_header(text):
    """-> ({name: (restype, argtypes)} of every prototype, {X: n} of every enum constant and `#define HOIG_X n`) of a header
    text.  Everything outside comments must be a prototype, a typedef, an enum or a preprocessor line: anything else raises."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    consts = {}

    def constant(name, value):
        if not re.fullmatch(r'-?(0[xX][0-9a-fA-F]+|\d+)', value):
            raise ValueError('%s: %s is not an integer literal: %r' % (os.path.basename(HEADER_PATH), name, value))
        consts[name[len('HOIG_'):]] = int(value, 0)

    def enum(m):
        for item in filter(None, (s.strip() for s in m.group(1).split(','))):
            name, _, value = (s.strip() for s in item.partition('='))
            constant(name, value)
        return ''

    def define(m):
        if m.group(2):                                   # (a bare `#define HOIG_KERNELS_H` is the include guard)
            constant(m.group(1), m.group(2).strip())
        return ''

    text = re.sub(r'^[ \t]*#[ \t]*define[ \t]+(HOIG_\w+)[ \t]*(.*)$', define, text, flags=re.M)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    text = re.sub(r'\benum\s*\{([^}]*)\}\s*;', enum, text)
    pointees = set(_POINTEES)
    text = re.sub(r'\btypedef\s+struct\s+\w*\s*\{[^}]*\}\s*(\w+)\s*;', lambda m: pointees.add(m.group(1)) or '', text)
    text = re.sub(r'\btypedef\s+void\s*\*\s*hoig_stream_t\s*;|\bextern\s+"C"\s*\{|\}\s*$', '', text.rstrip())
    protos = {}
    for stmt in filter(None, (s.strip() for s in text.split(';'))):
        m = re.fullmatch(r'([\w\s*]+?)\s*\b(hoig_[a-z0-9_]+)\s*\(([^()]*)\)', stmt)
        if not m:
            raise ValueError('%s: not a prototype: %r' % (os.path.basename(HEADER_PATH), ' '.join(stmt.split())[:120]))
        ret, name, params = m.groups()
        if name in protos:
            raise ValueError('%s: %s is declared twice' % (os.path.basename(HEADER_PATH), name))
        params = [] if params.strip() in ('', 'void') else params.split(',')
        # a parameter is its type and then its name: the name is the last word, unless that is a '*' or the only word
        types = [re.sub(r'(?<=[\s*])\w+\s*$', '', p.strip()) for p in params]
        protos[name] = (_ctype(ret, pointees, name), [_ctype(t, pointees, name) for t in types])
    return protos, consts


_PROTOS, _CONSTS = parse_header(open(HEADER_PATH).read())
globals().update(_CONSTS)          # OK, EINVAL, ACT_*, PREC_*, LOSS_*, POOL_*, GEMM_*, PNG_E*, DAUG_*, SWD_K, ...: HOIG_X is L.X
_SIGS = {name: args for name, (ret, args) in _PROTOS.items() if ret is ctypes.c_int}   # the entry points that return a status
FM_NONFINITE, FM_CLAMPED = 1, 2     # the bits of a feature-metric status word (feature_metrics.h: no name in the public header)
_ERR = {EINVAL: 'invalid argument', ELAUNCH: 'kernel launch failed', EUNSUPPORTED: 'unsupported shape'}   # noqa: F821


def declared_symbols():
    """Entry points the header declares (used by the CPU test that checks the library exports all of them)."""
    return sorted(_PROTOS)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'hoig_amd: %s not found. The HIP extension is mandatory (no CPU / eager fallback exists); build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` or `bash hoig_amd/csrc/build.sh`.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (ret, args) in _PROTOS.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes = args
        fn.restype = ret
    # the three values that the header defines AND the library answers for
    for const, query in (('SORT_LDS_MAX', 'hoig_sort_segments_lds_max'), ('SORT_TILE', 'hoig_sort_segments_tile'),
                         ('GRAD_CHUNK', 'hoig_grad_stats_chunk')):
        if getattr(lib, query)() != _CONSTS[const]:
            raise ImportError('hoig_amd: %s() = %d, but the header says HOIG_%s = %d: rebuild the library'
                              % (query, getattr(lib, query)(), const, _CONSTS[const]))
    return lib


lib = _load()
GRAD_MAX_GRID = lib.hoig_grad_stats_max_grid()   # the most workgroups stage 1 of hoig_grad_stats uses


def set_tuning(key, value):
    """hoig_set_tuning: kernel-variant choice `key` -> `value` (returns the previous value)."""
    prev = lib.hoig_set_tuning(key.encode(), int(value))
    if prev < 0:
        raise KeyError('unknown tuning key %r' % key)
    return prev


# HOIG_TUNING="key=value,key=value": variant choices for A/B runs (bench.py and the tools set them through this one variable)
for _kv in filter(None, os.environ.get('HOIG_TUNING', '').split(',')):
    set_tuning(*_kv.split('='))


ROUTE_FWD, ROUTE_DGRAD, ROUTE_WGRAD = 0, 1, 2


def route_names():
    """The library's table of convolution routes (hoig_amd/csrc/conv_route.h), by id."""
    names, i = [], 0
    while True:
        n = lib.hoig_conv_route_name(i)
        if n is None:
            return names
        names.append(n.decode())
        i += 1


def last_route(which):
    """hoig_conv_last_route: the name of the convolution launcher that ran last on this thread (0 forward, 1 data gradient,
    2 weight gradient; 'none' before the first)."""
    rid = lib.hoig_conv_last_route(int(which))
    if rid < 0:
        raise ValueError('last_route(%r): 0 forward, 1 data gradient, 2 weight gradient' % (which,))
    return lib.hoig_conv_route_name(rid).decode()


def check(rc, what):
    if rc != 0:
        raise HoigKernelError('%s failed: %s (code %d)' % (what, _ERR.get(rc, 'unknown'), rc))


# Every launch of the package goes through one of these two, reached as `L.call` / `L.attempt` (an attribute of this module, read at
# call time): a tool that rebinds the two names sees every launch (tools/op_table.py, tools/conv_table.py).
def call(name, *args):
    check(getattr(lib, name)(*args), name)


def attempt(name, *args):
    """call() for an entry point that may refuse the shape: False on EUNSUPPORTED (nothing ran: the caller takes its next kernel)."""
    rc = getattr(lib, name)(*args)
    if rc == EUNSUPPORTED:          # noqa: F821
        return False
    check(rc, name)
    return True
