"""hoig_amd._lib derives its ctypes signatures and its constants from include/hoig_kernels.h: the parser on synthetic declarations,
its completeness over the real header, pinned signatures of one entry point per type class, every constant's value, and what happens
when an ops_* family is imported before hoig_amd.ops.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from hoig_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, I, I64, U64, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double
DESC = ctypes.POINTER(L.ConvDesc)

SYNTHETIC = '''
/* a block comment that names hoig_not_a_function(int x); and spans
   two lines */
#ifndef HOIG_KERNELS_H
#define HOIG_KERNELS_H
#include <stdint.h>
extern "C" {
typedef void *hoig_stream_t; /* hipStream_t */
enum { HOIG_OK = 0, HOIG_EINVAL = -1 };
enum { HOIG_BIT_A = 1,   /* first */
       HOIG_BIT_B = 0x10 /* second */ };
#define HOIG_CHUNK 4096   /* elements */
typedef struct hoig_plan {
    int32_t a; float b;
} hoig_plan;
int hoig_scalars(int a, int32_t b, int64_t c, uint64_t d, size_t e, float f, double g, hoig_stream_t stream);
int hoig_pointers(const hoig_conv_desc *d, const char *key, hoig_stream_t *out, const float *x, float *y /*nullable*/,
                  const uint16_t *w /*[Co][3][3][Ci]*/, void *ws, const hoig_plan *plans, uint8_t *bytes,   // a line comment
                  const float *const *table, unsigned char *mask, double *stats /*nullable*/);
int64_t hoig_bytes(int n);
size_t hoig_size(void);
const char *hoig_name();
int
hoig_split_over_lines(
    int a,
    const int64_t *rows
);
}
#endif
'''


def test_parser_on_synthetic_declarations():
    protos, consts = L.parse_header(SYNTHETIC)
    assert protos == {
        'hoig_scalars': (I, [I, I, I64, U64, ctypes.c_size_t, F, D, VP]),
        'hoig_pointers': (I, [DESC, ctypes.c_char_p, ctypes.POINTER(VP), VP, VP, VP, VP, VP, VP, VP, VP, VP]),
        'hoig_bytes': (I64, [I]),
        'hoig_size': (ctypes.c_size_t, []),
        'hoig_name': (ctypes.c_char_p, []),
        'hoig_split_over_lines': (I, [I, VP]),
    }
    assert consts == {'OK': 0, 'EINVAL': -1, 'BIT_A': 1, 'BIT_B': 16, 'CHUNK': 4096}


@pytest.mark.parametrize('decl, word', [
    ('int hoig_bad_scalar(unsigned n);', 'hoig_bad_scalar'),          # a scalar outside the map does not become c_int
    ('int hoig_bad_pointer(const half *x);', 'hoig_bad_pointer'),     # an unknown pointee does not become c_void_p
    ('int hoig_bad_text(char *out);', 'hoig_bad_text'),               # only `const char *` is a string
    ('void hoig_bad_return(int n);', 'hoig_bad_return'),
    ('int hoig_bad_unnamed(long);', 'hoig_bad_unnamed'),
    ('static inline int hoig_body(int n) { return n; }', 'not a prototype'),
    ('#define HOIG_SHIFTED (1 << 3)', 'HOIG_SHIFTED'),
    ('enum { HOIG_IMPLICIT };', 'HOIG_IMPLICIT'),
    ('int hoig_twice(int n);\nint hoig_twice(int n);', 'hoig_twice'),
])
def test_parser_is_closed(decl, word):
    with pytest.raises((TypeError, ValueError), match=re.escape(word)):
        L.parse_header(decl)


def test_every_declared_entry_point_is_bound():
    text = open(L.HEADER_PATH).read()
    text = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    declared = set(re.findall(r'\b(hoig_[a-z0-9_]+)\s*\(', text))
    assert len(declared) >= 216
    assert declared == set(L._PROTOS) == set(L.declared_symbols())
    for name in declared:
        fn = getattr(L.lib, name)
        assert (fn.restype, list(fn.argtypes)) == L._PROTOS[name], name
    assert L._SIGS == {n: a for n, (r, a) in L._PROTOS.items() if r is I}
    assert len(L._SIGS) >= 187 and 'hoig_inorm_workspace_bytes' not in L._SIGS and 'hoig_version' not in L._SIGS


PINNED = {
    'hoig_conv2d_fwd': (I, [DESC, VP, VP, VP, VP, VP]),
    'hoig_conv2d_fwd_packed_normin': (I, [DESC, VP, I, VP, VP, VP, VP, VP, VP, I, VP, VP, VP]),
    'hoig_stream_create': (I, [ctypes.POINTER(VP)]),
    'hoig_set_tuning': (I, [ctypes.c_char_p, I]),
    'hoig_version': (ctypes.c_char_p, []),
    'hoig_conv_route_name': (ctypes.c_char_p, [I]),
    'hoig_rasterize_workspace_bytes': (ctypes.c_size_t, [I, I]),
    'hoig_inorm_workspace_bytes': (I64, [I, I, I]),
    'hoig_swd_positions': (I, [U64, I, I64, I, I, I, I, I, VP, VP]),
    'hoig_adam_step': (I, [VP, VP, VP, VP, I64, D, D, D, D, I, F, VP]),
    'hoig_png_deflate_host': (I, [VP, I64, I, I, I, VP, I64, VP, VP]),
    'hoig_conv2d_fwd_heads': (I, [DESC, VP, VP, VP, VP, U64, VP]),
    'hoig_loss_fwd_bwd': (I, [I, VP, VP, F, F, VP, VP, I64, VP]),
    'hoig_mano_lbs': (I, [VP] * 9 + [I, I] + [VP] * 5 + [I, VP, I, VP]),
    'hoig_stream_scratch_bytes': (I64, []),
}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_pinned_signatures(name):
    fn = getattr(L.lib, name)
    assert (fn.restype, list(fn.argtypes)) == PINNED[name]


CONSTANTS = dict(
    OK=0, EINVAL=-1, ELAUNCH=-2, EUNSUPPORTED=-3,
    ACT_NONE=0, ACT_RELU=1, ACT_LRELU=2, ACT_TANH=3, ACT_SIGMOID=4,
    PREC_F32=0, PREC_BF16X3=1, PREC_BF16=2, PREC_F16X2=3, PREC_F16F6=4,
    LOSS_L1=0, LOSS_MSE=1, LOSS_BCE=2, POOL_MAX=0, POOL_AVG=1,
    JPEG_SUBSEQ_BYTES=64, PNG_SEGMENT_BYTES=8192, GEMM_ACCUMULATE=1, GEMM_SYMMETRIC=2, GEMM_F32=4,
    FM_NONFINITE=1, FM_CLAMPED=2,
    PNG_ECODE=1, PNG_EBTYPE=2, PNG_ESTORED=4, PNG_EDIST=8, PNG_EEARLY=16, PNG_EMORE=32, PNG_ELESS=64, PNG_EFILTER=128,
    PNG_EADLER=256,
    DAUG_COLOR=1, DAUG_TRANSLATION=2, DAUG_CUTOUT=4, DAUG_STATE_WORDS=16, DAUG_MAX_PARTS=16,
    SWD_K=147, SWD_DEGENERATE=7, SORT_NAN=8, SORT_LDS_MAX=2048, SORT_TILE=4096,
    REGION_MAX=7, REGION_BAD_LABEL=1, GUARD_SKIP=1, GRAD_CHUNK=4096, GRAD_MAX_GRID=1024,
    ROUTE_FWD=0, ROUTE_DGRAD=1, ROUTE_WGRAD=2,
)


def test_constants_keep_their_values():
    got = {k: getattr(L, k, None) for k in CONSTANTS}
    assert got == CONSTANTS
    assert all(type(v) is int for v in got.values())
    # the three that the library also answers for
    assert L.lib.hoig_sort_segments_lds_max() == L.SORT_LDS_MAX and L.lib.hoig_sort_segments_tile() == L.SORT_TILE
    assert L.lib.hoig_grad_stats_chunk() == L.GRAD_CHUNK and L.lib.hoig_grad_stats_max_grid() == L.GRAD_MAX_GRID


def test_both_pointer_call_styles_pass():
    """byref() of a struct or of a c_int64 and a plain address both pass POINTER(ConvDesc) / c_void_p (the two places where the
    derived table is stricter / looser than the hand-written one was); no launch: the arguments are refused first."""
    d = L.ConvDesc(1, 8, 8, 4, 9, 9, 4, 3, 3, 1, 1, 0, 0, 0.0, 0)          # inconsistent output size
    assert L.lib.hoig_conv2d_fwd_packed_normin(ctypes.byref(d), None, 0, None, None, None, None, None, None, 0, None, None, None) \
        != L.OK
    size = ctypes.c_int64(-7)
    buf = (ctypes.c_uint8 * 64)()
    assert L.lib.hoig_png_deflate_host(buf, 64, 1000, 0, 0, buf, 64, ctypes.byref(size), None) == L.EINVAL and size.value == -7
    assert L.lib.hoig_png_deflate_host(buf, 64, 1000, 0, 0, buf, 64, ctypes.addressof(size), None) == L.EINVAL


@pytest.mark.parametrize('family', ['ops_norm', 'ops_small', 'ops_attn', 'ops_loss', 'ops_daug'])
def test_a_family_imported_first_leaves_no_incomplete_ops(family):
    code = ('import hoig_amd.%s\n'
            'from hoig_amd import ops\n'
            'missing = [n for n in ("instance_norm", "small_map_sums", "add", "local_attention", "l1_loss", "augment_cat")'
            ' if not hasattr(ops, n)]\n'
            'assert not missing, missing\n' % family)
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if out.returncode != 0:
        assert 'ImportError' in out.stderr and 'import hoig_amd.ops first' in out.stderr, out.stderr
