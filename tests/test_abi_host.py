"""The binding takes the C ABI from include/mgcn_hip.h (kgc-gcn_amd/_native.py: _parse_abi, _abi_defines), host only: the parser on a
header written here, what it refuses, the tree's header against five prototypes written out by hand, and the loaded library's
restype / argtypes against the parsed table."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'mgcn_hip.h')

I32, I64, U32, U64, F32, F64, PTR = (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float,
                                     ctypes.c_double, ctypes.c_void_p)

SYNTHETIC = """
/* prose that looks like a call: mgcn_in_prose(x) returns 0;
 * int mgcn_in_block_comment(int32_t a);
 */
typedef struct mgcn_ingest mgcn_ingest;
// int mgcn_after_slashes(int32_t a);
#define MGCN_SOME_BATCH 64 /* tensors per launch */
int mgcn_under_define(const int64_t n, const float *x_dev, void *stream);   // trailing: mgcn_in_trailing(void);
size_t mgcn_three_lines(int a, int32_t b, int64_t c, uint32_t d,
                        uint64_t e, size_t f,
                        float g, double h);
int mgcn_no_args(void);
void mgcn_void_return(mgcn_ingest *h);
const char *mgcn_name_of(const char *path, char *bytes_host, mgcn_ingest **out, const uint16_t *ee_dev,
                         const float *const *grads_host);
"""


def _loose(nat, text):
    stripped = re.sub(r'^[ \t]*#[^\n]*', ' ', nat._strip_comments(text), flags=re.M)
    return set(re.findall(r'\b(mgcn_\w+)\s*\(', stripped))


def test_parser_on_a_synthetic_header(pkg):
    nat = pkg._native
    assert nat._parse_abi(SYNTHETIC) == {
        'mgcn_under_define': (ctypes.c_int, [I64, PTR, PTR]),
        'mgcn_three_lines': (ctypes.c_size_t, [ctypes.c_int, I32, I64, U32, U64, ctypes.c_size_t, F32, F64]),
        'mgcn_no_args': (ctypes.c_int, []),
        'mgcn_void_return': (None, [PTR]),
        'mgcn_name_of': (ctypes.c_char_p, [ctypes.c_char_p, PTR, PTR, PTR, PTR]),
    }
    assert nat._abi_defines(SYNTHETIC) == {'MGCN_SOME_BATCH': 64}
    assert nat._abi_defines('/* #define MGCN_A 1 */\n// #define MGCN_B 2\n# define MGCN_C 3\n') == {'MGCN_C': 3}


@pytest.mark.parametrize('decl, names', [
    ('int mgcn_bad_scalar(int32_t a, long x);', ['mgcn_bad_scalar', 'long x']),
    ('int mgcn_bad_unsigned(unsigned int x);', ['mgcn_bad_unsigned', 'unsigned int x']),
    ('long mgcn_bad_return(void);', ['mgcn_bad_return', 'long']),
    ('int mgcn_bad_void(void x);', ['mgcn_bad_void', 'void x']),
    ('int mgcn_bad_array(const float x[4]);', ['mgcn_bad_array', 'x[4]']),
    ('int mgcn_bad_ptr_array(const float *x[4]);', ['mgcn_bad_ptr_array', 'x[4]']),
    ('int mgcn_bad_callback(void (*fn)(int32_t), void *stream);', ['mgcn_bad_callback']),     # strict pattern skips it, loose scan sees it
    ('int mgcn_bad_nested(int32_t (a));', ['mgcn_bad_nested']),
    ('int mgcn_bad_unterminated(int32_t a)\nint mgcn_fine(void);', ['mgcn_bad_unterminated']),
])
def test_parser_refuses_what_it_cannot_map(pkg, decl, names):
    nat = pkg._native
    with pytest.raises(nat.NativeError) as e:
        nat._parse_abi('int mgcn_before(void);\n' + decl + '\nint mgcn_after(void);\n')
    for n in names:
        assert n in str(e.value), str(e.value)
    assert 'mgcn_before' not in str(e.value) and 'mgcn_after' not in str(e.value)


def test_real_header(pkg):
    nat = pkg._native
    text = open(HEADER).read()
    table = nat._parse_abi(text)
    assert set(table) == _loose(nat, text) and len(table) > 90
    assert table == nat._SIGNATURES and nat.EXPORTS == tuple(sorted(table))
    # written out by hand from the header's text
    assert table['mgcn_last_error'] == (ctypes.c_char_p, [])
    assert table['mgcn_ingest_close'] == (None, [PTR])
    assert table['mgcn_conve_packed_bytes'] == (ctypes.c_size_t, [I32] * 5)
    assert table['mgcn_adam_step'] == (ctypes.c_int, [I64] + [PTR] * 6 + [F32, F32] + [F64] * 4 + [PTR])
    res, args = table['mgcn_dropout_apply']
    assert res is ctypes.c_int and len(args) == 11 and args[-5:] == [U64, U64, U32, F32, PTR]
    # the three host-only entry points whose out-parameters are plain addresses now: their wrappers pass ctypes.byref(...)
    assert table['mgcn_ingest_open'][1] == [ctypes.c_char_p] * 3 + [PTR]
    assert table['mgcn_csr_live_view_host'][1][-2:] == [PTR, PTR] and table['mgcn_filter_index_build'][1][-2:] == [PTR, PTR]


def test_missing_header_names_the_path(pkg, monkeypatch, tmp_path):
    nat = pkg._native
    missing = str(tmp_path / 'include' / 'mgcn_hip.h')
    monkeypatch.setattr(nat, '_HEADER_PATH', missing)
    with pytest.raises(nat.NativeError, match=re.escape(missing)):
        nat._read_header()


def test_built_library_is_bound_as_parsed(pkg):
    nat = pkg._native
    handle, table = nat.lib(), nat._parse_abi(open(HEADER).read())
    assert len(nat.EXPORTS) == len(table)
    for name in nat.EXPORTS:
        fn = getattr(handle, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == table[name][1], name
    defines = dict(re.findall(r'^#define (MGCN_[A-Z_]+) (\d+)', open(HEADER).read(), re.M))
    for const, macro in (('ABI_VERSION', 'MGCN_ABI_VERSION'), ('ADAM_CHUNK', 'MGCN_ADAM_CHUNK'), ('ADAM_BATCH', 'MGCN_ADAM_BATCH'),
                         ('QUERY_MAX_BATCH', 'MGCN_QUERY_MAX_BATCH')):
        value = getattr(nat, const)
        assert type(value) is int and value == int(defines[macro]), const
    assert handle.mgcn_abi_version() == nat.ABI_VERSION
