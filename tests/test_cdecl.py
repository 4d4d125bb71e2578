"""CPU: mere_fusion_amd._cdecl on literal snippets, one per construct include/merefusion.h uses, and on declarations it must refuse.
(tests/test_abi.py holds what it makes of the real header against the library and the compiler.)"""
import os

import pytest

from conftest import ROOT
from mere_fusion_amd import _cdecl
from mere_fusion_amd._cdecl import CDeclError, parse


def test_it_imports_neither_ctypes_nor_torch():
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r); import _cdecl; assert 'ctypes' not in sys.modules and 'torch' not in sys.modules" % os.path.dirname(_cdecl.__file__)
    assert subprocess.run([sys.executable, "-S", "-c", code], capture_output=True, text=True).returncode == 0


def test_block_comments_even_with_parentheses_and_function_names():
    h = parse("/* mf_ghost(int a); calls mf_other(x, y) (see above) */\nint mf_real(int a); /* int mf_ghost2(void); */")
    assert h.functions == {"mf_real": ("int", [("int", "a")])}
    with pytest.raises(CDeclError, match="unterminated block comment"):
        parse("int mf_a(int a); /* no end")


def test_preprocessor_lines_and_extern_c_braces():
    h = parse('#ifndef X_H\n#define X_H\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n#define MF_K 3   /* (x) */\n  #define MF_LONG(a) \\\n     ((a) + 1)\n'
              'int mf_a(int n);\n#ifdef __cplusplus\n}\n#endif\n#endif\n')
    assert list(h.functions) == ["mf_a"] and not h.structs
    with pytest.raises(CDeclError, match="unbalanced"):
        parse("int mf_a(int n);\n}\n")
    with pytest.raises(CDeclError, match="unterminated"):
        parse('extern "C" {\nint mf_a(int n);\n')


def test_typedef_enum_and_bare_enum():
    h = parse("typedef enum mf_status { MF_OK = 0, MF_ERR = -1 /* bad (x) */ } mf_status;\ntypedef enum mf_p { A = 0, B = 1 } mf_p;\nenum { MF_C = 0, MF_D = 1 };\n"
              "mf_status mf_f(mf_p p, const mf_p* q);")
    assert h.enums == {"mf_status", "mf_p"} and h.functions["mf_f"] == ("mf_status", [("mf_p", "p"), ("const mf_p*", "q")])
    with pytest.raises(CDeclError, match="cannot classify"):
        parse("typedef enum { A } ;")
    with pytest.raises(CDeclError, match="cannot classify"):
        parse("enum mf_e { A } mf_e;")


def test_opaque_struct_typedef_and_handle_pointers():
    h = parse("typedef struct mf_x mf_x;\nint mf_x_create(int n, mf_x** out);\nvoid mf_x_destroy(mf_x* h);\nint mf_x_n(const mf_x* h);")
    assert h.opaque == {"mf_x"} and not h.structs
    assert h.functions == {"mf_x_create": ("int", [("int", "n"), ("mf_x**", "out")]), "mf_x_destroy": ("void", [("mf_x*", "h")]),
                           "mf_x_n": ("int", [("const mf_x*", "h")])}
    with pytest.raises(CDeclError, match="cannot classify"):
        parse("typedef struct mf_x mf_y;")
    with pytest.raises(CDeclError, match="unknown type 'mf_x'"):
        parse("void mf_x_destroy(mf_x* h);")                                    # used before anybody declared it


def test_named_and_anonymous_struct_typedefs():
    h = parse("typedef struct mf_t {\n    const char* name;   /* e.g. \"a.b\" */\n    const float* data;\n    int ndim;\n} mf_t;\n"
              "typedef struct {\n    int hidden;\n    float eps;\n} mf_cfg;\nint mf_f(const mf_cfg* cfg, const mf_t* w, mf_t* out);")
    assert h.structs == {"mf_t": [("name", "const char*", None), ("data", "const float*", None), ("ndim", "int", None)],
                         "mf_cfg": [("hidden", "int", None), ("eps", "float", None)]}
    assert list(h.structs) == ["mf_t", "mf_cfg"]                                # declaration order
    assert h.functions["mf_f"][1] == [("const mf_cfg*", "cfg"), ("const mf_t*", "w"), ("mf_t*", "out")]
    with pytest.raises(CDeclError, match="cannot classify"):
        parse("typedef struct mf_a { int x; } mf_b;")
    with pytest.raises(CDeclError, match="declared twice"):
        parse("typedef struct { int x; } mf_a;\ntypedef struct { int y; } mf_a;")
    with pytest.raises(CDeclError, match="empty struct"):
        parse("typedef struct { } mf_a;")
    with pytest.raises(CDeclError, match="cannot classify"):
        parse("typedef struct { struct { int x; } in; } mf_a;")               # nothing nested in our header


def test_several_declarators_on_one_line():
    h = parse("typedef struct mf_d {\n    float *bg_out, *torso_alpha, *deform;   /* outputs */\n    int cbuf, coff, c, h, w, halo;\n    const float *rays_o, *rays_d;\n"
              "    float bg_const, density_thresh;\n    int n_conv, conv_dim[8], conv_bias;\n} mf_d;")
    assert h.structs["mf_d"] == [("bg_out", "float*", None), ("torso_alpha", "float*", None), ("deform", "float*", None)] + [
        (n, "int", None) for n in ("cbuf", "coff", "c", "h", "w", "halo")] + [("rays_o", "const float*", None), ("rays_d", "const float*", None),
        ("bg_const", "float", None), ("density_thresh", "float", None), ("n_conv", "int", None), ("conv_dim", "int", 8), ("conv_bias", "int", None)]
    one_line = parse("typedef struct mf_g { int cbuf, coff, c, h, w, halo; } mf_g;")
    assert [f[0] for f in one_line.structs["mf_g"]] == ["cbuf", "coff", "c", "h", "w", "halo"]
    with pytest.raises(CDeclError, match="named twice"):
        parse("typedef struct { int a, b, a; } mf_a;")


def test_array_fields():
    h = parse("typedef struct mf_a { int64_t shape[4]; float frame_consts[50]; int offsets[ 33 ]; uint8_t* p; } mf_a;")
    assert h.structs["mf_a"] == [("shape", "int64_t", 4), ("frame_consts", "float", 50), ("offsets", "int", 33), ("p", "uint8_t*", None)]
    for bad in ("typedef struct { int a[]; } mf_a;", "typedef struct { int a[N]; } mf_a;", "typedef struct { int a[2][2]; } mf_a;", "int mf_f(int a[4]);"):
        with pytest.raises(CDeclError):
            parse(bad)


def test_prototypes_over_several_lines_and_every_pointer_shape():
    h = parse("int mf_f(const float* q, const float* k,\n             float* out, int batch,\n\n             void* stream);\n"
              "size_t mf_bytes(int batch, int n);\nconst char*   mf_err(void);\ndouble mf_flops(const void *p, char* name, uint16_t*  hi);\n"
              "int mf_heads(const float* const* heads, int64_t stride, uint32_t n, const int16_t* c, const double* m, double * s);")
    assert h.functions["mf_f"] == ("int", [("const float*", "q"), ("const float*", "k"), ("float*", "out"), ("int", "batch"), ("void*", "stream")])
    assert h.functions["mf_bytes"][0] == "size_t" and h.functions["mf_err"] == ("const char*", [])
    assert h.functions["mf_flops"] == ("double", [("const void*", "p"), ("char*", "name"), ("uint16_t*", "hi")])
    assert h.functions["mf_heads"][1] == [("const float* const*", "heads"), ("int64_t", "stride"), ("uint32_t", "n"), ("const int16_t*", "c"),
                                          ("const double*", "m"), ("double*", "s")]


def test_void_argument_list():
    assert parse("int mf_abi_version(void);").functions == {"mf_abi_version": ("int", [])}
    for bad in ("int mf_f();", "int mf_f(void, int a);", "int mf_f(void x);"):
        with pytest.raises(CDeclError):
            parse(bad)


@pytest.mark.parametrize("bad, names", [
    ("int mf_f(int);", "mf_f"),                                 # an argument without a name
    ("int mf_f(unsigned n);", "mf_f"),                          # a type the header does not use
    ("int mf_f(unsigned int n);", "mf_f"),
    ("int mf_f(long n);", "mf_f"),
    ("int mf_f(int n, ...);", "mf_f"),
    ("int mf_f(int (*cb)(int));", "mf_f"),                      # no function pointers
    ("int mf_f(int n)", "mf_f"),                                # the semicolon is missing
    ("int mf_f(int n) { return n; }", "return n"),              # a definition
    ("int mf_f(int n); int mf_f(int n);", "mf_f"),              # declared twice
    ("int mf_f(int n, float n);", "mf_f"),
    ("int mf_f(const n);", "mf_f"),
    ("int mf_f(int const);", "mf_f"),
    ("static int mf_f(int n);", "mf_f"),
    ("int mf_v;", "mf_v"),                                      # a variable
    ("typedef int mf_i;", "mf_i"),                              # a typedef of another kind
    ("struct mf_s { int a; };", "mf_s"),
    ("typedef struct { int a } mf_s;", "mf_s"),                 # the field's semicolon is missing
    ("typedef struct { mf_q* p; } mf_s;", "mf_q"),
    ("typedef struct { void v; } mf_s;", "mf_s"),
    ("int mf_f(int n); // trailing", "trailing"),               # no line comments in our header
])
def test_a_malformed_or_foreign_declaration_raises_and_is_named(bad, names):
    with pytest.raises(CDeclError, match=names):
        parse(bad)


def test_the_real_header_parses_whole():
    h = parse(open(os.path.join(ROOT, "include", "merefusion.h")).read())
    assert len(h.functions) >= 166 and len(h.structs) == 15 and h.enums == {"mf_status", "mf_precision"} and len(h.opaque) == 15
    assert h.functions["mf_s3fd_detect_tensors"][1][0] == ("const float* const*", "heads")
    assert h.functions["mf_wav2lip_create"] == ("int", [("const mf_tensor*", "weights"), ("int", "n_weights"), ("int", "precision"), ("mf_wav2lip**", "out")])
    assert h.structs["mf_nerf_torso_desc"][-3:] == [("bg_out", "float*", None), ("torso_alpha", "float*", None), ("deform", "float*", None)]
    assert "mf_wav2vec2_config" in h.structs and h.structs["mf_wav2vec2_config"][6] == ("conv_dim", "int", 8)
