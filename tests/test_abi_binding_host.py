"""CPU: the ctypes binding is derived from include/hsp.h (megatts2_hierspeechpp_amd/_lib.py: parse_header).  The reader
on synthetic headers -- every form it accepts, every form it refuses -- hand-written expectations for one declaration of
each shape of the real header (rows the reader cannot satisfy by agreeing with itself), and the import-time errors."""
import ctypes as C
import importlib.util
import os
import shutil

import pytest

from megatts2_hierspeechpp_amd import _lib as L

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


# ------------------------------------------------------------------------------------------ accepted forms
def test_constants_enums_and_defines():
    consts, structs, protos = L.parse_header("""
        #ifndef HSP_H_
        #define HSP_H_          /* the include guard: a define without a value is no constant */
        #include <stdint.h>
        #define HSP_VERSION 104 /* a comment over
                                   two lines; with { and ; inside */
        #define HSP_EINVAL (-1)
        #define HSP_PLUS +7
        #  define HSP_SPACED ( 3 )
        // enum { HSP_NOT = 9 };
        enum {
          HSP_PRO_NONE = 0,
          HSP_PRO_LRELU = 1, /* F.leaky_relu */
          HSP_NEG = -2
        };
        enum { HSP_MASK_NONE = 0, HSP_MASK_PRE = 1 };
        #endif /* HSP_H_ */
    """)
    assert consts == {"HSP_VERSION": 104, "HSP_EINVAL": -1, "HSP_PLUS": 7, "HSP_SPACED": 3, "HSP_PRO_NONE": 0,
                      "HSP_PRO_LRELU": 1, "HSP_NEG": -2, "HSP_MASK_NONE": 0, "HSP_MASK_PRE": 1}
    assert structs == {} and protos == {}


def test_directives_and_the_extern_c_block_are_read_through():
    consts, structs, protos = L.parse_header("""
        #ifdef __cplusplus
        extern "C" {
        #endif
        #if defined(__GNUC__) || defined(__clang__)
        #pragma GCC visibility push(default)
        #endif
        int hsp_version(void);
        #ifdef __cplusplus
        }
        #endif
    """)
    assert protos == {"hsp_version": (C.c_int, [])} and consts == {} and structs == {}


def test_struct_members_in_both_typedef_forms():
    _, structs, _ = L.parse_header("""
        typedef struct hsp_a_args {
          /* input */
          const float* x;
          int64_t x_bs, x_cs, x_ts;
          const float *q, *k, *v;
          float* o;
          float *k_cache, *v_cache;
          void* workspace;
          const int64_t* lengths;
          int16_t* pcm;
          int32_t B;
          float eps;
          int flag;
          double d;
        } hsp_a_args;
        typedef struct {
          int32_t n;
          int64_t* codes;
        } hsp_b_args;
    """)
    assert list(structs) == ["hsp_a_args", "hsp_b_args"]
    a, b = structs["hsp_a_args"], structs["hsp_b_args"]
    assert issubclass(a, C.Structure) and a.__name__ == "hsp_a_args"
    assert a._fields_ == [("x", vp), ("x_bs", i64), ("x_cs", i64), ("x_ts", i64), ("q", vp), ("k", vp), ("v", vp), ("o", vp),
                          ("k_cache", vp), ("v_cache", vp), ("workspace", vp), ("lengths", vp), ("pcm", vp), ("B", i32),
                          ("eps", f32), ("flag", C.c_int), ("d", C.c_double)]
    assert b._fields_ == [("n", i32), ("codes", vp)]
    assert all(t is vp for n, t in a._fields_ if n in ("x", "q", "k", "v", "o", "workspace", "pcm"))   # `is`, not ==


def test_prototypes_of_every_parameter_kind():
    _, structs, protos = L.parse_header("""
        typedef struct { int32_t n; } hsp_s_args;
        int hsp_version(void);
        const char* hsp_arch(void);
        int64_t hsp_bytes(int32_t B, int64_t n);
        int hsp_run_f32(const float* x, int64_t x_bs, const int64_t* lengths, float gain, int16_t* out,
                        double* coefs, int32_t* pos,
                        void* stream);
        int hsp_two(const hsp_s_args* inv, const hsp_s_args *fwd, void* stream);
        int hsp_plan(const hsp_s_args* a, int32_t out4[4]);
    """)
    ps = C.POINTER(structs["hsp_s_args"])
    assert protos == {
        "hsp_version": (C.c_int, []),
        "hsp_arch": (C.c_char_p, []),
        "hsp_bytes": (i64, [i32, i64]),
        "hsp_run_f32": (C.c_int, [vp, i64, vp, f32, vp, vp, vp, vp]),
        "hsp_two": (C.c_int, [ps, ps, vp]),
        "hsp_plan": (C.c_int, [ps, C.POINTER(i32 * 4)]),
    }
    assert all(isinstance(args, list) for _, args in protos.values())


# ------------------------------------------------------------------------------------------------ refusals
REFUSED = [
    # (what, header text, a word of the offending declaration the message must carry)
    ("unknown member type", "typedef struct { size_t n; } hsp_x_args;", "size_t n"),
    ("by-value int16 member", "typedef struct { int16_t n; } hsp_x_args;", "int16_t n"),
    ("two-word type", "typedef struct { unsigned int n; } hsp_x_args;", "unsigned int n"),
    ("array member", "typedef struct { int32_t out4[4]; } hsp_x_args;", "out4"),
    ("bit-field", "typedef struct { int32_t flag : 1; } hsp_x_args;", "flag"),
    ("pointer to pointer", "typedef struct { float** rows; } hsp_x_args;", "rows"),
    ("struct pointer member", "typedef struct { int32_t n; } hsp_s_args; typedef struct { hsp_s_args* s; } hsp_x_args;",
     "hsp_s_args * s"),
    ("nested struct", "typedef struct { struct { int32_t a; } inner; int32_t b; } hsp_x_args;", "inner"),
    ("union", "typedef union { int32_t a; float b; } hsp_u_args;", "union"),
    ("plain struct declaration", "struct hsp_x_args { int32_t a; };", "struct hsp_x_args"),
    ("typedef of a scalar", "typedef int32_t hsp_index;", "hsp_index"),
    ("enum member without a value", "enum { HSP_A = 0, HSP_B };", "HSP_B"),
    ("enum value that is an expression", "enum { HSP_A = 1 << 3 };", "HSP_A"),
    ("named enum", "enum hsp_kind { HSP_A = 0 };", "hsp_kind"),
    ("function-like macro", "#define HSP_MAX(a, b) ((a) > (b) ? (a) : (b))", "HSP_MAX"),
    ("hex define", "#define HSP_MASK 0xff", "HSP_MASK"),
    ("define of another name", "#define OTHER 3", "OTHER"),
    ("unknown directive", "#undef HSP_VERSION", "undef"),
    ("unknown parameter type", "int hsp_f(size_t n, void* stream);", "size_t n"),
    ("unknown struct parameter", "int hsp_f(const hsp_missing_args* a, void* stream);", "hsp_missing_args"),
    ("struct by value", "typedef struct { int32_t n; } hsp_s_args; int hsp_f(hsp_s_args a);", "hsp_s_args a"),
    ("unnamed parameter", "int hsp_f(int32_t, void* stream);", "hsp_f"),
    ("function-pointer parameter", "int hsp_f(void (*done)(int), void* stream);", "done"),
    ("array of pointers parameter", "int hsp_f(float* rows[4]);", "rows"),
    ("empty parameter list", "int hsp_f();", "hsp_f"),
    ("foreign prefix", "int other_f(void);", "other_f"),
    ("unknown return type", "float hsp_f(void);", "hsp_f"),
    ("void return", "void hsp_f(void);", "hsp_f"),
    ("a variable", "extern int hsp_counter;", "hsp_counter"),
    ("a function body", "static inline int hsp_f(void) { return 0; }", "hsp_f"),
    ("a stray closing brace", "int hsp_version(void); }", "}"),
]


@pytest.mark.parametrize("what,text,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_name_the_declaration(what, text, word):
    with pytest.raises(L.HspError) as e:
        L.parse_header("#include <stdint.h>\nint hsp_version(void);\n" + text + "\nint hsp_last(void);\n")
    assert word in str(e.value), str(e.value)


# -------------------------------------------------------------------- the real header, against rows written by hand
def test_real_header_prototypes_of_each_shape():
    S, conv, sample = L.SIGNATURES, C.POINTER(L.Conv1dArgs), C.POINTER(L.SampleArgs)
    assert S["hsp_version"] == (C.c_int, [])
    assert S["hsp_arch"] == (C.c_char_p, [])
    assert S["hsp_loudness_workspace_bytes"] == (i64, [i32, i64])
    assert S["hsp_conv1d_mfma_plan"] == (C.c_int, [conv, C.POINTER(i32 * 4)])
    assert S["hsp_wn_layer_f32"] == (C.c_int, [conv, conv, conv, vp])
    assert S["hsp_loudness_coefs_f64"] == (C.c_int, [i32, vp])
    assert S["hsp_peak_int16"] == (C.c_int, [vp, i64, vp, f32, vp, i64, i32, i64, vp])
    assert S["hsp_duration_scaled_f32"] == (C.c_int, [vp, i64, vp, f32, vp, i64, vp, i32, i32, vp, i64, vp])
    assert S["hsp_dftseg_tables_f32"] == (C.c_int, [vp, vp])                       # host buffers, no stream
    assert S["hsp_mha_proj_supported"] == (C.c_int, [i32, i32, i32, i32])
    assert S["hsp_plm_embed_sample_f32"] == (C.c_int, [vp, i64, i64, i32, vp, i64, vp, i32, i32, vp, i32, vp, vp, i64, i64,
                                                       i32, i32, vp, i64, i64, i32, i32, sample, vp])   # 24 parameters
    for name, (res, args) in S.items():
        assert name.startswith("hsp_") and isinstance(args, list) and res in (C.c_int, i64, C.c_char_p), name


def test_real_header_struct_fields_written_out():
    assert L.SampleArgs._fields_ == [("temperature", f32), ("top_k", i32), ("top_p", f32), ("repetition_penalty", f32),
                                     ("seeds", vp), ("probs", vp), ("probs_bs", i64)]
    assert L.MhaArgs._fields_ == [
        ("q", vp), ("k", vp), ("v", vp), ("o", vp), ("q_bs", i64), ("k_bs", i64), ("v_bs", i64), ("o_bs", i64),
        ("B", i32), ("H", i32), ("D", i32), ("Tq", i32), ("Tk", i32), ("qk_scale", f32),
        ("mask_q", vp), ("mask_k", vp), ("rel_k", vp), ("rel_v", vp), ("window", i32),
        ("q_cs", i64), ("k_cs", i64), ("v_cs", i64), ("o_cs", i64), ("mask_dense", vp), ("mask_dense_bs", i64)]


def test_real_header_structs_have_their_python_names():
    names = {"hsp_conv1d_args": "Conv1dArgs", "hsp_mha_args": "MhaArgs", "hsp_mha_proj_args": "MhaProjArgs",
             "hsp_dftseg_args": "DftSegArgs", "hsp_cprod3_args": "Cprod3Args", "hsp_sample_args": "SampleArgs",
             "hsp_plm_decode_args": "PlmDecodeArgs", "hsp_plm_prefill_attn_args": "PlmPrefillAttnArgs",
             "hsp_prosody_args": "ProsodyArgs", "hsp_limiter_args": "LimiterArgs", "hsp_f0_edit_args": "F0EditArgs"}
    assert set(L.STRUCTS) == set(names)
    for cname, pyname in names.items():
        cls = getattr(L, pyname)
        assert cls is L.STRUCTS[cname] and cls.__name__ == pyname and cls.__doc__, cname


def test_real_header_constants():
    want = dict(VERSION=104, EINVAL=-1, PRO_NONE=0, PRO_LRELU=1, PRO_ACT1D=2, PRO_SILU=3, ACT_NONE=0, ACT_GELU_ERF=7,
                ACT_ACT1D=8, ROWS_PLAIN=0, ROWS_GATE_WN=1, ROWS_GATE_GLU=2, ROWS_SHUFFLE=3, MASK_NONE=0, MASK_PRE=1,
                MASK_POST=2, MASK_BOTH=3, MHA_TOK=0, MHA_MFMA_STREAM=3, MHA_ROW_STREAM=5, WSPEC_BLOCK=0, WSPEC_THREE=1,
                PLM_DECODE_SPLIT=12, PLM_PREFILL_MAX_N=65536, DFTSEG_TABLE_FLOATS=4160)
    for name, value in want.items():
        assert getattr(L, name) == value, name
    assert not hasattr(L, "H_")                                                   # the include guard is no constant


# ---------------------------------------------------------------------------------------- import-time errors
def _import_copy(tmp_path, header):
    """Import a copy of _lib.py whose checkout holds ``header`` (None: no header at all)."""
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    shutil.copy(os.path.join(os.path.dirname(L.__file__), "_lib.py"), pkg / "_lib.py")
    if header is not None:
        (tmp_path / "include").mkdir()
        (tmp_path / "include" / "hsp.h").write_text(header)
    spec = importlib.util.spec_from_file_location("_lib_copy", pkg / "_lib.py")
    spec.loader.exec_module(importlib.util.module_from_spec(spec))


def test_import_errors(tmp_path):
    real = open(L.HEADER_PATH).read()
    (tmp_path / "ok").mkdir()
    _import_copy(tmp_path / "ok", real)                                       # the copy itself imports
    cases = [("missing", None, os.path.join("include", "hsp.h")),
             ("unnamed", real.replace("int hsp_version(void);", "typedef struct { int32_t n; } hsp_new_args;\n"
                                      "int hsp_version(void);"), "hsp_new_args"),
             ("unbacked", "int hsp_version(void);\n", "hsp_conv1d_args")]
    for what, header, word in cases:
        (tmp_path / what).mkdir()
        with pytest.raises(RuntimeError) as e:
            _import_copy(tmp_path / what, header)
        assert type(e.value).__name__ == "HspError" and word in str(e.value), (what, str(e.value))
