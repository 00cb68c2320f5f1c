"""ctypes binding of libhsp.so (the C ABI declared in include/hsp.h).

The product path has no CPU or eager fallback: if the shared library is missing, or a
tensor is not an fp32 tensor on a ROCm device, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HSP_LIB", os.path.join(_HERE, "libhsp.so"))  # HSP_LIB: kernel A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hsp.h")   # the checkout's, as build.source_id finds it


class HspError(RuntimeError):
    pass


# ------------------------------------------------------------------ the reader of include/hsp.h
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_POINTEES = {*_SCALARS, "int16_t", "void"}     # a pointer to one of these travels as c_void_p
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}
_DEFINE = re.compile(r"# ?define (HSP_\w+)(?: ([-+]?\d+)| \( ?([-+]?\d+) ?\))?")
_DIRECTIVE = re.compile(r"# ?(include|ifdef|ifndef|if|endif|pragma)\b")
_TOP = re.compile(r' ?(?:(extern "C" \{)|(\})|enum \{([^{}]*)\} ;|typedef struct(?: \w+)? \{([^{}]*)\} (\w+) ;|([^;{}]+);)')
_PROTO = re.compile(r"(int|int64_t|const char \*) (\w+) \( (.*) \)")


def _declare(decl, structs, where):
    """One member line of a struct (``structs`` None) or one parameter of ``where``, its tokens one space apart:
    ``[const] T a , b`` or ``[const] T * p , * q`` (and, as a parameter, ``T v [ n ]``) -> [(name, ctype), ...]."""
    m = re.fullmatch(r"(?:const )?(\w+) (.+)", decl)
    base, declarators = (m[1], m[2].split(" , ")) if m else (None, [""])
    param, out = structs is not None, []
    for d in declarators:
        dm = re.fullmatch(r"(\* )?(\w+)(?: \[ (\d+) \])?", d)
        star, name, dim = dm.groups() if dm else (None, None, None)
        if star and not dim and base in _POINTEES:
            ctype = C.c_void_p
        elif star and not dim and param and base in structs:
            ctype = C.POINTER(structs[base])
        elif name and not star and not dim and base in _SCALARS:
            ctype = _SCALARS[base]
        elif name and not star and dim and param and base in _SCALARS:
            ctype = C.POINTER(_SCALARS[base] * int(dim))
        else:
            raise HspError(f"hsp.h: {where}: unsupported declaration {decl!r}")
        out.append((name, ctype))
    return out


def parse_header(text):
    """(consts, structs, protos) of the text of include/hsp.h: {HSP_NAME: int}, {hsp_x_args: ctypes.Structure class},
    {hsp_name: (restype, [argtypes])}.  It reads the forms the header uses -- anonymous enums and integer #defines;
    typedef structs of scalars and pointers; prototypes over scalars, pointers, struct pointers and ``int32_t v[n]`` --
    and raises HspError, naming the declaration, on anything else: nothing is skipped."""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    consts, structs, protos, body, depth, pos = {}, {}, {}, [], 0, 0
    for line in (" ".join(ln.split()) for ln in text.split("\n")):
        m = _DEFINE.fullmatch(line)
        if m and (m[2] or m[3]):
            consts[m[1]] = int(m[2] or m[3])
        elif line.startswith("#") and not m and not _DIRECTIVE.match(line):     # m without a value: the include guard
            raise HspError(f"hsp.h: unsupported directive {line!r}")
        elif not line.startswith("#"):
            body.append(line)
    src = " ".join(re.sub(r"([*(),;=\[\]{}])", r" \1 ", " ".join(body)).split())
    while pos < len(src):
        m = _TOP.match(src, pos)
        extern, close, enum, members, sname, decl = m.groups() if m else (None,) * 6
        depth += 1 if extern else -1 if close else 0
        if not m or depth < 0:
            raise HspError(f"hsp.h: cannot classify the declaration at {src[pos:pos + 120]!r}")
        pos = m.end()
        for item in enum.split(" , ") if enum is not None else ():
            em = re.fullmatch(r" ?(HSP_\w+) = ([-+]?\d+) ?", item)
            if not em:
                raise HspError(f"hsp.h: unsupported enum member {item!r}")
            consts[em[1]] = int(em[2])
        if sname:
            fields = [f for d in members.split(" ; ") if d.strip() for f in _declare(d.strip(), None, sname)]
            structs[sname] = type(sname, (C.Structure,), {"_fields_": fields})
        elif decl:
            pm = _PROTO.fullmatch(decl.strip())
            if not pm or not pm[2].startswith("hsp_"):
                raise HspError(f"hsp.h: not a prototype of an hsp_ function: {decl.strip()!r}")
            params = [] if pm[3] == "void" else [t for p in pm[3].split(" , ") for _, t in _declare(p, structs, pm[2])]
            protos[pm[2]] = (_RETURNS[pm[1]], params)
    return consts, structs, protos


# ------------------------------------------------------------------ the binding, built from the header at import
try:
    with open(HEADER_PATH) as _f:
        _CONSTS, STRUCTS, SIGNATURES = parse_header(_f.read())    # SIGNATURES: symbol -> (restype, argtypes)
except OSError as e:
    raise HspError(f"{HEADER_PATH}: the C header the binding is derived from cannot be read ({e})") from None
_unbound = set(STRUCTS)                                           # STRUCTS: C name -> class


def _struct(cname, doc):
    """The ctypes class of a struct of the header, claimed under a Python name (each struct exactly once)."""
    if cname not in _unbound:
        raise HspError(f"{HEADER_PATH} declares no struct {cname} (or it is bound twice)")
    _unbound.remove(cname)
    STRUCTS[cname].__doc__ = doc
    return STRUCTS[cname]


Conv1dArgs = _struct("hsp_conv1d_args", "Arguments of the fused conv launches -- field order is the ABI.")
MhaArgs = _struct("hsp_mha_args", "Arguments of hsp_mha_f32 / hsp_mha_plan.")
MhaProjArgs = _struct("hsp_mha_proj_args", "Arguments of hsp_mha_proj_f32: attention + output projection.")
DftSegArgs = _struct("hsp_dftseg_args", "Arguments of the hsp_dftseg_* transforms.")
Cprod3Args = _struct("hsp_cprod3_args", "Arguments of hsp_cprod3_f32.")
SampleArgs = _struct("hsp_sample_args", "Sampling controls of the PLM decision kernels.")
PlmDecodeArgs = _struct("hsp_plm_decode_args", "Arguments of hsp_plm_decode_layer_f32 / _pos_f32.")
PlmPrefillAttnArgs = _struct("hsp_plm_prefill_attn_args", "Arguments of hsp_plm_prefill_attn_f32.")
ProsodyArgs = _struct("hsp_prosody_args", "Arguments of hsp_prosody_encode_f32.")
LimiterArgs = _struct("hsp_limiter_args", "Arguments of hsp_limiter_f32.")
F0EditArgs = _struct("hsp_f0_edit_args", "Arguments of hsp_f0_edit_rows_f32.")
if _unbound:
    raise HspError(f"{HEADER_PATH}: no Python name is bound to {sorted(_unbound)}: add a _struct line above")
for _name, _cls in list(globals().items()):          # a class answers to its Python name (launch hooks report it)
    if isinstance(_cls, type) and issubclass(_cls, C.Structure):
        _cls.__name__ = _cls.__qualname__ = _name

# every enum member and integer #define of the header under its name without the HSP_ prefix: PRO_NONE, ACT_ACT1D,
# ROWS_SHUFFLE, MASK_POST, EINVAL, VERSION, MHA_TOK, WSPEC_THREE, DFTSEG_TABLE_FLOATS, PLM_PREFILL_MAX_N, ...
globals().update({k[len("HSP_"):]: v for k, v in _CONSTS.items()})

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libhsp.so once.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HspError(
                f"{LIB_PATH} not found: build the HIP kernels first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C megatts2_hierspeechpp_amd/csrc). "
                "There is no CPU fallback for the product path.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        kind = "invalid arguments" if code == EINVAL else f"hipError_t {code}"
        raise HspError(f"{what} failed: {kind}")


def call(name: str, *args) -> None:
    """One launch on the current stream: ``lib().<name>(*args, stream_ptr())``, its status checked under that name."""
    check(getattr(lib(), name)(*args, stream_ptr()), name)


def timed(hook, kind: str, launch, soft: bool = False):
    """The event bracket of a measured launch: ``launch()`` performs the C call and returns its status, checked under
    ``kind``; when ``hook`` (the caller's measurement hook, or None) is set it runs between two timing events on the
    current stream.  Without a hook no event is created.  ``soft``: a launch the library refuses with HSP_EINVAL is not
    an error and has no events.  Returns (status, ev_start, ev_end); the caller reports them to its hook."""
    e0 = e1 = None
    if hook is not None:
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
    rc = launch()
    if soft and rc == EINVAL:
        return rc, None, None
    check(rc, kind)
    if hook is not None:
        e1.record()
    return 0, e0, e1


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of an fp32 (or int) ROCm tensor; None passes through as NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HspError("libhsp kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
    return t.data_ptr()


def fptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is not None and t.dtype != torch.float32:
        raise HspError(f"expected float32, got {t.dtype}")
    return ptr(t)


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream
