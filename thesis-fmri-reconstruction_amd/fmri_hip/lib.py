"""ctypes binding of libfmri_hip.so (C ABI: include/fmri_hip.h and the headers it includes, ``EXT_HEADERS``).

There is no fallback: if the shared library is missing or a kernel returns an error the caller gets a
RuntimeError.  PyTorch is used only as the allocator / stream provider (tensor.data_ptr(),
torch.cuda.current_stream()).
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FMRI_LIB_PATH: another build of the same library (A/B timing of two builds in one job)
LIB_PATH = os.environ.get("FMRI_LIB_PATH") or os.path.join(_HERE, "libfmri_hip.so")

HEADER_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "include", "fmri_hip.h"))

_CTYPES = {"int": C.c_int, "int32_t": C.c_int, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double}
_INT = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))"


def _ctype(decl):
    """ctypes type of a C return type or parameter ('int64_t', 'const float* x'); None when the table has no row."""
    if "*" in decl:
        return C.c_char_p if re.fullmatch(r"(?:const\s+)?char\s*\*\s*\w*", decl) else C.c_void_p
    m = re.fullmatch(r"(?:const\s+)?(\w+)(?:\s+\w+)?", decl)
    return _CTYPES.get(m[1]) if m else None


def read_header(text):
    """The C ABI as include/fmri_hip.h states it: (name -> argtypes, name -> restype, FMRI_* constant -> int).
    Every file-scope ``RET fmri_name(ARGS);`` is an entry point (the ``static inline`` helpers are not); a declaration
    whose shape or types are not understood raises -- a guessed prototype would hand a kernel shifted arguments."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    const = {m[1]: int(m[2], 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(FMRI_\w+)[ \t]+" + _INT +
                                                     r"[uUlL]*[ \t]*$", text, re.M)}
    const.update((m[1], int(m[2], 0)) for m in re.finditer(r"\b(FMRI_\w+)\s*=\s*" + _INT + r"\s*[,}]", text))
    sigs, ret = {}, {}
    for stmt in re.split(r"[;{}]", re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)):
        found = re.search(r"\bfmri_[a-z0-9_]+(?=\s*\()", stmt)
        if not found or stmt.lstrip().startswith("static"):
            continue
        name, stmt = found[0], " ".join(stmt.split())
        m = re.fullmatch(r"([\w *]+?)\b(fmri_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        if not m or m[2] != name or name in sigs:
            raise RuntimeError(f"include/fmri_hip.h: cannot read the declaration of {name} (or it is a second one): `{stmt}`")
        decls = [m[1].strip()] + ([] if m[3].strip() == "void" else [a.strip() for a in m[3].split(",")])
        types = [_ctype(d) for d in decls]
        if None in types:
            raise RuntimeError(f"include/fmri_hip.h: no ctypes type for `{decls[types.index(None)]}` in the declaration "
                               f"of {name}: `{stmt}`")
        ret[name], sigs[name] = types[0], types[1:]
    return sigs, ret, const


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes prototypes of libfmri_hip.so are read from it.")
with open(HEADER_PATH) as _f:
    _SIGS, _RET, CONST = read_header(_f.read())     # name -> argtypes, name -> restype, FMRI_* -> int
EXPORTS = sorted(_SIGS)
# Headers that fmri_hip.h includes, read the same way (name -> header file).  They are kept in tables of their own because
# tests/test_abi.py pins ``_SIGS`` / ``EXPORTS`` to the entry points fmri_hip.h itself declares, by number; an entry point
# added since goes into an included header (one line here) and is looked up through ``prototype``.
EXT_HEADERS = ("fmri_hip_contrast.h",)
_EXT_SIGS, _EXT_RET, EXT_EXPORTS = {}, {}, {}
for _h in EXT_HEADERS:
    _path = os.path.join(os.path.dirname(HEADER_PATH), _h)
    if not os.path.exists(_path):
        raise RuntimeError(f"{_path} is missing: include/fmri_hip.h includes it and the ctypes prototypes are read from it.")
    with open(_path) as _f:
        _s, _r, _c = read_header(_f.read())
    if set(_s) & (set(_SIGS) | set(_EXT_SIGS)):
        raise RuntimeError(f"include/{_h}: declares {sorted(set(_s) & (set(_SIGS) | set(_EXT_SIGS)))} a second time")
    _EXT_SIGS.update(_s)
    _EXT_RET.update(_r)
    CONST.update(_c)
    EXT_EXPORTS.update({n: _h for n in _s})


def prototype(name):
    """(argtypes, restype) of an entry point, whichever header declares it."""
    if name in _SIGS:
        return _SIGS[name], _RET[name]
    return _EXT_SIGS[name], _EXT_RET[name]


class Epilogue(C.Structure):
    """``fmri_epilogue`` of include/fmri_hip.h (BatchNorm statistics out of a contraction's epilogue)."""
    _fields_ = [("stat_part", C.c_void_p), ("stat_rows_cap", C.c_int32), ("stat_group_n", C.c_int32),
                ("bn_x", C.c_void_p), ("bn_gamma", C.c_void_p), ("bn_beta", C.c_void_p),
                ("bn_mean", C.c_void_p * 4), ("bn_rstd", C.c_void_p * 4), ("bn_x_img0", C.c_int32 * 4),
                ("bn_relu", C.c_int32), ("reserved", C.c_int32), ("act_y", C.c_void_p),
                ("aff_scale", C.c_void_p), ("aff_shift", C.c_void_p), ("aff_relu", C.c_int32), ("reserved2", C.c_int32)]


class WgradPlan(C.Structure):
    """``fmri_wgrad_plan`` of include/fmri_hip.h (what fmri_wgrad_route plans for a weight-gradient geometry)."""
    _fields_ = [("atomic", C.c_int32), ("splits", C.c_int32), ("slabs", C.c_int32), ("zeroed", C.c_int32),
                ("stored", C.c_int32), ("colsum", C.c_int32), ("pieces", C.c_int32 * 4), ("kernel", C.c_char * 64)]


class StatSeg(C.Structure):
    """``fmri_stat_seg`` of include/fmri_hip.h (one segment of fmri_tensor_stats)."""
    _fields_ = [("x", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int64), ("ld", C.c_int64), ("div", C.c_void_p),
                ("gate", C.c_void_p), ("out", C.c_void_p), ("scale", C.c_float), ("clamp", C.c_float)]


class StateSeg(C.Structure):
    """``fmri_state_seg`` of include/fmri_hip.h (one segment of a training-state slot)."""
    _fields_ = [("live", C.c_void_p), ("offset", C.c_int64), ("bytes", C.c_int64), ("chunk0", C.c_int64)]


class EmaSeg(C.Structure):
    """``fmri_ema_seg`` of include/fmri_hip.h (one (live, shadow) pair of a weight-average table)."""
    _fields_ = [("live", C.c_void_p), ("shadow", C.c_void_p), ("n", C.c_int64), ("chunk0", C.c_int64)]


class Schedule(C.Structure):
    """``fmri_schedule`` of include/fmri_hip.h (the device-resident state of an epoch-end schedule)."""
    _fields_ = [("lr_base", C.c_double * 4), ("margin_base", C.c_double), ("equilibrium_base", C.c_double),
                ("lambda_mse_base", C.c_double), ("lr_gamma", C.c_double), ("decay_margin", C.c_double),
                ("decay_equilibrium", C.c_double), ("decay_mse", C.c_double), ("lr", C.c_double * 4),
                ("margin", C.c_double), ("equilibrium", C.c_double), ("lambda_mse", C.c_double),
                ("lr_step", C.c_int64), ("applied_epoch", C.c_int64)]


SCHED_MAX_LR = CONST["FMRI_SCHED_MAX_LR"]
STATE_MAGIC = CONST["FMRI_STATE_MAGIC"]
STATE_HEADER = CONST["FMRI_STATE_HEADER"]
STATE_CHUNK = CONST["FMRI_STATE_CHUNK"]
EMA_CHUNK = CONST["FMRI_EMA_CHUNK"]            # floats
STAT_BYTES = 32                                # sizeof(fmri_stat): the header has no macro for it
STAT_MAX_SEGS = CONST["FMRI_STAT_MAX_SEGS"]
EP_ACT_APPLIED = CONST["FMRI_EP_ACT_APPLIED"]
EP_AFFINE_APPLIED = CONST["FMRI_EP_AFFINE_APPLIED"]

_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m fmri_hip.build` (hipcc --offload-arch=gfx950). "
            "The engine has no CPU / eager fallback.")
    lib = C.CDLL(LIB_PATH)
    for name in list(_SIGS) + list(_EXT_SIGS):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = prototype(name)
    _lib = lib
    return lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """Raw handle of torch's current stream on the current device (the fast private accessor when torch has it:
    ``torch.cuda.current_stream()`` costs ~8 us per call, which adds up over ~370 launches per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def check(code, what=""):
    if code != 0:
        msg = load().fmri_last_error_string(code).decode()
        raise RuntimeError(f"fmri_hip: {what} failed: {msg} ({code})")


# bench.py sets PROFILE to a list: every entry-point call is then bracketed by HIP events on the stream it is launched
# on and recorded as (entry point, note, start event, end event).  ``note(...)`` attaches what the caller knows about the
# NEXT call -- the kernel the library routes the geometry to, its algorithmic FLOPs and bytes -- so that bench.py can
# group launches into kernel families and price them against their rooflines.
PROFILE = None
_NOTE = None


def note(**kw):
    global _NOTE
    if PROFILE is not None:
        _NOTE = kw


def call(name, *args):
    """Invoke an entry point on torch's current stream and raise on error."""
    global _NOTE
    lib = load()
    if PROFILE is None:
        code = getattr(lib, name)(*args, stream())
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        code = getattr(lib, name)(*args, stream())
        e1.record()
        PROFILE.append((name, _NOTE, e0, e1))
        _NOTE = None
    if code != 0:
        check(code, name)


def tconv_class(k, pad, cy, cx, ci, rows_pad):
    lib = load()
    py, px, th, tw, kpad = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    woff = C.c_int64()
    check(lib.fmri_tconv_class(k, pad, cy, cx, ci, rows_pad, *map(C.byref, (py, px, th, tw, kpad, woff))),
          "fmri_tconv_class")
    return dict(py=py.value, px=px.value, th=th.value, tw=tw.value, kpad=kpad.value, w_off=woff.value)


def kpad(taps, ci):
    return load().fmri_kpad(taps, ci)
