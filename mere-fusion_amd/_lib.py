"""ctypes binding of include/merefusion.h (the C ABI of libmerefusion_hip.so).

Nothing of the ABI is restated here: the argument types of every entry point (SIGNATURES) and the mirrors of every struct (MfTensor, MfConv2dDesc, ...)
are computed from the header by _cdecl.parse, once per process, the first time lib() or one of those names is asked for.  One mapping rule:
  scalars           int and the enum types -> c_int; float, double, size_t, int64_t, uint32_t, uint8_t -> their ctypes twins
  characters        const char* and char* -> c_char_p
  mirrored structs  a pointer to a struct the header defines -> POINTER(its mirror), except the tables named in DEVICE_TABLES
  other pointers    data pointers, opaque handles, handle out-parameters, streams -> c_void_p; so is every pointer field of a struct
  return types      void -> None
The header cannot tell a host `const int*` from a device one, and call sites pass data_ptr() integers, ctypes arrays, byref(...) and None: c_void_p takes
all four.  A typed POINTER(struct) does not take an integer, so the two struct tables that live in DEVICE memory are listed by hand.

There is no CPU fallback anywhere in this package: if the library is missing or a call fails, a RuntimeError carrying mf_last_error() is raised.
"""
import ctypes as C
import os

from . import _cdecl

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmerefusion_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(HERE, "..", "include", "merefusion.h"))

MF_PREC_BF16 = 0
MF_PREC_BF16X3 = 1
MF_PREC_F16Q = 2
PRECISIONS = {"bf16": MF_PREC_BF16, "bf16x3": MF_PREC_BF16X3, "f16q": MF_PREC_F16Q}

MF_CROP_LINEAR = 0
MF_CROP_LANCZOS4 = 1
CROP_MODES = {"linear": MF_CROP_LINEAR, "lanczos4": MF_CROP_LANCZOS4}

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint8_t": C.c_uint8}
CLASS_NAMES = {"mf_wav2vec2_config": "MfWav2Vec2Config"}          # where CamelCase of the C name is not the name the package exports
# (function, argument): mf_crop_job tables in DEVICE memory -- written by one launch, read by the next, handed over as data_ptr() integers
DEVICE_TABLES = {("mf_avatar_lip_boxes", "jobs"), ("mf_crop_resize_u8", "jobs")}


def class_name(c_name):
    return CLASS_NAMES.get(c_name) or "".join(w.capitalize() for w in c_name.split("_"))


def _ctype(t, header, classes, what):
    """the mapping rule of the module docstring for one normalised C type; classes = None inside a struct (every pointer but a string is c_void_p)"""
    base = t.replace("const ", "").rstrip("*")
    if t.endswith("*"):
        if base == "char" and t.count("*") == 1:
            return C.c_char_p
        return C.POINTER(classes[base]) if classes and base in classes and t.count("*") == 1 else C.c_void_p
    if base in header.enums:
        return C.c_int
    if base not in SCALARS:
        raise RuntimeError(f"{HEADER_PATH}: no ctypes mapping for the type {t!r} of {what}")
    return SCALARS[base]


def derive(header):
    """(SIGNATURES, {class name: Structure subclass}) from a parsed header"""
    classes = {}
    for c_name, fields in header.structs.items():
        types = [(f, _ctype(t, header, None, f"{c_name}.{f}")) for f, t, _ in fields]
        classes[c_name] = type(class_name(c_name), (C.Structure,), {
            "__doc__": f"{c_name} of include/merefusion.h", "_fields_": [(f, t if n is None else t * n) for (f, t), (_, _, n) in zip(types, fields)]})
    signatures = {}
    for name, (ret, args) in header.functions.items():
        argtypes = [C.c_void_p if (name, a) in DEVICE_TABLES else _ctype(t, header, classes, f"{name}({a})") for t, a in args]
        signatures[name] = (None if ret == "void" else _ctype(ret, header, None, name), argtypes)
    missing = [d for d in DEVICE_TABLES if d[0] not in header.functions or d[1] not in [a for _, a in header.functions[d[0]][1]]]
    if missing:
        raise RuntimeError(f"{HEADER_PATH} declares no {missing}: DEVICE_TABLES is stale")
    return signatures, {cls.__name__: cls for cls in classes.values()}


def _derive_once():
    """parses the header and sets HEADER, SIGNATURES and the struct classes as module globals: once per process, never on a step's path"""
    if "SIGNATURES" not in globals():
        if not os.path.exists(HEADER_PATH):
            raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes signatures are derived from it, and this package has no other statement of the ABI.")
        with open(HEADER_PATH) as f:
            header = _cdecl.parse(f.read())
        signatures, classes = derive(header)
        globals().update(classes, HEADER=header, SIGNATURES=signatures)


def __getattr__(name):
    # HEADER, SIGNATURES and the Mf* classes exist once the header has been read; asking for one reads it
    if "SIGNATURES" not in globals() and (name in ("HEADER", "SIGNATURES") or name.startswith("Mf")):
        _derive_once()
        if name in globals():
            return globals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def tensor_array(state_dict):
    """(ctypes array of MfTensor, keep-alive list) for a {name: fp32 cpu tensor} dict."""
    import torch
    _derive_once()
    items = [(k.encode(), v.detach().to("cpu", torch.float32).contiguous()) for k, v in state_dict.items()
             if torch.is_tensor(v) and v.is_floating_point()]
    arr = (MfTensor * len(items))()
    for i, (k, v) in enumerate(items):
        arr[i].name, arr[i].data, arr[i].ndim = k, v.data_ptr(), v.dim()
        for d in range(min(v.dim(), 4)):
            arr[i].shape[d] = v.shape[d]
    return arr, items


def stream_ptr(device=None):
    """torch's current stream on `device` as the `void* stream` argument of an entry point"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is not built. Run `python -m mere_fusion_amd.build` (needs hipcc); "
                "this package has no CPU fallback.")
        _derive_once()
        # torch first: its wheel carries its own HIP / HSA runtime, and device buffers are torch's.  Loading this library
        # before torch would bring a second runtime (/opt/rocm) into the process, which then sees no device.
        import torch  # noqa: F401
        # MF_LIB_PATH: an alternative build of the same library (kernel ablation studies, tools/halo_ablate.sh)
        l = C.CDLL(os.environ.get("MF_LIB_PATH") or LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().mf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"merefusion {what} failed (status {rc}): {msg}")


_inited = set()
_device_inited = False          # read by placement.py: once HIP is up in this process, HIP_VISIBLE_DEVICES can no longer choose its GPU


def init_device(index):
    global _device_inited
    if index not in _inited:
        check(lib().mf_init(int(index)), "mf_init")
        _inited.add(index)
        _device_inited = True
