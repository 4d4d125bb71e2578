"""CPU: the C-ABI library builds, loads, and exports every symbol include/merefusion.h declares; the ctypes signatures and struct mirrors
that _lib derives from the header match what the C compiler makes of the same header.
No compute is attempted without a GPU; error paths that need no device are exercised."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT


def test_header_symbols_exported(lib_built):
    from mere_fusion_amd import _lib
    lib = C.CDLL(lib_built)
    names = sorted(_lib.HEADER.functions)
    assert len(names) >= 14 and all(n.startswith("mf_") for n in names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in merefusion.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and header disagree"
    for n, (ret, args) in _lib.HEADER.functions.items():
        restype, argtypes = _lib.SIGNATURES[n]
        assert len(argtypes) == len(args) and (restype is None) == (ret == "void"), n
        for (t, a), ct in zip(args, argtypes):                              # a pointer travels as a pointer, a scalar as the scalar of its own width and kind
            is_ptr = ct in (C.c_void_p, C.c_char_p) or issubclass(ct, C._Pointer)
            assert is_ptr == t.endswith("*"), (n, a, t, ct)
            if not is_ptr:
                assert ct is {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64,
                              "uint32_t": C.c_uint32}[t], (n, a, t, ct)
    assert _lib.lib().mf_abi_version() == 4
    fn = _lib.lib().mf_gemm_bt_forward                                       # what lib() installed is the table
    assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES["mf_gemm_bt_forward"][1] and fn.argtypes[8] is C.c_int64


def test_every_exported_class_keeps_its_name():
    from mere_fusion_amd import _lib
    want = {"MfTensor", "MfConv2dDesc", "MfUnetConfig", "MfNerfFieldConfig", "MfNerfTorsoConfig", "MfNerfFrameDesc", "MfNerfBgDesc", "MfNerfTorsoDesc",
            "MfNerfOutDesc", "MfVaeConfig", "MfWav2Vec2Config", "MfRowsGeom", "MfPasteJob", "MfFrameSrc", "MfCropJob"}
    assert {_lib.class_name(c) for c in _lib.HEADER.structs} == want
    for name in want:
        assert issubclass(getattr(_lib, name), C.Structure) and getattr(_lib, name).__name__ == name


def test_stream_ptr_hands_over_the_current_stream_of_the_device(monkeypatch):
    from types import SimpleNamespace
    from mere_fusion_amd import _lib
    asked = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: asked.append(device) or SimpleNamespace(cuda_stream=0x7F00DEAD0000 if device else 0))
    p = _lib.stream_ptr("cuda:1")
    assert isinstance(p, C.c_void_p) and p.value == 0x7F00DEAD0000 and _lib.stream_ptr().value is None and asked == ["cuda:1", None]


def _host_compiler():
    """the compiler the build uses (hipcc compiles plain C++ for the host), else a C compiler of the system"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")                   # as mere_fusion_amd.build finds it
    if shutil.which(hipcc):
        return [hipcc, "-x", "c++"]
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    return [cc, "-x", "c"] if cc else None


def test_struct_layouts_are_the_compiler_s(tmp_path):
    """sizeof and every offsetof, printed by a program that includes the header, against the ctypes mirrors"""
    from mere_fusion_amd import _lib
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host compiler found (neither hipcc nor cc / gcc / clang)")
    structs = _lib.HEADER.structs
    assert len(structs) == 15
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "merefusion.h"', 'int main(void) {']
    for c_name, fields in structs.items():
        lines.append(f'    printf("{c_name} sizeof %zu\\n", sizeof({c_name}));')
        lines += [f'    printf("{c_name} {f} %zu %zu\\n", offsetof({c_name}, {f}), sizeof((({c_name}*)0)->{f}));' for f, _, _ in fields]
    src = tmp_path / "layout_probe.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    exe = tmp_path / "layout_probe"
    subprocess.run(cc + [str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    want = []
    for c_name, fields in structs.items():
        cls = getattr(_lib, _lib.class_name(c_name))
        assert [f for f, _ in cls._fields_] == [f for f, _, _ in fields], c_name
        want.append([c_name, "sizeof", str(C.sizeof(cls))])
        want += [[c_name, f, str(getattr(cls, f).offset), str(getattr(cls, f).size)] for f, _, _ in fields]
    assert got == want
    assert sum(len(f) for f in structs.values()) + len(structs) == len(got) > 130


def test_errors_without_device(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    assert l.mf_melspec_frames(16640) == 84 and l.mf_melspec_frames(7040) == 36 and l.mf_melspec_frames(48000) == 241
    if not torch.cuda.is_available():
        rc = l.mf_init(0)
        assert rc == -3 and b"no HIP device" in l.mf_last_error()
    # null handle -> MF_ERR_INVALID, never a crash
    assert l.mf_wav2lip_forward(None, None, None, None, 1, None) == -1
    assert b"null" in l.mf_last_error()
    assert l.mf_melspec(None, 10, None, 0, None) == -1 and l.mf_melspec(None, 0, None, 0, None) == -1


def test_product_refuses_cpu_tensors(lib_built, sd0):
    from mere_fusion_amd.wav2lip.models import Wav2Lip
    m = Wav2Lip()
    missing, unexpected = m.load_state_dict(sd0)
    assert not missing and not unexpected
    assert sorted(m.state_dict().keys()) == sorted(sd0.keys())
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 1, 80, 16), torch.zeros(1, 6, 96, 96))
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.zeros(1, 1, 80, 16), torch.zeros(1, 6, 96, 96))


def test_product_never_imports_oracle():
    """The product path must not route through the oracle (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "mere-fusion_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "oracle/" not in src or f.endswith(".md"), f


def test_dropin_import_paths(lib_built):
    """The two imports the reference makes (lipreal.py:25, lipasr.py:10) resolve to this repository when
    mere-fusion_amd/dropin precedes the reference on sys.path."""
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = [%r, %r]; "
            "from wav2lip.models import Wav2Lip; from wav2lip import audio; "
            "import mere_fusion_amd.wav2lip.models as M; "
            "assert Wav2Lip is M.Wav2Lip and hasattr(audio, 'melspectrogram'); print('ok')"
            % (os.path.join(ROOT, "mere-fusion_amd", "dropin"), ROOT))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr
