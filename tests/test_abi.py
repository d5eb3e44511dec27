"""The C-ABI library: loads on a machine without a GPU, exports every symbol include/s360.h
declares, and its host-only entry points behave (no compute calls here)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from splatter360_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def _declared():
    txt = (ROOT / "include" / "s360.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    names = _declared()
    assert len(names) >= 11 and set(_lib.EXPORTS) == set(names)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.s360_abi_version() == _lib.ABI_VERSION
    assert lib.s360_error_string(0) == b"ok" and lib.s360_error_string(-2) == b"workspace too small"


def test_layout_is_monotone_and_aligned():
    prm = _lib.S360Params(P=1000, V=6, H=64, W=64, sh_degree=4, M=25, flags=1, max_instances=5000)
    lay = _lib.layout(prm)
    offs = [getattr(lay, n) for n, _ in _lib.S360Layout._fields_ if n not in ("total_bytes", "backward_bytes")]
    assert offs == sorted(offs) and all(o % 16 == 0 for o in offs)
    assert (lay.rec_b, lay.rec_c) == (lay.rec_a + 16, lay.rec_a + 32)
    assert lay.total_bytes > offs[-1] and lay.part_c >= lay.surv_count + 6 * 16 * 4 and lay.backward_bytes >= 5000 * 4 * 48
    assert C.sizeof(_lib.S360Params) == 48


def test_bad_arguments_are_rejected_before_any_gpu_work():
    lib = _lib.lib()
    bad = _lib.S360Params(P=10, V=9, H=64, W=64, sh_degree=4, M=25, flags=0, max_instances=100)
    out = _lib.S360Layout()
    assert lib.s360_layout(C.byref(bad), C.byref(out)) == -1
    ok = _lib.S360Params(P=10, V=1, H=64, W=64, sh_degree=4, M=25, flags=0, max_instances=100)
    # null views / images / workspace
    assert lib.s360_forward(C.byref(ok), None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.s360_cube2erp_forward(None, None, None, 3, 64, 128, 256, None, None, None) == -1
    # ABI v24: the stitch's adjoint takes the grid's inverse (plan offsets + entries); a missing plan is a bad argument
    assert _lib.ABI_VERSION == 25
    assert lib.s360_cube2erp_backward(None, None, None, None, None, 3, 64, 128, 256, None, None, None) == -1
    with pytest.raises(RuntimeError):
        _lib.check(-4, "x")


@pytest.mark.parametrize("flags", [_lib.FLAG_SHARED_CAMPOS, _lib.FLAG_SHARED_CAMPOS | _lib.FLAG_ATOMIC_GRADS,
                                   _lib.FLAG_SHARED_CAMPOS | _lib.FLAG_LEAN_LISTS | _lib.FLAG_SPLIT_LISTS])
def test_pair_records_accessor_is_aligned_fits_and_rejects_bad_arguments(flags):
    """s360_backward_pair_records (ABI v25): host arithmetic on an address it never dereferences, so any base will do.  The records
    start on a 256-byte boundary of the address and end inside backward_bytes, in the default and in the atomic layout."""
    lib = _lib.lib()
    prm = _lib.S360Params(P=1000, V=6, H=64, W=80, sh_degree=4, M=25, flags=flags, max_instances=5000)
    lay = _lib.layout(prm)
    offs = set()
    for base in (1 << 20, (1 << 20) + 16, (1 << 20) + 255):
        off = C.c_size_t(123)
        assert lib.s360_backward_pair_records(C.byref(prm), C.c_void_p(base), lay.backward_bytes, C.byref(off)) == 0
        assert (base + off.value) % 256 == 0
        assert off.value + prm.V * prm.P * 48 <= lay.backward_bytes
        offs.add(off.value)
    assert len(offs) == 3                                   # the offset belongs to the pointer it was asked for
    atomic = bool(flags & _lib.FLAG_ATOMIC_GRADS)
    assert (min(offs) < 5000 * 4 * 48) == atomic            # default layout: behind the [cap] x 4 partial records; atomic: no such block
    off = C.c_size_t(123)
    base = C.c_void_p(1 << 20)
    assert lib.s360_backward_pair_records(None, base, lay.backward_bytes, C.byref(off)) == -1
    assert lib.s360_backward_pair_records(C.byref(prm), None, lay.backward_bytes, C.byref(off)) == -1
    assert lib.s360_backward_pair_records(C.byref(prm), base, lay.backward_bytes, None) == -1
    assert lib.s360_backward_pair_records(C.byref(prm), base, lay.backward_bytes - 1, C.byref(off)) == -2
    fwd_only = _lib.S360Params(P=1000, V=6, H=64, W=80, sh_degree=4, M=25, flags=flags | _lib.FLAG_FORWARD_ONLY, max_instances=5000)
    assert lib.s360_backward_pair_records(C.byref(fwd_only), base, lay.backward_bytes, C.byref(off)) == -1
    bad_v = _lib.S360Params(P=1000, V=9, H=64, W=80, sh_degree=4, M=25, flags=flags, max_instances=5000)
    assert lib.s360_backward_pair_records(C.byref(bad_v), base, lay.backward_bytes, C.byref(off)) == -1
    assert off.value == 123                                 # a refused call writes nothing


def test_rasterizer_refuses_cpu_tensors():
    import torch
    from splatter360_amd import rasterizer
    views = torch.zeros(1, rasterizer.VIEW_FLOATS)
    with pytest.raises(RuntimeError):
        rasterizer.rasterize_views(torch.zeros(4, 3), torch.zeros(4, 6), torch.zeros(4), colors_precomp=torch.zeros(4, 3),
                                   views=views, image_height=16, image_width=16)
    with pytest.raises(Exception):
        rasterizer.rasterize_views(torch.zeros(4, 3), torch.zeros(4, 6), torch.zeros(4), views=views, image_height=16, image_width=16)


def test_header_is_plain_c_and_a_c_program_can_call_the_library(tmp_path):
    """examples/c_abi_layout.c is compiled as C99 with -pedantic against include/s360.h, linked to libs360.so and
    run: the boundary is a C ABI (no C++ / torch types), usable without Python, and the host-only entry points
    need no GPU."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    _lib.lib()
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "c_abi_layout"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{root / 'include'}", str(root / "examples" / "c_abi_layout.c"),
           f"-L{root / 'splatter360_amd'}", "-ls360", f"-Wl,-rpath,{root / 'splatter360_amd'}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"abi {_lib.ABI_VERSION} " in r.stdout and "bad V -> -1" in r.stdout


def test_ctypes_argtypes_match_the_header_prototypes():
    """Every function include/s360.h declares has an entry in _lib.SIGNATURES, and the loaded library carries it: the header's
    return type, as many parameters as the prototype (none for `void`), pointers where the header has pointers and sizes /
    integers / 64-bit integers / floats where it has those: a signature changed on one side only (the ABI moved twice in
    round 2) fails here, on CPU."""
    import ctypes as C
    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    lib = _lib.lib()
    restypes = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
    checked = set()
    for m in re.finditer(r"\b(int|size_t|const char\s*\*)\s+(s360_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        ret, name, params = re.sub(r"\s+\*", "*", m.group(1)), m.group(2), m.group(3).strip()
        assert name in _lib.SIGNATURES, f"{name}: declared in the header, missing in _lib.SIGNATURES"
        fn = getattr(lib, name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), f"{name}: lib() did not apply the table"
        assert restype is restypes[ret], f"{name}: header returns {ret}, ctypes {restype}"
        plist = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
        assert len(plist) == len(fn.argtypes), f"{name}: header has {len(plist)} parameters, ctypes {len(fn.argtypes)}"
        for p, a in zip(plist, fn.argtypes):
            is_ptr_h = "*" in p
            is_ptr_c = a in (C.c_void_p, C.c_char_p) or hasattr(a, "_type_") and isinstance(a._type_, type) and issubclass(a, C._Pointer)
            assert is_ptr_h == bool(is_ptr_c), f"{name}: parameter '{p}' vs ctypes {a}"
            if not is_ptr_h:
                if "float" in p:
                    assert a is C.c_float, f"{name}: '{p}' vs {a}"
                elif "size_t" in p:
                    assert a in (C.c_size_t, C.c_uint64), f"{name}: '{p}' vs {a}"
                elif "int64_t" in p:
                    assert a is C.c_int64, f"{name}: '{p}' vs {a}"
                else:
                    assert a in (C.c_int, C.c_int32, C.c_uint32), f"{name}: '{p}' vs {a}"
        checked.add(name)
    assert checked == set(_declared()) == set(_lib.SIGNATURES) and len(checked) >= 71


class _StubLibrary:
    """Stands in for the loaded library: every entry point records its arguments and returns `code`."""

    def __init__(self, code):
        self.code, self.calls = code, []

    def s360_error_string(self, code):
        return b"stub says no"

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or self.code


def test_call_helper_checks_the_status_and_names_the_entry_point(monkeypatch):
    """_call.invoke reaches the library through _lib.lib() at call time, returns on 0, and on another code raises RuntimeError
    naming the entry point with s360_error_string's text; ptr(None) is None (NULL for c_void_p and POINTER parameters)."""
    from splatter360_amd import _call
    ok = _StubLibrary(0)
    monkeypatch.setattr(_lib, "lib", lambda: ok)
    assert _call.invoke("s360_anything", 1, None, 2.5) is None
    assert ok.calls == [("s360_anything", (1, None, 2.5))]
    bad = _StubLibrary(-3)
    monkeypatch.setattr(_lib, "lib", lambda: bad)               # replaced after import: the helper must not have cached a handle
    with pytest.raises(RuntimeError, match=r"s360_forward_depth failed: stub says no \(-3\)"):
        _call.invoke("s360_forward_depth", 7)
    assert bad.calls == [("s360_forward_depth", (7,))] and len(ok.calls) == 1
    assert _call.ptr(None) is None


def test_native_calls_go_through_the_one_helper():
    """The package's sources: only _call.py takes a stream's handle, no module defines a pointer / stream / float32-check helper of
    its own (_call.py holds the one _check_cuda_f32), and none imports a private name from the cost volume."""
    sources = {f.name: f.read_text() for f in sorted((ROOT / "splatter360_amd").glob("*.py"))}
    assert "_call.py" in sources and len(sources) >= 20
    assert [n for n, s in sources.items() if "cuda_stream" in s] == ["_call.py"]
    defined = {n: sorted(set(re.findall(r"^\s*(?:def\s+(_ptr|_p|_stream|_check_cuda_f32)\b|(_ptr|_p|_stream|_check_cuda_f32)\s*=)", s, flags=re.M)))
               for n, s in sources.items()}
    defined = {n: sorted({a or b for a, b in d}) for n, d in defined.items() if d}
    assert defined == {"_call.py": ["_check_cuda_f32"]}, defined
    for n, s in sources.items():
        for m in re.finditer(r"^\s*from\s+\.cost_volume\s+import\s+(\([^)]*\)|[^\n]*)", s, flags=re.M):
            names = [x.strip().split(" as ")[0] for x in m.group(1).strip("()").split(",") if x.strip()]
            assert not [x for x in names if x.startswith("_")], f"{n} imports {names} from .cost_volume"


def test_native_sources_share_the_host_rules_and_the_tile_bookkeeping():
    """csrc/*.hip and csrc/*.h: the launch check and the grid bound live in s360_launch.h alone (besides it, hipGetLastError only
    clears the error of a failed attribute / occupancy query, in the three places named here), no translation unit keeps an
    alignment helper of its own, and the MFMA accumulator's vector type and row rule are defined once."""
    csrc = ROOT / "splatter360_amd" / "csrc"
    sources = {f.name: f.read_text() for f in sorted(list(csrc.glob("*.hip")) + list(csrc.glob("*.h")))}
    assert "s360_launch.h" in sources and len(sources) >= 25
    uses = {n: [ln.strip() for ln in s.splitlines() if "hipGetLastError" in ln] for n, s in sources.items() if n != "s360_launch.h"}
    uses = {n: u for n, u in uses.items() if u}
    assert {n: len(u) for n, u in uses.items()} == {"s360_device.h": 2, "s360_backward.hip": 1}, uses
    assert all("(void)hipGetLastError();" in ln for u in uses.values() for ln in u), uses
    assert [n for n, s in sources.items() if "0x7fffffffLL" in s] == ["s360_launch.h"]
    helpers = {n: re.findall(r"\w*aligned\w*\(const void", s) for n, s in sources.items() if n.endswith(".hip")}
    assert not {n: h for n, h in helpers.items() if h}, helpers
    typedefs = {n: len(re.findall(r"typedef\s+float\s+\w+\s+__attribute__\(\(ext_vector_type\(16\)\)\)", s)) for n, s in sources.items()}
    assert {n: c for n, c in typedefs.items() if c} == {"s360_device.h": 1}, typedefs
    rows = {n: s.count("(r & 3) + 8 * (r >> 2) + 4 * hf") for n, s in sources.items()}
    assert {n: c for n, c in rows.items() if c} == {"s360_device.h": 1}, rows


def test_loading_the_library_brings_torch_in_first():
    """libs360.so links the system libamdhip64; torch's wheel bundles its own.  Loaded before torch, the library would start
    a second HIP runtime in the process and every later launch on torch's streams fails (build() + smoke() in one process
    did exactly that).  lib() therefore imports torch before dlopen — checked in a fresh interpreter."""
    import subprocess
    import sys
    code = ("import sys; from splatter360_amd import _lib; assert 'torch' not in sys.modules; "
            "_lib.lib(); assert 'torch' in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
