"""The C-ABI library loads on a GPU-less box and exports every symbol that
include/xaac_amd.h declares; argument errors follow the reference's error-code
convention.  No compute calls here."""
import ast
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import libxaac_amd
from libxaac_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HOST_HEADERS = ("xaac_parse.h",)  # the CPU front end's boundary: libxaac_amd/libxaac_host.so


def _declared_functions(host=False):
    names = set()
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):  # every header of the boundary
        if (h in HOST_HEADERS) != host:
            continue
        txt = open(os.path.join(ROOT, "include", h)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        names |= set(re.findall(r"\b(xaac_[a-z0-9_]+)\s*\(", txt))
    return sorted(names)


def test_library_exports_every_declared_symbol():
    lib = libxaac_amd.load_library()
    names = _declared_functions()
    assert "xaac_imdct_process_batch" in names and "xaac_create" in names and "xaac_hbe_cplx_anal_batch" in names
    for n in names:
        assert hasattr(lib, n), n


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_libraries_export_nothing_but_the_declared_symbols():
    """-fvisibility=hidden + XAAC_API (and libxaac_amd/csrc/exports.map for what the HIP front end forces visible): the
    dynamic symbol tables are the headers' function lists, no launch helpers, kernel handles or C++ names beside them"""
    from libxaac_amd import decoder
    libxaac_amd.load_library()
    decoder.load_host_library()
    assert _exported(libxaac_amd.library_path()) == _declared_functions()
    assert _exported(decoder.host_library_path()) == _declared_functions(host=True)


def test_host_library_exports_every_declared_symbol():
    """include/xaac_parse.h <-> libxaac_amd/libxaac_host.so (CPU only: loads and parses without a GPU)"""
    from libxaac_amd import decoder
    lib = decoder.load_host_library()
    names = _declared_functions(host=True)
    assert "xaac_parse_adts_frame" in names and "xaac_parse_sbr_side" in names and "xaac_sbr_state_init" in names
    for n in names:
        assert hasattr(lib, n), n


def test_version_string():
    assert b"gfx950" in libxaac_amd.load_library().xaac_version()


# Workspace sizes are part of the ABI (callers cache them, and an entry point refuses one byte less): the values the library gave
# before the layouts were stated once in xaac_abi.cpp, taken from that build for these counts.
WS_COUNTS = (-1, 0, 1, 2, 3, 64, 255, 8192)
WS_BYTES = {
    ("xaac_sbr_lp_workspace_bytes",): (0, 384, 10640, 20896, 31152, 656768, 2615664, 84017536),
    ("xaac_sbr_hq_workspace_bytes", 0): (0, 640, 21140, 41640, 62140, 1312640, 5228140, 167936640),
    ("xaac_sbr_hq_workspace_bytes", 1): (0, 640, 37540, 74440, 111340, 2362240, 9410140, 302285440),
    ("xaac_sbr_eld_workspace_bytes",): (0, 0, 8720, 16928, 25136, 525824, 2093552, 67240448),
    ("xaac_esbr_workspace_bytes",): (0, 0, 98304, 196608, 294912, 6291456, 25067520, 805306368),
    ("xaac_esbr_workspace_bytes_ratio", 0): (0, 0, 98304, 196608, 294912, 6291456, 25067520, 805306368),
    ("xaac_esbr_workspace_bytes_ratio", 1): (0, 0, 98304, 196608, 294912, 6291456, 25067520, 805306368),
    ("xaac_esbr_workspace_bytes_ratio", 2): (0, 0, 119808, 239616, 359424, 7667712, 30551040, 981467136),
    ("xaac_peak_limiter_workspace_bytes",): (0, 256, 4360, 8464, 12568, 262912, 1046776, 33620224),
}


def test_workspace_sizes_are_the_published_ones():
    lib = libxaac_amd.load_library()
    for (name, *rest), want in sorted(WS_BYTES.items()):
        fn = getattr(lib, name)
        got = tuple(int(fn(n, *rest)) for n in WS_COUNTS)
        assert got == want, (name, rest)


def test_null_and_bad_arguments_are_fatal_codes():
    lib = libxaac_amd.load_library()
    assert lib.xaac_create(None, 0, None) & 0x80000000
    assert lib.xaac_destroy(None) & 0x80000000
    assert lib.xaac_sync(None) & 0x80000000
    assert lib.xaac_imdct_process_batch(None, None) & 0x80000000
    # every batch entry point turns a missing context or descriptor into a fatal code before it looks at anything else
    import re
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("xaac_amd.h", "xaac_esbr.h", "xaac_hbe.h", "xaac_pvc.h"))
    names = set(re.findall(r"XAAC_API int32_t (xaac_\w+)\(xaac_ctx \*\w+, const \w+ \*\w+\);", text))
    assert len(names) >= 25 and "xaac_hbe_dft_apply_batch_run" in names and "xaac_esbr_sbr_process_batch" in names
    for n in sorted(names):
        fn = getattr(lib, n)
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        assert fn(None, None) & 0x80000000, n


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(libxaac_amd.XaacError) as e:
        libxaac_amd.XaacContext(0)
    assert e.value.code == 0xFFFF8002


def _header_text(h):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)


def _header_groups():
    """(device headers, host headers)"""
    hs = sorted(os.listdir(os.path.join(ROOT, "include")))
    return [h for h in hs if h not in HOST_HEADERS], [h for h in hs if h in HOST_HEADERS]


def test_registry_is_the_headers_struct_list():
    declared = set()
    for h in sum(_header_groups(), []):
        declared |= set(re.findall(r"^\}\s*(xaac_\w+);", _header_text(h), flags=re.M))
    assert len(declared) >= 73 and declared == set(abi.STRUCTS)
    assert all(cls.c_name == name for name, cls in abi.STRUCTS.items())


def test_struct_layouts_match_headers(tmp_path):
    """every mirror of libxaac_amd.abi against what a C compiler makes of the headers: sizeof, and the offset and size of every
    field the mirror names; one generated program per header group"""
    got, want = {}, {}
    for k, group in enumerate(_header_groups()):
        names = [n for h in group for n in re.findall(r"^\}\s*(xaac_\w+);", _header_text(h), flags=re.M)]
        body = []
        for n in names:
            body.append('printf("%s %%zu\\n", sizeof(%s));' % (n, n))
            want[n] = ctypes.sizeof(abi.STRUCTS[n])
            for f, _ in abi.STRUCTS[n]._fields_:
                body.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (n, f, n, f, n, f))
                want[n + "." + f] = (getattr(abi.STRUCTS[n], f).offset, getattr(abi.STRUCTS[n], f).size)
        src, exe = tmp_path / ("layout%d.c" % k), tmp_path / ("layout%d" % k)
        src.write_text("#include <stdio.h>\n#include <stddef.h>\n%s\nint main(void) {\n%s\nreturn 0; }\n"
                       % ("\n".join('#include "%s"' % h for h in group), "\n".join(body)))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        for line in subprocess.check_output([str(exe)], text=True).splitlines():
            key, *v = line.split()
            got[key] = int(v[0]) if len(v) == 1 else (int(v[0]), int(v[1]))
    assert len(want) > 700 and set(got) == set(want)
    assert {k: (got[k], want[k]) for k in want if got[k] != want[k]} == {}


def test_flag_row_names_match_the_headers_enum(tmp_path):
    """abi.SBR_FLAG_NAMES / abi.F_* / abi.SBR_FLAG_WORDS against enum xaac_sbr_flag of include/xaac_sbr.h, through both headers
    that hand the row on, and against the members xaac_sbr_side starts with"""
    from libxaac_amd import decoder
    enum = re.search(r"enum xaac_sbr_flag \{(.*?)\}", _header_text("xaac_sbr.h"), flags=re.S).group(1)
    declared = re.findall(r"XAAC_SBR_FLAG_(\w+)", enum)
    assert declared == list(abi.SBR_FLAG_NAMES) + ["WORDS"]           # every enumerator has its name here, in the enum's order
    body = "\n".join('printf("%%d\\n", (int)XAAC_SBR_FLAG_%s);' % n for n in declared)
    for k, h in enumerate(("xaac_parse.h", "xaac_amd.h")):
        src, exe = tmp_path / ("flags%d.c" % k), tmp_path / ("flags%d" % k)
        src.write_text('#include <stdio.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0; }\n' % (h, body))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
        assert got == [getattr(abi, "F_" + n) for n in abi.SBR_FLAG_NAMES] + [abi.SBR_FLAG_WORDS]
    assert got == list(range(8)) + [8]                                # the published row
    assert [f for f, _ in abi.SbrSide._fields_[:abi.SBR_FLAG_WORDS]] == [n.lower() for n in abi.SBR_FLAG_NAMES]
    assert all(getattr(decoder, "F_" + n) == getattr(abi, "F_" + n) for n in abi.SBR_FLAG_NAMES)


# The sizes of the states and side-info rows are ABI facts like the workspace sizes (device tensors and golden files are cut to
# them): the values libxaac_amd stated as literals before it read them off the mirrors.
SIZES = {
    "CORE_TOOLS_SIDE_BYTES": 1652, "CORE_TOOLS_STATE_BYTES": 516, "DRC_SIDE_WORDS": 33, "ESBR_ANA_STATE_WORDS": 322,
    "ESBR_PS_STATE_BYTES": 23048, "ESBR_PVC_SIDE_BYTES": 84, "ESBR_PVC_STATE_BYTES": 12656, "ESBR_SIDE_BYTES": 2036,
    "ESBR_STATE_BYTES": 38012, "ESBR_SYN_STATE_WORDS": 1282, "HBE_DFT_CFG_BYTES": 23648, "HBE_DFT_FULL_STATE_BYTES": 24120,
    "HBE_DFT_STATE_BYTES": 2568, "HBE_STATE_BYTES": 61232, "LIMITER_STATE_BYTES": 17328, "PS_FRAME_BYTES": 972,
    "PS_STATE_BYTES": 7764, "PVC_FRAME_BYTES": 40, "PVC_STATE_BYTES": 188, "QMF_ANA_ELD_STATE_WORDS": 324,
    "QMF_ANA_STATE_WORDS": 322, "QMF_SYN_ELD_STATE_WORDS": 1284, "QMF_SYN_STATE_WORDS": 1282, "SBR_ELD_STATE_BYTES": 4236,
    "SBR_FRAME_BYTES": 1072, "SBR_HEADER_BYTES": 336, "SBR_STATE_BYTES": 7300, "USAC_FAC_IN_WORDS": 402,
}


def test_sizes_are_the_published_ones():
    from libxaac_amd import decoder
    assert {k: v for k, v in vars(libxaac_amd).items() if k.endswith(("_BYTES", "_WORDS"))} == SIZES
    for k, v in vars(decoder).items():
        if k.endswith(("_BYTES", "_WORDS")):
            assert v == SIZES[k], k


def test_literal_layout_facts():
    assert ctypes.sizeof(abi.ImdctBatch) == 80   # 2 x int32 + 7 pointers + int32 (+ pad) + status pointer on LP64
    assert (abi.QmfAnaEldState.fp.offset, abi.QmfSynEldState.sixty4.offset) == (646, 2566)
    S, B = abi.LimiterState, abi.LimiterBatch
    assert (S.pre_smoothed_gain.offset, S.max_buf.offset, S.delayed_input.offset) == (32, 48, 1968)
    assert (ctypes.sizeof(B), B.stride.offset, B.pcm16.offset, B.workspace_bytes.offset) == (80, 16, 48, 72)


def test_entry_point_table_is_the_headers_prototype_list():
    """every XAAC_API int32_t f(xaac_ctx *, const T *) of the device headers is in the table under T's mirror, every other device
    function is listed with its own prototype, and bind() leaves POINTER(mirror) / c_int32 on the function objects"""
    text = "".join(_header_text(h) for h in _header_groups()[0])
    protos = dict(re.findall(r"XAAC_API int32_t (xaac_\w+)\(xaac_ctx \*\w+, const (\w+) \*\w+\);", text))
    assert len(protos) >= 39 and set(protos) == set(abi.BATCH_ENTRY_POINTS)
    assert sorted(set(abi.BATCH_ENTRY_POINTS) | set(abi.OTHER_ENTRY_POINTS)) == _declared_functions()
    lib = abi.bind(ctypes.CDLL(libxaac_amd.library_path()))   # a handle of its own: other tests rebind the shared one's functions
    for name, t in protos.items():
        assert abi.BATCH_ENTRY_POINTS[name] is abi.STRUCTS[t], name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and list(fn.argtypes) == [ctypes.c_void_p, ctypes.POINTER(abi.STRUCTS[t])], name
    with pytest.raises(ctypes.ArgumentError):
        lib.xaac_drc_apply_batch(None, ctypes.byref(abi.ImdctBatch()))   # a wrong descriptor type is caught


def test_names_bench_and_entry_module_use_resolve():
    """bench.py cannot run without a GPU: every libxaac_amd.NAME (and NAME of a submodule imported from it) that it and
    __graft_entry__.py mention exists"""
    import importlib
    seen = set()
    for f in ("bench.py", "__graft_entry__.py"):
        tree = ast.parse(open(os.path.join(ROOT, f)).read())
        alias = {"libxaac_amd": "libxaac_amd"}
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "libxaac_amd":
                for a in node.names:
                    seen.add((node.module, a.name))
                    alias[a.asname or a.name] = node.module + "." + a.name
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and ast.unparse(node.value) in alias:
                seen.add((alias[ast.unparse(node.value)], node.attr))
    assert len(seen) >= 12 and ("libxaac_amd", "PVC_FRAME_BYTES") in seen and ("libxaac_amd.decoder", "decode_streams") in seen
    for mod, name in sorted(seen):
        try:
            m = importlib.import_module(mod)
        except ImportError:
            continue   # `from libxaac_amd import X` made an alias of a plain name, checked under ("libxaac_amd", X)
        assert hasattr(m, name) or importlib.util.find_spec(mod + "." + name), (mod, name)


def test_call_helper_raises_the_named_error():
    """the check every XaacContext method shares, without a GPU: a context object whose handle is null"""
    ctx = libxaac_amd.XaacContext.__new__(libxaac_amd.XaacContext)
    ctx._lib, ctx._h = libxaac_amd.load_library(), None
    n = 2
    with pytest.raises(libxaac_amd.XaacError) as e:
        ctx.imdct_process_batch_host(np.zeros((n, 1024), np.int32), np.zeros((n, 2), np.uint8), np.zeros((n, 512), np.int32),
                                     np.zeros((n, 2), np.uint8), out32=np.zeros((n, 1024), np.int32))
    assert e.value.code == 0xFFFF8000 and str(e.value) == "xaac_imdct_process_batch_host failed: 0xFFFF8000"   # XAAC_FATAL_NULL_ARG
