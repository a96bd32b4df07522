"""The C-ABI library loads on a CPU-only host and exports every symbol include/camkifu_amd.h
declares (no compute call is made here: that needs a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "camkifu_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ck_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported():
    from camkifu_amd import capi
    capi.build()
    lib = ctypes.CDLL(capi.SO_PATH)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(capi.EXPORTS) == names


def _declared_params():
    """name -> number of parameters, by this file's own reading of the header"""
    src = open(os.path.join(ROOT, "include", "camkifu_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: 0 if params.strip() in ("", "void") else params.count(",") + 1
            for name, params in re.findall(r"\b(ck_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def test_every_export_is_called_with_the_types_the_header_declares():
    """capi.lib() reads the signatures from the header: no export is left to ctypes' defaults (an int for everything, which
    cuts a pointer passed as a Python int to 32 bits and cannot pass a double)"""
    from camkifu_amd import capi
    capi.build()
    L = capi.lib()
    counts = _declared_params()
    assert sorted(counts) == _declared()
    for name, n in counts.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    c = ctypes
    assert L.ck_mog2_apply.argtypes[4] is c.c_double
    assert L.ck_jpeg_probe.argtypes[1] is c.c_size_t
    assert L.ck_rng_set.argtypes[1] is c.c_uint64
    assert list(L.ck_debug_scratch_fill.argtypes) == [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p]
    assert tuple(L.ck_policy_watch.argtypes[4:6]) == (c.c_double, c.c_longlong)
    harvest = list(L.ck_harvest_patches.argtypes)
    assert harvest.count(c.c_uint32) == 1 and harvest.count(c.c_longlong) == 1
    assert L.ck_round10.restype is c.c_double
    assert L.ck_last_error.restype is c.c_char_p
    assert L.ck_stream.restype is c.c_void_p
    assert L.ck_ctx_destroy.restype is None
    assert L.ck_version.restype is c.c_int and len(L.ck_version.argtypes) == 0


def test_a_prototype_the_parser_cannot_map_is_an_error(tmp_path):
    from camkifu_amd import capi
    import pytest
    h = tmp_path / "odd.h"
    h.write_text("int ck_fine(int a, const float* b);\nint ck_odd(int a, float scale);\n")
    with pytest.raises(capi.CkError, match="ck_odd.*float scale"):
        capi._signatures(str(h))
    h.write_text("float ck_odd(int a);\n")
    with pytest.raises(capi.CkError, match="ck_odd.*float"):
        capi._signatures(str(h))


def test_header_constants_equal_the_python_side():
    """the enums of include/camkifu_amd.h (status codes, memory spaces, classifier modes) and their mirrors in capi.py"""
    from camkifu_amd import capi
    src = open(os.path.join(ROOT, "include", "camkifu_amd.h")).read()
    consts = {k: int(v) for body in re.findall(r"enum\s*\{([^}]*)\}", src) for k, v in re.findall(r"(CK_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)}
    assert {"CK_CNN_FP32", "CK_CNN_BF16", "CK_CNN_F16X2", "CK_CNN_F16Q8"} <= set(consts)
    mirrored = [k for k in consts if hasattr(capi, k)]
    assert len(mirrored) >= 6, mirrored
    for k in mirrored:
        assert getattr(capi, k) == consts[k], k
    assert capi.CK_CNN_DEFAULT == consts["CK_CNN_F16X2"]        # the f32-equivalent mode stays the default


def test_no_gpu_means_loud_failure():
    import pytest
    import torch
    from camkifu_amd import capi
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.CkError):
        capi.Context(0)


def test_product_never_imports_oracle():
    """the product path must not import, link or dlopen anything under oracle/"""
    pkg = os.path.join(ROOT, "camkifu_amd")
    bad = re.compile(r"(import\s+oracle|from\s+oracle|libck_oracle|ora_[a-z0-9_]+\s*\(|oracle[/\\.]oracle|ck_oracle\.h)")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", "Makefile")):
                txt = open(os.path.join(dp, f)).read()
                assert not bad.search(txt), os.path.join(dp, f)
