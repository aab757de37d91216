"""ABI 0.2.15 (additive): the multi-column big fronts of the multi-right-hand-side solve, without a GPU.

The three entry points exist in the built library, the ctypes mirror of `struct madipm_ldl_multi_big_info` has the
header's fields in the header's order (4 + 4 + 8 + 8 = 24 bytes), and `struct madipm_ldl_multi_info` is what it
was."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "madipm_hip.h")
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64}


def _header_struct(name):
    """[(field, ctype)] of `struct name { ... };` in the header (scalar int32_t / int64_t fields)."""
    text = open(HEADER).read()
    body = re.search(r"struct %s \{(.*?)\n\};" % re.escape(name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(m.group(2), CTYPES[m.group(1)]) for m in re.finditer(r"(int32_t|int64_t)\s+(\w+)\s*;", body)]


def test_symbols_exist():
    from madipm_amd import _lib as L
    for name in ("madipm_ldl_set_multi_big", "madipm_ldl_multi_big_info", "madipm_solver_multi_big_info"):
        assert hasattr(L.lib, name), name
    assert L.madipm_version() == 203       # additive: the version number of the 0.2 line stays
    text = open(HEADER).read()
    for name in ("madipm_ldl_set_multi_big", "madipm_ldl_multi_big_info", "madipm_solver_multi_big_info"):
        assert re.search(r"\bint %s\(" % name, text), name
    assert "ABI 0.2.15" in text


def test_struct_layout_is_the_header_s():
    from madipm_amd import _lib as L
    want = _header_struct("madipm_ldl_multi_big_info")
    assert [f for f, _ in want] == ["multi_big", "n_big_levels", "n_big_passes", "big_bytes"]
    assert list(L.LDLMultiBigInfo._fields_) == want
    assert C.sizeof(L.LDLMultiBigInfo) == 24
    offs = [getattr(L.LDLMultiBigInfo, f).offset for f, _ in want]
    assert offs == [0, 4, 8, 16]


def test_the_old_struct_did_not_change():
    from madipm_amd import _lib as L
    want = _header_struct("madipm_ldl_multi_info")
    assert [f for f, _ in want] == ["width", "native", "n_calls", "n_chunks", "n_columns", "n_big_fronts"]
    assert list(L.LDLMultiInfo._fields_) == want and C.sizeof(L.LDLMultiInfo) == 40


def test_null_arguments_are_refused():
    from madipm_amd import _lib as L
    info = L.LDLMultiBigInfo()
    assert L.lib.madipm_ldl_multi_big_info(None, C.byref(info)) != 0
    assert L.lib.madipm_solver_multi_big_info(None, C.byref(info)) != 0
    assert L.lib.madipm_ldl_set_multi_big(None, 1) != 0
