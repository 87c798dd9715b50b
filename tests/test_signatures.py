"""The ctypes signature table (diff_gaussian_rasterization/_signatures.py) against the prototypes of include/gsraster.h:
with calls of up to 23 positional pointers a wrong count or width is silent undefined behaviour, and nothing else compares
the two.  Needs neither the library nor a device."""
import ctypes
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3d-gaussian-splat-attack_amd")

_SCALARS = {"int32_t": "i32", "int64_t": "i64", "uint32_t": "u32", "float": "f32", "double": "f64", "int": "int",
            "gsr_chunk_fn": "chunk_fn"}


def _param_kind(decl: str) -> str:
    decl = decl.strip()
    if "*" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    assert len(words) == 2, f"unexpected parameter declaration {decl!r}"
    return _SCALARS[words[0]]


def _header_prototypes():
    """name -> (return kind, [parameter kinds]) of every `int|void|const char* gsr_...(...);` of the header."""
    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    protos = {}
    for m in re.finditer(r"\b(int|void|const\s+char\s*\*)\s*(gsr_\w+)\s*\(([^;{)]*)\)\s*;", src):
        ret = {"int": "int", "void": "void"}.get(m.group(1), "str")
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = (ret, [] if params in ("", "void") else [_param_kind(p) for p in params.split(",")])
    return protos


def _table():
    from diff_gaussian_rasterization import _signatures as S
    kinds = {ctypes.c_void_p: "ptr", ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_uint32: "u32",
             ctypes.c_float: "f32", ctypes.c_double: "f64", S.CHUNK_FN: "chunk_fn"}
    rets = {ctypes.c_int: "int", None: "void", ctypes.c_char_p: "str"}

    def kind(t):
        if t in kinds:
            return kinds[t]
        assert issubclass(t, ctypes._Pointer), f"no kind for argtype {t!r}"       # POINTER(struct) is allowed
        return "ptr"
    return {name: (rets[res], [kind(t) for t in args]) for name, (res, args) in S.SIGNATURES.items()}


def test_header_parse_finds_the_abi():
    protos = _header_prototypes()
    assert len(protos) >= 55 and protos["gsr_last_error"] == ("str", []) and protos["gsr_trim_pool"] == ("void", [])
    assert protos["gsr_backward_raw_chunked"][1][11:] == ["i32", "i32", "chunk_fn", "ptr", "ptr"]
    assert protos["gsr_points_in_hull"][1][5] == "f64" and protos["gsr_ctx_rerender"][1][8] == "u32"


def test_every_table_entry_matches_its_prototype():
    protos, table = _header_prototypes(), _table()
    missing = sorted(set(table) - set(protos))
    assert not missing, f"declared for ctypes but not in include/gsraster.h: {missing}"
    for name, (ret, params) in table.items():
        h_ret, h_params = protos[name]
        assert ret == h_ret, f"{name}: return kind {ret}, header {h_ret}"
        assert len(params) == len(h_params), f"{name}: {len(params)} parameters declared, header has {len(h_params)}"
        for i, (p, h) in enumerate(zip(params, h_params)):
            assert p == h, f"{name}: parameter {i} declared {p}, header {h}"


def test_chunk_callback_matches_the_typedef():
    from diff_gaussian_rasterization import _signatures as S
    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    m = re.search(r"typedef\s+void\s*\(\*gsr_chunk_fn\)\s*\(([^)]*)\)\s*;", src)
    assert [_param_kind(p) for p in m.group(1).split(",")] == ["ptr", "i32", "i64", "i64"]
    assert S.CHUNK_FN._restype_ is None
    assert list(S.CHUNK_FN._argtypes_) == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]


def test_every_entry_point_the_binding_calls_is_declared():
    """Every `<library>.gsr_xxx(` in the package's Python sources: an undeclared one would be called with ctypes' defaults
    (int arguments, int result), which truncates 64-bit values."""
    table = _table()
    called = set()
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        called |= set(re.findall(r"\.(gsr_[a-z0-9_]+)\(", open(path).read()))
    assert "gsr_knn_dist2" in called and "gsr_forward_raw_batch" in called       # (the scan sees simple_knn and the package)
    assert not called - set(table), f"called but not declared: {sorted(called - set(table))}"


def test_no_module_declares_signatures_on_its_own():
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        src = open(path).read()
        if path.endswith(os.path.join("diff_gaussian_rasterization", "__init__.py")):
            assert src.count(".argtypes") == 1                                    # the table's application in _load()
        else:
            assert ".argtypes" not in src and ".restype" not in src, path
