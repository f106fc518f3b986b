"""include/scrubvae_hip.h against its hand-written mirror scrubvae_amd/_lib.py, in full and in one place: the set of entry points,
every return and argument type, every struct, every limit, the limits the eval modules re-publish, and the build's source lists.
The compiler holds the header to the definitions (every .hip unit includes it); this holds the header to the Python side.  Feature
tests do not re-check the binding: they pin only literals this test cannot know (tests/abi_header.py)."""
import ctypes as C
import importlib
import inspect
import os

from scrubvae_amd import _lib, build, ops
from tests import abi_header as H

# header struct -> its ctypes mirror
MIRRORS = {"svae_conv_desc": _lib.ConvDesc, "svae_split_task": _lib.SplitTask, "svae_bn_bwd_fuse": _lib.BnBwdFuse,
           "svae_tree": _lib.Tree, "svae_colsum_task": _lib.ColsumTask, "svae_colsum_part_task": _lib.ColsumPartTask,
           "svae_ens_layer": _lib.EnsLayer, "svae_ens_member": _lib.EnsMember, "svae_ens_desc": _lib.EnsDesc}
STRUCT_OF = {cls: name for name, cls in MIRRORS.items()}
SCALARS = {None: "void", C.c_int: "int", C.c_longlong: "long long", C.c_size_t: "size_t", C.c_float: "float", C.c_double: "double"}
# #defines of the header that _lib.py has no use for, each with its reason
HEADER_ONLY = {"SVAE_MMD_NULL_COLS": "permutations per pass of svae_mmd_null: used only inside the library (svae_mmd_null_blocks sizes the work)"}
# limits that the eval modules publish again: (module, its name, the _lib constant)
REEXPORTS = [("metrics", "MMD_MAX_PERMUTATIONS", "MMD_NULL_MAX")] + [(m, n, n) for m, n in (
    ("neighbors", "KNN_MAX_K"), ("density", "DENSITY_MAX_GRID"), ("silhouette", "SIL_MAX_CLUSTERS"), ("independence", "HSIC_MAX_Y"),
    ("mutual_info", "MI_MAX_K"), ("mutual_info", "MI_MAX_Y"), ("conditional_mi", "CMI_MAX_C"), ("conditional_mi", "CMI_MAX_DONORS"),
    ("transport", "OT_MAX_COLS"))]


def matches(ctype, kind):
    """does the ctypes type stand for the header kind?  c_void_p / c_char_p: any pointer; POINTER(X): X's struct, or a plain pointer"""
    if ctype in SCALARS:
        return SCALARS[ctype] == kind
    if ctype in (C.c_void_p, C.c_char_p):
        return kind == "pointer" or kind in MIRRORS
    if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
        return kind == STRUCT_OF.get(ctype._type_, "pointer" if ctype._type_ in (C.c_int, C.c_float, C.c_void_p) else None)
    return False


def test_same_set_of_names():
    declared, bound = set(H.declarations()), set(_lib.SIGNATURES)
    assert not declared - bound, f"declared in the header without a row in _lib.SIGNATURES: {sorted(declared - bound)}"
    assert not bound - declared, f"rows of _lib.SIGNATURES that the header does not declare: {sorted(bound - declared)}"
    assert _lib.lib().svae_version() >= 100  # lib() binds every row: a symbol the library does not export raises here


def test_same_types():
    wrong, header = [], H.declarations()
    for name in sorted(set(header) & set(_lib.SIGNATURES)):  # a name on one side only is test_same_set_of_names's to report
        (ret, kinds), (res, args) = header[name], _lib.SIGNATURES[name]
        if not matches(res, ret):
            wrong.append(f"{name}: returns {ret}, bound as {res}")
        if len(args) != len(kinds):
            wrong.append(f"{name}: {len(kinds)} arguments, {len(args)} bound")
        wrong += [f"{name}: argument {i} is {k}, bound as {a.__name__}" for i, (a, k) in enumerate(zip(args, kinds)) if not matches(a, k)]
    assert not wrong, "\n".join(wrong)


def mirror_fields(cls):
    """[(field, kind, [array extents])] of a ctypes.Structure, in the vocabulary of abi_header.structs()"""
    out = []
    for field, t in cls._fields_:
        extents = []
        while issubclass(t, C.Array):
            extents.append(t._length_)
            t = t._type_
        out.append((field, "pointer" if t is C.c_void_p else STRUCT_OF.get(t) or SCALARS.get(t), extents))
    return out


def test_same_structs():
    header = H.structs()
    classes = {c for _, c in inspect.getmembers(_lib, inspect.isclass) if issubclass(c, C.Structure) and c.__module__ == _lib.__name__}
    assert set(header) == set(MIRRORS), f"structs of the header and the mirrors named here differ: {sorted(set(header) ^ set(MIRRORS))}"
    assert classes == set(STRUCT_OF) and len(STRUCT_OF) == len(MIRRORS), \
        f"ctypes.Structure classes of _lib.py and the mirrors named here differ: {sorted(c.__name__ for c in classes ^ set(STRUCT_OF))}"
    for name, cls in MIRRORS.items():
        want, got = header[name], mirror_fields(cls)
        assert [f for f, _, _ in got] == [f for f, _, _ in want], f"{name}: fields {[f for f, _, _ in want]}, {cls.__name__} has {[f for f, _, _ in got]}"
        for w, g in zip(want, got):
            assert w == g, f"{name}.{w[0]}: the header has {w[1:]}, {cls.__name__} has {g[1:]}"


def test_same_limits():
    defines, status = H.defines(), H.status()
    limits = {n: v for n, v in vars(_lib).items() if n.isupper() and type(v) is int}  # the module-level integer constants
    for name, value in limits.items():
        table, what = (status, "svae_status") if name.startswith("ERR_") else (defines, "the header's #define")
        assert table.get("SVAE_" + name) == value, f"_lib.{name} = {value}, {what} SVAE_{name} is {table.get('SVAE_' + name)}"
    assert set(status) == {"SVAE_OK"} | {"SVAE_" + n for n in limits if n.startswith("ERR_")} and status["SVAE_OK"] == 0, f"svae_status is {status}"
    segment = {int(n.rsplit("_", 1)[1]): v for n, v in defines.items() if n.startswith("SVAE_HMM_SEGMENT_")}
    assert _lib.HMM_SEGMENT == segment, f"_lib.HMM_SEGMENT = {_lib.HMM_SEGMENT}, the header's SVAE_HMM_SEGMENT_<kp> give {segment}"
    assert ops.F16X2 == defines["SVAE_PIECES_F16X2"], f"ops.F16X2 = {ops.F16X2}, SVAE_PIECES_F16X2 = {defines['SVAE_PIECES_F16X2']}"
    mirrored = {"SVAE_" + n for n in limits} | {f"SVAE_HMM_SEGMENT_{kp}" for kp in segment} | {"SVAE_PIECES_F16X2"}
    assert set(defines) - mirrored == set(HEADER_ONLY), \
        f"#defines with neither a mirror in _lib.py nor a reason in HEADER_ONLY, or reasons gone stale: {sorted((set(defines) - mirrored) ^ set(HEADER_ONLY))}"


def test_reexports_are_the_lib_values():
    for module, name, source in REEXPORTS:
        value = getattr(importlib.import_module("scrubvae_amd.eval." + module), name)
        assert value == getattr(_lib, source), f"eval.{module}.{name} = {value}, _lib.{source} = {getattr(_lib, source)}"


def test_sources_and_headers_are_listed():
    on_disk = os.listdir(build.CSRC)
    missing = [s for s in build.SOURCES if s not in on_disk] + [h for h in build.HEADERS if not os.path.isfile(h)]
    assert not missing, f"listed in build.py but not there: {missing}"
    unlisted = {f for f in on_disk if f.endswith(".hip")} - set(build.SOURCES)
    assert not unlisted, f".hip files under csrc/ that build.SOURCES does not list: {sorted(unlisted)}"
    listed = {os.path.realpath(h) for h in build.HEADERS}
    stray = [f for f in on_disk if f.endswith(".h") and os.path.realpath(os.path.join(build.CSRC, f)) not in listed]
    assert not stray, f"headers under csrc/ that build.HEADERS does not list (an edit would leave stale objects): {sorted(stray)}"
