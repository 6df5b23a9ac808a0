"""The Python binding's declarations of the C ABI, without a GPU.

* ygzfe/_abi.py's table against the prototypes of include/ygzfe.h, parsed here;
* the loaded library's function objects carry the table's restype and argtypes;
* a wrong argument is refused before the call, and 64-bit values arrive whole;
* the ctypes.Structure classes and numpy dtypes of ygzfe/__init__.py against sizeof / offsetof of the
  header's structs, printed by tests/host/abi_layout.c (built with AddressSanitizer and UBSan).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-ygz-slam_amd")
INCLUDE = os.path.join(ROOT, "include")
SCALARS = {"int": "i", "int32_t": "i", "float": "f", "size_t": "z", "double": "d", "uint64_t": "Q"}


@pytest.fixture(scope="module")
def ygzfe():
    if not os.path.exists(os.path.join(PKG, "lib", "libygzfe.so")):  # hipcc cross-compiles for gfx950 without a GPU
        subprocess.check_call(["make", "-s", "-C", PKG])
    import ygzfe as m
    return m


@pytest.fixture(scope="module")
def header():
    """include/ygzfe.h without comments and preprocessor lines."""
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, "ygzfe.h")).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("#")).replace('extern "C" {', " ")


def kind(ctype, ret=False):
    """The table's kind letter of a C type; a type outside the table's kinds is a KeyError."""
    t = " ".join(ctype.replace("*", " * ").split())
    if "*" in t:
        return "s" if t == "const char *" else "p"
    return "v" if ret and t == "void" else SCALARS[t]


def prototypes(header):
    """{function: "return kind:parameter kinds"}: every statement of the header with a parenthesis in it
    has to parse as a prototype over the known kinds."""
    out = {}
    for st in re.sub(r"\{[^{}]*\}", " ", header).split(";"):
        st = " ".join(st.split())
        if "(" not in st:
            continue
        m = re.fullmatch(r"(.*[\s*])(\w+)\s*\(([^()]*)\)", st)
        assert m, f"not a plain prototype: {st}"
        ret, name, params = m.groups()
        kinds = ""
        for p in ([] if params.strip() == "void" else params.split(",")):
            pm = re.fullmatch(r"(.*[\s*])\w+", p.strip())
            assert pm, f"{name}: parameter {p!r}"
            kinds += kind(pm.group(1))
        assert name not in out
        out[name] = kind(ret, ret=True) + ":" + kinds
    return out


def test_table_matches_header(ygzfe, header):
    A = ygzfe._abi
    want = prototypes(header)
    assert len(want) >= 91
    got = A.table("ygzfe_", A.YGZFE)
    assert len(got) == len(A.YGZFE.split()), "a function is listed twice"
    assert sorted(got) == sorted(want)
    assert {n: (got[n], want[n]) for n in want if got[n] != want[n]} == {}
    for text in (A.YGZFE, A.SYNTH, A.SYNTH_HIP):
        assert all(re.fullmatch(r"\w+=[a-zA-Z]:[a-zA-Z]*", e) and set(e.split("=")[1]) - {":"} <= set(A.KINDS)
                   for e in text.split())


def test_loaded_functions_carry_the_table(ygzfe):
    A = ygzfe._abi
    for lib, table in [(ygzfe.lib(), A.table("ygzfe_", A.YGZFE)), (ygzfe.synth(), A.table("ygzs_", A.SYNTH)),
                       (ygzfe._synth_hip_lib(), A.table("ygzs_", A.SYNTH_HIP))]:
        for name, kinds in table.items():
            fn = getattr(lib, name)
            assert fn.restype is A.KINDS[kinds[0]], name
            assert fn.argtypes is not None and list(fn.argtypes) == [A.KINDS[k] for k in kinds[2:]], name


def test_wrong_arguments_are_refused_before_the_call(ygzfe):
    """ygzfe_orb_plan(const ygzfe_orb_params *, int width, int height, five int32_t *) is host-only."""
    p = ygzfe.OrbParams(1000, 2.0, 4, 20, 7, ygzfe.BLUR_CV4)
    out = [np.zeros(16, np.int32) for _ in range(5)]
    plan = ygzfe.lib().ygzfe_orb_plan
    assert plan(C.byref(p), 752, 480, *[ygzfe._p(a) for a in out]) == ygzfe.OK
    with pytest.raises(C.ArgumentError):
        plan(C.byref(p), 752.0, 480, *[ygzfe._p(a) for a in out])
    with pytest.raises(C.ArgumentError):
        plan(1.5, 752, 480, *[ygzfe._p(a) for a in out])  # a float is no pointer either
    with pytest.raises(TypeError):
        plan(C.byref(p), 752, 480, *[ygzfe._p(a) for a in out[:4]])


def test_64_bit_values_arrive_whole(ygzfe):
    """Addresses passed as plain Python ints (as tensor.data_ptr() is) reach the callee unclipped, and a size_t
    comes back whole."""
    rng = np.random.default_rng(5)
    keep = []
    for _ in range(64):
        a, b = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2))
        keep += [a, b]
        if max(a.ctypes.data, b.ctypes.data) >= 1 << 32:
            break
    assert max(a.ctypes.data, b.ctypes.data) >= 1 << 32, "no buffer above 4 GiB: the case would test nothing"
    assert ygzfe.lib().ygzfe_descriptor_distance(a.ctypes.data, b.ctypes.data) == int(np.unpackbits(a ^ b).sum())
    # include/ygzfe.h: a 64-byte header, kp_cap rows of 28 + 32 bytes, zero padding to a 16-byte multiple
    assert ygzfe.slot_bytes(1001) == 60128 == -(-(64 + 1001 * 60) // 16) * 16
    assert ygzfe.lib().ygzfe_slot_bytes.restype is C.c_size_t


def header_structs(header):
    """{struct: [field, ...]} of every struct the header defines (ygzfe_ prefix dropped)."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+ygzfe_(\w+)\s*\{([^{}]*)\}", header):
        out[name] = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            for part in decl.split(","):
                out[name].append(re.fullmatch(r".*?(\w+)\s*(\[\d+\])?", part.strip()).group(1))
    return out


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """({struct: sizeof}, {struct: {field: (offsetof, sizeof)}}) as the C compiler sees include/ygzfe.h."""
    exe = str(tmp_path_factory.mktemp("abi") / "abi_layout")
    subprocess.check_call(["gcc", "-std=c11", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", INCLUDE, os.path.join(ROOT, "tests", "host", "abi_layout.c"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    sizes, fields = {}, {}
    for line in r.stdout.splitlines():
        name, *nums = line.split()
        if "." in name:
            s, f = name.split(".", 1)
            fields[s][f] = (int(nums[0]), int(nums[1]))
        else:
            sizes[name], fields[name] = int(nums[0]), {}
    return sizes, fields


def test_layout_program_covers_the_header(header, c_layout):
    sizes, fields = c_layout
    want = header_structs(header)
    assert len(want) >= 12 and sorted(sizes) == sorted(want)
    for s, names in want.items():
        assert [f for f in fields[s] if "." not in f] == names, s


CTYPES_MIRRORS = {"orb_params": "OrbParams", "camera": "Camera", "se3": "SE3", "align_result": "AlignResult",
                  "bounds": "Bounds", "direct_view": "DirectView", "direct_keyframes": "_DirectKeyframes",
                  "direct_candidates": "_DirectCandidates", "direct_map_result": "_DirectMapResult",
                  "pose_opt_result": "PoseOptResult"}


@pytest.mark.parametrize("struct", sorted(CTYPES_MIRRORS))
def test_ctypes_structures_match_the_header(ygzfe, c_layout, struct):
    sizes, fields = c_layout
    cls = getattr(ygzfe, CTYPES_MIRRORS[struct])
    assert C.sizeof(cls) == sizes[struct]
    assert [n for n, _ in cls._fields_] == [f for f in fields[struct] if "." not in f]
    for f, want in fields[struct].items():
        off, t = 0, cls
        for part in f.split("."):
            d = getattr(t, part)
            off, size, t = off + d.offset, d.size, dict(t._fields_)[part]
        assert (off, size) == want, f"{struct}.{f}"


# dtype field -> the header's field, where the dtype flattens a nested ygzfe_se3
DTYPE_MIRRORS = {"kp": ("KP_DTYPE", {}), "se3": ("SE3_DTYPE", {}), "match_query": ("MATCH_QUERY_DTYPE", {}),
                 "align_result": ("ALIGN_RESULT_DTYPE", {"q": "T_cur_ref.q", "t": "T_cur_ref.t"}),
                 "pose_opt_result": ("POSE_OPT_RESULT_DTYPE", {"Tq": "T_cw.q", "Tt": "T_cw.t"})}


@pytest.mark.parametrize("struct", sorted(DTYPE_MIRRORS))
def test_numpy_dtypes_match_the_header(ygzfe, c_layout, struct):
    sizes, fields = c_layout
    name, renamed = DTYPE_MIRRORS[struct]
    dt = getattr(ygzfe, name)
    assert dt.itemsize == sizes[struct]
    got = {renamed.get(n, n): (dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names}
    leaves = {f: v for f, v in fields[struct].items() if not any(g.startswith(f + ".") for g in fields[struct])}
    assert got == leaves
    assert [renamed.get(n, n) for n in dt.names] == list(leaves), "field order"
