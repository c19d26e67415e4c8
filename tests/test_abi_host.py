"""The join between include/edtts.h and edge_diffusion_tts_amd/native.py, checked in one place: every prototype against its entry
in native._ABI, every struct against its ctypes.Structure (and against what the host C compiler makes of the header), every Python
mirror of a header constant, and that native.py is the package's only user of ctypes.  No GPU, and no built library."""
import ast
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from edge_diffusion_tts_amd import audio, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.abspath(native.__file__))
with open(os.path.join(REPO, "include", "edtts.h")) as _f:
    HEADER = _f.read()

SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
# The header's convention is "0 or a negative EDTTS_ERR_*"; these are the int returns its comments describe as values.  A prototype
# cannot say which it is, so this list stands against the table's: the two are kept by different hands and must agree.
VALUE_RETURNS = {"edtts_version", "edtts_num_global_slots", "edtts_num_layer_slots", "edtts_train_dw_slab_rows", "edtts_set_substreams",
                 "edtts_substreams_for", "edtts_set_coop", "edtts_optim_chunk_size"}
STRUCTS = ("EdttsDims", "EdttsDropout", "EdttsSemDims", "EdttsOptimState", "EdttsOptimGroup", "EdttsOptimTensor", "EdttsHubertDims")


# ---------------------------------------------------------------------------------------------- reading the header
def strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def c_type(decl):
    """'const void* const* slots' -> ('void**', 'slots'): const dropped, the stars gathered behind the base type."""
    m = re.match(r"^(.*?)(\w+)$", decl.strip(), flags=re.S)
    words = re.sub(r"\bconst\b", " ", m.group(1))
    return "".join(words.replace("*", " ").split()) + "*" * words.count("*"), m.group(2)


def header_prototypes(text):
    """{name: (return type, [(type, parameter name)])} of every prototype, in the header's order."""
    out = {}
    for m in re.finditer(r"^[ \t]*(const\s+char\s*\*|int)\s*(edtts_\w+)\s*\(([^)]*)\)\s*;", strip_comments(text), flags=re.M):
        params = [p for p in m.group(3).split(",") if p.strip() and p.strip() != "void"]
        out[m.group(2)] = ("int" if m.group(1) == "int" else "char*", [c_type(p) for p in params])
    return out


def header_structs(text):
    """{struct name: [(field name, element type, array length or None)]} of every typedef struct."""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", strip_comments(text), flags=re.S):
        assert m.group(1) == m.group(3)
        fields = []
        for decl in (d.strip() for d in m.group(2).split(";")):
            if not decl:
                continue
            base, names = re.match(r"^(\w+\s*\**)\s*(.*)$", decl, flags=re.S).groups()
            for name in (n.strip() for n in names.split(",")):
                arr = re.match(r"^(\w+)\[(\d+)\]$", name)
                fields.append((arr.group(1), "".join(base.split()), int(arr.group(2))) if arr else (name, "".join(base.split()), None))
        out[m.group(1)] = fields
    return out


def header_constants(text):
    """{name: value} of every enumerator with a value and every '#define NAME integer'."""
    text = strip_comments(text)
    out = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(EDTTS_\w+)[ \t]+(-?\w+)[ \t]*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S):
        for item in (i.strip() for i in body.split(",")):
            if item:
                name, value = (s.strip() for s in item.split("="))
                out[name] = int(value, 0)
    return out


# ---------------------------------------------------------------------------------------------- the comparison
def is_pointer(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def param_problem(ctype, py):
    """None when the table's ctypes class `py` fits the header's type, else what is wrong.  Classes are compared by identity:
    c_uint64, c_size_t and c_ulong are one object where they are one type, and their names would not say so."""
    base = ctype.rstrip("*")
    if not ctype.endswith("*"):
        if base not in SCALARS:
            return f"the checker does not know the C type {ctype!r}"
        return None if py is SCALARS[base] else f"header {ctype}, table {getattr(py, '__name__', py)}"
    if ctype == base + "*" and base.startswith("Edtts"):
        struct = getattr(native, base, None)
        if struct is None:
            return f"native.py has no Structure {base}"
        return None if py is C.POINTER(struct) else f"header {ctype}, table {getattr(py, '__name__', py)}"
    return None if is_pointer(py) else f"header {ctype} (a pointer), table {getattr(py, '__name__', py)}"


def abi_problems(header_text, abi, value_returns=VALUE_RETURNS):
    """Every disagreement between the header's prototypes and the table, one line each, beginning with the export's name."""
    protos = header_prototypes(header_text)
    out = [f"{n}: declared in the header, missing from the table" for n in protos if n not in abi]
    out += [f"{n}: in the table, not declared in the header" for n in abi if n not in protos]
    for name, (ret, params) in protos.items():
        if name not in abi:
            continue
        kind, args = abi[name]
        want = native._STR if ret == "char*" else native._VALUE if name in value_returns else native._STATUS
        if kind != want:
            out.append(f"{name}: returns {ret} ({want}), the table says {kind}")
        if len(args) != len(params):
            out.append(f"{name}: {len(params)} parameters in the header, {len(args)} in the table")
            continue
        for i, ((ctype, pname), py) in enumerate(zip(params, args)):
            what = param_problem(ctype, py)
            if what:
                out.append(f"{name}: parameter {i} ({pname}): {what}")
    return out


def test_the_header_is_read_whole():
    """The reader finds a prototype for every edtts_ name that is followed by '(' anywhere in the header's code, in order."""
    protos = header_prototypes(HEADER)
    called = re.findall(r"\b(edtts_[a-z_0-9]+)\s*\(", strip_comments(HEADER))
    assert list(protos) == called and len(set(called)) == len(called)
    assert {ret for ret, _ in protos.values()} == {"int", "char*"}
    assert set(header_structs(HEADER)) == set(STRUCTS)


def test_every_prototype_matches_its_table_entry():
    assert set(header_prototypes(HEADER)) == set(native._ABI)
    assert list(header_prototypes(HEADER)) == list(native._ABI), "the table keeps the header's order"
    assert native.EXPORTED_SYMBOLS == tuple(native._ABI)
    assert abi_problems(HEADER, native._ABI) == []


def _edit(name, fn):
    abi = dict(native._ABI)
    kind, args = abi[name]
    abi[name] = fn(kind, list(args))
    return abi


def _swap(args, i, j):
    args[i], args[j] = args[j], args[i]
    return args


FAULTS = {
    "one pointer dropped": ("edtts_decoder_forward", lambda k, a: (k, a[:-1]), "13 parameters in the header, 12 in the table"),
    "an int swapped with a float": ("edtts_griffin_lim", lambda k, a: (k, _swap(a, 7, 8)), "parameter 7 (n_iter): header int, table c_float"),
    "a uint32_t widened to 64 bits": ("edtts_randn", lambda k, a: (k, a[:3] + [C.c_uint64] + a[4:]), "parameter 3 (stream_id): header uint32_t"),
    "a struct pointer of the wrong struct": ("edtts_sem_encode", lambda k, a: (k, [C.POINTER(native.EdttsDims)] + a[1:]),
                                             "parameter 0 (dims): header EdttsSemDims*"),
    "a status return marked as a value": ("edtts_profile_enable", lambda k, a: (native._VALUE, a), "returns int (status), the table says value"),
    "a value return marked as a status": ("edtts_set_coop", lambda k, a: (native._STATUS, a), "returns int (value), the table says status"),
    "an export left out": ("edtts_resample", None, "declared in the header, missing from the table"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_checker_reports_a_planted_fault(fault):
    name, fn, text = FAULTS[fault]
    if fn is None:
        abi = {k: v for k, v in native._ABI.items() if k != name}
    else:
        abi = _edit(name, fn)
    problems = abi_problems(HEADER, abi)
    assert problems and all(p.startswith(name + ": ") for p in problems), problems
    assert any(text in p for p in problems), problems


# ---------------------------------------------------------------------------------------------- structs
def test_struct_fields_match_the_header():
    structs = header_structs(HEADER)
    for sname in STRUCTS:
        py = getattr(native, sname)
        assert issubclass(py, C.Structure)
        assert [f[0] for f in py._fields_] == [f[0] for f in structs[sname]], sname
        for (fname, ftype), (_, ctype, length) in zip(py._fields_, structs[sname]):
            where = f"{sname}.{fname}"
            if length is not None:
                assert issubclass(ftype, C.Array) and ftype._length_ == length and ftype._type_ is SCALARS[ctype], where
            elif ctype.endswith("*"):
                assert is_pointer(ftype), where
            else:
                assert ftype is SCALARS[ctype], where


def host_c_compilers():
    """The C compiler of the ROCm the build uses (next to its hipcc), then $CC, then cc / gcc / clang on the PATH."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))))
    found = [os.path.join(rocm, *parts) for parts in (("llvm", "bin", "clang"), ("lib", "llvm", "bin", "clang"))]
    found += [os.environ.get("CC") or "", *(shutil.which(n) or "" for n in ("cc", "gcc", "clang"))]
    return [c for c in found if c and os.path.exists(c)]


def test_struct_layout_matches_the_host_c_compiler(tmp_path):
    compilers = host_c_compilers()
    if not compilers:
        pytest.skip("no host C compiler on this machine")
    lines = []
    for sname, fields in header_structs(HEADER).items():
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f[0]} %zu\\n", offsetof({sname}, {f[0]}));' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edtts.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    errors = []
    for cc in compilers:
        r = subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
        if r.returncode == 0:
            break
        errors.append(f"{cc}: {r.stderr[-400:]}")
    else:
        pytest.fail("no host C compiler could build the layout probe:\n" + "\n".join(errors))
    c_layout = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    py_layout = {}
    for sname in STRUCTS:
        py = getattr(native, sname)
        py_layout[sname] = str(C.sizeof(py))
        py_layout.update({f"{sname}.{f[0]}": str(getattr(py, f[0]).offset) for f in py._fields_})
    assert py_layout == c_layout
    assert {s: int(c_layout[s]) for s in STRUCTS} == {"EdttsDims": 48, "EdttsDropout": 16, "EdttsSemDims": 84, "EdttsOptimState": 32,
                                                      "EdttsOptimGroup": 40, "EdttsOptimTensor": 80, "EdttsHubertDims": 224}


# ---------------------------------------------------------------------------------------------- constants
def test_python_mirrors_of_header_constants():
    k = header_constants(HEADER)
    assert k["EDTTS_VERSION"] == 400
    assert k["EDTTS_OK"] == 0 and k["EDTTS_ERR_ARG"] == native.EDTTS_ERR_ARG  # what native._errcheck tests a return code for
    assert (native.EDTTS_IDX_SEM, native.EDTTS_IDX_STEP, native.EDTTS_IDX_LEN) == (k["EDTTS_IDX_SEM"], k["EDTTS_IDX_STEP"], k["EDTTS_IDX_LEN"])
    assert (k["EDTTS_IDX_SEM"], k["EDTTS_IDX_STEP"], k["EDTTS_IDX_LEN"]) == (1, 2, 4)  # bits of a word callers keep: they do not move
    f32, bf16 = k["EDTTS_F32"], k["EDTTS_BF16"]
    assert native.COMPUTE_DTYPES == {"f32": f32, "fp32": f32, "float32": f32, "bf16": bf16, "bfloat16": bf16}
    assert native.KERNELS == {"compiled": 0, "generic": k["EDTTS_KERNELS_GENERIC"], "auto": k["EDTTS_KERNELS_AUTO"]}
    assert (native.SEM_FSQ, native.SEM_VQ) == (k["EDTTS_SEM_FSQ"], k["EDTTS_SEM_VQ"])
    assert (native.OPT_CLIP, native.OPT_SKIP_NONFINITE, native.OPT_ZERO_GRADS, native.OPT_EMA_ONLY) == (
        k["EDTTS_OPT_CLIP"], k["EDTTS_OPT_SKIP_NONFINITE"], k["EDTTS_OPT_ZERO_GRADS"], k["EDTTS_OPT_EMA_ONLY"])
    assert native.HUBERT_DTYPES == {"fp32": k["EDTTS_HUBERT_FP32"], "bf16": k["EDTTS_HUBERT_BF16"]}
    assert (audio.EDTTS_MEL_POWER, audio.EDTTS_MEL_LOG) == (k["EDTTS_MEL_POWER"], k["EDTTS_MEL_LOG"])
    # and whatever else a module of the package names after a header constant
    for fname in sorted(os.listdir(PKG)):
        if fname.endswith(".py"):
            mod = __import__("edge_diffusion_tts_amd." + fname[:-3], fromlist=["_"])
            for name, value in vars(mod).items():
                if name.startswith("EDTTS_") and isinstance(value, int):
                    assert k.get(name) == value, f"{fname}: {name}"


# ---------------------------------------------------------------------------------------------- the door
def test_native_is_the_only_module_that_touches_ctypes():
    for fname in sorted(os.listdir(PKG)):
        if not fname.endswith(".py") or fname == "native.py":
            continue
        with open(os.path.join(PKG, fname)) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            where = f"{fname}:{getattr(node, 'lineno', 0)}"
            if isinstance(node, ast.Import):
                assert not any(a.name.split(".")[0] in ("ctypes", "_ctypes") for a in node.names), where
            elif isinstance(node, ast.ImportFrom):
                assert (node.module or "").split(".")[0] not in ("ctypes", "_ctypes"), where
                assert not any(a.name in ("lib", "_lib") for a in node.names), where
            elif isinstance(node, ast.Attribute):
                assert node.attr not in ("lib", "_lib", "CDLL"), where
            elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name):
                assert node.func.id != "lib", where
