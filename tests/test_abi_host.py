"""CPU-side checks of the binding (mmx/_lib.py): the argument types it reads from include/mmx_hip.h against lists typed out here,
the typed functions and call() refusing a wrong call before anything runs, every call site of the package against the parsed
prototypes, and the five ctypes struct mirrors against the layout the host C compiler gives the header's structs."""
import ast
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmx_hip.h")
P, I, Q, U, F, D = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_parsed_argtypes_equal_hand_written_lists():
    """Typed out from reading the header, not from the parser."""
    from mmx import _lib
    S = _lib.SIGNATURES
    # x, ldx, x_bstride, rows, C, batch | gamma, beta, eps, rms, act | rowmask, rm_bstride, addvec, av_bstride |
    # out_f32, ldo_f, of_bstride | out_act, ldo_a, oa_bstride, dtype, stream
    assert S["mmx_rownorm"] == [P, Q, Q, I, I, I, P, P, F, I, I, P, Q, P, Q, P, Q, Q, P, Q, Q, I, P]
    # logits, ldl, V, B, eos_id, top_k, top_p | win_size, tau_r, seed, state, out_tokens, max_out | sampled, forced, speech_emb, E,
    # next_x | ldx, logp_out, stream
    assert S["mmx_sample_step"] == [P, Q, I, I, I, I, F, I, F, U, P, P, I, P, P, P, I, P, Q, P, P]
    # x, x_bs, y, y_bs, L, B, lens, h_lens | basis, filt, n_fft, n_mels, eps, pow, work, cap | out, stream
    assert S["mmx_spec_dist"] == [P, Q, P, Q, I, I, P, P, P, P, I, I, D, D, P, I, P, P]


def test_every_prototype_is_parsed_and_counted():
    from mmx import _lib
    declared = sorted(set(re.findall(r"\bint\s+(mmx_[a-z0-9_]+)\s*\(", _header())))
    assert sorted(_lib.SYMBOLS) == declared and len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    assert _lib.SIGNATURES["mmx_abi_version"] == []
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.findall(r"\((\d+) entry points", readme) == [str(len(declared))]


def test_parser_refuses_what_it_does_not_know(tmp_path):
    from mmx import _lib
    bad = tmp_path / "bad.h"
    bad.write_text("int mmx_ok(const float* x, int64_t n);\nint mmx_odd(const float* x, size_t n);\n")
    with pytest.raises(_lib.MmxError, match="mmx_odd.*size_t n"):
        _lib.parse_header(str(bad))
    with pytest.raises(_lib.MmxError, match="absent.h"):
        _lib.parse_header(str(tmp_path / "absent.h"))


def test_typed_functions_refuse_a_wrong_type_or_too_few_arguments():
    """ctypes converts every argument before it enters the function: nothing runs."""
    from mmx import _lib
    lib = _lib.load()
    with pytest.raises(C.ArgumentError):
        lib.mmx_row_absmax(None, 0, 1.5, 0, None, None, None)            # a float for `int L`
    with pytest.raises(TypeError):
        lib.mmx_row_absmax(None, 0, 0)


def test_call_refuses_a_wrong_argument_count():
    from mmx import _lib
    with pytest.raises(_lib.MmxError, match="mmx_abi_version takes 0 arguments, 1 given"):
        _lib.call("mmx_abi_version", 1)
    with pytest.raises(_lib.MmxError, match="mmx_row_absmax takes 7 arguments, 8 given"):
        _lib.call("mmx_row_absmax", None, 0, 0, 0, None, None, None, None)
    with pytest.raises(_lib.MmxError, match="mmx_row_absmax takes 7 arguments, 6 given"):
        _lib.call("mmx_row_absmax", None, 0, 0, 0, None, None)
    with pytest.raises(KeyError, match="mmx_no_such_thing"):
        _lib.call("mmx_no_such_thing")


def test_call_turns_a_code_into_mmx_error():
    """mmx_row_absmax checks its arguments in its first statement (csrc/degrade.hip: MMX_CHECK_ARG before any HIP call), so this
    runs without a GPU."""
    from mmx import _lib
    with pytest.raises(_lib.MmxError, match=r"mmx_row_absmax failed with code -1 \(argument/shape error\)"):
        _lib.call("mmx_row_absmax", None, 0, 0, 0, None, None, None)
    assert _lib.load().mmx_row_absmax(None, 0, 0, 0, None, None, None) == -1      # the raw function still returns the code


def test_call_sites_agree_with_the_prototypes():
    """Every call("mmx_x", ...) in mmx/ names a parsed entry point with a literal, passes as many arguments as the prototype has
    parameters, none of them starred; no raw lib.mmx_x(...) call is left besides mmx_abi_version inside load()."""
    from mmx import _lib
    sites, bad = 0, []
    for path in sorted(glob.glob(os.path.join(ROOT, "minimax-speech_amd", "mmx", "*.py"))):
        tree = ast.parse(open(path).read())
        inside_load = {id(n) for f in ast.walk(tree) if isinstance(f, ast.FunctionDef) and f.name == "load" for n in ast.walk(f)}
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            where = f"{os.path.basename(path)}:{node.lineno}"
            fn = node.func
            if isinstance(fn, ast.Attribute) and fn.attr.startswith("mmx_"):
                if not (fn.attr == "mmx_abi_version" and os.path.basename(path) == "_lib.py" and id(node) in inside_load):
                    bad.append(f"{where}: raw call of {fn.attr}")
            if (isinstance(fn, ast.Name) and fn.id == "call") or (isinstance(fn, ast.Attribute) and fn.attr == "call"):
                sites += 1
                name = node.args[0] if node.args else None
                if not (isinstance(name, ast.Constant) and isinstance(name.value, str)):
                    bad.append(f"{where}: the entry point is not a string literal")
                elif name.value not in _lib.SIGNATURES:
                    bad.append(f"{where}: {name.value} is not declared in the header")
                elif any(isinstance(a, ast.Starred) for a in node.args) or node.keywords:
                    bad.append(f"{where}: {name.value} with a starred or keyword argument")
                elif len(node.args) - 1 != len(_lib.SIGNATURES[name.value]):
                    bad.append(f"{where}: {name.value} takes {len(_lib.SIGNATURES[name.value])} arguments, {len(node.args) - 1} written")
    assert not bad, "\n".join(bad)
    assert sites >= 60                                       # the walk found the call sites at all


# ------------------------------------------------------------------------------------------------ struct mirrors
STRUCTS = {"MmxGemmParams": "GemmParams", "MmxEstNext": "EstNext", "MmxEstTailParams": "EstTailParams",
           "MmxEstResnetParams": "EstResnetParams", "MmxDacRuParams": "DacRuParams"}


def _header_fields(struct):
    """The field names of `struct` in the header's order, read from its text."""
    body = re.search(r"typedef struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*" + struct + r"\s*;", _header()).group(1)
    return [re.findall(r"(\w+)\s*$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """{struct: (sizeof, {field: (offsetof, sizeof)})} as the host C compiler lays the header's structs out."""
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = next((p for p in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), rocm_clang) if p and os.path.exists(p)), None)
    assert cc, "no host C compiler (cc, gcc, clang, ROCm's clang): the struct mirrors cannot be checked"
    lines = []
    for s in STRUCTS:
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'    printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in _header_fields(s)]
    d = tmp_path_factory.mktemp("abi")
    src, exe = d / "layout.c", d / "layout"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"mmx_hip.h\"\nint main(void) {\n" + "\n".join(lines) + "\n    return 0;\n}\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = {s: [None, {}] for s in STRUCTS}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if line:
            key, *vals = line.split()
            s, _, f = key.partition(".")
            if f:
                out[s][1][f] = tuple(int(v) for v in vals)
            else:
                out[s][0] = int(vals[0])
    return out


@pytest.mark.parametrize("struct", list(STRUCTS))
def test_struct_mirror_has_the_compilers_layout(compiled_layout, struct):
    from mmx import _lib
    cls = getattr(_lib, STRUCTS[struct])
    names = [f[0] for f in cls._fields_]
    assert names == _header_fields(struct)                   # order and names, from the header's text
    size, offsets = compiled_layout[struct]
    assert C.sizeof(cls) == size
    assert {n: (getattr(cls, n).offset, getattr(cls, n).size) for n in names} == offsets
