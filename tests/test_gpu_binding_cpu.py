"""freddy_amd/gpu.py against include/freddy_gpu.h: every prototype of gpu.PROTOTYPES, what load() binds from it, the layouts of
the ctypes structures and the copies of the header's constants.  No GPU: the header is parsed here, the structures are measured
by a C program gcc compiles from it."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "freddy_gpu.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}
STRUCTS = {"freddy_pq_desc": "PQDesc", "freddy_ivf_desc": "IVFDesc", "freddy_ivpq_desc": "IVPQDesc", "freddy_vec_desc": "VecDesc",
           "freddy_encode_desc": "EncodeDesc", "freddy_insert_desc": "InsertDesc", "freddy_track": "Track",
           "freddy_alloc_stats": "AllocStats"}


def _gpu():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu
    return gpu


def header_text():
    """The header without comments, continuation lines joined."""
    src = open(HEADER).read().replace("\\\n", " ")
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def _split_params(params):
    """A parameter list cut at its top-level commas ("char (*names)[64]" has brackets of its own)."""
    out, depth, cur = [], 0, ""
    for ch in params:
        if ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return [p.strip() for p in out + [cur]]


def _param_type(p):
    if "*" in p or "[" in p:
        return C.c_char_p if re.fullmatch(r"const\s+char\s*\*\s*\w*", p) else C.c_void_p
    ctype = " ".join(p.split()[:-1])          # the last word is the parameter's name
    if ctype not in SCALARS:
        raise ValueError(f"C type this test does not know: {p!r}")
    return SCALARS[ctype]


def header_prototypes(src):
    """{name: (restype, [argtypes])} of every function the header declares; an unknown C type or a statement with a
    parameter list that is no freddy_gpu_* prototype raises."""
    body = "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("#"))
    body = re.sub(r'extern\s+"C"\s*\{', " ", body)
    body = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", body, flags=re.S)
    protos = {}
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if "(" not in stmt:
            continue                           # the opaque handle's typedef, the closing brace of extern "C"
        m = re.fullmatch(r"(.*?)\b(freddy_gpu_\w+) ?\((.*)\)", stmt)
        if not m:
            raise ValueError(f"not a freddy_gpu_* prototype: {stmt!r}")
        ret, name, params = re.sub(r"\s*\*", "*", m.group(1).strip()), m.group(2), m.group(3).strip()
        if ret not in RETURNS:
            raise ValueError(f"return type this test does not know: {stmt!r}")
        if name in protos:
            raise ValueError(f"{name} is declared twice")
        protos[name] = (RETURNS[ret], [] if params == "void" else [_param_type(p) for p in _split_params(params)])
    return protos


def header_structs(src):
    """{struct name: [field names in order]} of every "typedef struct NAME { ... } NAME;" of the header."""
    out = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        assert name == alias, (name, alias)
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                fields += [re.fullmatch(r".*?(\w+)", part.strip()).group(1) for part in decl.split(",")]
        out[name] = fields
    return out


def header_defines(src):
    """{NAME: int} of the object-like #defines whose value is an integer, bare or in brackets."""
    return {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", src, flags=re.M)}


def mismatches(table, declared):
    """Every way `table` (name -> (restype, [argtypes])) differs from the header's prototypes, as text; [] when they agree."""
    bad = [f"{n}: declared in the header, not in the table" for n in declared if n not in table]
    bad += [f"{n}: in the table, not declared in the header" for n in table if n not in declared]
    for n in declared:
        if n in table and (table[n][0], list(table[n][1])) != declared[n]:
            bad.append(f"{n}: the table has {table[n]}, the header declares {declared[n]}")
    return bad


def test_the_parser_reads_the_header_as_expected():
    """The parser itself on prototypes whose types are known by hand: a char array pointer, a fixed array, void, const char*."""
    src = header_text()
    d = header_prototypes(src)
    v, i32, i64, f = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert set(d) == set(re.findall(r"\b(freddy_gpu_\w+)\s*\(", src)) and len(d) >= 74      # every name that is followed by "("
    assert d["freddy_gpu_profile_read"] == (C.c_int, [v, i32, v, v, v])
    assert d["freddy_gpu_scan_elastic_stats"] == (C.c_int, [v, v])
    assert d["freddy_gpu_abi_version"] == (C.c_int, [])
    assert d["freddy_gpu_last_error"] == (C.c_char_p, [])
    assert d["freddy_gpu_set_option"] == (C.c_int, [v, C.c_char_p, i64])
    assert d["freddy_gpu_index_bytes"] == (i64, [v])
    assert d["freddy_gpu_host_alloc"] == (C.c_int, [v, C.c_size_t])
    assert d["freddy_gpu_pin_ivf_multi"] == (C.c_int, [v, v, C.c_int, v])
    assert d["freddy_gpu_pq_search"] == (C.c_int, [v, v, i32, i32, f, v, i64, v, v])
    assert d["freddy_gpu_grouping_pq"] == (C.c_int, [v, v, i32, v, i64, v, v, v])
    assert d["freddy_gpu_encode"] == (C.c_int, [v, C.c_int, v, i64, v, v])
    for bad in ("int freddy_gpu_x(unsigned n);", "long freddy_gpu_x(void);", "int other_name(int n);"):
        try:
            header_prototypes(bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad!r}")


def test_prototypes_equal_the_header():
    gpu = _gpu()
    declared = header_prototypes(header_text())
    assert mismatches(gpu.PROTOTYPES, declared) == []
    assert isinstance(gpu.EXPORTS, list) and gpu.EXPORTS == list(gpu.PROTOTYPES)


def test_the_comparison_can_fail():
    """On copies of the table only: nothing is ever called with wrong types."""
    gpu = _gpu()
    declared = header_prototypes(header_text())
    name = "freddy_gpu_grouping_pq"
    res, args = gpu.PROTOTYPES[name]
    at = args.index(C.c_int64)                 # int64_t n_subset
    narrowed = dict(gpu.PROTOTYPES)
    narrowed[name] = (res, args[:at] + [C.c_int32] + args[at + 1:])
    bad = mismatches(narrowed, declared)
    assert len(bad) == 1 and bad[0].startswith(name + ":"), bad
    dropped = {n: p for n, p in gpu.PROTOTYPES.items() if n != name}
    bad = mismatches(dropped, declared)
    assert len(bad) == 1 and bad[0].startswith(name + ":"), bad
    extra = dict(gpu.PROTOTYPES, freddy_gpu_no_such_call=(C.c_int, []))
    assert len(mismatches(extra, declared)) == 1
    assert mismatches(gpu.PROTOTYPES, declared) == []      # the table itself was not touched


def test_load_binds_every_function_as_the_table_says():
    gpu = _gpu()
    lib = gpu.load()
    for name, (res, args) in gpu.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype == res, name
        assert fn.argtypes is not None and list(fn.argtypes) == args, name


def test_a_library_without_some_symbols_loads_and_leaves_them_unbound(tmp_path):
    """What the timing tools rely on when they load a build of an earlier commit: a stand-in library that exports two functions
    loads (in a process of its own: a process binds one library), they are bound, and a missing one fails when it is called."""
    _gpu()
    src, so = tmp_path / "few.c", str(tmp_path / "libfew.so")
    src.write_text('#include "freddy_gpu.h"\nint freddy_gpu_abi_version(void) { return FREDDY_GPU_ABI_VERSION; }\n'
                   "int freddy_gpu_unpin(freddy_gpu_index_t* index) { return index ? FREDDY_E_ARG : FREDDY_OK; }\n")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", so, "-I" + os.path.join(ROOT, "include"), str(src)])
    child = ("import sys, ctypes\nfrom freddy_amd import gpu\n"
             "lib = gpu.load(sys.argv[1], optional=('freddy_gpu_pq_search',))\n"
             "assert lib.freddy_gpu_unpin.argtypes == [ctypes.c_void_p] and lib.freddy_gpu_unpin(None) == 0\n"
             "for name in ('freddy_gpu_pq_search', 'freddy_gpu_grouping_pq'):\n"
             "    try:\n        getattr(lib, name)\n    except AttributeError as e:\n        assert name in str(e), e\n"
             "    else:\n        raise SystemExit(name + ' is bound')\n"
             "print('ok')\n")
    path = os.pathsep.join(p for p in (os.path.join(ROOT, "postgres-word2vec_amd"), os.environ.get("PYTHONPATH")) if p)
    env = dict(os.environ, PYTHONPATH=path)
    p = subprocess.run([sys.executable, "-c", child, so], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_struct_layouts_equal_the_header(tmp_path):
    gpu = _gpu()
    structs = header_structs(header_text())
    assert set(structs) == set(STRUCTS)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "freddy_gpu.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append(f'  printf("{s} sizeof %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s} {f} %zu\\n", offsetof({s}, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layouts.c", str(tmp_path / "layouts")
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, "-I" + os.path.join(ROOT, "include"), str(src)])
    measured = {}
    for ln in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines():
        s, f, n = ln.split()
        measured.setdefault(s, {})[f] = int(n)
    for s, fields in structs.items():
        cls = getattr(gpu, STRUCTS[s])
        assert [n for n, _ in cls._fields_] == fields, s
        assert C.sizeof(cls) == measured[s]["sizeof"], s
        for f in fields:
            assert getattr(cls, f).offset == measured[s][f], (s, f)


def test_constants_equal_the_header():
    gpu = _gpu()
    defs = header_defines(header_text())
    checked = 0
    for n, v in defs.items():
        if re.match(r"FREDDY_(FOUND|METHOD|QIDS)_", n):
            assert getattr(gpu, n[len("FREDDY_"):]) == v, n
            checked += 1
    assert checked == 8
    assert gpu.ANALOGY_METHODS == {n[len("FREDDY_ANALOGY_"):].lower(): v for n, v in defs.items() if n.startswith("FREDDY_ANALOGY_")}
    assert len(gpu.ANALOGY_METHODS) == 3
    assert gpu.TOK_MAX_LEN == defs["FREDDY_TOK_MAX_LEN"]
    assert gpu.ABI_VERSION == defs["FREDDY_GPU_ABI_VERSION"]
    assert gpu.E_NOMEM == defs["FREDDY_E_NOMEM"]
    join = open(os.path.join(ROOT, "postgres-word2vec_amd", "csrc", "join.hip")).read()
    (base, shift), = re.findall(r"^static constexpr int64_t STAT_PASS = (\d+) << (\d+);", join, flags=re.M)
    assert gpu.STAT_PASS == int(base) << int(shift)
