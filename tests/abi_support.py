"""Shared helpers of the ABI suites (tests/test_*_abi.py, tests/test_binding_cpu.py): the built and bound library, the headers' NPB_API
prototypes, the compiled sizeof / offsetof probe, and the drivers of the "exported, bound, NULL handle refused" and refusal-table checks."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

from nuclear_sim_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nuclear_sim_amd", "libnpb.so")
HEADERS = ("npb.h", "npb_seeds.h")      # the headers with NPB_API declarations


@functools.lru_cache(None)
def library():
    """libnpb.so built (if absent) and bound: _lib.load()"""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nuclear_sim_amd", "csrc"), "-s"])
    return _lib.load()


@functools.lru_cache(None)
def header_text(name="npb.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def define(name, header="npb.h"):
    """the integer of ``#define NAME <digits>``"""
    return int(re.search(r"#define %s (\d+)" % name, header_text(header)).group(1))


@functools.lru_cache(None)
def declared():
    """{name: (return type, [parameter type, ...])} of every NPB_API declaration of HEADERS, comments stripped, a declaration taken up to
    its semicolon however many lines it spans; types as written, without the parameter's name, one space between words and before the
    ``*``s (``const double *``, ``void **``).  Every NPB_API occurrence outside comments and preprocessor lines must parse."""
    out = {}
    for header in HEADERS:
        text = re.sub(r"/\*.*?\*/", " ", header_text(header), flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^[ \t]*#[^\n]*(?:\\\n[^\n]*)*", " ", text, flags=re.M)
        found = re.findall(r"\bNPB_API\b([^;(]*?)\b(npb_\w+)\s*\(([^;]*)\)\s*;", text)
        assert len(found) == len(re.findall(r"\bNPB_API\b", text)), "%s: an NPB_API declaration did not parse" % header
        for ret, name, params in found:
            assert name not in out and "(" not in params, name
            types = [_c_type(ret)] + [_c_type(re.sub(r"\b\w+\s*(\[\s*\w*\s*\])?$", lambda m: "*" if m.group(1) else "", p.strip()))
                                      for p in params.split(",") if params.strip() != "void"]
            assert all(types), (name, types)
            out[name] = (types[0], types[1:])
    return out


def _c_type(text):
    return re.sub(r"\s*(\*+)\s*", r" \1", " ".join(text.split())).strip()


def layout(structs):
    """[sizeof, offset of every field ...] of each ctypes class of ``structs`` ({C name: class}), in order: what ``probe`` must print"""
    return [x for S in structs.values() for x in [ctypes.sizeof(S)] + [getattr(S, f[0]).offset for f in S._fields_]]


@functools.lru_cache(None)
def _run_probe(source, std):
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        open(src, "w").write(source)
        subprocess.check_call([os.environ.get("CC", "gcc")] + (["-std=" + std] if std else []) + ["-I", os.path.join(ROOT, "include"), "-o", exe, src])
        return tuple(int(x) for x in subprocess.check_output([exe]).split())


def probe(structs, constants=(), rename=None, std=None):
    """What the C compiler ($CC, gcc by default; ``std``: e.g. "c99") makes of include/npb.h: (layouts, values).  ``layouts``: sizeof and
    the offsetof of every field of the paired ctypes class, per entry of ``structs`` ({C name: class}) as ``layout`` orders them;
    ``rename``: {ctypes field name: C member name} where the two differ.  ``values``: the integer C expressions of ``constants``."""
    rename = rename or {}
    lines = []
    for c_name, S in structs.items():
        lines.append('  printf("%%zu\\n", sizeof(%s));\n' % c_name)
        lines += ['  printf("%%zu\\n", offsetof(%s, %s));\n' % (c_name, rename.get(f[0], f[0])) for f in S._fields_]
    lines += ['  printf("%%lld\\n", (long long)(%s));\n' % c for c in constants]
    got = list(_run_probe('#include <stdio.h>\n#include <stddef.h>\n#include "npb.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n", std))
    n = len(got) - len(constants)
    return got[:n], got[n:]


def check_exported(names):
    library()
    raw = ctypes.CDLL(LIB)
    for s in names:
        assert hasattr(raw, s), "libnpb.so does not export %s" % s


def check_bound(names):
    L = library()
    for s in names:
        assert getattr(L, s).argtypes is not None, s


def check_null_refused(calls):
    """``calls``: (name, arguments): each returns -1 (the first argument, the handle, is NULL)"""
    L = library()
    for name, *args in calls:
        assert getattr(L, name)(*args) == -1, name


def check_entry_points(names, calls=()):
    check_exported(names)
    check_bound(names)
    check_null_refused(calls)


def why(check, *args):
    """the reason a library check (npb_*_check) gives, or None"""
    r = check(*args)
    return None if r is None else r.decode()


def set_path(path, value):
    """a change of a refusal table: walks ``path`` from the suite's descriptor holder (a name = an attribute, an int = an index) and sets
    the last step to ``value``"""
    def change(D):
        obj = D
        *head, last = path
        for name in head:
            obj = obj[name] if isinstance(name, int) else getattr(obj, name)
        if isinstance(last, int):
            obj[last] = value
        else:
            setattr(obj, last, value)
    return change


def set_members(**members):
    """a change of a refusal table: sets members of the holder's descriptor ``D.d``"""
    def change(D):
        for name, value in members.items():
            setattr(D.d, name, value)
    return change


def both(*changes):
    def change(D):
        for c in changes:
            c(D)
    return change


def check_refusal(make, why_of, prefix, what, change, reason, kw=None):
    """one row of a refusal table: a fresh ``make()`` with ``change`` applied is refused by ``why_of(D, **kw)``, the text starting with
    ``prefix`` and holding ``reason``.  A ``change`` of None is the row "n_plants": nothing changed, asked with n=0."""
    D = make()
    if change is None:
        kw = {"n": 0}
    else:
        change(D)
    got = why_of(D, **(kw or {}))
    assert got is not None and got.startswith(prefix) and reason in got, (what, got)
