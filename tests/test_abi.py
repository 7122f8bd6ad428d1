"""include/*.h <-> _C.ABI <-> what the built libraries export, header by header (host only: no kernel is called).

Names: the functions a header declares are the keys of its table.  Types: every prototype's return and parameter types, and
the fields of the two descriptor structs, are the ctypes the table states -- a c_float where the prototype says int64_t would
bind, pass every name check and corrupt the call.  Exports: the emulated build and libadp_hip.so export every declared name,
and the source that implements an extension header includes it.  (Which entry points a header's placement file places is
asserted there, beside its cases: test_every_*_entry_point_is_placed.)"""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_int

import pytest

from audio_diffusion_pytorch_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"adp_conv_desc": _C.ConvDesc, "adp_wgrad_desc": _C.WgradDesc}
SCALARS = {"int64_t": _C.I, "float": _C.F, "int": c_int}
# the headers whose entry points share a prefix of their own: the library exports no other name under it
PREFIX = {"adp_ar.h": "adp_arv_", "adp_lt.h": "adp_lt_", "adp_enc.h": "adp_enc_", "adp_t5.h": "adp_t5_",
          "adp_clip.h": "adp_clip_", "adp_gated.h": "adp_gated_", "adp_rf.h": "adp_rf_"}


def code_of(header):
    """The header without its comments (they name functions of other headers)."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def ctype_of(decl):
    """'const float* x' / 'int64_t n' / 'void' (a return type) -> the ctypes type of the table."""
    decl = decl.replace("const", " ").strip()
    if "*" in decl:
        base = decl.split("*")[0].strip()
        return POINTER(STRUCTS[base]) if base in STRUCTS else c_char_p if base == "char" else _C.P
    return SCALARS[decl.split()[0]]


def prototypes(header):
    """name -> (restype, argtypes) as the header's prototypes state them."""
    found = {}
    for res, name, params in re.findall(r"\b(int64_t|int)\s+(adp_\w+)\s*\(([^)]*)\)\s*;", code_of(header)):
        assert name not in found, name
        found[name] = (SCALARS[res], [] if params.strip() == "void" else [ctype_of(q) for q in params.split(",")])
    return found


def fields(header, struct):
    """[(field, ctypes type)] of `typedef struct <struct> { ... } <struct>;`, in order."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), code_of(header), flags=re.S).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")
        out += [(n.strip(), ctype_of(first)) for n in [re.split(r"[\s*]+", first.strip())[-1]] + more]
    return out


def exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", _C.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in syms.splitlines() if ln.split() and ln.split()[-1].startswith("adp_")}


def test_the_table_has_one_entry_per_header_file():
    assert sorted(_C.ABI) == sorted(os.listdir(os.path.join(ROOT, "include")))
    assert set(_C.HEADER_SOURCE) == set(_C.ABI) - {"adp.h"}
    assert sum(len(t) for t in _C.ABI.values()) == len(_C.SIGNATURES) and all(_C.ABI.values())


@pytest.mark.parametrize("header", list(_C.ABI))
def test_names(header):
    declared = set(re.findall(r"\b(adp_[a-z0-9_]+)\s*\(", code_of(header))) - set(STRUCTS)
    assert declared == set(_C.ABI[header]), declared ^ set(_C.ABI[header])
    assert declared == set(prototypes(header)), "a declaration the prototype pattern of this test does not read"


@pytest.mark.parametrize("header", list(_C.ABI))
def test_types(header):
    problems = []
    for name, (res, args) in prototypes(header).items():
        want_res, want_args = _C.ABI[header][name]
        if res is not want_res:
            problems.append(f"{name}: returns {res.__name__} in {header}, {want_res.__name__} in the table")
        if len(args) != len(want_args):
            problems.append(f"{name}: {len(args)} parameters in {header}, {len(want_args)} in the table")
        problems += [f"{name}: parameter {i} is {a.__name__} in {header}, {b.__name__} in the table"
                     for i, (a, b) in enumerate(zip(args, want_args)) if a is not b]
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("struct", list(STRUCTS))
def test_descriptor_fields(struct):
    assert fields("adp.h", struct) == list(STRUCTS[struct]._fields_)


@pytest.mark.parametrize("header", list(_C.ABI))
def test_exports(emul, header):
    declared = set(_C.ABI[header])
    for name in declared:
        assert hasattr(_C.lib(), name), name            # the emulated build of the same sources
    assert os.path.exists(_C.LIB_PATH), "libadp_hip.so is not built (run __graft_entry__.build())"
    hip_lib = ctypes.CDLL(_C.LIB_PATH)
    for name in declared:
        assert hasattr(hip_lib, name), name
    if header == "adp.h":
        assert hip_lib.adp_version() >= 100
    else:
        source = open(os.path.join(ROOT, "audio_diffusion_pytorch_amd", "csrc", _C.HEADER_SOURCE[header])).read()
        assert f'#include "{header}"' in source
    if header in PREFIX:   # the library's dynamic symbol table holds exactly the names the header declares under its prefix
        under = {name for name in exported() if name.startswith(PREFIX[header])}
        assert under == declared, under ^ declared


def test_the_library_exports_nothing_undeclared():
    assert os.path.exists(_C.LIB_PATH), "libadp_hip.so is not built (run __graft_entry__.build())"
    assert exported() == set(_C.SIGNATURES), exported() ^ set(_C.SIGNATURES)
