"""The ctypes signatures of _hip.SIGNATURES against the prototypes of include/bas.h: return type, argument count and
every argument type.  The lists are written by hand and up to 37 entries long; an `int` where the header says `long`
would truncate a stride without any other test noticing (test_library_exports_every_declared_symbol compares names)."""
import ctypes
import os
import re

from conftest import ROOT
import binaural_audio_synthesis_amd as bas

SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "double": ctypes.c_double}


def c_type(text, where):
    """The ctypes type of one C parameter or return type of bas.h: a pointer or bas_stream_t is c_void_p, the four
    scalar types map to their namesakes.  A returned `const char *` is c_char_p (ctypes then hands back bytes)."""
    t = re.sub(r"\bconst\b", " ", text)
    t = re.sub(r"\s+", " ", t).strip()
    if "*" in t or t.split(" ")[0] == "bas_stream_t":
        return ctypes.c_void_p
    base = t.split(" ")[0]
    assert base in SCALARS, f"{where}: no rule for the C type in '{text.strip()}'"
    return SCALARS[base]


def prototypes():
    hdr = open(os.path.join(ROOT, "include", "bas.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)                     # comments
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)                      # preprocessor lines
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \t\n]*?[ \t\n\*]+)(bas_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        ret = ret.replace("extern", " ").strip()
        if ret.startswith("typedef"):
            continue
        out[name] = (ret, [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


def test_the_parser_reads_the_header():
    protos = prototypes()
    assert len(protos) >= 54 and set(protos) == set(bas._hip.SIGNATURES), set(protos) ^ set(bas._hip.SIGNATURES)
    assert protos["bas_version"] == ("int", [])
    assert protos["bas_last_error"][0].replace(" ", "") == "constchar*"
    assert protos["bas_render_workspace_bytes"] == ("size_t", ["int n_src", "long T_in", "int K", "int S", "int L"])
    assert len(protos["bas_scene_params_f64"][1]) == 37
    # the rules themselves
    assert c_type("const float *x", "") is ctypes.c_void_p and c_type("bas_stream_t stream", "") is ctypes.c_void_p
    assert c_type("unsigned long long *status", "") is ctypes.c_void_p and c_type("const long *lengths", "") is ctypes.c_void_p
    assert c_type("long x_stride", "") is ctypes.c_long and c_type("int K", "") is ctypes.c_int
    assert c_type("size_t ws_bytes", "") is ctypes.c_size_t and c_type("double max_delay", "") is ctypes.c_double


def test_every_signature_matches_its_prototype():
    protos = prototypes()
    wrong = []
    for name, (res, args) in bas._hip.SIGNATURES.items():
        ret, params = protos[name]
        want_res = ctypes.c_char_p if ret.replace(" ", "") == "constchar*" else c_type(ret, name)
        if res is not want_res:
            wrong.append(f"{name}: returns {ret.strip()}, restype is {res.__name__}")
        if len(args) != len(params):
            wrong.append(f"{name}: {len(params)} parameters in bas.h, {len(args)} argtypes")
            continue
        for i, (got, p) in enumerate(zip(args, params)):
            if got is not c_type(p, name):
                wrong.append(f"{name}: argument {i} is '{p}', argtype is {got.__name__}")
    assert not wrong, "\n".join(wrong)
