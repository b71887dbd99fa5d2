"""Reads the C ABI out of include/pn2_abi.h: per declared function its ctypes return type, argument types and parameter names,
plus the integer #defines and anonymous-enum constants.  _lib.py binds the library from this, so the header is the one place an
entry point's signature is written down.  Strict: whatever it does not understand raises, naming the prototype; nothing
defaults to int.  Needs neither torch nor the library."""
import collections
import ctypes
import re

Function = collections.namedtuple("Function", "restype argtypes argnames")
Abi = collections.namedtuple("Abi", "functions constants")  # name -> Function in header order; name -> int

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
_INT = r"\(?\s*(-?\d+)\s*\)?"


def _canon(ctype):
    return " ".join(re.findall(r"\w+|\*", ctype))


def _function(proto):
    m = re.fullmatch(r"([\w\s*]+?)\s*\b(\w+)\s*\((.*)\)", proto, flags=re.S)
    if not m or _canon(m.group(1)) not in _RETURNS:
        raise ValueError("pn2 ABI header: cannot split the prototype %r into a known return type, a name and parameters" % proto)
    params = m.group(3)
    if "(" in params or "[" in params:
        raise ValueError("pn2 ABI header: array or function-pointer parameter in %r" % proto)
    argtypes, argnames = [], []
    for p in ([] if params.strip() == "void" else params.split(",")):
        pm = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(\w+)\s*", p, flags=re.S)
        ctype = _canon(pm.group(1)) if pm else ""
        if "*" in ctype:
            argtypes.append(ctypes.c_void_p)
        else:
            scalar = " ".join(t for t in ctype.split() if t != "const")
            if scalar not in _SCALARS:
                raise ValueError("pn2 ABI header: parameter %r of %r is not `<known type> <name>`" % (p.strip(), proto))
            argtypes.append(_SCALARS[scalar])
        argnames.append(pm.group(2))
    return m.group(2), Function(_RETURNS[_canon(m.group(1))], argtypes, tuple(argnames))


def parse(text):
    """header text -> Abi"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        m = re.fullmatch(_INT, value)
        if not m:
            raise ValueError("pn2 ABI header: #define %s %s is not an integer constant" % (name, value))
        constants[name] = int(m.group(1))
    for body in re.findall(r"\benum\s*\{([^}]*)\}\s*;", text):
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"(\w+)\s*=\s*" + _INT, item)
            if not m:
                raise ValueError("pn2 ABI header: enum item %r is not NAME = integer" % item)
            constants[m.group(1)] = int(m.group(2))
    # what is left after the preprocessor lines, the enums and the extern "C" braces is a run of prototypes
    text = re.sub(r"^[ \t]*#[^\n]*$|\benum\s*\{[^}]*\}\s*;|extern\s+\"C\"\s*\{|^[ \t]*\}[ \t]*$", " ", text, flags=re.M)
    *protos, rest = text.split(";")
    if rest.strip():
        raise ValueError("pn2 ABI header: no `;` after %r" % rest.strip())
    functions = {}
    for proto in protos:
        name, fn = _function(proto.strip())
        if name in functions:
            raise ValueError("pn2 ABI header: %s is declared twice" % name)
        functions[name] = fn
    return Abi(functions, constants)


def load(path):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise ImportError("the pn2 ctypes binding is read from the C header, looked for at %s: %s" % (path, e))
    return parse(text)
