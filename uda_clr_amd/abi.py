"""The C ABI as ctypes objects, read from include/uda_clr_hip.h: the header is the one place where a constant, an argument block
or a signature is written down.  Needs no GPU and no library.  ``read_header`` reads that header's dialect and is no C parser:
comments, preprocessor lines, the extern "C" braces, ``typedef struct`` blocks and prototypes - whatever else it meets, it raises.
Types: int, int32_t, int64_t, uint64_t, size_t, float, double by value; [const] char* = c_char_p; a pointer to a struct of the
header = POINTER(that struct); any other pointer = c_void_p."""
import ctypes as C
import os
import re

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uda_clr_hip.h")
_VALUE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
          "float": C.c_float, "double": C.c_double}


def _ctype(text, structs, decl):
    """the ctypes type of the type ``text`` of one declarator of the declaration ``decl``"""
    base, stars = re.fullmatch(r"(.*?)(\**)", re.sub(r"\bconst\b|\s", "", text)).groups()
    if not stars and (base in _VALUE or base in structs):
        return _VALUE.get(base) or structs[base]
    if stars and re.fullmatch(r"\w+", base):
        if base + stars == "char*":
            return C.c_char_p
        return C.POINTER(structs[base]) if base in structs and stars == "*" else C.c_void_p
    raise ValueError("uda_clr_hip.h: type %r in `%s`" % (text.strip(), decl))


def read_header(text):
    """header text -> (CONSTANTS {name: int}, STRUCTS {typedef name: ctypes.Structure}, SYMBOLS {name: (restype, argtypes)})"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#define[ \t]+(UDA_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    structs, symbols = {}, {}

    def declarator(text, decl):         # "const float* x" -> ("const float*", "x")
        m = re.fullmatch(r"\s*(.*\W)(\w+)\s*", text, flags=re.S)
        if not m:
            raise ValueError("uda_clr_hip.h: declarator %r in `%s`" % (text.strip(), decl))
        return m[1], m[2]

    def struct(m):
        decl, fields = "typedef struct %s" % m[1], []
        for member in filter(str.strip, m[2].split(";")):
            first, *more = member.split(",")            # "int32_t N, H, W, C": by-value types only
            kind, name = declarator(first, decl)
            if more and "*" in kind:
                raise ValueError("uda_clr_hip.h: several pointers in one member `%s` of `%s`" % (member.strip(), decl))
            fields += [(n.strip(), _ctype(kind, structs, decl)) for n in [name] + more]
        structs[m[3]] = type(m[3], (C.Structure,), {"_fields_": fields})
        return " "

    rest = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    *statements, tail = rest.split(";")
    for s in statements:
        decl = " ".join(s.split())
        m = re.fullmatch(r"(.*\W)(\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise ValueError("uda_clr_hip.h: cannot read `%s`" % decl)
        params = [] if m[3].strip() == "void" else m[3].split(",")
        symbols[m[2]] = (_ctype(m[1], structs, decl), [_ctype(declarator(p, decl)[0], structs, decl) for p in params])
    if tail.strip():
        raise ValueError("uda_clr_hip.h: cannot read `%s`" % " ".join(tail.split()))
    return constants, structs, symbols


if not os.path.exists(_HEADER):
    raise RuntimeError("include/uda_clr_hip.h not found at %s: the bindings are read from it" % _HEADER)
with open(_HEADER) as _f:
    CONSTANTS, STRUCTS, SYMBOLS = read_header(_f.read())
