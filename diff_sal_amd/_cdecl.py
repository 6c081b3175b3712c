"""Reader of the declarations in include/diffsal.h, from which _lib.py derives its ctypes binding.

Not a C parser: it reads the forms that header uses -- /* */ comments, `#define DIFFSAL_X <integer>[u]`, the
`#ifdef __cplusplus` guards, enums whose enumerators all carry `= value`, `typedef struct X {...} X;`, the stream handle typedef
and prototypes of `diffsal_*` functions over a closed vocabulary of types -- and raises ValueError on anything else.  C types are
kept as spellings with single spaces and `*` attached to the left ("const void* const*"); ctype() maps a spelling to ctypes.
"""
import collections
import ctypes as C
import re

Decls = collections.namedtuple("Decls", "prototypes structs constants")

SCALARS = {
    "int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned int": C.c_uint, "unsigned long long": C.c_uint64,
    "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "diffsal_stream_t": C.c_void_p,
}
_POINTEES = set(SCALARS) | {"void", "char", "unsigned char"}
_WORDS = {w for t in _POINTEES for w in t.split()} | {"const"}
_INT = r"(-?\d+)[uU]?"


def ctype(spelling, structs):
    """ctypes type of a C type spelling.  `structs` maps the names of the known structs to the Structure a single pointer to
    them is passed as, or to None; every other pointer, of any depth, travels as an integer (c_void_p)."""
    if spelling in SCALARS:
        return SCALARS[spelling]
    if spelling == "const char*":
        return C.c_char_p
    m = re.fullmatch(r"(?:const )?(\w+(?: \w+)*?)(?: const)?((?:\*(?: const)?)+)", spelling)
    if not m or not (m.group(1) in _POINTEES or m.group(1) in structs):
        raise ValueError(f"type {spelling!r} is outside the binding's vocabulary")
    by_ref = structs.get(m.group(1)) if m.group(2).count("*") == 1 else None
    return C.POINTER(by_ref) if by_ref is not None else C.c_void_p


def structure(name, fields, structs, doc=None):
    """ctypes.Structure subclass `name` with the parsed `fields` [(field, spelling)]."""
    return type(name, (C.Structure,), {"_fields_": [(f, ctype(t, structs)) for f, t in fields], "__doc__": doc})


def _declarator(text, structs, named):
    """`const float* x` -> ("const float*", "x"); the name is None for an unnamed parameter."""
    tokens = re.findall(r"\w+|\S", text)
    name = None
    if len(tokens) > 1 and re.fullmatch(r"[A-Za-z_]\w*", tokens[-1]) and tokens[-1] not in _WORDS and tokens[-1] not in structs:
        name = tokens.pop()
    if named and name is None:
        raise ValueError(f"no field name in {text.strip()!r}")
    spelling = " ".join(tokens).replace(" *", "*")
    ctype(spelling, dict.fromkeys(structs))      # the vocabulary is closed: an unknown type is an error here, not where it is first used
    return spelling, name


def parse(text):
    """Header text -> Decls(prototypes {name: (return type, [parameter types])}, structs {name: [(field, type)]},
    constants {name: int}), each in header order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef __cplusplus\b.*?^[ \t]*#[ \t]*endif\b.*?$", "", text, flags=re.S | re.M)
    constants, structs, prototypes = {}, {}, {}
    for name, value in re.findall(rf"^[ \t]*#[ \t]*define[ \t]+(DIFFSAL_\w+)[ \t]+{_INT}[ \t]*$", text, flags=re.M):
        constants[name] = int(value)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\btypedef\s+void\s*\*\s*diffsal_stream_t\s*;", "", text)

    def enum(m):
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            e = re.fullmatch(rf"(\w+)\s*=\s*{_INT}", item)
            if not e:
                raise ValueError(f"enumerator {item!r} has no explicit integer value")
            constants[e.group(1)] = int(e.group(2))
        return ""

    def struct(m):
        if m.group(1) != m.group(3):
            raise ValueError(f"struct {m.group(1)} is given the other name {m.group(3)}")
        fields = []
        for line in filter(None, (s.strip() for s in m.group(2).split(";"))):
            try:
                first, *more = line.split(",")
                spelling, name = _declarator(first, structs, named=True)
                for n in [name] + [s.strip() for s in more]:
                    if not re.fullmatch(r"[A-Za-z_]\w*", n):
                        raise ValueError(f"declarator {n!r}")
                    fields.append((n, spelling))
            except ValueError as e:
                raise ValueError(f"struct {m.group(1)}: {e}") from None
        structs[m.group(1)] = fields
        return ""

    text = re.sub(r"\benum\s*\{(.*?)\}\s*;", enum, text, flags=re.S)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(diffsal_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise ValueError(f"not a declaration this reader knows: {' '.join(stmt.split())[:80]!r}")
        try:
            params = [] if m.group(3).strip() == "void" else [_declarator(p, structs, named=False)[0] for p in m.group(3).split(",")]
            prototypes[m.group(2)] = (_declarator(m.group(1), structs, named=False)[0], params)
        except ValueError as e:
            raise ValueError(f"{m.group(2)}: {e}") from None
    return Decls(prototypes, structs, constants)
