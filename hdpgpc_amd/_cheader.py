"""include/hdpgpc_hip.h as ctypes: the one place the C boundary is read.  Pure text in, ctypes types out - no library, no torch."""
import ctypes
import re

_SCALAR = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32}
_DECL = re.compile(r"((?:const\s+)?(\w+))\s*(\*{0,2})\s*(\w+)(?:\s*\[(\d+)\])?$")     # (const base) stars name [count]
_RET = re.compile(r"(?:const\s+)?(\w+)\s*(\*{0,2})$")
_TYPEDEF = re.compile(r"typedef\s+struct\s+(\w+)\s*(?:\{([^{}]*)\}\s*)?(\w+)\s*;\s*")
_FUNC = re.compile(r"([^;{}()]+?)\b(\w+)\s*\(([^;{}()]*)\)\s*;\s*")


def _declarator(text, pointees, where, array_ok=False):
    """`const double* st[8]` -> ("st", c_void_p * 8, "const double"); anything that does not map completely raises."""
    m = _DECL.match(" ".join(text.split()))
    if not m or (m[5] and not array_ok) or m[2] not in (pointees if m[3] else _SCALAR):
        raise ValueError(f"hdpgpc_hip.h: cannot map {text.strip()!r} in {where}")
    prefix, base, stars, name, count = m.groups()
    if not stars:
        t = _SCALAR[base]
    elif stars == "**":
        t = ctypes.POINTER(ctypes.c_void_p)
    elif name.endswith("_host") and base in _SCALAR:                  # the header's convention: `_host` = host memory, typed
        t = ctypes.POINTER(_SCALAR[base])
    else:
        t = ctypes.c_void_p                                           # device pointers (and `void* stream`) travel as integers
    return name, (t * int(count) if count else t), prefix


def parse_header(text):
    """The C boundary as the header's text states it: ({function: (restype, [argtypes])}, {struct: [(field, ctype)]} for every
    `typedef struct NAME { ... } NAME;` with a body, {NAME: int} for every integer #define).  Strict: a declaration that does
    not map completely onto ctypes raises ValueError naming it - nothing is guessed and nothing is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S).strip()
    pointees = {"void", *_SCALAR, *re.findall(r"typedef\s+struct\s+(\w+)", text)}
    funcs, structs, pos = {}, {}, 0
    while pos < len(text):
        m = _TYPEDEF.match(text, pos) or _FUNC.match(text, pos)
        if not m or (m.re is _TYPEDEF and m[1] != m[3]):
            raise ValueError(f"hdpgpc_hip.h: cannot parse the declaration at {' '.join(text[pos:pos + 120].split())!r}")
        pos = m.end()
        if m.re is _TYPEDEF:
            if m[2] is not None:
                fields = structs[m[1]] = []
                for stmt in filter(str.strip, m[2].split(";")):
                    first, *more = stmt.split(",")
                    name, t, prefix = _declarator(first, pointees, f"struct {m[1]}", array_ok=True)
                    fields.append((name, t))
                    fields += [_declarator(f"{prefix} {d}", pointees, f"struct {m[1]}", array_ok=True)[:2] for d in more]
            continue
        ret, name, args = m.groups()
        r = _RET.match(" ".join(ret.split()))
        if not r or not (r[1] in _SCALAR and not r[2] or r[1] == "void" and not r[2] or len(r[2]) == 1 and r[1] in pointees):
            raise ValueError(f"hdpgpc_hip.h: cannot map the return type {ret.strip()!r} of {name}")
        restype = ctypes.c_void_p if r[2] else _SCALAR.get(r[1])     # `void` -> None
        args = [] if args.strip() == "void" else [_declarator(a, pointees, name)[1] for a in args.split(",")]
        funcs[name] = (restype, args)
    return funcs, structs, defines
