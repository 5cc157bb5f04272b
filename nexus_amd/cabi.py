"""The ctypes signatures of the C-ABI, read from its contract: the prototypes in ``include/nexus_hip.h`` and ``include/nexus_host.h``.

Deliberately coarse: every pointer or array is a ``c_void_p`` (``const char*`` a ``c_char_p``), the scalars are their ctypes twins.
A prototype with anything else is refused with its text, never guessed at.
"""
import ctypes as C
import os
import re

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = ("nexus_hip.h", "nexus_host.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
_PROTOTYPE = re.compile(r"(.*?)\b((?:nxhip|nxh|nxs)_\w+)\s*\((.*)\)", re.S)


class NexusError(RuntimeError):
    pass


def _statements(text):
    """The declarations at file scope, one string each.  Comments, preprocessor lines and whatever stands between braces are dropped; the
    braces of ``extern "C"`` are seen through.  A function body ends its statement, so a ``static inline`` helper is one statement."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    out, cur, open_braces = [], "", []  # open_braces: True for a body, False for a linkage block
    for tok in re.split(r"([{};])", text):
        bodies = sum(open_braces)
        if tok == "{":
            linkage = not bodies and re.fullmatch(r'\s*extern\s*"C"\s*', cur) is not None
            open_braces.append(not linkage)
            cur = "" if linkage else cur + ("{}" if not bodies else "")
        elif tok == "}":
            if not open_braces:
                raise NexusError("unbalanced '}' after: %s" % " ".join(cur.split()))
            if open_braces.pop() and bodies == 1 and ")" in cur.split("{}")[0]:  # the end of a function's body
                out.append(cur)
                cur = ""
        elif tok == ";":
            if not bodies:
                out.append(cur)
                cur = ""
        elif not bodies:
            cur += tok
    if open_braces or cur.strip():
        raise NexusError("the header ends inside a declaration: %s" % " ".join(cur.split()))
    return [" ".join(s.split()) for s in out if s.strip()]


def _ctype(decl, proto, is_return):
    """The ctypes type of one parameter declaration (with or without its name) or of a return type."""
    if "*" in decl or "[" in decl:
        return C.c_char_p if re.fullmatch(r"\s*const\s+char\s*\*\s*\w*\s*", decl) else C.c_void_p
    names = re.sub(r"\b(?:const|struct)\b", " ", decl).split()
    if not is_return and len(names) > 1:
        names.pop()  # the parameter's name
    if is_return and names == ["void"]:
        return None
    if len(names) != 1 or names[0] not in SCALARS:
        raise NexusError("cannot classify '%s' in the prototype: %s" % (decl.strip(), proto))
    return SCALARS[names[0]]


def parse(text):
    """{name: (restype, [argtypes])} of every exported nxhip_* / nxh_* / nxs_* prototype in a header's text."""
    table = {}
    for s in _statements(text):
        if re.match(r"(?:typedef|static inline)\b", s) or re.fullmatch(r"(?:struct|enum|union)\b[^()]*", s):
            continue  # types, and header-only helpers such as nxhip_header_abi_stamp
        m = _PROTOTYPE.fullmatch(s)
        if not m or "(" in m.group(3) or "..." in m.group(3) or "{}" in s:
            raise NexusError("not a prototype this binding understands: %s" % s)
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        table[name] = (_ctype(ret, s, True), [_ctype(p, s, False) for p in params])
    return table


def signatures(include_dir=INCLUDE_DIR):
    """{header: {name: (restype, [argtypes])}} for the two headers of the C-ABI."""
    tables = {}
    for header in HEADERS:
        path = os.path.join(include_dir, header)
        if not os.path.exists(path):
            raise NexusError(f"{path} is missing: the binding takes its signatures from the C headers")
        with open(path) as f:
            tables[header] = parse(f.read())
    return tables
