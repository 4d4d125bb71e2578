"""A parser for include/merefusion.h -- our own header, plain and regular C -- and for nothing else.

parse(text) returns a Header:
  functions  {name: (return_type, [(type, arg_name), ...])}
  structs    {c_name: [(field, type, array_len or None), ...]}, fields in declaration order
  enums      names of the `typedef enum` types (they travel as int)
  opaque     names of the handle types (`typedef struct mf_x mf_x;`)
C types are normalised strings: "int", "const float*", "mf_nerf_head**", "const float* const*".

What it copes with is what the header contains: block comments, preprocessor lines, the `extern "C"` braces, enums, opaque and
defined struct typedefs (named or anonymous), several declarators on one line, array fields, prototypes over several lines and
`(void)`.  A declaration of any other shape, or one that uses a type nobody declared, raises CDeclError with the declaration in
the message: nothing is skipped.  _lib.py turns the result into ctypes; this module imports neither ctypes nor torch.
"""
import re
from collections import namedtuple

Header = namedtuple("Header", "functions structs enums opaque")

BUILTIN = {"void", "char", "int", "float", "double", "size_t", "int64_t", "uint32_t", "uint16_t", "int16_t", "uint8_t"}
_IDENT = r"[A-Za-z_]\w*"
# [const] base, then stars (each may carry a const) or blank, then the name, then an optional [n]
_DECLARATOR = re.compile(r"\s*(const\s+)?(%s)((?:\s*\*(?:\s*const\b)?)+\s*|\s+)(%s)\s*(?:\[\s*(\d+)\s*\])?\s*" % (_IDENT, _IDENT))


class CDeclError(ValueError):
    pass


def _statements(text):
    """top-level declarations (each up to its `;` outside braces) of comment-free, preprocessor-free text; the `extern "C"` braces are dropped"""
    out, cur, depth, c_blocks = [], [], 0, 0
    for ch in text:
        if ch in "{};" and depth == 0:
            head = " ".join("".join(cur).split())
            if ch == "{" and re.fullmatch(r'extern ?"C"', head):
                cur, c_blocks = [], c_blocks + 1
                continue
            if ch == "}":
                if c_blocks == 0 or head:
                    raise CDeclError("unbalanced '}' after: %r" % head[-80:])
                c_blocks -= 1
                continue
            if ch == ";":
                out.append(head)
                cur = []
                continue
        depth += (ch == "{") - (ch == "}")
        cur.append(ch)
    rest = "".join(cur).strip()
    if rest or depth or c_blocks:
        raise CDeclError("unterminated declaration or brace: %r" % rest[:80])
    return out


def _declarator(text, known, where):
    """'const float* const* heads' -> ('const float* const*', 'heads', None);  'int64_t shape[4]' -> ('int64_t', 'shape', 4)"""
    m = _DECLARATOR.fullmatch(text)
    if not m or "const" in (m.group(2), m.group(4)):
        raise CDeclError("no 'type name' in %r of: %s" % (text.strip(), where))
    const, base, stars, name, length = m.groups()
    if base not in known:
        raise CDeclError("unknown type %r in: %s" % (base, where))
    ctype = ("const " if const else "") + base + " ".join("".join(stars.split()).replace("*const", "* const").split())
    return ctype, name, None if length is None else int(length)


def _fields(body, known, where):
    """the members of a struct body; 'float *bg_out, *torso_alpha;' and 'int n_conv, conv_dim[8];' give one entry per declarator"""
    fields, *members, tail = [], *body.split(";")
    if tail.strip():
        raise CDeclError("no ';' after %r in: %s" % (tail.strip(), where))
    for member in members:
        first, *more = member.split(",")
        ctype, name, length = _declarator(first, known, where)
        fields.append((name, ctype, length))
        base = ctype.split("*")[0]                                          # the stars belong to each declarator, the base to the line
        fields += [(n, t, l) for t, n, l in (_declarator(base + " " + d, known, where) for d in more)]
    names = [f[0] for f in fields]
    if not fields or len(set(names)) != len(names) or any(t == "void" or t.endswith("void") for _, t, _ in fields):
        raise CDeclError("empty struct, a field named twice or a void field in: %s" % where)
    return fields


def parse(text):
    if text.count("/*") != text.count("*/"):
        raise CDeclError("unterminated block comment")
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text.replace("\\\n", " "), flags=re.M)
    h = Header({}, {}, set(), set())
    known = set(BUILTIN)

    def declare(name, where):
        if name in known or name in h.functions:
            raise CDeclError("%r is declared twice: %s" % (name, where))
        known.add(name)
        return name

    for decl in _statements(text):
        m = re.fullmatch(r"(typedef )?enum( %s)? ?\{[^{}]*\} ?(%s)?" % (_IDENT, _IDENT), decl)
        if m and bool(m.group(1)) == bool(m.group(3)):                       # typedef enum [tag] {...} name;   or constants alone: enum {...};
            if m.group(3):
                h.enums.add(declare(m.group(3), decl))
            continue
        m = re.fullmatch(r"typedef struct (%s) (%s)" % (_IDENT, _IDENT), decl)
        if m and m.group(1) == m.group(2):
            h.opaque.add(declare(m.group(2), decl))
            continue
        m = re.fullmatch(r"typedef struct( %s)? ?\{([^{}]*)\} ?(%s)" % (_IDENT, _IDENT), decl)
        if m and m.group(1) in (None, " " + m.group(3)):
            h.structs[declare(m.group(3), decl)] = _fields(m.group(2), known, decl)
            continue
        m = re.fullmatch(r"([^(){}]+)\(([^(){}]*)\)", decl)
        if m and m.group(2).strip() and not decl.startswith(("typedef ", "struct ", "enum ")):
            ret, name, length = _declarator(m.group(1), known, decl)
            args = [] if m.group(2).strip() == "void" else [_declarator(a, known, decl) for a in m.group(2).split(",")]
            if length is not None or any(l is not None or t == "void" for t, _, l in args) or len({n for _, n, _ in args}) != len(args):
                raise CDeclError("array or void argument, an array returned or an argument named twice in: %s" % decl)
            if name in known or name in h.functions:
                raise CDeclError("%r is declared twice: %s" % (name, decl))
            h.functions[name] = (ret, [(t, n) for t, n, _ in args])
            continue
        raise CDeclError("cannot classify: %s" % decl)
    return h
