"""ctypes signatures and structures read from the text of include/gi2d.h, the one place the C ABI is written down.

parse(text) understands the subset of C that header is written in -- `/* */` comments, `#define NAME <integer>`,
`typedef <pointer> name;`, `[typedef] struct name { fields } [name];` and function prototypes over scalar types (`long
long` among them) and pointers -- and refuses everything else with a ValueError that quotes the declaration: a
declaration it skipped would leave a function unbound or a structure short, which is worse than no binding at all.
Standard library only.
"""
from __future__ import annotations

import ctypes as C
import keyword
import re
from typing import Dict, List, NamedTuple, Tuple

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "long_long": C.c_longlong}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p}
_POINTEES = set(_SCALARS) | {"void", "char"}  # what a `T *` may point to besides a struct or a pointer typedef

_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)([A-Za-z_]\w*)\s*(?:\[\s*(\w+)\s*\])?")
_BASE = re.compile(r"(?:const\s+)?(struct\s+)?([A-Za-z_]\w*)(?:\s+const\b)?\s*")
_FUNCTION = re.compile(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)")
_STRUCT = re.compile(r"(typedef\s+)?struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w*)")


class Abi(NamedTuple):
    functions: Dict[str, Tuple[type, List[type]]]  # name -> (restype, argtypes)
    structs: Dict[str, type]                       # name -> ctypes.Structure subclass


def _quote(decl: str) -> str:
    return "`" + " ".join(decl.split()) + "`"


def _declarations(text: str) -> List[str]:
    """The top-level declarations: split at every `;` outside braces."""
    out, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif ch == ";" and depth == 0:
            out.append(text[start:i].strip())
            start = i + 1
    if depth != 0 or text[start:].strip():
        raise ValueError(f"gi2d.h: unterminated declaration {_quote(text[start:][:200])}")
    return out


class _Parser:
    def __init__(self, text: str):
        self.plain = text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        self.bounds = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\d+)[ \t]*$",
                                                            text, flags=re.M)}
        text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
        text = re.sub(r"\blong\s+long\b", "long_long", text)  # the one two-word scalar: read as one name (_SCALARS)
        text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", text)
        if wrapped:
            body, brace, tail = text.rpartition("}")
            if not brace or tail.strip():
                raise ValueError('gi2d.h: `extern "C" {` is not closed by the last brace of the file')
            text = body
        self.text = text
        self.pointer_types = set()  # typedef names of pointers (gi2d_stream_t)
        self.struct_types = set()   # typedef names of structs, usable without the `struct` keyword
        self.functions, self.structs = {}, {}

    def ctype(self, piece: str, base: str, is_struct: bool, in_struct: bool, decl: str):
        """`piece` is one declarator (`*const *states`, `side[16]`) of type `base` -> (name, ctypes type)."""
        m = _DECLARATOR.fullmatch(piece.strip())
        if not m:
            raise ValueError(f"gi2d.h: cannot read the declarator {_quote(piece)} of {_quote(decl)}")
        stars, name, bound = m[1].count("*"), m[2], m[3]
        struct = is_struct or base in self.struct_types
        if stars:
            if not (struct or base in _POINTEES or base in self.pointer_types):
                raise ValueError(f"gi2d.h: unknown type `{base}` in {_quote(decl)}")
            typ = C.c_void_p
        elif struct:
            raise ValueError(f"gi2d.h: struct `{base}` by value in {_quote(decl)}")
        elif base in self.pointer_types:
            typ = C.c_void_p
        elif base in _SCALARS:
            typ = _SCALARS[base]
        else:
            raise ValueError(f"gi2d.h: unknown type `{base}` in {_quote(decl)}")
        if bound is not None:
            if not in_struct:
                typ = C.c_void_p  # an array parameter is a pointer
            elif bound.isdigit() or bound in self.bounds:
                typ = typ * (int(bound) if bound.isdigit() else self.bounds[bound])
            else:
                raise ValueError(f"gi2d.h: array bound `{bound}` of {_quote(decl)} is neither a literal nor a #define")
        return name, typ

    def split_base(self, decl: str):
        m = _BASE.match(decl)
        if not m or m[2] in ("const", "struct", "union", "enum"):
            raise ValueError(f"gi2d.h: cannot read the type of {_quote(decl)}")
        return m[2], bool(m[1]), decl[m.end():]

    def function(self, m, decl: str) -> None:
        ret = re.sub(r"\s*\*\s*", " *", " ".join(m[1].split()))
        if ret not in _RETURNS:
            raise ValueError(f"gi2d.h: return type `{ret}` of {_quote(decl)} is not one of {', '.join(_RETURNS)}")
        args = []
        if m[3].strip() != "void":
            for param in m[3].split(","):
                base, is_struct, rest = self.split_base(param.strip())
                args.append(self.ctype(rest, base, is_struct, False, decl)[1])
        self.functions[m[2]] = (_RETURNS[ret], args)

    def struct(self, m, decl: str) -> None:
        tag, alias = m[2], m[4]
        if alias != (tag if m[1] else ""):
            raise ValueError(f"gi2d.h: struct `{tag}` is neither `struct {tag} {{...}};` nor `typedef struct {tag} "
                             f"{{...}} {tag};`")
        fields = []
        for line in _declarations(m[3]):
            base, is_struct, rest = self.split_base(line)
            for piece in rest.split(","):  # `float *xyz, *chol, *feat;` declares three fields, in order
                name, typ = self.ctype(piece, base, is_struct, True, f"struct {tag} {{ {line}; }}")
                fields.append((name + "_" if keyword.iskeyword(name) else name, typ))
        self.structs[tag] = type(tag, (C.Structure,), {"_fields_": fields, "__doc__": f"struct {tag} (include/gi2d.h)"})
        if alias:
            self.struct_types.add(alias)

    def run(self) -> Abi:
        for decl in _declarations(self.text):
            m = _STRUCT.fullmatch(decl)
            if m:
                self.struct(m, decl)
                continue
            m = _FUNCTION.fullmatch(decl)
            if m and not decl.startswith("typedef"):
                self.function(m, decl)
                continue
            if decl.startswith("typedef"):  # only `typedef void *gi2d_stream_t;`: a name for a pointer
                base, is_struct, rest = self.split_base(decl[len("typedef"):].strip())
                name, _ = self.ctype(rest, base, is_struct, False, decl)
                if "*" not in rest:
                    raise ValueError(f"gi2d.h: only pointer typedefs are understood, got {_quote(decl)}")
                self.pointer_types.add(name)
                continue
            raise ValueError(f"gi2d.h: cannot read the declaration {_quote(decl[:300])}")
        # nothing the header declares may have slipped through: hold the result against a plain search of the text
        missed = [n for n in re.findall(r"\b(gi2d_[a-z0-9_]+)\s*\(", self.plain) if n not in self.functions]
        missed += [n for n in re.findall(r"\bstruct\s+(gi2d_\w+)\s*\{", self.plain) if n not in self.structs]
        if missed:
            raise ValueError(f"gi2d.h: declared but not parsed: {', '.join(sorted(set(missed)))}")
        return Abi(self.functions, self.structs)


def parse(text: str) -> Abi:
    """Header text -> Abi(functions: name -> (restype, argtypes), structs: name -> ctypes.Structure subclass)."""
    return _Parser(text).run()
