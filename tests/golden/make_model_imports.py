#!/usr/bin/env python3
"""What the reference's model files ask of the modules they import (run in the DEV container only; writes
model_imports.json).    usage: make_model_imports.py <reference checkout>

Per model file: its import statements as (module, names), and every name it uses that neither an explicit import, a
builtin nor the file itself binds -- the names its two star imports (`from utils import *`, `from quantize import *`)
have to deliver -- each with the reference file whose top level defines it (models/utils.py, quantize.py, the top-level
utils.py; null: defined nowhere in the reference, dead code).  Only names are stored, no code of the reference.
"""
import ast
import builtins
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_FILES = ["models/gaussianimage_cholesky.py"]
DEFINING = ["models/utils.py", "utils.py", "quantize.py"]  # looked up in this order (quantize.py re-imports from utils.py)


def top_level_names(tree):
    out = set()
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            out.add(node.name)
        elif isinstance(node, (ast.Import, ast.ImportFrom)):
            out |= {(a.asname or a.name).split(".")[0] for a in node.names}
        elif isinstance(node, ast.Assign):
            out |= {t.id for t in node.targets if isinstance(t, ast.Name)}
    return out


def describe(tree):
    imports, bound = [], set(dir(builtins))
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            imports.append([node.module, [a.name for a in node.names]])
            bound |= {a.asname or a.name for a in node.names}
        elif isinstance(node, ast.Import):
            bound |= {(a.asname or a.name).split(".")[0] for a in node.names}
        elif isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            bound.add(node.name)
        elif isinstance(node, ast.arg):
            bound.add(node.arg)
        elif isinstance(node, ast.Name) and not isinstance(node.ctx, ast.Load):
            bound.add(node.id)
        elif isinstance(node, ast.ExceptHandler) and node.name:
            bound.add(node.name)
    used = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)}
    return imports, sorted(used - bound)


def main(ref):
    parse = lambda rel: ast.parse(open(os.path.join(ref, rel)).read())
    defined = {rel: top_level_names(parse(rel)) for rel in DEFINING}
    out = {}
    for rel in MODEL_FILES:
        imports, free = describe(parse(rel))
        out[rel] = {"imports": imports,
                    "free_names": {n: next((d for d in DEFINING if n in defined[d]), None) for n in free}}
    json.dump(out, open(os.path.join(HERE, "model_imports.json"), "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
