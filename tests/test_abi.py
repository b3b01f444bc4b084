"""CPU-only: the C-ABI library loads and exports every symbol include/gi2d.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "gi2d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gi2d_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_twelve_reference_ops():
    syms = declared_symbols()
    for op in ["project_gaussians_2d_forward", "project_gaussians_2d_backward",
               "project_gaussians_2d_covariance_forward", "project_gaussians_2d_covariance_backward",
               "project_gaussians_2d_scale_rot_forward", "project_gaussians_2d_scale_rot_backward",
               "compute_cov2d_bounds", "map_gaussian_to_intersects", "get_tile_bin_edges",
               "rasterize_sum_forward", "rasterize_sum_backward", "rasterize_sum_plus_forward",
               "rasterize_sum_plus_backward"]:
        assert "gi2d_" + op in syms, op


def test_library_exports_every_declared_symbol():
    from gaussianimage_plus_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} declared in include/gi2d.h but not exported"


def test_python_binding_covers_every_declared_symbol():
    """The binding's tables come from the header's parser (_abi.py): what it found against the plain search above."""
    from gaussianimage_plus_amd import _lib
    bound = set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
    assert set(declared_symbols()) == bound
    assert _lib.version().startswith("gi2d")


def parsed_header():
    from gaussianimage_plus_amd import _abi
    with open(os.path.join(ROOT, "include", "gi2d.h")) as f:
        return _abi.parse(f.read())


def test_parser_pinned_signatures_and_fields():
    """One literal example per class of type the header uses, written out here and nowhere else."""
    i, u, f, d, p, sz = (ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t)
    abi = parsed_header()
    assert len(abi.functions) == len(declared_symbols()) and set(abi.functions) == set(declared_symbols())
    assert abi.functions["gi2d_train_steps"] == (i, [p, p, d, d, f, i, i, p])  # struct pointer, doubles, stream
    assert abi.functions["gi2d_fast_workspace_bytes"] == (sz, [i, i, i])
    assert abi.functions["gi2d_codec_rans_expand_delta"] == (
        i, [i, i, i, i, i, i, i, u, u, p, sz, p, p, sz, sz, p, sz, p, i, p])  # unsigned next to size_t
    assert abi.functions["gi2d_train_steps_loss_batched"] == (
        i, [i, p, p, p, sz, p, sz, p, d, d, f, i, i, p])  # `T *const *`: pointers to pointers
    assert abi.functions["gi2d_version"] == (ctypes.c_char_p, [])
    assert abi.functions["gi2d_fast_workspace_views"][1][-2:] == [p, p]  # int32_t **
    assert abi.structs["gi2d_train_quant"]._fields_ == [
        ("xy_bits", i), ("cov_bits", i), ("color_bits", i), ("defer_capacity", i),
        ("qparams", p), ("qm", p), ("qv", p), ("range", p), ("qfeat", p), ("partial", p), ("defer", p),
        ("best_qparams", p), ("dbg_qgrads", p), ("lr", d * 3), ("eps", f * 3), ("pad1", i), ("beta1", d), ("beta2", d),
        ("first_step", i), ("rot_bits", i)]
    # a bound that is a #define, fixed-width integers, and a field named like a Python keyword
    assert abi.structs["gi2d_quant_spec"]._fields_ == [
        ("channels", ctypes.c_int32), ("kind", ctypes.c_int32 * 4), ("qmin", f * 4), ("qmax", f * 4)]
    assert abi.structs["gi2d_ssim_pair"]._fields_[3] == ("x_stride", ctypes.c_int64 * 3)
    assert [n for n, _ in abi.structs["gi2d_train_loss"]._fields_][:2] == ["type", "lambda_"]


def c_compiler():
    import shutil
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    return shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)


def test_generated_structs_have_the_c_compilers_layout(tmp_path):
    """sizeof and every offsetof of every struct of the header, as the host C compiler lays them out, against the
    ctypes classes generated from the same text."""
    import keyword
    import subprocess
    cc = c_compiler()
    if cc is None:
        pytest.skip("no C compiler found (cc, clang)")
    structs = parsed_header().structs
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    assert sorted(structs) == sorted(re.findall(r"\bstruct\s+(gi2d_\w+)\s*\{", text)) and len(structs) == 10
    lines, expect = [], {}
    for name, cls in structs.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof(struct {name}));')
        expect[name] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            c_field = field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field
            lines.append(f'    printf("{name}.{field} %zu\\n", offsetof(struct {name}, {c_field}));')
            expect[f"{name}.{field}"] = getattr(cls, field).offset
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gi2d.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == expect
    assert [got[n] for n in ("gi2d_train_state", "gi2d_train_quant", "gi2d_train_loss", "gi2d_loss_image",
                             "gi2d_quant_spec", "gi2d_ssim_pair", "gi2d_codec_picture", "gi2d_codec_affine",
                             "gi2d_codec_rans_stream")] == [352, 152, 40, 64, 52, 104, 160, 36, 112]  # LP64


REFUSED = {
    "unknown type": ("int gi2d_f(int n, foo_t x);", "foo_t"),
    "unknown pointee": ("int gi2d_f(const foo_t *x);", "foo_t"),
    "function-pointer parameter": ("int gi2d_g(void (*done)(int), int n);", "gi2d_g"),
    "by-value struct parameter": ("typedef struct gi2d_s { int a; } gi2d_s;\nint gi2d_h(int n, gi2d_s s);", "gi2d_h"),
    "by-value struct field": ("struct gi2d_s { int a; };\nstruct gi2d_t { struct gi2d_s inner; };", "gi2d_t"),
    "bit-field": ("struct gi2d_b { int a; unsigned flags : 3; };", "flags"),
    "nested union": ("struct gi2d_n { int kind; union { int i; float f; } u; };", "gi2d_n"),
    "function with a body": ("int gi2d_k(int a) { return a; }\nint gi2d_ok(void);", "gi2d_k"),
    "body at the end of the file": ("int gi2d_ok(void);\nstatic inline int gi2d_k(int a) { return a; }", "gi2d_k"),
    "function-like macro": ("#define gi2d_m(x) ((x) + 1)\nint gi2d_ok(void);", "gi2d_m"),
    "unknown return type": ("long gi2d_r(void);", "gi2d_r"),
    "unknown array bound": ("struct gi2d_a { float v[GI2D_MISSING]; };", "GI2D_MISSING"),
}


def test_parser_reads_a_small_header():
    from gaussianimage_plus_amd import _abi
    ok = _abi.parse("/* c */\n#define GI2D_N 2\nstruct gi2d_a { float v[GI2D_N], *p; };\n"
                    "int gi2d_ok(const struct gi2d_a *a, float w[3]);")
    assert ok.functions == {"gi2d_ok": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])}
    assert ok.structs["gi2d_a"]._fields_ == [("v", ctypes.c_float * 2), ("p", ctypes.c_void_p)]


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_parser_refuses_what_it_cannot_read(what):
    """Each of these raises and names the declaration; none is skipped (a skipped one would be an unbound function or a
    struct whose later fields sit at the wrong offsets)."""
    from gaussianimage_plus_amd import _abi
    header, named = REFUSED[what]
    with pytest.raises(ValueError, match=named):
        _abi.parse(header)


def test_binding_reads_the_header_once_and_names_it_when_missing(monkeypatch):
    from gaussianimage_plus_amd import _lib
    assert _lib.struct("gi2d_train_state") is _lib.struct("gi2d_train_state")  # one class per process
    assert _lib.SIGNATURES["gi2d_train_render"] == [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.load().gi2d_train_render.argtypes == [ctypes.c_void_p, ctypes.c_void_p]
    monkeypatch.setattr(_lib, "_abi_parsed", None)
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(RuntimeError, match="no_such_header.h"):
        _lib.struct("gi2d_train_state")


def test_size_queries_need_no_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    assert lib.gi2d_sort_workspace_bytes(1000, 64) >= 4 * (1000 + 3 * 64)
    assert lib.gi2d_rasterize_backward_workspace_bytes(100, 1000) >= 1000 * 48
    # The layouts are part of the ABI (callers size and reuse buffers by these numbers): every region on a 256-byte
    # boundary, empty sizes counted as one element.
    exact = {
        "gi2d_sort_workspace_bytes": {(0, 0): 1280, (1000, 64): 5376, (63, 64): 1536, (123457, 1536): 513024},
        "gi2d_bin_workspace_bytes": {(0, 0): 1024, (1000, 64): 10496, (511, 1025): 101120, (200000, 1536): 947712},
        "gi2d_rasterize_backward_workspace_bytes": {(0, 0): 1280, (100, 1000): 53760, (64, 63): 4352,
                                                    (50000, 231077): 12616704},
        "gi2d_nd_rasterize_backward_workspace_bytes": {(0, 0, 1): 1280, (100, 1000, 2): 37632, (100, 1000, 3): 53760,
                                                       (64, 63, 7): 5376, (50000, 231077, 12): 20011264},
    }
    for fn, rows in exact.items():
        for args, want in rows.items():
            assert getattr(lib, fn)(*args) == want, (fn, args)


def test_quant_argument_checks_need_no_gpu():
    """Bad quantiser specs are rejected before anything is launched."""
    import ctypes as C
    from gaussianimage_plus_amd import _lib
    from gaussianimage_plus_amd.quantize import make_spec
    lib = _lib.load()
    assert lib.gi2d_quant_workspace_bytes(30000) >= (30000 // 256) * 16 * 4
    bad_kind = make_spec([7], [0], [255])
    bad_range = make_spec([0, 1], [0, 5], [255, 5])
    five = make_spec([0], [0], [255])
    five.channels = 5
    for spec in (bad_kind, bad_range, five):
        rc = lib.gi2d_quant_compress(C.byref(spec), 4, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None)
        assert rc == -1, rc
        assert b"quant" in lib.gi2d_last_error_string()
    ok = make_spec([0, 1], [0, 0], [63, 1023])
    assert lib.gi2d_quant_forward(C.byref(ok), 10, C.c_void_p(8), C.c_void_p(8), None, None, None, 0, None) == -2
    assert lib.gi2d_quant_forward(C.byref(ok), 0, None, None, None, None, None, 0, None) == 0  # empty input: nothing to do


def test_product_library_carries_no_development_switch():
    """Cut-off / knock-out / trace builds (`make VARIANT=... EXTRA=-DGI2D_...`) live under build/variants/ and say so
    in gi2d_version(); the in-tree library must be a plain build, and the loader refuses anything else."""
    import subprocess
    import sys
    from gaussianimage_plus_amd import _lib
    assert "dev[" not in _lib.version(), _lib.version()
    variant = os.path.join(ROOT, "build", "variants")
    libs = [os.path.join(d, "libgi2d_hip.so") for d, _, f in os.walk(variant) if "libgi2d_hip.so" in f] \
        if os.path.isdir(variant) else []
    for path in libs[:1]:  # any development library in the tree: loading it without the override must fail
        ver = ctypes.CDLL(path).gi2d_version
        ver.restype = ctypes.c_char_p
        if b"dev[" not in ver():
            continue
        env = dict(os.environ, GI2D_LIB=path)
        env.pop("GI2D_ALLOW_DEV_BUILD", None)
        r = subprocess.run([sys.executable, "-c", "from gaussianimage_plus_amd import _lib; _lib.load()"], cwd=ROOT,
                           env=env, capture_output=True, text=True)
        assert r.returncode != 0 and "development build" in r.stderr
