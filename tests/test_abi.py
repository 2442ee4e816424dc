"""CPU-only checks of the C-ABI boundary: the library loads, exports every symbol include/gsrast.h
declares, validates arguments without touching a GPU, and the drop-in Python surface has the
reference's shape (gaussian_renderer/__init__.py:36-51,85-93)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def test_header_symbols_are_exported(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert {"gsr_forward_preprocess", "gsr_forward_render", "gsr_backward_render", "gsr_backward_geom",
            "gsr_mark_visible", "gsr_workspace_sizes", "gsr_binning_size", "gsr_version", "gsr_last_error"} <= declared
    lib = native.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in gsrast.h but not exported"
    assert set(native.EXPORTS) == declared
    assert lib.gsr_version() == 12


def test_argument_validation_without_gpu(native):
    lib = native.load()
    bad = native.make_desc(10, 5, 16, 64, 64, 0.5, 0.5, 1.0, False, False)
    g, i = C.c_size_t(0), C.c_size_t(0)
    assert lib.gsr_workspace_sizes(C.byref(bad), C.byref(g), C.byref(i)) == -1
    assert b"sh_degree" in lib.gsr_last_error()
    ok = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    gb, ib = native.workspace_sizes(ok)
    assert gb >= 1000 * 57 and ib >= 100 * 60 * 8 + 7 * 4 * 8
    # six u32 and one flag byte per instance, one 4 KB checkpoint per segment of them, the blend backward's unit lists
    seg = native.bwd_segment_entries()
    assert 5000 * 25 + (5000 // seg) * 4096 <= native.binning_size(ok, 5000) < 5000 * 25 + (5000 // seg + 2) * 4096 + 64 * (5000 // seg + 1 + 16 * 8 * 5) + 4096
    # backward-only gradient rows: 48 B per EMITTED instance; the emission bound when the count stayed on the device
    plan = native.FramePlan(); plan.instances_emitted = 1234
    assert 1234 * 48 <= native.backward_rows_size(ok, plan) < 1234 * 48 + 512
    plan.instances_emitted = -1; plan.chunks_run = 2; plan.chunk_instances_max[0] = 1000; plan.chunk_instances_max[1] = 500
    assert 1500 * 48 <= native.backward_rows_size(ok, plan) < 1500 * 48 + 512
    with pytest.raises(native.GsrError, match="sh_coeffs"):
        native.workspace_sizes(native.make_desc(10, 1, 99, 64, 64, 0.5, 0.5, 1.0, False, False))
    # exactly-one-of rules are enforced at the ABI too (NULL device pointers are never dereferenced here)
    cam = native.Camera(1, 1, 1, 1)
    gs = native.Gaussians(1, None, None, 1, 1, 1, None)
    plan = native.FramePlan()
    rc = lib.gsr_forward_preprocess(C.byref(ok), C.byref(cam), C.byref(gs), C.c_void_p(1), None, C.c_void_p(1), C.byref(plan), None)
    assert rc == -1 and b"shs / colors_precomp" in lib.gsr_last_error()


def test_python_surface_matches_reference_call_site():
    import diff_gaussian_rasterization as dgr
    assert dgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")
    rs = dgr.GaussianRasterizationSettings(8, 8, .5, .5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                           torch.zeros(3), False, False)
    r = dgr.GaussianRasterizer(raster_settings=rs)
    z = torch.zeros(4, 3)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=z, means2D=z, opacities=torch.zeros(4, 1), scales=z, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair"):
        r(means3D=z, means2D=z, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3))
    # CPU tensors: the product has no CPU path and says so
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(means3D=z, means2D=z, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3), scales=z, rotations=torch.zeros(4, 4))
    assert hasattr(r, "markVisible")
    import gaussian_renderer
    assert callable(gaussian_renderer.render)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "structured-gaussian-splatting_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "libgsr_oracle" not in src, f


def test_python_mirror_of_binning_size_matches_the_library():
    """diff_gaussian_rasterization._binning_bytes / the first-chunk capacity rule are evaluated in Python between the plan
    readback and the first launch of stage 2 (no ctypes round trips while the stream idles): they must equal the C ABI's."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    desc = N.make_desc(1000, 3, 16, 640, 480, 0.5, 0.5, 1.0, False, False)
    for n in (0, 1, 63, 64, 65, 1000, 123_457, 28_201_899, 492_421_683):
        assert dgr._binning_bytes(n, 40 * 30) == N.binning_size(desc, n), n
    plan = N.FramePlan()
    for chunks, first, R in ((1, 500, 500), (3, 2_000_000, 28_000_000), (2, 900_000, 1_000_000), (4, 10, 5_000_000_000)):
        plan.num_chunks, plan.num_rendered = chunks, R
        plan.chunk_instances_max[0] = first
        want = min(first + first // 4 + (1 << 20), R) if chunks > 1 else R
        assert N.binning_first_chunk_capacity(plan) == want


# ---- the header, read as text -----------------------------------------------------------------------------------------------------

def _header():
    """include/gsrast.h without its comments."""
    with open(os.path.join(ROOT, "include", "gsrast.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


PROTOTYPE = re.compile(r"^\s*(int|const char \*)\s*(gsr_\w+)\s*\(([^;{]*)\)\s*;", re.M)
SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int}


def header_prototypes(code):
    """{name: (return type, [parameter declarations])} of every function the header declares."""
    out = {}
    for ret, name, params in PROTOTYPE.findall(code):
        params = " ".join(params.split())
        out[name] = (ret, [] if params == "void" else [p.strip() for p in params.split(",")])
    return out


def header_struct_typedefs(code):
    return re.findall(r"\btypedef\s+struct\s+(gsr_\w+)", code)


def signature_mismatches(protos, table, mirrors):
    """What the binding's table says differently from the header's prototypes, one line each (empty: they agree)."""
    bad = [f"{n}: in the header, not in the table" for n in protos if n not in table]
    bad += [f"{n}: in the table, not in the header" for n in table if n not in protos]
    for name, (ret, params) in protos.items():
        if name not in table:
            continue
        restype, argtypes = table[name]
        if restype is not {"int": C.c_int, "const char *": C.c_char_p}[ret]:
            bad.append(f"{name}: returns {ret}, the table says {restype}")
        if len(params) != len(argtypes):
            bad.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
            continue
        for i, (decl, got) in enumerate(zip(params, argtypes)):
            m = re.fullmatch(r"(?:const )?(gsr_\w+) \*\w+", decl)
            if m:                                                   # [const] gsr_X *: the mirror of gsr_X, and no other
                ok = m.group(1) in mirrors and got is C.POINTER(mirrors[m.group(1)])
            elif "*" in decl or "[" in decl:                        # any other pointer: void *, or a pointer to the matching scalar
                base = re.sub(r"\bconst\b", "", decl.split("*")[0]).strip()
                pointee = C.c_void_p if decl.count("*") == 2 else SCALARS.get(base)
                ok = got is C.c_void_p or (pointee is not None and got is C.POINTER(pointee))
            else:                                                   # a scalar: exactly its type
                ok = got is SCALARS[decl.rsplit(" ", 1)[0]]
            if not ok:
                bad.append(f"{name}: parameter {i} is `{decl}`, the table says {got.__name__}")
    return bad


def test_signature_table_matches_every_prototype_of_the_header(native):
    code = _header()
    protos = header_prototypes(code)
    # every `gsr_x(` of the header outside a #define is a prototype this parser read: one it cannot read fails here
    assert len(protos) == len(set(re.findall(r"\b(gsr_\w+)\s*\(", re.sub(r"^\s*#.*$", "", code, flags=re.M)))) == 77
    assert set(header_struct_typedefs(code)) == set(native.MIRRORS)
    bad = signature_mismatches(protos, native.SIGNATURES, native.MIRRORS)
    assert not bad, "\n".join(bad)
    assert native.EXPORTS == tuple(native.SIGNATURES)
    lib = native.load()
    for name, (restype, argtypes) in native.SIGNATURES.items():      # load() applied the table to the CDLL it returns
        assert getattr(lib, name).restype is restype and tuple(getattr(lib, name).argtypes) == tuple(argtypes), name


def test_selfcheck_signature_mismatches_are_reported(native):
    protos = header_prototypes(_header())

    def mutated(name, f):
        table = dict(native.SIGNATURES)
        restype, argtypes = table[name]
        table[name] = (restype, tuple(f(list(argtypes))))
        return signature_mismatches(protos, table, native.MIRRORS)

    assert signature_mismatches(protos, native.SIGNATURES, native.MIRRORS) == []
    bad = mutated("gsr_forward", lambda a: a[:-1])                                                   # a parameter dropped
    assert len(bad) == 1 and "gsr_forward: 12 parameters, the table has 11" in bad[0], bad
    bad = mutated("gsr_binning_size", lambda a: [a[0], C.c_int32, a[2]])                             # int64_t bound as int32
    assert len(bad) == 1 and "gsr_binning_size: parameter 1 is `int64_t num_rendered`" in bad[0], bad
    bad = mutated("gsr_forward_preprocess", lambda a: [a[1], a[0]] + a[2:])                          # two struct types swapped
    assert len(bad) == 2 and all("gsr_forward_preprocess: parameter" in b for b in bad), bad
    bad = mutated("gsr_backward_rows_size", lambda a: [a[0], C.POINTER(native.FrameDesc), a[2]])     # a FrameDesc for a plan
    assert len(bad) == 1 and "const gsr_frame_plan *plan_host" in bad[0], bad
    bad = mutated("gsr_workspace_sizes", lambda a: [a[0], C.POINTER(C.c_int32), a[2]])               # a pointer to the wrong scalar
    assert len(bad) == 1 and "size_t *geom_bytes" in bad[0], bad
    bad = mutated("gsr_adam_step", lambda a: a[:5] + [C.c_double] + a[6:])                           # float bound as double
    assert len(bad) == 1 and "float lr" in bad[0], bad
    table = dict(native.SIGNATURES)
    del table["gsr_vq_update"]
    table["gsr_last_error"] = (C.c_int, ())
    bad = signature_mismatches(protos, table, native.MIRRORS)
    assert len(bad) == 2 and any("gsr_vq_update: in the header, not in the table" in b for b in bad) and any("gsr_last_error: returns" in b for b in bad)
    mirrors = dict(native.MIRRORS)
    del mirrors["gsr_camera"]                                                                        # a struct without a mirror
    assert any("const gsr_camera *cam" in b for b in signature_mismatches(protos, native.SIGNATURES, mirrors))


def test_typed_calls_refuse_what_the_header_does_not_declare(native):
    """With argtypes set, a wrong arity or a mirror of another struct is an error of the call, not undefined behaviour."""
    lib = native.load()
    desc = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    g, i = C.c_size_t(0), C.c_size_t(0)
    with pytest.raises(TypeError):
        lib.gsr_workspace_sizes(desc, g)
    with pytest.raises(C.ArgumentError):
        lib.gsr_workspace_sizes(C.byref(native.FramePlan()), g, i)
    with pytest.raises(C.ArgumentError):
        native.backward_rows_size(desc, desc)
    # the checked call raises under the function's own name, with the status and the library's message
    with pytest.raises(native.GsrError, match=r"^gsr_workspace_sizes failed \(status -1\): .*sh_degree") as e:
        native.workspace_sizes(native.make_desc(10, 5, 16, 64, 64, 0.5, 0.5, 1.0, False, False))
    assert e.value.status == -1
    assert lib.gsr_workspace_sizes(desc, g, i) == 0 and (g.value, i.value) == native.workspace_sizes(desc)


def test_every_struct_of_the_header_has_one_mirror_with_its_layout(native, tmp_path):
    """include/gsrast.h is plain C: gcc compiles it, and size + every field offset of each struct equals the ctypes
    mirror's (the layout a cgo / JNI / ctypes binding of the header would see).  Every struct typedef of the header has exactly
    one mirror, found through the names the mirror records; only gsr_children and gsr_children_grads share one."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not on PATH")
    typedefs = header_struct_typedefs(_header())
    assert len(typedefs) == len(set(typedefs)) == 20
    assert {"gsr_frame_desc", "gsr_frame_plan", "gsr_camera", "gsr_gaussians", "gsr_grads", "gsr_debug_views", "gsr_aux_outputs",
            "gsr_camera_grads", "gsr_contrib_stats", "gsr_contrib_error", "gsr_structured_desc", "gsr_structures", "gsr_children",
            "gsr_children_grads", "gsr_structured_grads", "gsr_decoder_desc", "gsr_decoder_params", "gsr_decoder_grads",
            "gsr_adam_tensor", "gsr_mcmc_tensor"} == set(typedefs)
    assert set(native.MIRRORS) == set(typedefs), "a struct of the header without a mirror, or a mirror of no struct"
    for cname, mirror in native.MIRRORS.items():
        assert cname in mirror.c_names
    shared = {c for c, m in native.MIRRORS.items() if len(m.c_names) > 1}
    assert shared == {"gsr_children", "gsr_children_grads"} and native.ChildrenGrads is native.Children
    pairs = [(cname, native.MIRRORS[cname]) for cname in typedefs]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsrast.h"', 'int main(void) {']
    for cname, mirror in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in pairs:
        assert int(got[cname]) == C.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, f"{cname}.{fname}"
        # no field of the header is missing from the mirror: the declared names are the mirror's, in order
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (cname, cname), _header(), re.S).group(1)
        declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:\[[^\]]*\])?\s*(?:,|$)", decl.strip())]
        assert declared == [f for f, _ in mirror._fields_], cname


def test_constants_mirrored_by_hand_match_the_header(native):
    code = _header()
    defines = dict(re.findall(r"^\s*#define\s+(GSR_\w+)\s+(\S+)", code, re.M))
    enum = dict(re.findall(r"\b(GSR_\w+)\s*=\s*(-?\d+)", code))
    assert int(defines["GSR_MAX_CHUNKS"]) == native.MAX_CHUNKS
    assert int(defines["GSR_SCREEN_GRAD_STRIDE"]) == native.SCREEN_GRAD_STRIDE
    assert int(defines["GSR_ADAM_MAX_TENSORS"]) == native.ADAM_MAX_TENSORS
    assert int(defines["GSR_MCMC_MAX_TENSORS"]) == native.MCMC_MAX_TENSORS
    assert {k[len("GSR_MCMC_ROLE_"):].lower(): int(v) for k, v in defines.items() if k.startswith("GSR_MCMC_ROLE_")} == native.MCMC_ROLES
    assert int(enum["GSR_ERR_WORKSPACE"]) == native.ERR_WORKSPACE
    assert defines["GSR_ADAM_STEP_UNCORRECTED"] == "INT64_MAX" and native.ADAM_STEP_UNCORRECTED == 2 ** 63 - 1
    assert int(defines["GSR_PROFILE_NAME_LEN"]) == native.PROFILE_NAME_LEN
    assert int(defines["GSR_VERSION"]) == native.load().gsr_version()
