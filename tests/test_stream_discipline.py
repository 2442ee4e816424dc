"""Source-level stream discipline of the native library and its ctypes binding (CPU only).

Every entry point of the C ABI takes the caller's stream.  A launch, memset, copy, event record or synchronisation that names any
other stream (or none) computes the right values on the default stream of an idle process - which is all the rest of the suite
runs - and corrupts a trainer that prefetches on a side stream.  tests/test_gpu_streams.py checks that dynamically; this file holds
the static property, on csrc/*.hip and *.h and on _native.py, and proves on mutated copies (strings, never files of the repository)
that it notices what it is for.

The C side is read with a small tokenizer: comments and string literals are blanked, #define bodies are checked against the macro's
own parameters (and, for a helper macro defined inside a function, that function's stream), code under the debug-trace switches
(DEBUG_ONLY_MACROS: not part of the library build) is dropped, calls are split at top-level commas with parentheses balanced (some
launches span lines), and the function around a call is the outermost brace block whose header has a parameter list."""
import ast
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "structured-gaussian-splatting_amd")
CSRC = os.path.join(PKG, "csrc")
NATIVE_PY = os.path.join(PKG, "diff_gaussian_rasterization", "_native.py")
HEADER = os.path.join(ROOT, "include", "gsrast.h")

# preprocessor switches of tools-only debug builds (csrc/gsr_render.hip: the block-trace dump); the library build defines neither
DEBUG_ONLY_MACROS = ("GSR_BWD_TRACE", "GSR_FWD_TRACE")


def source_files():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


# ---- tokenizer ------------------------------------------------------------------------------------------------------------------

def blank_comments_and_strings(text: str) -> str:
    """The text with comments, string and character literals replaced by spaces (newlines kept: positions and lines stay)."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i)); i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("".join(ch if ch == "\n" else " " for ch in text[i:j])); i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            j = min(j + 1, n)
            out.append(c + " " * (j - i - 2) + c if j - i >= 2 else c); i = j
        else:
            out.append(c); i += 1
    return "".join(out)


def split_preprocessor(clean: str):
    """(code, macros): `code` is `clean` with every preprocessor directive (continuation lines included) and every region under a
    DEBUG_ONLY_MACROS conditional blanked; macros = [(name, [params], body, offset of the body in the text)] of the #defines."""
    lines = clean.split("\n")
    keep = [True] * len(lines)          # False: blank the line
    macros, stack, i, offset = [], [], 0, 0
    offsets = []
    for ln in lines:
        offsets.append(offset); offset += len(ln) + 1
    while i < len(lines):
        if not lines[i].lstrip().startswith("#"):
            keep[i] = not any(stack)
            i += 1
            continue
        j = i
        while lines[j].rstrip().endswith("\\") and j + 1 < len(lines):
            j += 1
        directive = "\n".join(lines[i:j + 1])
        m = re.match(r"\s*#\s*(\w+)(.*)", directive, re.S)
        word, rest = (m.group(1), m.group(2)) if m else ("", "")
        if word in ("if", "ifdef", "ifndef"):
            stack.append(word != "ifndef" and any(re.search(r"\b%s\b" % d, rest) for d in DEBUG_ONLY_MACROS))
        elif word in ("else", "elif") and stack:
            stack[-1] = False                    # the other branch of a debug-only conditional is library code
        elif word == "endif" and stack:
            stack.pop()
        elif word == "define" and not any(stack):
            d = re.match(r"\s*(\w+)(\(([^)]*)\))?(.*)", rest, re.S)
            if d:
                params = [p.strip() for p in (d.group(3) or "").split(",") if p.strip()]
                body = d.group(4).replace("\\\n", " \n")
                macros.append((d.group(1), params, body, offsets[i] + directive.index(d.group(4)) if d.group(4) else offsets[i]))
        for k in range(i, j + 1):
            keep[k] = False
        i = j + 1
    code = "\n".join(ln if k else " " * len(ln) for ln, k in zip(lines, keep))
    return code, macros


def call_args(code: str, open_paren: int):
    """The arguments of the call whose '(' is at `open_paren`, split at top-level commas ((), [], {} balanced; <> are not brackets
    here: kernel template arguments with commas sit inside the parentheses hipLaunchKernelGGL asks for), and the offset behind
    its ')'."""
    assert code[open_paren] == "("
    depth, args, start, i = 0, [], open_paren + 1, open_paren
    while i < len(code):
        c = code[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(code[start:i])
                return [a.strip() for a in args], i + 1
        elif c == "," and depth == 1:
            args.append(code[start:i]); start = i + 1
        i += 1
    raise ValueError("unbalanced parentheses")


def function_blocks(code: str):
    """[(header, body_begin, body_end)] of the outermost brace blocks whose header (the text since the last ';', '{' or '}') has a
    parameter list: the functions of a translation unit (namespace / extern / struct blocks have none and are looked into)."""
    blocks, stack, last = [], [], 0
    for i, c in enumerate(code):
        if c == "{":
            header = code[last:i]
            is_fn = "(" in header and not re.match(r"\s*(namespace|extern|struct|class|union|enum)\b[^()]*$", header)
            inside_fn = any(s[0] for s in stack)
            stack.append((is_fn and not inside_fn, header, i))
            last = i + 1
        elif c == "}":
            if stack:
                outer, header, begin = stack.pop()
                if outer:
                    blocks.append((header, begin, i))
            last = i + 1
        elif c == ";":
            last = i + 1
    return blocks


def norm(expr: str) -> str:
    return re.sub(r"\s+", "", expr)


def streams_of(header: str, body: str):
    """The spellings of the caller's stream inside one function: its hipStream_t parameters, `(hipStream_t)stream` of a `void
    *stream` parameter, and locals initialised from one of those."""
    names = set(re.findall(r"\bhipStream_t\s+(\w+)", header))
    if re.search(r"\bvoid\s*\*\s*stream\b", header):
        names.add("(hipStream_t)stream")
    for _ in range(2):
        for m in re.finditer(r"\bhipStream_t\s+(\w+)\s*=\s*([^;]+);", body):
            if norm(m.group(2)) in names:
                names.add(m.group(1))
    return names


ASYNC_OK = re.compile(r"hipMem(set|cpy)\w*Async$")
CALL = re.compile(r"\b(hipLaunchKernelGGL|hipMem(?:set|cpy)\w*|hipDeviceSynchronize|hipStreamSynchronize|hipEventRecord|"
                  r"hipStreamWaitEvent|GSR_LAUNCH_CHECK)\s*\(")


def check_source(text: str, name: str = "<string>"):
    """(violations, launches): every rule of this file on one translation unit's text."""
    clean = blank_comments_and_strings(text)
    code, macros = split_preprocessor(clean)
    bad, launches = [], 0

    def line_of(pos):
        return clean.count("\n", 0, pos) + 1

    def check_call(fn, args, streams, where):
        nonlocal launches
        if fn == "hipLaunchKernelGGL":
            launches += 1
            if len(args) < 5 or norm(args[4]) not in streams:
                bad.append(f"{where}: hipLaunchKernelGGL's stream argument is `{args[4] if len(args) > 4 else ''}`, not the function's "
                           f"stream {sorted(streams)}")
        elif fn == "hipDeviceSynchronize":
            bad.append(f"{where}: hipDeviceSynchronize")
        elif fn.startswith("hipMem"):
            if not ASYNC_OK.match(fn):
                bad.append(f"{where}: {fn} is not the Async form")
            elif norm(args[-1]) not in streams:
                bad.append(f"{where}: {fn}'s last argument is `{args[-1]}`, not the function's stream {sorted(streams)}")
        elif fn in ("hipStreamSynchronize", "hipStreamWaitEvent"):
            if norm(args[0]) not in streams:
                bad.append(f"{where}: {fn}({args[0]}) does not name the function's stream {sorted(streams)}")
        elif fn in ("hipEventRecord", "GSR_LAUNCH_CHECK"):
            if len(args) < 2 or norm(args[-1]) not in streams:
                bad.append(f"{where}: {fn}'s last argument is `{args[-1]}`, not the function's stream {sorted(streams)}")

    if "<<<" in code or any("<<<" in m[2] for m in macros):
        bad.append(f"{name}: a <<< >>> launch (use hipLaunchKernelGGL: its stream is the fifth argument)")
    blocks = function_blocks(code)
    for m in CALL.finditer(code):
        where = f"{name}:{line_of(m.start())}"
        args, _ = call_args(code, m.end() - 1)
        fn_block = next(((h, b, e) for h, b, e in blocks if b < m.start() < e), None)
        if fn_block is None:
            bad.append(f"{where}: {m.group(1)} outside any function")
            continue
        header, b, e = fn_block
        check_call(m.group(1), args, streams_of(header, code[b:e]), where)
    for mname, params, body, off in macros:
        # a helper macro defined inside a function (and used there) may also name that function's stream
        around = next((streams_of(h, code[b:e]) for h, b, e in blocks if b < off < e), set())
        for m in CALL.finditer(body):
            args, _ = call_args(body, m.end() - 1)
            check_call(m.group(1), args, set(params) | around, f"{name}:{line_of(off + m.start())} (#define {mname})")
    return bad, launches


# ---- the C side -----------------------------------------------------------------------------------------------------------------

def test_every_launch_memset_copy_and_sync_names_the_callers_stream():
    bad, launches, plain = [], 0, 0
    for path in source_files():
        with open(path) as f:
            text = f.read()
        b, n = check_source(text, os.path.relpath(path, ROOT))
        bad += b
        launches += n
        plain += len(re.findall(r"\bhipLaunchKernelGGL\b", blank_comments_and_strings(text)))
    assert not bad, "\n".join(bad)
    # the parser sees every launch a plain text search sees (comments aside; 102 when this test was written): what the preprocessor
    # pass leaves out holds no launch, and a launch the parser cannot read is not a launch it passes
    assert launches == plain and launches > 0, f"{launches} launches parsed, {plain} in the text"


def test_debug_only_regions_are_the_only_code_left_out():
    """What DEBUG_ONLY_MACROS hides is not compiled into the library: csrc/Makefile defines none of them."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    for d in DEBUG_ONLY_MACROS:
        assert d not in mk, f"csrc/Makefile mentions {d}: code under it is part of the build and must be checked"


def _one_file():
    path = os.path.join(CSRC, "gsr_render.hip")          # holds a launch that spans lines
    with open(path) as f:
        return f.read()


def _mutate_nth_launch(text: str, n: int, new_stream: str) -> str:
    clean = blank_comments_and_strings(text)
    hits = [m for m in re.finditer(r"\bhipLaunchKernelGGL\s*\(", clean)]
    m = hits[n]
    args, _ = call_args(clean, m.end() - 1)
    # the fifth argument's span: re-walk to find its offsets
    depth, commas, i = 0, [], m.end() - 1
    while True:
        c = clean[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                commas.append(i); break
        elif c == "," and depth == 1:
            commas.append(i)
        i += 1
    begin, end = commas[3] + 1, commas[4]
    assert norm(text[begin:end]) == norm(args[4])
    return text[:begin] + " " + new_stream + text[end:]


def test_selfcheck_a_launch_on_stream_0_is_reported():
    text = _one_file()
    base, launches = check_source(text, "copy")
    assert not base and launches >= 4
    for n in range(launches):                            # every launch of the file, the multi-line one included
        bad, _ = check_source(_mutate_nth_launch(text, n, "0"), "copy")
        assert len(bad) == 1 and "hipLaunchKernelGGL" in bad[0], (n, bad)
    bad, _ = check_source(_mutate_nth_launch(text, 0, "nullptr"), "copy")
    assert len(bad) == 1


@pytest.mark.parametrize("old, new, what", [
    ("hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), s)",
     "hipMemset(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float))", "not the Async form"),
    ("hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), s)",
     "hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), 0)", "last argument"),
    ("hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), s)",
     "hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), s)); GSR_HIP_CHECK(hipDeviceSynchronize()",
     "hipDeviceSynchronize"),
    ("hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), s)",
     "hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), s)); GSR_HIP_CHECK(hipStreamSynchronize(nullptr)",
     "hipStreamSynchronize"),
])
def test_selfcheck_other_violations_are_reported(old, new, what):
    text = _one_file()
    assert text.count(old) == 1
    bad, _ = check_source(text.replace(old, new), "copy")
    assert len(bad) == 1 and what in bad[0], bad


def test_selfcheck_triple_chevron_and_macro_and_comment():
    bad, n = check_source("__global__ void k(int *p);\nint f(int *p, hipStream_t s)\n{\n    k<<<1, 64, 0, s>>>(p);\n    return 0;\n}\n")
    assert len(bad) == 1 and "<<<" in bad[0]
    # a macro is held to its own parameters, and its uses to the function's stream
    macro = "#define CHECK(debug, stream) \\\n    do { if (debug) (void)hipStreamSynchronize(%s); } while (0)\n"
    assert check_source(macro % "stream")[0] == []
    assert len(check_source(macro % "0")[0]) == 1
    use = ("int f(int n, hipStream_t s)\n{\n    GSR_LAUNCH_CHECK(\"k\", true, %s);\n    return 0;\n}\n"
           "int g(void *stream) { GSR_LAUNCH_CHECK(\"k\", 1, %s); return 0; }\n")
    assert check_source(use % ("s", "(hipStream_t)stream"))[0] == []
    assert len(check_source(use % ("s", "s"))[0]) == 1              # g has no `s`
    assert len(check_source(use % ("0", "(hipStream_t) stream"))[0]) == 1
    # comments and strings are not code; a local alias of the stream is the stream
    ok = ("int f(void *stream)\n{\n    hipStream_t s = (hipStream_t)stream;   // hipDeviceSynchronize() would stall every stream\n"
          "    set_error(\"hipMemcpy(a, b) failed\");\n    hipLaunchKernelGGL((k<1, 2>), dim3(1), dim3(64), 0, s,\n        1, 2);\n    return 0;\n}\n")
    assert check_source(ok) == ([], 1)
    assert len(check_source(ok.replace("0, s,", "0, 0,"))[0]) == 1


# ---- the Python side ------------------------------------------------------------------------------------------------------------

def _abi_functions_taking_a_stream():
    with open(HEADER) as f:
        code = blank_comments_and_strings(f.read())
    out = set()
    for m in re.finditer(r"\b(gsr_\w+)\s*\(", code):
        args, _ = call_args(code, m.end() - 1)
        if args and re.fullmatch(r"void\s*\*\s*stream", args[-1]):
            out.add(m.group(1))
    return out


def check_native_py(text: str):
    """Violations of the binding's rule: every call of an ABI function that takes a stream passes, last, `_stream(d)` with d the
    wrapper's `device` parameter, `t.device` of a tensor `t` named in the same wrapper, or a local assigned from one; and
    torch.cuda.current_stream() is never called without a device."""
    tree = ast.parse(text)
    with_stream = _abi_functions_taking_a_stream()
    bad, seen = [], set()

    def device_expr_ok(node, fn):
        params = {a.arg for a in fn.args.args + fn.args.kwonlyargs}
        local_dev = {t.id for n in ast.walk(fn) if isinstance(n, ast.Assign) and isinstance(n.value, ast.Attribute) and n.value.attr == "device"
                     for t in n.targets if isinstance(t, ast.Name)}
        local_names = params | {n.id for n in ast.walk(fn) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
        if isinstance(node, ast.Name):
            return (node.id == "device" and node.id in params) or node.id in local_dev
        if isinstance(node, ast.Attribute) and node.attr == "device":
            root = node.value
            while isinstance(root, (ast.Subscript, ast.Attribute)):
                root = root.value
            return isinstance(root, ast.Name) and root.id in local_names
        return False

    for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        for call in [n for n in ast.walk(fn) if isinstance(n, ast.Call)]:
            f = call.func
            if isinstance(f, ast.Attribute) and f.attr == "current_stream" and fn.name != "_stream":
                if not call.args and not call.keywords:
                    bad.append(f"line {call.lineno}: torch.cuda.current_stream() without a device in {fn.name}")
            if not (isinstance(f, ast.Attribute) and f.attr.startswith("gsr_")):
                continue
            if f.attr not in with_stream:
                continue
            seen.add(f.attr)
            last = call.args[-1] if call.args else None
            if not (isinstance(last, ast.Call) and isinstance(last.func, ast.Name) and last.func.id == "_stream" and len(last.args) == 1):
                bad.append(f"line {call.lineno}: {f.attr} does not pass _stream(<device>) as its last argument")
            elif not device_expr_ok(last.args[0], fn):
                bad.append(f"line {call.lineno}: {f.attr} passes _stream({ast.unparse(last.args[0])}): not the device of one of the call's tensors")
    # indirect calls: `fn = load().gsr_x ... fn(..., _stream(device))` (backward_render, backward_geom) name the function outside a Call
    for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        named = {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and n.attr in with_stream}
        if named - seen:
            streams = [n for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "_stream"]
            if not streams or not all(device_expr_ok(s.args[0], fn) for s in streams):
                bad.append(f"{fn.name}: {sorted(named - seen)} called without _stream(<device>)")
            seen |= named
    return bad, seen


def test_native_binding_passes_the_tensors_stream_to_every_call():
    with open(NATIVE_PY) as f:
        text = f.read()
    bad, seen = check_native_py(text)
    assert not bad, "\n".join(bad)
    # every ABI function that takes a stream is bound (tests/test_abi.py holds the export list); none escaped this walk
    missing = _abi_functions_taking_a_stream() - seen
    assert not missing, f"not called from _native.py, or called in a way this test cannot read: {sorted(missing)}"
    m = re.search(r"def _stream\(device\)[^\n]*\n\s+return C\.c_void_p\(torch\.cuda\.current_stream\(device\)\.cuda_stream\)", text)
    assert m, "_native._stream(device) must read torch.cuda.current_stream(device)"


def test_selfcheck_native_binding_violations_are_reported():
    with open(NATIVE_PY) as f:
        text = f.read()
    one = "_gsr.gsr_dist2_knn3(P, _ptr(pts), _ptr(out), _ptr(ws), _stream(pts.device))"
    assert text.count(one) == 1
    for new in ("_gsr.gsr_dist2_knn3(P, _ptr(pts), _ptr(out), _ptr(ws), None)",
                "_gsr.gsr_dist2_knn3(P, _ptr(pts), _ptr(out), _ptr(ws), _stream(None))",
                "_gsr.gsr_dist2_knn3(P, _ptr(pts), _ptr(out), _ptr(ws), _stream(torch.device('cuda:0')))",
                "_gsr.gsr_dist2_knn3(P, _ptr(pts), _ptr(out), _ptr(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))"):
        bad, _ = check_native_py(text.replace(one, new))
        assert bad and any("gsr_dist2_knn3" in b or "current_stream" in b for b in bad), (new, bad)


def test_no_package_module_asks_for_the_current_stream_without_a_device():
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        with open(path) as f:
            tree = ast.parse(f.read())
        for n in ast.walk(tree):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "current_stream":
                assert n.args or n.keywords, f"{os.path.relpath(path, ROOT)}:{n.lineno}: torch.cuda.current_stream() without a device"
