"""The size word - a byte count or (uint32_t)-code - is stated once, in csrc/zsmi_status.h: the header compiled ALONE into a host program
(tests/c/size_word.cpp, under the address and undefined-behaviour sanitizers) checks itself and prints its verdicts, which are held here
against the library's zsmi_isError; and the sources keep the rule - no other file spells the boundary out, and the host code talks to the
device and the stream through the context's verbs (csrc/zsmi_ctx.h)."""
import os, re, subprocess
import pytest
from zstandard_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")


@pytest.fixture(scope="module")
def words(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("size_word") / "size_word")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "size_word.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr                   # (its own checks, and the sanitizers')
    return [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]


def test_every_code_makes_an_error_word(words):
    """(word, verdict, code, bytes) of the codes 1 .. 119, then of 0xFFFFFF88, 0xFFFFFF89, 0 and the one-shot capacity clamp"""
    assert len(words) == 119 + 4
    for code, (w, verdict, got, nbytes) in enumerate(words[:119], 1):
        assert (w, verdict, got, nbytes) == ((1 << 32) - code, 1, code, 0)
    last, above, zero, clamp = words[119:]
    assert last == (0xFFFFFF88, 0, 0, 0xFFFFFF88) and above == (0xFFFFFF89, 1, 119, 0) and zero == (0, 0, 0, 0)
    assert clamp[1] == 0 and clamp[0] == clamp[3] < (1 << 32) - 119            # a size, below the first error word


def test_verdicts_are_zsmi_isError_of_the_widened_word(words):
    """the 32-bit verdict is the C ABI's of the same code as a size_t: an error word widens to (size_t)-code, a size to itself"""
    _lib.build()
    L = _lib.lib()
    for w, verdict, code, _ in words:
        wide = (1 << 64) - code if verdict else w
        assert L.zsmi_isError(wide) == verdict, hex(w)
        assert L.zsmi_getErrorCode(wide) == code, hex(w)
    assert L.zsmi_isError((1 << 64) - 120) == 0 and L.zsmi_isError((1 << 64) - 119) == 1      # (size_t)-120 is the largest that is none


def _code(path):
    txt = open(path, errors="replace").read()
    return re.sub(r"#[^\n]*", "", txt) if path.endswith(".py") else re.sub(r"//[^\n]*|/\*.*?\*/", "", txt, flags=re.S)


def _sources():
    for root, _, files in os.walk(os.path.join(ROOT, "zstandard_amd")):
        for f in sorted(files):
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                yield f, os.path.join(root, f)


def test_the_boundary_is_spelled_once():
    """with comments stripped, no source of the package outside zsmi_status.h holds the literal"""
    for f, path in _sources():
        if f != "zsmi_status.h":
            assert not re.search(r"0xFFFFFF88", _code(path), flags=re.I), f
    assert "ZSMI_error_maxCode" in _code(os.path.join(CSRC, "zsmi_status.h"))


# where the five runtime calls may stand in host code outside zsmi_ctx.h: the function (as the text that opens it) and the calls it holds
HIP_CALLS = r"\b(hipMemcpyAsync|hipMemsetAsync|hipStreamSynchronize|hipGetLastError|hipSetDevice)\b"
ALLOWED = {
    "zsmi_api.hip": {"zsmi_ctx *zsmi_createCtx(": {"hipSetDevice": 1, "hipGetLastError": 1}, "void zsmi_freeCtx(": {"hipStreamSynchronize": 1},
                     "int zsmi_getKernelTimes(": {"hipStreamSynchronize": 1}, "int zsmi_dbg_copyScratch(": {"hipStreamSynchronize": 1}},
    "seekable.hip": {"zsmi_seekable *zsmi_openSeekable(": {"hipGetLastError": 1}},
}


def test_host_code_speaks_to_the_stream_through_the_verbs():
    """hipMemcpyAsync, hipMemsetAsync, hipStreamSynchronize, hipGetLastError and hipSetDevice: in zsmi_ctx.h (the verbs, TurnBufs), and outside
    it only where the comment at the verbs says - each occurrence inside the function that is allowed it, and no more of them than listed"""
    for f, path in _sources():
        if f == "zsmi_ctx.h" or f.endswith(".py"):
            continue
        code = _code(path)
        found = {}
        for m in re.finditer(HIP_CALLS, code):
            # the function an occurrence is in: the last line before it that starts at column 0 with a declaration and opens a parameter list
            heads = [h for h in re.finditer(r"^(?:extern \"C\" |static )?[A-Za-z_][^\n;{}]*\(", code[:m.start()], flags=re.M)]
            head = heads[-1].group(0) if heads else ""
            key = next((k for k in ALLOWED.get(f, {}) if k in head), None)
            assert key is not None, (f, m.group(0), head)
            found.setdefault(key, {}).setdefault(m.group(0), 0)
            found[key][m.group(0)] += 1
        assert found == ALLOWED.get(f, {}), f
