"""Every diagnostic build of the kernels (tools/README.md, table "diagnostic builds") still compiles.

No test, build() or smoke() builds these variants, so a kernel change can break the build a tool needs without anything
noticing.  This is the cheap half of the check: a device-side, syntax-only hipcc pass over zsmi_api.hip per set of flags
(no code generation, no library loaded, no GPU).  BUILDS is the list the table in tools/README.md is written from.
"""
import os, re, shutil, subprocess
from concurrent.futures import ThreadPoolExecutor
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOOKS = "-DZSMI_DEBUG_HOOKS"

BUILDS = [
    (),                                     # the product library
    (HOOKS,),                               # the debug-hook library (zsmi_dbg_copyScratch, ZSMI_STOP_* stage stops)
    (HOOKS, "-DZS_DEC_PROFILE"),            # tools/dec_profile.py
    (HOOKS, "-DZS_PREP_PROFILE"),           # tools/prep_profile.py
    (HOOKS, "-DZS_WALK_PROFILE"),           # tools/walk_profile.py
    (HOOKS, "-DZS_CHAIN_COUNT"),            # tools/chain_count.py
    ("-DZS_DEC_ERRLINE",),
    ("-DZS_EXEC_STOP=1",), ("-DZS_EXEC_STOP=2",), ("-DZS_EXEC_STOP=3",), ("-DZS_EXEC_STOP=4",), ("-DZS_EXEC_STOP=5",), ("-DZS_EXEC_STOP=6",),
    ("-DZS_WALK_STOP=1",),
    ("-DZS_STITCH_STOP=1",), ("-DZS_STITCH_STOP=2",),
]


def _syntax_check(flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", *flags,
           os.path.join(ROOT, "zstandard_amd", "csrc", "zsmi_api.hip")]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def compiled():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    with ThreadPoolExecutor(max_workers=8) as pool:                  # ~5 s of one CPU each
        return dict(zip(BUILDS, pool.map(_syntax_check, BUILDS)))


@pytest.mark.parametrize("flags", BUILDS, ids=lambda f: " ".join(f) or "default")
def test_diagnostic_build_compiles(compiled, flags):
    out = compiled[flags]
    assert out.returncode == 0, out.stderr[-4000:]


def test_table_and_list_name_the_same_builds():
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    table = text[text.index("## Diagnostic builds"):]
    rows = set()
    for macro, values in re.findall(r"^\| `-D(\w+)(?:=([\d, ]+))?`", table, flags=re.M):
        rows |= {"-D%s=%s" % (macro, v.strip()) for v in values.split(",")} if values else {"-D" + macro}
    assert rows == {f for flags in BUILDS for f in flags}
