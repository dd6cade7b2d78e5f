"""Host-side checks of the digested-dictionary calls (no device): the header, _lib.EXPORTS and the library agree on their names; the
calls that take a NULL CDict without touching a device."""
import ctypes, os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zsmi_createCDict", "zsmi_freeCDict", "zsmi_getDictID_fromCDict", "zsmi_sizeofCDict",
         "zsmi_compressBatchDevice_usingCDict", "zsmi_compressBatchHost_usingCDict", "zsmi_compress_usingCDict"]


def test_header_exports_and_library_agree():
    from zstandard_amd import _lib
    so = ctypes.CDLL(_lib.build())
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zsmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(zsmi_[A-Za-z0-9_]+)\s*\(", hdr))
    assert "typedef struct zsmi_cdict zsmi_cdict;" in hdr
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(so, n), n
    L = _lib.lib()
    for n in NAMES:
        assert getattr(L, n).argtypes is not None, n                      # a ctypes prototype each


def test_null_cdict_is_harmless():
    from zstandard_amd import _lib
    L = _lib.lib()
    L.zsmi_freeCDict(None)
    assert L.zsmi_getDictID_fromCDict(None) == 0
    assert L.zsmi_sizeofCDict(None) == 0
    err = ctypes.c_int(-1)
    assert not L.zsmi_createCDict(None, b"abc", 3, 3, ctypes.byref(err)) and err.value == 62       # init_missing: no context
