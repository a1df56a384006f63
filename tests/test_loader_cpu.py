"""The one loader every binding uses (terrain_diffusion_amd._lib.Library), against a tiny C library built in tmp_path: no GPU."""
import ctypes as C
import subprocess

import pytest

_SRC = """
static const char* text = "";
const char* tiny_last_error(void) { return text; }
int tiny_call(int fail) { text = fail ? "tiny_call: asked to fail" : ""; return fail ? -1 : 0; }
"""


def test_library_loads_once_binds_every_entry_and_checks_return_codes(tmp_path):
    from terrain_diffusion_amd._lib import Library, TdError
    (tmp_path / "tiny.c").write_text(_SRC)
    so = str(tmp_path / "libtiny.so")
    subprocess.check_call(["cc", "-shared", "-fPIC", "-o", so, str(tmp_path / "tiny.c")])
    sigs = {"tiny_last_error": (C.c_char_p, []), "tiny_call": (C.c_int, [C.c_int])}
    tiny = Library(so, sigs, "tiny_last_error", "tiny")
    assert tiny.handle is None and tiny.path == so                 # nothing is loaded before the first use
    handle = tiny.lib()
    assert tiny.lib() is handle                                    # a second call returns the same handle
    assert handle.tiny_call.restype is C.c_int and handle.tiny_call.argtypes == [C.c_int]
    assert handle.tiny_last_error.restype is C.c_char_p
    tiny.check(handle.tiny_call(0))                                # check(0) passes
    tiny.check(0)
    with pytest.raises(TdError, match=r"^tiny error -1: tiny_call: asked to fail$"):
        tiny.check(handle.tiny_call(1))                            # check(-1) carries the library's last-error text
    with pytest.raises(AttributeError):                            # a signature naming a symbol the library lacks
        Library(so, dict(sigs, tiny_absent=(C.c_int, [])), "tiny_last_error", "tiny").lib()
    with pytest.raises(TdError, match="no CPU fallback"):
        Library(str(tmp_path / "libnone.so"), sigs, "tiny_last_error", "tiny").lib()
