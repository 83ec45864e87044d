"""CPU checks of elp_get_mip_info's boundary (no GPU): the header declares it,
the struct's size agrees between the C compiler and the ctypes mirror, the
library exports the symbol, and the ABI version did not move."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "easylp_hip.h")


def _lib():
    import torch
    if torch.cuda.is_available():  # (a GPU box: torch starts the HIP runtime first, as tests/test_abi.py)
        torch.cuda.init()
    from easylp_amd._lib import load
    return load()


def test_header_declares_mip_info():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+elp_get_mip_info\s*\(\s*elp_handle\s*\*\s*\w+\s*,\s*elp_mip_info\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+elp_mip_info\s*\{", text)
    from easylp_amd._lib import EXPORTS
    assert "elp_get_mip_info" in EXPORTS


def test_struct_size_matches_the_compiler(tmp_path):
    from easylp_amd._lib import ElpMipInfo
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "easylp_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(elp_mip_info), offsetof(elp_mip_info, tree_launches),'
                   ' offsetof(elp_mip_info, reserved)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    size, off_tl, off_res = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(ElpMipInfo) == 64
    assert off_tl == ElpMipInfo.tree_launches.offset == 16
    assert off_res == ElpMipInfo.reserved.offset == 48


def test_library_exports_the_symbol():
    lib = _lib()
    assert hasattr(lib, "elp_get_mip_info")
    from easylp_amd._lib import ElpMipInfo
    info = ElpMipInfo()
    assert lib.elp_get_mip_info(None, ctypes.byref(info)) == -1  # (ELP_E_ARG: a NULL handle)
    assert b"elp_get_mip_info" in lib.elp_last_error()


def test_abi_version_is_still_7():
    from easylp_amd._lib import ABI_VERSION
    assert ABI_VERSION == 7
    assert _lib().elp_abi_version() == 7
    assert re.search(r"#define\s+ELP_ABI_VERSION\s+7\b", open(HEADER).read())
