"""m355_ssim_desc and m355_ssim (include/de265_mi355x.h) as a C compiler lays them out, against the ctypes mirrors of libde265_amd/capi.py:
sizeof and the offset of every member.  No device."""
import ctypes
import os
import subprocess

from libde265_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"m355_ssim_desc": capi.SsimDesc, "m355_ssim": capi.Ssim}


def test_structs_match_the_ctypes_mirrors(tmp_path):
    names = [(s, f) for s, mirror in STRUCTS.items() for f, _ in mirror._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"de265_mi355x.h\"\nint main(void){\n"
    src += "".join("printf(\"%%zu\\n\", sizeof(%s));\n" % s for s in STRUCTS)
    src += "".join("printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (s, f) for s, f in names)
    src += "printf(\"%d\\n\", M355_SSIM_REQUESTS);\nreturn 0;}\n"
    exe = str(tmp_path / "ssim_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:len(STRUCTS)] == [ctypes.sizeof(m) for m in STRUCTS.values()]
    for (s, f), off in zip(names, got[len(STRUCTS):]):
        assert off == getattr(STRUCTS[s], f).offset, "%s.%s" % (s, f)
    assert got[-1] == capi.SSIM_REQUESTS
    assert ctypes.sizeof(capi.SsimDesc) == 152 and ctypes.sizeof(capi.Ssim) == 88
